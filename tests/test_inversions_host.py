"""The small-inversion logic the device stage runs (ma_amd/host/ma_inv_dev.h: scanDrops, stretchJob, assemble, kept, place) on
the host: tests/emul/inv_dev_test.cpp compares it with the host module's restatement (SmallInversions::DropScan of
ma_amd/host/ma_modules.h, the yardstick) and with the inversion records of the dumps the compiled reference wrote
(tests/golden/inv.*, tests/golden/f4.default.inv1.pair0.zd100.opt0); once as an optimised build, once under AddressSanitizer +
UBSan (a stand-alone program, nothing is preloaded anywhere)."""
import os
import re
import subprocess

import pytest

from ma_testlib import ROOT, gunzip_to

G = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(ROOT, "tests", "emul", "inv_dev_test.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
# (case, dump, paired, Z Drop Inversions, inversion records of the dump -- tests/golden/make_inv_golden.py prints them)
GOLDENS = [("inv.case", "inv.default.pair0.zd40.opt3", 0, 40, 26), ("inv.case", "inv.default.pair1.zd40.opt1", 1, 40, 26),
           ("inv.case", "inv.default.pair0.zd100.opt0", 0, 100, 14), ("f4.case", "f4.default.inv1.pair0.zd100.opt0", 0, 100, 5)]


def build_exe(kind="plain"):
    exe = os.path.join(ROOT, "tests", "emul", "inv_dev_test" + ("" if kind == "plain" else "_san"))
    deps = [SRC, os.path.join(ROOT, "tests", "emul", "inv_common.h"), os.path.join(ROOT, "tests", "emul", "sam_dev_common.h"), os.path.join(ROOT, "include", "ma_amd.h"),
            os.path.join(ROOT, "oracle", "dump_format.h"), os.path.join(ROOT, "ma_amd", "libma_amd.so"),
            os.path.join(ROOT, "ma_amd", "csrc", "nw.h")] + [
        os.path.join(ROOT, "ma_amd", "host", h) for h in ("ma_inv_dev.h", "ma_sam_dev.h", "ma_flat_sam.h", "ma_sam.h", "ma_modules.h", "ms_graph.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + BUILDS[kind] + [
            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ma_amd", "host"), SRC, "-o", exe,
            "-L" + os.path.join(ROOT, "ma_amd"), "-lma_amd", "-Wl,-rpath," + os.path.join(ROOT, "ma_amd"), "-lpthread"])
    return exe


def run(args):
    # (the HIP runtime the library links against keeps allocations of its own until the process ends)
    return subprocess.check_output(args, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0")).decode()


@pytest.fixture(scope="module", params=list(BUILDS))
def exe(request):
    return build_exe(request.param)


@pytest.mark.parametrize("golden", GOLDENS, ids=[g[1] for g in GOLDENS])
def test_golden_records(tmp_path, exe, golden):
    """every 'f' record of the reference's dump: scanDrops == DropScan under "Z Drop Inversions" 1, 40, 100 and 100000; at the
    dump's own value the records behind a parent are exactly its stretches' records, in stretch order, and assemble rebuilds
    each of them from its own ops and the bases of the case: bounds, score, ops, flags, mapq bits, strip index"""
    case, dump, paired, zd, want = golden
    c = gunzip_to(os.path.join(G, case + ".gz"), str(tmp_path / case))
    d = gunzip_to(os.path.join(G, dump + ".f4.gz"), str(tmp_path / "ref.f4"))
    out = run([exe, "golden", c, d, str(paired), str(zd)])
    print(out)
    m = re.match(r"golden ok: (\d+) records, (\d+) scans compared, (\d+) stretches, (\d+) inversion records rebuilt, (\d+) without", out)
    records, _, stretches, rebuilt, filtered = [int(x) for x in m.groups()]
    # stretches == inversion records rebuilt + stretches whose record the score filter dropped; all records of the dump are found
    assert records > 100 and stretches == rebuilt + filtered and rebuilt == want


def test_hand_made_records(exe):
    """no seed op at all, a drop only behind the last seed, a drop before the first seed, two stretches in one record, a
    stretch with qlen 0 and one with tlen 0, >= at the exact drop, a window score of exactly harm_score_min * match (dropped)
    and one match more (kept), disable_heuristics keeping an empty record, a parent on the reverse strand (window on the
    forward strand), stretches beyond the read / the text / across the strands refused, M runs split and merged"""
    assert run([exe, "handmade"]).startswith("handmade ok")
