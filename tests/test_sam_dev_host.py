"""The record formatter the device stage runs (ma_amd/host/ma_sam_dev.h) on the host: tests/emul/sam_dev_test.cpp compares it,
and the host's flat writer on top of it (flat::formatRead, ma_amd/host/ma_flat_sam.h), byte for byte with ma_amd's FileWriter on
Alignment containers (ma_amd/host/ma_sam.h, the independent yardstick) and with the SAM text the reference's FileWriter printed
(tests/golden/small_ref.*.sam.gz); once as an optimised build, once under AddressSanitizer + UBSan (a stand-alone program,
nothing is preloaded anywhere)."""
import os
import subprocess

import pytest

from ma_testlib import ROOT, gunzip_to

G = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(ROOT, "tests", "emul", "sam_dev_test.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def build_exe(kind="plain"):
    exe = os.path.join(ROOT, "tests", "emul", "sam_dev_test" + ("" if kind == "plain" else "_san"))
    deps = [SRC, os.path.join(ROOT, "tests", "emul", "sam_dev_common.h"), os.path.join(ROOT, "include", "ma_amd.h"),
            os.path.join(ROOT, "oracle", "dump_format.h"), os.path.join(ROOT, "ma_amd", "libma_amd.so")] + [
        os.path.join(ROOT, "ma_amd", "host", h) for h in ("ma_sam_dev.h", "ma_flat_sam.h", "ma_sam.h", "ma_modules.h", "ms_graph.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall"] + BUILDS[kind] + ["-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "ma_amd", "host"), SRC, "-o", exe, "-L" + os.path.join(ROOT, "ma_amd"),
                               "-lma_amd", "-Wl,-rpath," + os.path.join(ROOT, "ma_amd"), "-lpthread"])
    return exe


def run(args):
    # (the HIP runtime the library links against keeps allocations of its own until the process ends)
    return subprocess.check_output(args, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0")).decode()


@pytest.fixture(scope="module", params=list(BUILDS))
def exe(request):
    return build_exe(request.param)


@pytest.mark.parametrize("preset,opt", [("default", 0), ("default", 1), ("default", 2), ("default", 3), ("illumina", 0)])
def test_golden_records(tmp_path, exe, preset, opt):
    """the MappingQuality records of the reference's pipeline dump: shared formatter == flat::formatRead == FileWriter == the
    golden's record lines; the counting sink returns exactly the bytes written"""
    case = gunzip_to(os.path.join(G, "small.case.gz"), str(tmp_path / "small.case"))
    pipe = gunzip_to(os.path.join(G, "small_ref.%s.pipe.gz" % preset), str(tmp_path / "p.pipe"))
    sam = gunzip_to(os.path.join(G, "small_ref.%s.opt%d.sam.gz" % (preset, opt)), str(tmp_path / "g.sam"))
    out = run([exe, "golden", case, pipe, sam, str(opt)])
    assert out.startswith("golden ok: 128 reads")


def test_random_record_lists(exe):
    """3000 seeded random lists under all 32 option sets: both strands, 1-3 contigs (two of one name), numbers on both sides of
    every decimal boundary up to 10^9, the read lengths around the wavefront's strides, codes above 3, with and without
    qualities, names of 1-40 bytes, empty lists and lists of zero-length alignments only; shared formatter == flat::formatRead ==
    FileWriter"""
    out = run([exe, "random", "20261018", "3000"])
    assert out.startswith("random ok: 3000 lists x 32 option sets")


def test_long_cigars_and_error_texts(exe):
    """65 535 / 65 536 ops (the CG:B:I tag and its switch), and the two texts of a record that ends beyond its read: FileWriter's
    exception == the shared formatter's error text == flat::formatRead's exception"""
    assert run([exe, "special"]).startswith("special ok")
