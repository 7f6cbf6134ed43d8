"""The paired-end record formatter the device stage runs (ma_amd/host/ma_sam_dev.h: ma_sam::formatPair) on the host:
tests/emul/sam_pair_dev_test.cpp compares it, and the host's flat writer on top of it (flat::formatPair,
ma_amd/host/ma_flat_sam.h), byte for byte with ma_amd's PairedFileWriter on Alignment containers (ma_amd/host/ma_sam.h, the
independent yardstick) and with the SAM text the reference's PairedFileWriter printed
(tests/golden/f4.illumina.inv0.pair1.zd100.opt3.sam.gz); once as an optimised build, once under AddressSanitizer + UBSan (a
stand-alone program, nothing is preloaded anywhere)."""
import os
import subprocess

import pytest

from ma_testlib import ROOT, gunzip_to

G = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(ROOT, "tests", "emul", "sam_pair_dev_test.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
PAIR_GOLDEN = "f4.illumina.inv0.pair1.zd100.opt3"


def build_exe(kind="plain"):
    exe = os.path.join(ROOT, "tests", "emul", "sam_pair_dev_test" + ("" if kind == "plain" else "_san"))
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


def test_golden_pairs(tmp_path, exe):
    """the PairedReads records of the reference's f4 dump under options 3: shared formatter == flat::formatPair ==
    PairedFileWriter == the golden's record lines; the counting sink returns exactly the bytes written"""
    case = gunzip_to(os.path.join(G, "f4.case.gz"), str(tmp_path / "f4.case"))
    dump = gunzip_to(os.path.join(G, PAIR_GOLDEN + ".f4.gz"), str(tmp_path / "ref.f4"))
    sam = gunzip_to(os.path.join(G, PAIR_GOLDEN + ".sam.gz"), str(tmp_path / "g.sam"))
    out = run([exe, "golden", case, dump, sam, "3"])
    print(out)
    assert out.startswith("golden ok: ") and int(out.split()[2]) > 50


def test_random_pairs(exe):
    """3000 seeded random pairs under all 32 option sets: picked pairs on every strand combination, single lists of 1-5 records
    with secondaries and supplementaries, lists the option bits empty, lists whose record 0 is filtered, zero-length records,
    1-3 contigs (two of one name), partners on another contig, mates of different lengths around the wavefront's strides, mapq
    beyond 255 after scaling and NaN, with and without qualities, codes above 3; shared formatter == flat::formatPair ==
    PairedFileWriter; the program fails if a shape never came up"""
    out = run([exe, "random", "20261018", "3000"])
    print(out)
    assert out.startswith("random ok: 3000 pairs x 32 option sets")


def test_long_cigars_and_error_texts_inside_a_pair(exe):
    """65 535 / 65 536 ops in either mate (the CG:B:I tag and its switch), and the two texts of a record that ends beyond its own
    mate, for a bad record in the first and in the second mate: PairedFileWriter's exception == the shared formatter's error
    text == flat::formatPair's exception"""
    assert run([exe, "special"]).startswith("special ok")
