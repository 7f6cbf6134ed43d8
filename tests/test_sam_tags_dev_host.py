"""The NGMLR tag emulation of the record formatter the device stage runs (ma_amd/host/ma_sam_dev.h, MA_SAM_NGMLR_TAGS) on the
host: tests/emul/sam_tags_dev_test.cpp compares it, byte for byte, with ma_amd's FileWriter under bEmulateNgmlrTags
(ma_amd/host/ma_sam.h) and with the SAM text the reference's FileWriter printed (tests/golden/small_ref.*.opt4 / opt5.sam.gz);
once as an optimised build, once under AddressSanitizer + UBSan (a stand-alone program, nothing is preloaded anywhere)."""
import os
import subprocess

import pytest

from ma_testlib import ROOT, gunzip_to

G = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(ROOT, "tests", "emul", "sam_tags_dev_test.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def build_exe(kind="plain"):
    exe = os.path.join(ROOT, "tests", "emul", "sam_tags_dev_test" + ("" if kind == "plain" else "_san"))
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


@pytest.mark.parametrize("preset,opt,bits", [("default", 4, 32), ("default", 5, 33), ("illumina", 4, 32)])
def test_golden_records_with_tags(tmp_path, exe, preset, opt, bits):
    """the MappingQuality records of the reference's pipeline dump with MA_SAM_NGMLR_TAGS (and soft clipping): shared formatter ==
    FileWriter with bEmulateNgmlrTags == the record lines of the golden the reference wrote with the option on"""
    case = gunzip_to(os.path.join(G, "small.case.gz"), str(tmp_path / "small.case"))
    pipe = gunzip_to(os.path.join(G, "small_ref.%s.pipe.gz" % preset), str(tmp_path / "p.pipe"))
    sam = gunzip_to(os.path.join(G, "small_ref.%s.opt%d.sam.gz" % (preset, opt)), str(tmp_path / "g.sam"))
    assert run([exe, "golden", case, pipe, sam, str(bits)]).startswith("golden ok: 128 reads")


def test_random_record_lists_with_tags(exe):
    """3000 seeded random lists over a two-contig genome with four holes, and the deterministic cases (the I/D runs on both
    strands, sister lists, records without reference or query bases, 0x10000 ops, begin_ref 10, records around holes), under
    the 32 option sets with the tag bit against FileWriter; the program asserts its census (every I/D run on the reverse
    strand, a swapped sister before and an unswapped one behind a record, deletion then mismatch, long mismatch sections,
    SV 0 - 3, begin_ref < 100, holes under matches, sisters of op length 0, secondary sisters, the CG tag and its switch, 0 / 0)
    and the three error kinds"""
    out = run([exe, "random", "20261019", "3000"])
    assert out.startswith("random ok: 3000 lists x 32 option sets")


def test_percent_f_formatter(exe):
    """the formatter of XI:f / CV:f == snprintf( "%f", (double)f ) for all a / b and 100 a / b with b <= 4096, a <= b, for 10 M
    seeded random floats of [0, 128) (subnormals among them), and the ratios == std::to_string of the host's arithmetic"""
    assert run([exe, "floats", "20261019", "10000000"]).startswith("floats ok: ")
