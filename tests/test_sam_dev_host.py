"""The record formatter the device stage runs (ma_amd/host/ma_sam_dev.h) on the host: tests/emul/sam_dev_test.cpp compares it,
byte for byte, with flat::formatRead (ma_amd/host/ma_flat_sam.h) and with the SAM text the reference's FileWriter printed
(tests/golden/small_ref.*.sam.gz); once as an optimised build, once under AddressSanitizer + UBSan (a stand-alone program)."""
import os
import subprocess

import pytest

from ma_testlib import ROOT, gunzip_to

G = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(ROOT, "tests", "emul", "sam_dev_test.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def build_exe(kind="plain"):
    exe = os.path.join(ROOT, "tests", "emul", "sam_dev_test" + ("" if kind == "plain" else "_san"))
    deps = [SRC, os.path.join(ROOT, "include", "ma_amd.h"), os.path.join(ROOT, "oracle", "dump_format.h")] + [
        os.path.join(ROOT, "ma_amd", "host", h) for h in ("ma_sam_dev.h", "ma_flat_sam.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall"] + BUILDS[kind] + ["-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "ma_amd", "host"), SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module", params=list(BUILDS))
def exe(request):
    return build_exe(request.param)


@pytest.mark.parametrize("preset,opt", [("default", 0), ("default", 1), ("default", 2), ("default", 3), ("illumina", 0)])
def test_golden_records(tmp_path, exe, preset, opt):
    """the MappingQuality records of the reference's pipeline dump: shared formatter == flat::formatRead == the golden's record
    lines; the counting sink returns exactly the bytes written"""
    case = gunzip_to(os.path.join(G, "small.case.gz"), str(tmp_path / "small.case"))
    pipe = gunzip_to(os.path.join(G, "small_ref.%s.pipe.gz" % preset), str(tmp_path / "p.pipe"))
    sam = gunzip_to(os.path.join(G, "small_ref.%s.opt%d.sam.gz" % (preset, opt)), str(tmp_path / "g.sam"))
    out = subprocess.check_output([exe, "golden", case, pipe, sam, str(opt)]).decode()
    assert out.startswith("golden ok: 128 reads")


def test_random_record_lists(exe):
    """3000 seeded random lists under all 32 option sets: both strands, 1-3 contigs (two of one name), numbers on both sides of
    every decimal boundary up to 10^9, the read lengths around the wavefront's strides, codes above 3, with and without
    qualities, names of 1-40 bytes, empty lists and lists of zero-length alignments only"""
    out = subprocess.check_output([exe, "random", "20261018", "3000"]).decode()
    assert out.startswith("random ok: 3000 lists x 32 option sets")


def test_long_cigars_and_error_texts(exe):
    """65 535 / 65 536 ops (the CG:B:I tag and its switch), and the two texts of a record that ends beyond its read"""
    assert subprocess.check_output([exe, "special"]).decode().startswith("special ok")
