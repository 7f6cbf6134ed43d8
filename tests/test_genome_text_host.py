"""The rules of the device's genome reader (ma_amd/host/ma_genome_dev.h: ma_genome_dev::parseHost over the functions the kernels of
ma_genome_append_text and the library call) on the host: tests/emul/genome_text_test.cpp compares them with the .ann / .amb / .pac
files the reference wrote for the fixtures of tests/golden/genome/ and with the tree's yardstick, FileReader + the base loop of
buildIndex after srand(seed); once as an optimised build, once under AddressSanitizer + UBSan (a stand-alone program, nothing is
preloaded anywhere)."""
import os
import subprocess

import pytest

from ma_testlib import ROOT

G = os.path.join(ROOT, "tests", "golden", "genome")
SRC = os.path.join(ROOT, "tests", "emul", "genome_text_test.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def build_exe(kind="plain"):
    exe = os.path.join(ROOT, "tests", "emul", "genome_text_test" + ("" if kind == "plain" else "_san"))
    deps = [SRC, os.path.join(ROOT, "include", "ma_amd.h"), os.path.join(ROOT, "ma_amd", "libma_amd.so")] + [
        os.path.join(ROOT, "ma_amd", "host", h) for h in ("ma_genome_dev.h", "ma_text_dev.h", "ma_sam.h", "ma_modules.h", "ms_graph.h")]
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


def test_fixtures_against_the_reference(exe):
    """the three fixtures (multi-line contigs of unequal line lengths, a last line without a line feed, "\\r\\n", lower case, a header
    with a comment, N runs at a contig's start and end with the next contig starting in N, a run across a line end, R and Y
    inside a run of N, a single N): contig names, starts, lengths and holes per contig == .ann, the holes == .amb, the 2-bit bases
    outside the holes == .pac; and everything, the fill of seeds 1 and 20261021 included, == the yardstick"""
    assert run([exe, "golden", G]).startswith("golden ok: 3 fixtures")


def test_random_genomes_against_the_yardstick(exe):
    """300 seeded strict genomes (1-6 contigs of 1-4 000 bases, hole bases in runs at 0-30 %, random line lengths, both line ends):
    all accepted; codes after the fill, the contig table, vHoles and vNumHoles == FileReader + packContigs after srand(seed)"""
    assert run([exe, "random", "20261021", "300"]).startswith("random ok: 300 genomes")


def test_cuts(exe):
    """every fixture appended as two chunks with the cut behind every line end, one line per chunk, and with a tail that has no line
    feed (consumed stops at the last line feed; a chunk without any consumes 0): == the one-piece result"""
    assert run([exe, "cuts", G]).startswith("cuts ok: ")


def test_refusals(exe):
    """one text per reason of the strict form and the '@' text; the violations in a second chunk name line and byte counted over
    both chunks; a refused chunk leaves the state unchanged and the corrected chunk gives the one-piece result; capacity; the
    refusals of ma_genome_build_index; the generator == libc's rand() after srand(seed)"""
    assert run([exe, "refusals"]).startswith("refusals ok: ")
