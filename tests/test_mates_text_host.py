"""The rules of ma_batch_set_mates_text (ma_amd/host/ma_text_dev.h: ma_text::pairHost, parseHost on each of two texts + interleave +
reverse complement) and BatchPairedTextReader (ma_amd/host/ma_batch_nodes.h) on the host: tests/emul/mates_text_test.cpp compares
them with PairedFileReader of ma_amd/host/ma_sam.h and with the reference's own reader output (tests/golden/reader/mates.*); once
as an optimised build, once under AddressSanitizer + UBSan (a stand-alone program, nothing is preloaded anywhere)."""
import os
import re
import subprocess

import pytest

from ma_testlib import ROOT

G = os.path.join(ROOT, "tests", "golden", "reader")
SRC = os.path.join(ROOT, "tests", "emul", "mates_text_test.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def build_exe(kind="plain"):
    exe = os.path.join(ROOT, "tests", "emul", "mates_text_test" + ("" if kind == "plain" else "_san"))
    deps = [SRC, os.path.join(ROOT, "include", "ma_amd.h"), os.path.join(ROOT, "ma_amd", "libma_amd.so")] + [
        os.path.join(ROOT, "ma_amd", "host", h) for h in ("ma_text_dev.h", "ma_batch_nodes.h", "ma_sam.h", "ma_modules.h", "ma_engine.h",
                                                          "ms_graph.h")]
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


def test_golden_mates_equal_the_references_reader(exe):
    """pairHost on mates_1.fq / mates_2.fq with rev_comp 0 and 1 equals mates.rc0.ref / mates.rc1.ref, the reference's own
    PairedFileReader output: the shorter file ends the stream, TTGACCNA becomes 35223100, the qualities are reversed"""
    assert run([exe, "golden", G]).splitlines()[-1] == "golden ok: 8 reads equal"


def test_generated_pairs_equal_the_paired_file_reader(exe):
    """400 seeded strict text pairs (FASTQ and FASTA of one to several lines, both line ends, with and without the final one, N,
    IUPAC and lower-case letters, a junk byte inside, 0-12 records, one text up to three records longer in either direction), each
    with rev_comp 0 and 1: pairHost equals PairedFileReader over in-memory streams; consumed cuts each text behind its last
    paired record"""
    out = run([exe, "random", "20261020", "400"])
    m = re.match(r"random ok: 400 text pairs, (\d+) of unequal counts, (\d+) reads equal", out.splitlines()[-1])
    assert m and int(m.group(1)) >= 200 and int(m.group(2)) >= 4000, out[-2000:]


def test_refusals_wording_and_precedence(exe):
    """a violation in text 1, in text 2, in both (text 1 is named), in a record beyond the pairs, beside an empty text; a text of
    neither kind on either side; FASTQ against FASTA, which a violation wins over: the message is messageMates's, and a refusal
    reports no pairs and no consumed bytes"""
    assert run([exe, "reasons"]).startswith("reasons ok: 12 text pairs")
    table = run([exe, "reasons", "print"]).splitlines()
    assert len(table) == 12 and all(l.split(" ", 2)[2].startswith("ma_batch_set_mates_text: ") for l in table)


@pytest.mark.parametrize("batch_bytes", [64, 257, 4096])
def test_batch_paired_text_reader_cuts_whole_pairs(exe, batch_bytes):
    """BatchPairedTextReader over in-memory streams of 0, 1, 2, 37 and 1 000 pairs of unequal read lengths, FASTQ and FASTA, with
    equal counts and with either file three records longer: every batch holds equally many records in both texts and is consumed
    entirely, the batches concatenate to each input up to the shorter file's record count, the stream ends where the shorter file
    ends, the reads are PairedFileReader's; a stream without block reads throws BatchTextReader's message"""
    out = run([exe, "reader", str(batch_bytes)])
    assert out.splitlines()[-1] == "reader ok: 30 runs, batches of %d bytes" % batch_bytes, out
