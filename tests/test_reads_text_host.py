"""The rules of the device's FASTQ / FASTA parser (ma_amd/host/ma_text_dev.h: parseHost over the per-line functions the kernels
of ma_batch_set_reads_text call) and BatchTextReader (ma_amd/host/ma_batch_nodes.h) on the host: tests/emul/text_dev_test.cpp
compares them with FileReader::parseRecord of ma_amd/host/ma_sam.h (the yardstick, which test_sam_writer.py pins to the reference's
reader goldens); once as an optimised build, once under AddressSanitizer + UBSan (a stand-alone program, nothing is preloaded
anywhere)."""
import os
import re
import subprocess

import pytest

from ma_testlib import ROOT

G = os.path.join(ROOT, "tests", "golden", "reader")
SRC = os.path.join(ROOT, "tests", "emul", "text_dev_test.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def build_exe(kind="plain"):
    exe = os.path.join(ROOT, "tests", "emul", "text_dev_test" + ("" if kind == "plain" else "_san"))
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


def test_golden_reader_fixtures(exe):
    """small24.fq, mates_1.fq, mates_2.fq and reader_plusname.fq are accepted and equal the yardstick and the reference's .ref
    dumps; reader_multi.fq, reader_multi.fa, reader_empty.fa and reader_notfasta.txt are refused, each naming a line"""
    out = run([exe, "golden", G])
    assert out.splitlines()[-1] == "golden ok: 30 reads of 4 files equal, 4 files refused"
    assert "reader_multi.fq: ma_batch_set_reads_text: line 3 (byte 15): " in out
    assert "reader_notfasta.txt: ma_batch_set_reads_text: line 1 (byte 0): " in out


def test_strict_texts_are_accepted_and_equal(exe):
    """1 900 seeded strict texts (1-12 records, both line ends, with and without the final one, descriptions behind a blank or a
    tab, IUPAC and lower-case letters, a lower-case first letter, junk inside and behind the bases, qualities that start with
    @ + > or a blank and end with a blank, +name lines, FASTA records of 1-4 lines, lengths 1 63 64 65 255 256 257 and 70 000):
    none refused -- "refuse everything" does not pass --, names, codes and qualities equal to the yardstick's"""
    out = run([exe, "strict", "20261019", "1900"])
    m = re.match(r"strict ok: 1900 texts, (\d+) reads equal, 0 refused", out.splitlines()[-1])
    assert m and int(m.group(1)) >= 1900, out[-2000:]


def test_mutants_are_refused_or_equal(exe):
    """three mutants per strict text (1-3 replacements, insertions or deletions of \\n \\r blank @ > + A x): each is refused or
    parses to what the yardstick parses (an exception of the yardstick: must be refused); at least a fifth are accepted, so
    the comparison is not empty"""
    out = run([exe, "mutants", "20261019", "1900"])
    m = re.match(r"mutants ok: (\d+) accepted, (\d+) refused, 0 different", out.splitlines()[-1])
    assert m, out[-2000:]
    accepted, refused = int(m.group(1)), int(m.group(2))
    assert accepted + refused == 5700 and 5 * accepted >= 5700


def test_reasons_name_line_byte_and_reason(exe):
    """one hand-made text per reason: lone \\r, \\r as the last byte, three lines, + line missing, quality one byte short / long,
    junk-only sequence, sequence starting with @, FASTA header behind header, blank-led line, first byte A, ...: the message is
    "ma_batch_set_reads_text: line <L> (byte <X>): <reason>" with the expected line, offset and reason; of two violations the
    lower line is named"""
    assert run([exe, "reasons"]).startswith("reasons ok: 16 texts")


@pytest.mark.parametrize("block", [1, 7, 64, 1 << 20])
def test_batch_text_reader_cuts_at_record_starts(exe, block):
    """BatchTextReader over a StdFileStream and a StringStream (small24.fq) and over a generated FASTA: the batches concatenate
    to the file, each starts at a record start, their parses concatenate to the yardstick's reads; a block read behind a line read
    goes on where that stopped; a stream without block reads throws and names BatchFileReader"""
    out = run([exe, "cut", str(block), os.path.join(G, "small24.fq")])
    assert out.splitlines()[-1] == "cut ok: block %d" % block, out
