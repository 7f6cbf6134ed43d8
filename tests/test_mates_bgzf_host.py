"""The rules of ma_batch_set_mates_bgzf (ma_amd/host/ma_mates_bgzf_dev.h: ma_bgzf::pairBgzfHost, inflateHost per side + head and
drop + ma_text::pairHost + the order of the refusals) on the host: tests/emul/mates_bgzf_test.cpp compares it with zlib (which writes
the members: the yardstick, not the code under test), with pairHost on the uncompressed texts, with PairedFileReader of
ma_amd/host/ma_sam.h and with the reference's own reader output (tests/golden/reader/mates.*); once as an optimised build, once
under AddressSanitizer + UBSan (a stand-alone program, nothing is preloaded anywhere)."""
import os
import re
import subprocess

import pytest

from ma_testlib import ROOT

G = os.path.join(ROOT, "tests", "golden", "reader")
SRC = os.path.join(ROOT, "tests", "emul", "mates_bgzf_test.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def build_exe(kind="plain"):
    exe = os.path.join(ROOT, "tests", "emul", "mates_bgzf_test" + ("" if kind == "plain" else "_san"))
    deps = [SRC, os.path.join(ROOT, "include", "ma_amd.h"), os.path.join(ROOT, "ma_amd", "libma_amd.so")] + [
        os.path.join(ROOT, "ma_amd", "host", h) for h in ("ma_mates_bgzf_dev.h", "ma_bgzf_dev.h", "ma_text_dev.h", "ma_batch_nodes.h", "ma_sam.h",
                                                          "ma_modules.h", "ma_engine.h", "ms_graph.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall"] + BUILDS[kind] + ["-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "ma_amd", "host"), SRC, "-o", exe, "-L" + os.path.join(ROOT, "ma_amd"),
                               "-lma_amd", "-Wl,-rpath," + os.path.join(ROOT, "ma_amd"), "-lpthread", "-lz"])
    return exe


def run(args):
    # (the HIP runtime the library links against keeps allocations of its own until the process ends)
    return subprocess.check_output(args, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0")).decode()


@pytest.fixture(scope="module", params=list(BUILDS))
def exe(request):
    return build_exe(request.param)


def test_golden_mates_equal_the_references_reader(exe):
    """mates_1.fq / mates_2.fq deflated with zlib into members of 40 text bytes (every kind in turn), rev_comp 0 and 1: pairBgzfHost
    equals mates.rc0.ref / mates.rc1.ref, the reference's own PairedFileReader output, and the texts it pairs are the files"""
    assert run([exe, "golden", G]).splitlines()[-1] == "golden ok: 8 reads equal"


def test_generated_pairs_equal_the_text_statement(exe):
    """200 seeded text pairs (FASTQ and FASTA, both line ends, 0-12 records, either text up to three records longer), each cut
    into members at random offsets -- mid-line, between \\r and \\n, empty members -- behind a random head (nothing .. a few
    records, also ending mid-line) and with a random drop (none, inside the last member, across two members), rev_comp 0 and 1:
    pairBgzfHost equals pairHost on (T_1, T_2) and PairedFileReader -- reads, sums, consumed -- and its texts are T_1 and T_2, so
    the rest is T_i[consumed_i ..); at least 80 of the 200 have unequal counts"""
    out = run([exe, "random", "20261020", "200"])
    m = re.match(r"random ok: 200 text pairs, (\d+) of unequal counts, (\d+) rests, (\d+) reads equal", out.splitlines()[-1])
    assert m and int(m.group(1)) >= 80 and int(m.group(2)) >= 80 and int(m.group(3)) >= 2000, out[-2000:]


@pytest.mark.parametrize("target", [2000, 4096, 65536])
def test_batch_paired_bgzf_reader(exe, target):
    """BatchPairedBgzfReader over in-memory BGZF streams (members of 700 text bytes + the end-of-file marker) of 0, 1, 2, 37 and
    1 000 pairs, records of 150 / 150, 150 / 450 and 450 / 150 bytes, equal counts or either file three records longer, the rests
    computed by pairBgzfHost and handed back: the pairs of all batches are PairedFileReader's over the uncompressed texts, the
    stream ends where the shorter file ends, the carried head of either stream never exceeds target / 2 + 2 x 700 + the longest
    record, and the peak for 1 000 pairs of 150 / 450 is not exceeded with 4 000; a batch destroyed without hand-back makes a
    second thread that waits in execute( ) and the next call throw (joined with a timeout); a plain-gzip stream throws
    BatchBgzfReader's message"""
    out = run([exe, "reader", str(target)])
    assert out.splitlines()[-1] == "reader ok: 47 runs, target %d bytes" % target, out[-2000:]


def test_refusals_wording_and_precedence(exe):
    """one case per row of the refusal table -- member (a bad header, a CRC mismatch), drop, line, kind, on either side -- and the
    precedence: a bad header in text 2 wins over a CRC mismatch in text 1 and names text 2, a CRC mismatch in text 2 wins over a
    line violation and over a drop too large in text 1, a drop wins over a line, violations of one class in both texts name
    text 1, a violation in a record beyond the pairs refuses; a refusal reports no pairs, no consumed bytes and no text bytes"""
    assert run([exe, "reasons"]).startswith("reasons ok: 20 cases")
    table = run([exe, "reasons", "print"]).splitlines()
    assert len(table) == 20 and all(l.split(" ", 2)[2].startswith("ma_batch_set_mates_bgzf: ") for l in table)
    assert sum(": member " in l for l in table) == 9 and sum("n_drop" in l for l in table) == 3
