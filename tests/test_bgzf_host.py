"""The rules of the device's BGZF inflate (ma_amd/host/ma_bgzf_dev.h: inflateHost over the routine the kernels of
ma_batch_set_reads_bgzf call) and BatchBgzfReader (ma_amd/host/ma_batch_nodes.h) on the host: tests/emul/bgzf_dev_test.cpp compares
them with zlib (<zlib.h>, the yardstick, which is not the code under test); once as an optimised build, once under
AddressSanitizer + UBSan (a stand-alone program, nothing is preloaded anywhere).  The program writes its BGZF itself."""
import os
import re
import subprocess

import pytest

from ma_testlib import ROOT

SRC = os.path.join(ROOT, "tests", "emul", "bgzf_dev_test.cpp")
FASTQ = os.path.join(ROOT, "tests", "golden", "reader", "small24.fq")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}
KINDS = ("stored", "fixed", "dynamic", "huffman-only", "rle", "blocks")


def build_exe(kind="plain"):
    exe = os.path.join(ROOT, "tests", "emul", "bgzf_dev_test" + ("" if kind == "plain" else "_san"))
    deps = [SRC, os.path.join(ROOT, "include", "ma_amd.h"), os.path.join(ROOT, "ma_amd", "libma_amd.so")] + [
        os.path.join(ROOT, "ma_amd", "host", h) for h in ("ma_bgzf_dev.h", "ma_text_dev.h", "ma_batch_nodes.h", "ma_sam.h", "ma_modules.h",
                                                          "ma_engine.h", "ms_graph.h")]
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


def test_members_of_every_kind_equal_zlib(exe):
    """stored, fixed, dynamic, Huffman-only, RLE and several-block members at 0 1 2 257 258 259 32767 32768 32769 65536 bytes of
    read text, of one repeated byte (distance-1 runs) and of short periods, a hand-made match of length 258 at distance 32768
    and a chain of members with empty ones in front, inside and at the end: ma_bgzf::inflate / inflateHost give zlib's bytes.
    (A stored member of more than 65 510 bytes has no BGZF form -- BSIZE is 16 bits: those three are compared on the deflate
    stream alone.)"""
    out = run([exe, "kinds", "20261020"])
    m = re.match(r"kinds ok: (\d+) streams equal, (\d+) of them also as members", out.splitlines()[-1])
    assert m and int(m.group(1)) == 181 and int(m.group(2)) == 178, out[-2000:]


def test_hand_made_dynamic_headers(exe):
    """a distance set of one code (incomplete: accepted, as zlib does) and of no code, the repeats 16 / 17 / 18 across the
    literal/distance border, the block that is its end code alone, and the unused pattern of a one-code distance set (refused):
    the verdict and the bytes are zlib's"""
    out = run([exe, "handmade"])
    assert out.splitlines()[-1] == "handmade ok: 7 streams, 6 accepted", out[-2000:]


def test_mutants_have_zlibs_verdict(exe):
    """per member kind 300 single-bit flips of the deflate bytes with the trailer left alone (family A: the verdict equals zlib's
    strict decode + CRC + ISIZE) and 300 with the trailer recomputed where zlib still decodes (family B: accepted with zlib's
    bytes, otherwise refused); at least a third of every kind's family B is accepted, so refusing everything does not pass"""
    out = run([exe, "mutants", "20261020", "300"])
    assert out.splitlines()[-1] == "mutants ok: 300 per family and kind, 6 kinds, 0 different", out[-2000:]
    for kind in KINDS:
        m = re.search(r"^%s: A (\d+) of 300 accepted, B (\d+) of 300 accepted$" % kind, out, re.M)
        assert m and 3 * int(m.group(2)) >= 300, out


def test_reasons_name_member_byte_and_reason(exe):
    """one hand-made stream per reason behind a good member: the message is "ma_batch_set_reads_bgzf: member 1 (byte <X>):
    <reason>" with X the size of the good member; plain gzip is named with GzFileStream; of several violations the lowest
    member is named, and a bad header wins over any stream"""
    out = run([exe, "reasons"])
    assert out.splitlines()[-1] == "reasons ok: 19 streams", out[-2000:]
    assert "member 1 (byte 284): a gzip member without the BGZF size field: single-member gzip stays with GzFileStream" in out
    assert len(set(out.splitlines()[:19])) == 19


def test_crc_and_its_fold(exe):
    """crcOf, crcCombine and the 64-lane fold of k_bgzf_crc against zlib's crc32 at 0 1 2 63 64 65 127 4097 65535 65536 bytes"""
    assert run([exe, "crc", "20261020"]).splitlines()[-1] == "crc ok"


@pytest.mark.parametrize("chunk", [1, 64, 1 << 20])
def test_batch_bgzf_reader_cuts_at_record_starts(exe, chunk):
    """BatchBgzfReader over small24.fq and over a generated FASTA whose records are longer than a member, compressed at 1, 7, 300
    and 65280 bytes of text per member (with empty members inside): the batches' texts (head + inflate - drop) concatenate to
    the file and each starts at a record start; a plain gzip stream throws and names GzFileStream, a file that ends inside a
    member throws"""
    out = run([exe, "reader", str(chunk), FASTQ])
    assert out.splitlines()[-1] == "reader ok: chunk %d" % chunk, out[-2000:]
