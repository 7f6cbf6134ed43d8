"""The rules of the device's BGZF deflate (ma_amd/host/ma_deflate_dev.h: deflateHost over the routines the kernels of
ma_sam_bgzf_batch call) on the host: tests/emul/sam_bgzf_test.cpp compares them with zlib (<zlib.h>, the yardstick, which is never
the code under test: it inflates what deflateHost wrote and gives the sizes to compare with); once as an optimised build, once
under AddressSanitizer + UBSan (a stand-alone program, nothing is preloaded anywhere)."""
import glob
import os
import re
import subprocess

import pytest

from ma_testlib import ROOT

SRC = os.path.join(ROOT, "tests", "emul", "sam_bgzf_test.cpp")
G = os.path.join(ROOT, "tests", "golden")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def build_exe(kind="plain"):
    exe = os.path.join(ROOT, "tests", "emul", "sam_bgzf_test" + ("" if kind == "plain" else "_san"))
    deps = [SRC, os.path.join(ROOT, "tests", "emul", "sam_dev_common.h"), os.path.join(ROOT, "include", "ma_amd.h"),
            os.path.join(ROOT, "oracle", "dump_format.h"), os.path.join(ROOT, "ma_amd", "libma_amd.so")] + [
        os.path.join(ROOT, "ma_amd", "host", h) for h in os.listdir(os.path.join(ROOT, "ma_amd", "host")) if h.endswith(".h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall"] + BUILDS[kind] + ["-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "ma_amd", "host"), SRC, "-o", exe, "-L" + os.path.join(ROOT, "ma_amd"),
                               "-lma_amd", "-Wl,-rpath," + os.path.join(ROOT, "ma_amd"), "-lpthread", "-lz"])
    return exe


def run(args):
    # (the HIP runtime the library links against keeps allocations of its own until the process ends)
    return subprocess.check_output(args, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0")).decode()


def golden_sams():
    return sorted(glob.glob(os.path.join(G, "**", "*.sam.gz"), recursive=True))


@pytest.fixture(scope="module", params=list(BUILDS))
def exe(request):
    return build_exe(request.param)


def test_round_trip_of_the_length_and_content_grid(exe):
    """0 1 2 3 4 5 257 258 259 65279 65280 65281 130560 130561 bytes of one repeated byte, of periods 2 3 4 5 64, of random bytes
    (stored), of two byte values and of all 256 in turn; a block repeated at distance 32768 and 32769; matches across a member's
    end; 22 symbols with Fibonacci counts (an unlimited Huffman tree is deeper than 15); a repeated 200-byte line (under a
    tenth): every member has the exact header, BSIZE, CRC32 and ISIZE, is at most its text + 31 bytes, there are ceil(n / 65280)
    of them, zlib's strict inflate and ma_bgzf::inflateHost over the chain with the end-of-file marker give the text, and two
    runs give the same bytes"""
    out = run([exe, "roundtrip", "20261020"])
    assert out.splitlines()[-1] == "roundtrip ok: 135 texts", out[-2000:]


def test_code_lengths_are_complete_and_limited(exe):
    """random, power-of-two, flat and Fibonacci histograms over the three alphabets: every code is complete (Kraft sum 1), within
    15 bits (7 for the code-length code), and a rarer symbol never has the shorter code"""
    out = run([exe, "codes", "20261020", "30000"])
    assert re.match(r"codes ok: 30000 histograms, \d+ at the limit$", out.splitlines()[-1]), out[-2000:]


def test_golden_sam_texts_round_trip_and_ratio(exe):
    """the record lines of every tests/golden/**/*.sam.gz round-trip; against zlib on the same 65 280-byte chunks
    (deflateInit2(level, Z_DEFLATED, -15, 9, strategy) + 26 bytes of frame per chunk) the members are smaller than Z_FIXED and
    than Z_HUFFMAN_ONLY at level 1 on small24.fq.sam.gz and small_ref.illumina.opt4.sam.gz, and over all sixteen texts
    together at most zlib level 1's"""
    files = golden_sams()
    assert len(files) == 16
    out = run([exe, "golden"] + files)
    print(out)
    rows = {}
    for line in out.splitlines():
        m = re.match(r"(\S+) text (\d+) ours (\d+) fixed1 (\d+) huffman (\d+) level1 (\d+) level6 (\d+)$", line)
        if m:
            rows[os.path.relpath(m.group(1), G)] = [int(x) for x in m.groups()[1:]]
    assert len(rows) == 16
    for name in (os.path.join("reader", "small24.fq.sam.gz"), "small_ref.illumina.opt4.sam.gz"):
        text, ours, fixed1, huffman, level1, level6 = rows[name]
        assert ours < fixed1 and ours < huffman, (name, rows[name])
    m = re.match(r"golden ok: 16 files text (\d+) ours (\d+) fixed1 (\d+) huffman (\d+) level1 (\d+) level6 (\d+)$", out.splitlines()[-1])
    assert m, out[-2000:]
    assert int(m.group(2)) == sum(r[1] for r in rows.values()) and int(m.group(5)) == sum(r[4] for r in rows.values())
    assert int(m.group(2)) <= int(m.group(5)), out.splitlines()[-1]


def test_deflate_mode_is_deterministic_and_gzip_reads_it(exe, tmp_path):
    """`deflate <in> <out>` twice: the same bytes; with the end-of-file marker Python's gzip reads the text back"""
    import gzip
    text = gzip.open(os.path.join(G, "small_ref.illumina.opt4.sam.gz"), "rb").read() * 2
    src = str(tmp_path / "in")
    open(src, "wb").write(text)
    outs = []
    for k in (0, 1):
        assert run([exe, "deflate", src, str(tmp_path / ("out%d" % k))]).startswith("deflate ok: %d members, " % ((len(text) + 65279) // 65280))
        outs.append(open(str(tmp_path / ("out%d" % k)), "rb").read())
    assert outs[0] == outs[1] and len(outs[0]) < len(text) // 2
    end = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0\x1b\0\x03\0\0\0\0\0\0\0\0\0"
    assert gzip.decompress(outs[0] + end) == text


def test_host_writers_write_bgzf_from_the_first_byte(exe, tmp_path):
    """BatchFileWriter (flat formatter under options 0 and soft clip + =/X, two batches; with the NGMLR tags its per-read
    writer), two FileWriters on one stream, and BatchPairedFileWriter over the flat records of the reference's pipeline dumps
    (small_ref.default.pipe, the f4 dump), with SamOptions::bBgzf: gzip-decompressing the stream gives byte for byte what the
    same writers give without the option, header included; every byte is inside a BGZF member, and the stream ends with the
    28-byte end-of-file marker, which is there once; members onto a plain stream are refused"""
    import gzip
    from ma_testlib import gunzip_to
    from test_sam_pair_dev_host import PAIR_GOLDEN
    case = gunzip_to(os.path.join(G, "small.case.gz"), str(tmp_path / "small.case"))
    pipe = gunzip_to(os.path.join(G, "small_ref.default.pipe.gz"), str(tmp_path / "p.pipe"))
    f4case = gunzip_to(os.path.join(G, "f4.case.gz"), str(tmp_path / "f4.case"))
    f4dump = gunzip_to(os.path.join(G, PAIR_GOLDEN + ".f4.gz"), str(tmp_path / "ref.f4"))
    out = str(tmp_path / "w")
    assert run([exe, "writers", case, pipe, f4case, f4dump, out]).startswith("writers ok: 128 reads, ")
    end = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0\x1b\0\x03\0\0\0\0\0\0\0\0\0"
    golden = {"batch0": "small_ref.default.opt0.sam.gz", "batch3": "small_ref.default.opt3.sam.gz", "batch32": "small_ref.default.opt4.sam.gz",
              "pairs": PAIR_GOLDEN + ".sam.gz"}
    for name in ("batch0", "batch3", "batch32", "perread", "pairs"):
        plain, packed = open("%s.%s.sam" % (out, name), "rb").read(), open("%s.%s.sam.gz" % (out, name), "rb").read()
        assert plain.startswith(b"@SQ\tSN:") and plain.count(b"\n") > 100
        assert gzip.decompress(packed) == plain, name
        assert packed.endswith(end) and packed.count(end) == 1, name
        # the stream is a chain of BGZF members and nothing else
        at, members = 0, 0
        while at < len(packed):
            assert packed[at:at + 16] == end[:16], (name, at)
            at += int.from_bytes(packed[at + 16:at + 18], "little") + 1
            members += 1
        assert at == len(packed) and members >= 2
        if name in golden:  # (what the writers write is pinned elsewhere; here only that the records are the reference's)
            want = [l for l in gzip.open(os.path.join(G, golden[name]), "rb").read().splitlines(True) if not l.startswith(b"@")]
            got = [l for l in plain.splitlines(True) if not l.startswith(b"@")]
            assert got == want * (2 if name.startswith("batch") else 1), name
