"""ma_batch_set_mates_bgzf / ma_batch_get_mates_rest: the two BGZF-compressed read files of a paired-end run inflated by ONE launch of
the inflate kernels (ma_amd/csrc/launch_mates_bgzf.h, stage_bgzf.h) and paired by the kernels of ma_batch_set_mates_text, through
the C ABI / ma_amd.api.  The yardsticks: set_mates_text on the uncompressed texts (Python's zlib writes the members: it is not the
code under test), and for the refusals ma_bgzf::pairBgzfHost (ma_amd/host/ma_mates_bgzf_dev.h, run by tests/emul/mates_bgzf_test.cpp,
which tests/test_mates_bgzf_host.py pins to zlib, pairHost and PairedFileReader)."""
import gzip
import subprocess
import zlib

import numpy as np
import pytest

from ma_testlib import rand_genome, sample_pairs
from test_gpu_bgzf import END, KINDS, deflate, last_record_start, member, split, wrap
from test_gpu_mates_text import mates, params, small  # noqa: F401 (small: a fixture)
from test_gpu_reads_text import MIXED
from test_mates_bgzf_host import build_exe

pytestmark = pytest.mark.gpu
ZERO = dict(reads=0, bases=0, name_bytes=0, has_qual=0)


def chain(text, m, first_kind=0):
    """text as exactly m members: one, or m - 2 pieces of every kind in turn with an empty member in the middle and at the end"""
    if m < 3:
        return split(text, [len(text) * i // m for i in range(1, m)], empty=False)
    k = m - 2
    edges = [len(text) * i // k for i in range(k + 1)]
    out = [member(text[a:b], (first_kind + i) % len(KINDS)) for i, (a, b) in enumerate(zip(edges, edges[1:]))]
    out.insert(len(out) // 2, END)
    return out + [END]


def state(b):
    off, codes = b.reads()
    names, quals = b.read_text()
    return b.read_counts(), off.tobytes(), codes.tobytes(), names, quals


@pytest.fixture(scope="module")
def batches(small):
    """(the batch under test, the batch of the text call, that call's results by texts)"""
    import ma_amd
    b, t = ma_amd.Batch(small[0], params(), 4096, 400000), ma_amd.Batch(small[0], params(), 4096, 400000)
    yield b, t, {}
    b.close()
    t.close()


@pytest.fixture(scope="module")
def texts():
    rng = np.random.default_rng(20261020)
    lens = lambda n: [int(x) for x in rng.integers(20, 120, size=n)]
    out = dict(fastq=(mates(rng, True, lens(200), 1, "\r\n"), mates(rng, True, lens(203), 2, "\r\n")),
               fasta=(mates(rng, False, lens(200), 1), mates(rng, False, lens(203), 2)))
    assert all(len(t) <= 65536 for p in out.values() for t in p)
    return out


def same_as_text(batches, t1, t2, rev, members1, members2, heads=(b"", b""), drops=(0, 0)):
    """after set_mates_bgzf the batch is as after set_mates_text on (t1, t2), and the rests are what lies behind consumed"""
    b, t, cache = batches
    if (t1, t2, rev) not in cache:
        cache[(t1, t2, rev)] = (t.set_mates_text(t1, t2, rev), state(t))
    (n_pairs, consumed), want = cache[(t1, t2, rev)]
    assert b.set_mates_bgzf(b"".join(members1), b"".join(members2), heads, drops, rev) == (n_pairs, consumed, (len(t1), len(t2)))
    assert state(b) == want
    assert b.mates_rest() == (t1[consumed[0]:], t2[consumed[1]:])
    return n_pairs


@pytest.mark.parametrize("name", ["fastq", "fasta"])
def test_parity_with_the_text_call(batches, texts, name):
    """two FASTQ texts with \\r\\n ends / two FASTA texts of 200 and 203 records as (m1, m2) members, which put the border between
    the two chains in the joint table at lane 1, 63 and 64 of a wavefront and beyond one workgroup; every kind in turn, an empty
    member in the middle and at the end of a side of three or more: n_pairs, consumed, read_counts(), reads() and read_text() equal
    those after set_mates_text on the same texts for rev_comp 0 and 1, text_bytes are the texts' sizes, and mates_rest() is
    (T1[c1:], T2[c2:]) -- three records of text 2"""
    t1, t2 = texts[name]
    for m1, m2 in ((1, 1), (63, 1), (64, 1), (1, 64), (65, 64), (129, 3)):
        for rev in (0, 1):
            assert same_as_text(batches, t1, t2, rev, chain(t1, m1), chain(t2, m2, 3)) == 200
    b = batches[0]
    assert b.mates_rest()[0] == b"" and b.mates_rest()[1].count(b">" if name == "fasta" else b"\n+\r\n") == 3
    assert same_as_text(batches, t2, t1, 1, chain(t2, 5), chain(t1, 7)) == 200  # (the longer text first)


def test_head_and_drop_per_side(batches, texts, small):
    """the shapes of the single-end call's head-and-drop test -- head empty / ending mid-line / nearly everything, drop 0 / inside
    the last member / the whole last member / across two members, a side that is its head alone (no members, and only an empty
    member), a side with nothing -- on side 1 only, on side 2 only and on both; a side with nothing gives 0 pairs, the other is
    still validated, and align() behaves as on an empty batch"""
    import ma_amd
    b = batches[0]
    t1, t2 = texts["fastq"]

    def shapes(text):
        extra = text[7:1507]
        out = []
        for cut in (0, 100, len(text) - 1):
            for drop in (0, 350, 600, 1050):  # the last member holds 600 bytes, the one before it 900
                whole = text[cut:] + extra[:drop]
                out.append((split(whole, [len(whole) - 1500, len(whole) - 600], empty=False), text[:cut], drop))
        return out + [([], text, 0), ([END], text, 0)]

    plain1, plain2 = ([member(t1)], b"", 0), ([member(t2)], b"", 0)
    s1, s2 = shapes(t1), shapes(t2)
    for x, y in [(x, plain2) for x in s1] + [(plain1, y) for y in s2] + list(zip(s1, s2[::-1])):
        assert same_as_text(batches, t1, t2, 1, x[0], y[0], (x[1], y[1]), (x[2], y[2])) == 200
    empty = ma_amd.Batch(small[0], params(), 16, 1024)
    empty.set_reads([])
    empty.align()
    for x, y, a, c in ((([], b"", 0), plain2, b"", t2), (plain1, ([END], b"", 0), t1, b""), (([member(t1)], b"", len(t1)), ([], b"", 0), b"", b"")):
        assert same_as_text(batches, a, c, 1, x[0], y[0], (x[1], y[1]), (x[2], y[2])) == 0
        assert b.read_counts() == ZERO and b.read_text() == ([], None)
        b.align()
        assert b.counts() == empty.counts() and b.counts()["alignments"] == 0
    # the other text is still validated
    broken = t2.replace(b"\n+\r\n", b"\n-\r\n", 1)
    with pytest.raises(ma_amd.MaError, match=r"ma_batch_set_mates_bgzf: text 2: line 3 \(byte \d+\): the third line of a FASTQ record"):
        b.set_mates_bgzf(b"", member(broken))
    empty.close()


def test_a_streamed_pair_of_files_in_three_calls(batches):
    """two FASTQ files of 240 records, R1's about twice as long as R2's, as 700-byte members, streamed in three calls as a reader
    cuts them: per stream the members up to the one that holds its last record start, drop = that member's bytes behind it; the
    next call's head is the device's rest of that stream followed by the dropped bytes.  Every call but the last leaves a rest;
    names, qualities and codes of the three calls are those of one set_mates_text on the whole texts"""
    b, t, _ = batches
    rng = np.random.default_rng(7)
    files = (mates(rng, True, [int(x) for x in rng.integers(180, 220, size=240)], 1), mates(rng, True, [int(x) for x in rng.integers(90, 110, size=240)], 2))
    assert t.set_mates_text(files[0], files[1], 1)[0] == 240
    want = state(t)
    parts = [[f[a:a + 700] for a in range(0, len(f), 700)] for f in files]
    sent, heads, carried = [0, 0], [b"", b""], [[], []]
    names, quals, codes, rests = [], [], [], []
    for r in range(3):
        sides, after = [], []
        for i in range(2):
            upto = len(parts[i]) * ((1, 2, 3)[r] if i == 0 else (2, 4, 5)[r]) // (3, 5)[i]  # (stream 2 runs ahead: its records are left over)
            chunk = carried[i] + parts[i][sent[i]:upto]
            sent[i] = upto
            whole = heads[i] + b"".join(chunk)
            cut = last_record_start(whole) if r < 2 else len(whole)
            assert cut > len(heads[i])
            size, m = len(heads[i]), 0
            while size + len(chunk[m]) < cut:
                size += len(chunk[m])
                m += 1
            drop = size + len(chunk[m]) - cut
            sides.append((b"".join(member(p, (r + k) % len(KINDS)) for k, p in enumerate(chunk[:m + 1])), heads[i], drop))
            after.append((whole[cut:cut + drop], chunk[m + 1:], whole[:cut]))
        n, consumed, size = b.set_mates_bgzf(sides[0][0], sides[1][0], (sides[0][1], sides[1][1]), (sides[0][2], sides[1][2]), 1)
        rest = b.mates_rest()
        assert n > 0 and size == (len(after[0][2]), len(after[1][2])) and rest == (after[0][2][consumed[0]:], after[1][2][consumed[1]:])
        rests.append(rest)
        s = state(b)
        names += s[3]
        quals += s[4]
        codes.append(s[2])
        for i in range(2):
            heads[i], carried[i] = rest[i] + after[i][0], after[i][1]
    assert all(any(r) for r in rests[:2]) and rests[2] == (b"", b"") and not any(carried)
    assert names == want[3] and quals == want[4] and b"".join(codes) == want[2]


def test_refusals(batches, texts, small):
    """every line of `mates_bgzf_test reasons print` gives pairBgzfHost's message byte for byte; afterwards the batch holds no reads,
    mates_rest() raises, and the next good call parses and aligns.  A bad member behind the first wavefront in text 1 against one
    inside it in text 2 names text 1, and with only text 2 bad text 2; gzip.compress's bytes on side 2 are refused as plain gzip,
    naming text 2; mates_rest() raises again once the batch got other reads"""
    import ma_amd
    b = batches[0]
    t1, t2 = texts["fastq"]
    table = []
    for line in subprocess.check_output([build_exe(), "reasons", "print"]).decode().splitlines():
        x, y, message = line.split(" ", 2)
        table.append(tuple((bytes.fromhex(s.split(":")[0]), int(s.split(":")[1])) for s in (x, y)) + (message,))
    assert len(table) == 20 and len(set(m for _, _, m in table)) >= 15
    good = lambda t: [member(t[a:a + 40]) for a in range(0, 40 * 130, 40)]
    bad_crc = lambda t, i: wrap(deflate(t[40 * i:40 * i + 40]), zlib.crc32(t[40 * i:40 * i + 40]) ^ 4, 40)
    g1, g2 = good(t1), good(t2)
    at = lambda g, i: sum(map(len, g[:i]))
    both = ((b"".join(g1[:70] + [bad_crc(t1, 70)] + g1[71:]), 0), (b"".join(g2[:3] + [bad_crc(t2, 3)] + g2[4:]), 0),
            "ma_batch_set_mates_bgzf: text 1: member 70 (byte %d): CRC mismatch" % at(g1, 70))
    second = ((b"".join(g1), 0), (b"".join(g2[:70] + [bad_crc(t2, 70)] + g2[71:]), 0),
              "ma_batch_set_mates_bgzf: text 2: member 70 (byte %d): CRC mismatch" % at(g2, 70))
    plain = ((member(t1), 0), (gzip.compress(t2), 0),
             "ma_batch_set_mates_bgzf: text 2: member 0 (byte 0): a gzip member without the BGZF size field: single-member gzip stays with GzFileStream")
    for (m1, d1), (m2, d2), want in table + [both, second, plain]:
        with pytest.raises(ma_amd.MaError) as e:
            b.set_mates_bgzf(m1, m2, drops=(d1, d2))
        assert str(e.value).startswith(want) and (str(e.value) == want or want is plain[2]) and e.value.n_pairs == 0
        assert b.read_counts() == ZERO
        with pytest.raises(ma_amd.MaError, match="ma_batch_get_mates_rest: run ma_batch_set_mates_bgzf first"):
            b.mates_rest()
        assert same_as_text(batches, t1, t2, 1, chain(t1, 4), chain(t2, 3)) == 200
    b.align()
    assert b.counts()["aligned_reads"] >= 0 and len(b.mates_rest()[1]) > 0  # (aligning leaves the rest alone)
    b.set_reads([])
    with pytest.raises(ma_amd.MaError, match="ma_batch_get_mates_rest: run ma_batch_set_mates_bgzf first"):
        b.mates_rest()
    fq = lambda rs, m: b"".join(("@r%d/%d\n%s\n+\n%s\n" % (i, m, "".join("ACGTN"[int(x)] for x in r), "I" * len(r))).encode() for i, r in enumerate(rs))
    reads = small[2]
    assert b.set_mates_bgzf(member(fq(reads[0:16:2], 1)), member(fq(reads[1:16:2], 2)))[0] == 8
    b.align()
    assert b.counts()["aligned_reads"] > 0


def test_capacity(small):
    """2 R = max_reads + 2 is refused with "batch capacity exceeded" and R reported; exactly max_reads reads pass, with surplus
    records on the longer side, which count against nothing"""
    import ma_amd
    b = ma_amd.Batch(small[0], params(), 8, 64)
    rec = lambda i, n: ("@r%d\n%s\n+\n%s\n" % (i, "ACGT" * (n // 4) + "A" * (n % 4), "I" * n)).encode()
    text = lambda lens: b"".join(rec(i, n) for i, n in enumerate(lens))
    with pytest.raises(ma_amd.MaError) as e:
        b.set_mates_bgzf(member(text([4] * 5)), member(text([4] * 5)))
    assert str(e.value) == "ma_batch_set_mates_bgzf: batch capacity exceeded" and e.value.n_pairs == 5
    assert b.read_counts() == ZERO
    t1, t2 = text([8] * 4), text([8] * 4)
    more = t1 + text([60, 61, 62])
    assert b.set_mates_bgzf(b"".join(chain(more, 3)), member(t2)) == (4, (len(t1), len(t2)), (len(more), len(t2)))
    assert b.read_counts()["reads"] == 8 and b.read_counts()["bases"] == 64 and b.mates_rest() == (more[len(t1):], b"")
    b.close()


def test_ma_align_text_input_on_two_bgzip_files(tmp_path, gpu_device):
    """examples/ma_align --text-input on the two mate files of small.case written as BGZF (60 000 text bytes per member, the
    end-of-file marker behind them; BatchPairedBgzfReader + BatchAligner::executePairedBgzfSam) writes, byte for byte, the file it
    writes from the plain files; with a .sam.gz output the file inflates to those bytes; R1 BGZF beside a plain R2, or beside R2
    as plain gzip, ends non-zero and says "compressed\""""
    from test_gpu_mates_text import write_small_mates
    from test_gpu_reads_text import build_ma_align
    exe = build_ma_align()
    fa, (r1, r2), pairs = write_small_mates(tmp_path)
    bgz = []
    for m, path in enumerate((r1, r2)):
        text = open(path, "rb").read()
        bgz.append(str(tmp_path / ("reads_%d.fq.gz" % (m + 1))))
        with open(bgz[-1], "wb") as f:
            f.write(b"".join(split(text, range(60000, len(text), 60000), kinds=False)))
    plain_gz = str(tmp_path / "plain_2.fq.gz")
    with open(plain_gz, "wb") as f:
        f.write(gzip.compress(open(r2, "rb").read()))
    a, z, zz = str(tmp_path / "text.sam"), str(tmp_path / "bgzf.sam"), str(tmp_path / "bgzf.sam.gz")
    subprocess.check_call([exe, "--text-input", fa, r1, a, "illuminapaired", r2])
    subprocess.check_call([exe, "--text-input", fa, bgz[0], z, "illuminapaired", bgz[1]])
    got, want = open(z, "rb").read(), open(a, "rb").read()
    assert got == want and got.count(b"\n") > 2 * pairs
    subprocess.check_call([exe, "--text-input", fa, bgz[0], zz, "illuminapaired", bgz[1]])
    assert gzip.open(zz, "rb").read() == want
    for other in (r2, plain_gz):
        p = subprocess.run([exe, "--text-input", fa, bgz[0], str(tmp_path / "o.sam"), "illuminapaired", other], stderr=subprocess.PIPE)
        assert p.returncode != 0 and b"compressed" in p.stderr


def test_end_to_end_paired_sam(gpu_device):
    """500 sampled 150 bp pairs under illuminapaired: set_mates_bgzf (3 000-byte members) + align + pair + pair_sam(bits) for bits 0
    and 31 equals the set_mates_text path -- SAM bytes and pair_off -- and so do the BGZF members of that text"""
    import ma_amd
    g = rand_genome(MIXED["seed"], MIXED["contig_lens"], repeat_unit=MIXED["repeat_unit"], repeat_copies=MIXED["repeat_copies"],
                    repeat_div=MIXED["repeat_div"])
    idx = ma_amd.Index.build(g)
    idx.set_contig_names(["chrA", "chrB"])
    rng = np.random.default_rng(71)
    pairs = [np.where(rng.random(len(r)) < 0.004, 4, r).astype(np.uint8) for r in sample_pairs(g, 500, 150, 72)]
    in_file = [r if i % 2 == 0 else np.where(r[::-1] < 4, 3 - r[::-1], 4).astype(np.uint8) for i, r in enumerate(pairs)]
    quals = [rng.integers(33, 127, size=len(r), dtype=np.uint8) for r in pairs]
    files = ["".join("@pair%d/%d\n%s\n+\n%s\n" % (i // 2, 1 + i % 2, "".join("ACGTN"[int(x)] for x in in_file[i]), quals[i].tobytes().decode())
                     for i in range(m, len(pairs), 2)).encode() for m in (0, 1)]
    P = params("illuminapaired")
    t, z = (ma_amd.Batch(idx, P, 1000, 150 * 1000 + 64) for _ in range(2))
    assert t.set_mates_text(files[0], files[1], 1) == (500, (len(files[0]), len(files[1])))
    cut = lambda f: split(f, range(3000, len(f), 3000))
    assert z.set_mates_bgzf(b"".join(cut(files[0])), b"".join(cut(files[1])))[:2] == (500, (len(files[0]), len(files[1])))
    for x in (t, z):
        x.align()
        x.pair()
    for bits in (0, 31):
        assert t.pair_sam(bits) == z.pair_sam(bits) > 0
        (to, tt), (zo, zt) = t.pair_sam_text(), z.pair_sam_text()
        assert tt == zt and np.array_equal(to, zo) and len(to) == 501
        assert t.sam_bgzf(pair=True) == z.sam_bgzf(pair=True)
    t.close()
    z.close()
    idx.close()
