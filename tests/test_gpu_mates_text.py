"""ma_batch_set_mates_text: the two FASTQ / FASTA texts of a paired-end run parsed, interleaved and reverse-complemented on the
device (k_text_mates_* of ma_amd/csrc/stage_text.h), through the C ABI / ma_amd.api and through the host layer.  The yardsticks:
ma_text::pairHost (ma_amd/host/ma_text_dev.h, run by tests/emul/mates_text_test.cpp in mode `dump`, which also compares every
accepted pair of texts with PairedFileReader of ma_amd/host/ma_sam.h), the reference's own reader output
(tests/golden/reader/mates.rc{0,1}.ref), the array path (set_reads + set_read_text), and plain examples/ma_align."""
import os
import subprocess

import numpy as np
import pytest

from ma_testlib import ROOT, gunzip_to, rand_genome, read_case, revcomp, sample_pairs
from test_gpu_reads_text import MIXED, build_ma_align
from test_mates_text_host import build_exe

pytestmark = pytest.mark.gpu
G = os.path.join(ROOT, "tests", "golden")
LENGTHS = [1, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257]
CHUNK, GROUP = 16, 4096  # bytes per lane and per workgroup of the byte-parallel kernels (stage_text.h)


def host_pairs(tmp, pairs, rev):
    """pairHost on every (text1, text2): (reads, consumed) with reads a list of (name, codes, qual or None) -- or the refusal's
    message (str)"""
    paths = []
    os.makedirs(str(tmp), exist_ok=True)
    for i, t in enumerate(x for p in pairs for x in p):
        paths.append(os.path.join(str(tmp), "m%d_%d.txt" % (i // 2, i % 2)))
        with open(paths[-1], "wb") as f:
            f.write(t)
    out, lines = [], subprocess.check_output([build_exe(), "dump", str(int(rev))] + paths).decode("latin-1").split("\n")
    k = 0
    for _ in pairs:
        head = lines[k]
        k += 1
        if head.startswith("ERR "):
            out.append(head[4:])
            continue
        tag, n, has_q, c1, c2, same = head.split(" ")
        assert tag == "OK" and same == "same", head  # (accepted texts pair to what the host's paired reader reads)
        reads = []
        for _ in range(int(n)):
            nm, cd, ql = lines[k].split(" ")
            k += 1
            reads.append((bytes.fromhex(nm[1:]), np.frombuffer(cd[1:].encode(), dtype=np.uint8) - ord("0"),
                          bytes.fromhex(ql[1:]) if int(has_q) else None))
        out.append((reads, (int(c1), int(c2))))
    return out


def check(b, t1, t2, rev, want):
    """the device's parse of (t1, t2) == want (host_pairs' entry)"""
    import ma_amd
    if isinstance(want, str):
        with pytest.raises(ma_amd.MaError) as e:
            b.set_mates_text(t1, t2, rev)
        assert str(e.value) == want and e.value.n_pairs == 0
        assert b.read_counts()["reads"] == 0
        return
    reads, consumed = want
    assert b.set_mates_text(t1, t2, rev) == (len(reads) // 2, consumed)
    off, codes = b.reads()
    names, quals = b.read_text()
    c = b.read_counts()
    assert c["reads"] == len(reads) and c["bases"] == int(off[-1]) == sum(len(r[1]) for r in reads)
    assert c["name_bytes"] == sum(len(r[0]) for r in reads)
    assert names == [r[0] for r in reads]
    assert np.array_equal(codes, np.concatenate([r[1] for r in reads] + [np.zeros(0, dtype=np.uint8)]))
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(r[1]) for r in reads])]).astype(np.uint64))
    if reads and reads[0][2] is not None:
        assert c["has_qual"] == 1 and quals == [r[2] for r in reads]
    else:
        assert c["has_qual"] == 0 and quals is None


def record(rng, fastq, length, name, end):
    """one record; a FASTA record of two or more bases on two lines"""
    seq = "".join("ACGTNacgtRYK"[int(x)] for x in rng.integers(0, 12, size=length))
    if fastq:
        q = "".join(chr(int(x)) for x in rng.integers(33, 127, size=length))
        return ("@%s%s%s%s+%s%s%s" % (name, end, seq, end, end, q, end)).encode()
    cut = int(rng.integers(1, length)) if length > 1 else 1
    return (">%s%s%s%s" % (name, end, end.join(s for s in (seq[:cut], seq[cut:]) if s), end)).encode()


def mates(rng, fastq, lengths, mate, end="\n", first_name=None):
    return b"".join(record(rng, fastq, n, ("p%d/%d" % (i, mate) if i or first_name is None else first_name) + (" x" if i % 3 == 1 else ""),
                           end) for i, n in enumerate(lengths))


@pytest.fixture(scope="module")
def small(tmp_path_factory, gpu_device):
    import ma_amd
    g, reads, names = read_case(gunzip_to(os.path.join(G, "small.case.gz"), str(tmp_path_factory.mktemp("mates") / "small.case")))
    idx = ma_amd.Index.build(g)
    idx.set_contig_names(names)
    yield idx, g, reads
    idx.close()


def params(preset="default"):
    import ma_amd
    P = ma_amd.Params.preset(preset)
    P.srand_seed = 1
    return P


def test_goldens(small):
    """mates_1.fq / mates_2.fq, rev_comp 0 / 1: reads(), read_text() and read_counts() equal mates.rc0.ref / mates.rc1.ref, the
    reference's PairedFileReader output -- the third record of mates_1.fq dropped, code 5 for the complemented N, the second
    mates' qualities reversed"""
    import ma_amd
    t1, t2 = (open(os.path.join(G, "reader", "mates_%d.fq" % m), "rb").read() for m in (1, 2))
    b = ma_amd.Batch(small[0], params(), 64, 4096)
    for rev in (0, 1):
        ref = [l.split(" ") for l in open(os.path.join(G, "reader", "mates.rc%d.ref" % rev)).read().splitlines()]
        want = [(nm.encode(), np.frombuffer(cd.encode(), dtype=np.uint8) - ord("0"), q.encode()) for nm, n, cd, q in ref]
        assert len(want) == 4 and all(len(w[1]) == int(r[1]) for w, r in zip(want, ref))
        n, consumed = b.set_mates_text(t1, t2, rev)
        assert n == 2 and consumed[1] == len(t2) and 0 < consumed[0] < len(t1) and t1[consumed[0]:consumed[0] + 1] == b"@"
        check(b, t1, t2, rev, (want, consumed))
    assert 5 in b.reads()[1]
    b.close()


@pytest.mark.parametrize("fastq,end", [(True, "\n"), (True, "\r\n"), (False, "\n"), (False, "\r\n")])
def test_strides(tmp_path, small, fastq, end):
    """pairs whose mate lengths run through 1 .. 257 in different orders for the two texts, with one mate of 5 000 and one of 70 000
    bases (a single line reversed across many workgroups), FASTA mates on two lines: with and without the final line end and
    rev_comp 0 / 1; then the first name of text 2 padded by 0 .. 33 and by 4 094 .. 4 096 bytes, so that every record start meets
    every position of a lane's 16 bytes and a workgroup border: all equal pairHost's dump"""
    import ma_amd
    rng = np.random.default_rng(20261020)
    len1, len2 = LENGTHS + [5000, 40], LENGTHS[::-1] + [33, 70000]
    cases = []
    for final in (True, False):
        for rev in (0, 1):
            t1, t2 = mates(rng, fastq, len1, 1, end), mates(rng, fastq, len2, 2, end)
            cases.append((t1 if final else t1[:-len(end)], t2 if final else t2[:-len(end)], rev))
    for pad in list(range(2 * CHUNK + 2)) + [GROUP - 2, GROUP - 1, GROUP]:
        t1, t2 = mates(rng, fastq, len1, 1, end), mates(rng, fastq, len2, 2, end, first_name="q" * pad)
        cases.append((t1, t2 if pad % 4 < 2 else t2[:-len(end)], pad % 2))
    want = {rev: host_pairs(tmp_path / str(rev), [c[:2] for c in cases if c[2] == rev], rev) for rev in (0, 1)}
    b = ma_amd.Batch(small[0], params(), 64, 200000)
    at = {0: 0, 1: 0}
    for t1, t2, rev in cases:
        w = want[rev][at[rev]]
        at[rev] += 1
        assert not isinstance(w, str) and len(w[0]) == 2 * len(len1), w
        check(b, t1, t2, rev, w)
    b.close()


@pytest.mark.parametrize("R", [1, 63, 64, 65])
def test_unequal_counts(tmp_path, small, R):
    """R1 = R2 + 3 and R2 = R1 + 3: n_pairs, consumed and the arrays equal pairHost; a second call on text + consumed of the longer
    text together with 3 new mate records yields those 3 pairs; an empty text on either side or both gives 0 pairs, after which
    align() behaves like on an empty batch"""
    import ma_amd
    rng = np.random.default_rng(R)
    idx = small[0]
    b = ma_amd.Batch(idx, params(), 256, 65536)
    empty = ma_amd.Batch(idx, params(), 256, 65536)
    empty.set_reads([])
    empty.align()
    for fastq in (True, False):
        lens = lambda n: [1 + int(x) for x in rng.integers(0, 70, size=n)]
        longer, shorter, more = mates(rng, fastq, lens(R + 3), 1), mates(rng, fastq, lens(R), 2), mates(rng, fastq, lens(3), 2)
        pairs = [(longer, shorter), (shorter, longer)]
        want = host_pairs(tmp_path / ("a%d" % fastq), pairs, 1)
        assert want[0][1][1] == want[1][1][0] == len(shorter) and 0 < want[0][1][0] == want[1][1][1] < len(longer)
        rest = [(longer[want[0][1][0]:], more), (more, longer[want[1][1][1]:])]
        want_rest = host_pairs(tmp_path / ("b%d" % fastq), rest, 1)
        for (t1, t2), w, (r1, r2), wr in zip(pairs, want, rest, want_rest):
            assert len(w[0]) == 2 * R
            check(b, t1, t2, 1, w)
            assert len(wr[0]) == 6 and wr[1] == (len(r1), len(r2))
            check(b, r1, r2, 1, wr)
        for t1, t2 in ((b"", shorter), (shorter, b""), (b"", b"")):
            assert b.set_mates_text(t1, t2) == (0, (0, 0))
            assert b.read_counts() == dict(reads=0, bases=0, name_bytes=0, has_qual=0) and b.read_text() == ([], None)
            b.align()
            assert b.counts() == empty.counts() and b.counts()["alignments"] == 0
    b.close()
    empty.close()


def test_refusals(small):
    """the table of tests/emul/mates_text_test.cpp `reasons`: the device's message is pairHost's, byte for byte -- a violation in
    both texts names text 1, one in a record beyond the pairs still refuses, FASTQ against FASTA gives the kind message; after each
    the batch holds no reads, read_text() raises, align() works, and a following valid call parses and aligns"""
    import ma_amd
    idx, g, reads = small
    unhex = lambda h: b"" if h == "-" else bytes.fromhex(h)
    table = [l.split(" ", 2) for l in subprocess.check_output([build_exe(), "reasons", "print"]).decode().splitlines()]
    assert len(table) >= 12 and sum("text 1: " in m for _, _, m in table) >= 3 and sum("differ in kind" in m for _, _, m in table) == 2
    fq = lambda rs, m: b"".join(("@r%d/%d\n%s\n+\n%s\n" % (i, m, "".join("ACGTN"[int(x)] for x in r), "I" * len(r))).encode() for i, r in enumerate(rs))
    empty = ma_amd.Batch(idx, params(), 4096, 100000)
    empty.set_reads([])
    empty.align()
    b = ma_amd.Batch(idx, params(), 4096, 100000)
    for h1, h2, want in table:
        with pytest.raises(ma_amd.MaError) as e:
            b.set_mates_text(unhex(h1), unhex(h2))
        assert str(e.value) == want and e.value.n_pairs == 0
        assert b.read_counts() == dict(reads=0, bases=0, name_bytes=0, has_qual=0)
        with pytest.raises(ma_amd.MaError):
            b.read_text()
        b.align()
        assert b.counts() == empty.counts() and b.counts()["alignments"] == 0
        assert b.set_mates_text(fq(reads[0:16:2], 1), fq(reads[1:16:2], 2)) == (8, (len(fq(reads[0:16:2], 1)), len(fq(reads[1:16:2], 2))))
        b.align()
        assert b.counts()["aligned_reads"] > 0
    b.pair()
    assert b.pair_sam(0) > 0
    b.close()
    empty.close()


def test_capacity(small):
    """2 R = max_reads + 2 and paired bases = max_bases + 1 fail with "batch capacity exceeded" and report R; exactly max_reads reads
    of exactly max_bases bases pass, and surplus records beyond R count against neither"""
    import ma_amd
    b = ma_amd.Batch(small[0], params(), 8, 64)
    rec = lambda i, n: ("@r%d\n%s\n+\n%s\n" % (i, "ACGT" * (n // 4) + "A" * (n % 4), "I" * n)).encode()
    text = lambda lens: b"".join(rec(i, n) for i, n in enumerate(lens))
    for t1, t2, pairs in ((text([4] * 5), text([4] * 5), 5), (text([8] * 4), text([8, 8, 8, 9]), 4), (text([8, 8, 8, 9, 1]), text([8] * 4), 4)):
        with pytest.raises(ma_amd.MaError) as e:
            b.set_mates_text(t1, t2)
        assert str(e.value) == "ma_batch_set_mates_text: batch capacity exceeded" and e.value.n_pairs == pairs
        assert b.read_counts() == dict(reads=0, bases=0, name_bytes=0, has_qual=0)
    t1, t2 = text([8] * 4), text([8] * 4)
    assert b.set_mates_text(t1, t2) == (4, (len(t1), len(t2)))
    assert b.read_counts()["reads"] == 8 and b.read_counts()["bases"] == 64
    assert b.set_mates_text(t1 + text([60, 61, 62]), t2) == (4, (len(t1), len(t2)))  # (the surplus: 3 records, 183 bases)
    assert b.set_mates_text(t1, t2 + text([9] * 5)) == (4, (len(t1), len(t2)))
    assert b.read_counts()["reads"] == 8 and b.read_counts()["bases"] == 64
    off, codes = b.reads()
    assert np.array_equal(codes[8:16], [3 - c for c in [0, 1, 2, 3] * 2][::-1])
    b.close()


@pytest.mark.parametrize("rev", [0, 1])
def test_text_path_equals_array_path(gpu_device, rev):
    """500 sampled pairs of 150 bp with some N under illuminapaired: set_mates_text + align + pair + pair_sam(bits) equals
    set_reads(interleaved, the second mates reverse-complemented on the host with code 5) + set_read_text + the same calls, for bits
    0 and 31: SAM bytes and pair_off; the MappingQuality records are equal as bytes"""
    import ma_amd
    g = rand_genome(MIXED["seed"], MIXED["contig_lens"], repeat_unit=MIXED["repeat_unit"], repeat_copies=MIXED["repeat_copies"],
                    repeat_div=MIXED["repeat_div"])
    idx = ma_amd.Index.build(g)
    idx.set_contig_names(["chrA", "chrB"])
    rng = np.random.default_rng(71)
    pairs = [np.where(rng.random(len(r)) < 0.004, 4, r).astype(np.uint8) for r in sample_pairs(g, 500, 150, 72)]
    # the files: R1 as sampled, R2 as a sequencer writes it (the other strand: rev_comp 1 brings it back)
    in_file = [r if i % 2 == 0 else np.where(r[::-1] < 4, 3 - r[::-1], 4).astype(np.uint8) for i, r in enumerate(pairs)]
    names = ["pair%d/%d" % (i // 2, 1 + i % 2) for i in range(len(pairs))]
    quals = [rng.integers(33, 127, size=len(r), dtype=np.uint8) for r in pairs]
    texts = ["".join("@%s\n%s\n+\n%s\n" % (names[i], "".join("ACGTN"[int(x)] for x in in_file[i]), quals[i].tobytes().decode())
                     for i in range(m, len(pairs), 2)).encode() for m in (0, 1)]
    if rev:  # what PairedFileReader makes of the second mates: reversed with their qualities, complemented, N -> 5
        reads = [r if i % 2 == 0 else np.where(r[::-1] < 4, 3 - r[::-1], 5).astype(np.uint8) for i, r in enumerate(in_file)]
        quals = [q if i % 2 == 0 else q[::-1].copy() for i, q in enumerate(quals)]
    else:
        reads = in_file
    P = params("illuminapaired")
    a = ma_amd.Batch(idx, P, len(reads), sum(len(r) for r in reads) + 64)
    a.set_reads(reads)
    a.set_read_text(names, quals)
    t = ma_amd.Batch(idx, P, len(reads), sum(len(r) for r in reads) + 64)
    assert t.set_mates_text(texts[0], texts[1], rev) == (500, (len(texts[0]), len(texts[1])))
    assert np.array_equal(t.reads()[1], np.concatenate(reads))
    for x in (a, t):
        x.align()
    for x, y in zip(a.mapq_alignments(), t.mapq_alignments()):
        assert len(x) == len(y) and x.tobytes() == y.tobytes()  # (bytes: a mapping quality may be NaN)
    for x in (a, t):
        x.pair()
    for bits in (0, 31 & ~32):
        assert a.pair_sam(bits) == t.pair_sam(bits) > 0
        (ao, at), (to, tt) = a.pair_sam_text(), t.pair_sam_text()
        assert at == tt and np.array_equal(ao, to) and len(ao) == 501
    a.close()
    t.close()
    idx.close()


# ---- through the host layer ---------------------------------------------------------------------------------------------------
def write_small_mates(tmp_path):
    """small.case as a genome FASTA and two FASTQ files of its reads split into mates (R2 one record longer); the pairs"""
    g, reads, names = read_case(gunzip_to(os.path.join(G, "small.case.gz"), str(tmp_path / "small.case")))
    fa = str(tmp_path / "genome.fa")
    with open(fa, "w") as f:
        for nm, c in zip(names, g):
            f.write(">%s\n%s\n" % (nm, "".join("ACGT"[int(b)] for b in c)))
    rng = np.random.default_rng(73)
    pairs = len(reads) // 2 - 1
    files = [str(tmp_path / ("reads_%d.fq" % m)) for m in (1, 2)]
    for m, path in enumerate(files):
        with open(path, "w") as f:
            for k in range(pairs + m):
                r = reads[2 * k + m] if m == 0 else revcomp(reads[2 * k + m])
                f.write("@r%d/%d\n%s\n+\n%s\n" % (k, m + 1, "".join("ACGTN"[int(b)] for b in r),
                                                  "".join(chr(int(q)) for q in rng.integers(35, 127, size=len(r)))))
    return fa, files, pairs


def test_ma_align_text_input_with_mates_writes_the_same_file(tmp_path, gpu_device):
    """examples/ma_align --text-input with a mates file (BatchPairedTextReader + BatchAligner::executePairedTextSam + one write per
    batch) writes, byte for byte, the file of the same command without the flag (PairedFileReader + executePairedFlatSam)"""
    exe = build_ma_align()
    fa, (r1, r2), pairs = write_small_mates(tmp_path)
    plain, text = str(tmp_path / "plain.sam"), str(tmp_path / "text.sam")
    subprocess.check_call([exe, fa, r1, plain, "illuminapaired", r2])
    subprocess.check_call([exe, "--text-input", fa, r1, text, "illuminapaired", r2])
    got, want = open(text, "rb").read(), open(plain, "rb").read()
    assert got == want and got.count(b"\n") > 2 * pairs


def test_ma_align_text_input_with_mates_refuses(tmp_path, gpu_device):
    """with --host-sam the paired text path ends with a non-zero status and says why; a multi-line FASTQ as the mates file ends it
    with the library's message, which names text 2 and line 3"""
    exe = build_ma_align()
    fa, (r1, r2), pairs = write_small_mates(tmp_path)
    p = subprocess.run([exe, "--text-input", "--host-sam", fa, r1, str(tmp_path / "o.sam"), "illuminapaired", r2], stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"--text-input" in p.stderr and b"not with --host-sam" in p.stderr
    p = subprocess.run([exe, "--text-input", fa, r1, str(tmp_path / "o.sam"), "illuminapaired", os.path.join(G, "reader", "reader_multi.fq")],
                       stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"ma_batch_set_mates_text: text 2: line 3 (byte 15): " in p.stderr
