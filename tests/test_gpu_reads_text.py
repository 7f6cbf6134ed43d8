"""ma_batch_set_reads_text: FASTQ / FASTA text parsed on the device (ma_amd/csrc/stage_text.h), through the C ABI / ma_amd.api
and through the host layer.  The yardsticks: ma_text::parseHost (ma_amd/host/ma_text_dev.h, the rules the kernels call, run by
tests/emul/text_dev_test.cpp in mode `dump`, which also compares every accepted text with FileReader::parseRecord of
ma_amd/host/ma_sam.h), the array path (set_reads + set_read_text), the SAM golden the compiled reference wrote from small24.fq,
and plain examples/ma_align."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from ma_testlib import ROOT, gunzip_to, rand_genome, read_case, sample_reads
from test_reads_text_host import build_exe

pytestmark = pytest.mark.gpu
G = os.path.join(ROOT, "tests", "golden")
LENGTHS = [1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257]
CHUNK, GROUP = 16, 4096  # bytes per lane and per workgroup of the byte-parallel kernels (stage_text.h)


def host_parse(tmp, texts):
    """parseHost on every text: a list of (names, codes, quals or None) per read -- or the refusal's message (str)"""
    paths = []
    for i, t in enumerate(texts):
        paths.append(os.path.join(str(tmp), "t%d.txt" % i))
        with open(paths[-1], "wb") as f:
            f.write(t)
    out, lines = [], subprocess.check_output([build_exe(), "dump"] + paths).decode("latin-1").split("\n")
    k = 0
    for _ in texts:
        head = lines[k]
        k += 1
        if head.startswith("ERR "):
            out.append(head[4:])
            continue
        tag, n, has_q, same = head.split(" ")
        assert tag == "OK" and same == "same", head  # (an accepted text parses to what the host reader parses)
        reads = []
        for _ in range(int(n)):
            nm, cd, ql = lines[k].split(" ")
            k += 1
            reads.append((bytes.fromhex(nm[1:]), np.frombuffer(cd[1:].encode(), dtype=np.uint8) - ord("0"),
                          bytes.fromhex(ql[1:]) if int(has_q) else None))
        out.append(reads)
    return out


def check(b, text, want):
    """the device's parse of text == want (host_parse's entry)"""
    import ma_amd
    if isinstance(want, str):
        with pytest.raises(ma_amd.MaError) as e:
            b.set_reads_text(text)
        assert str(e.value) == want
        assert b.read_counts()["reads"] == 0
        return
    assert b.set_reads_text(text) == len(want)
    off, codes = b.reads()
    names, quals = b.read_text()
    c = b.read_counts()
    assert c["reads"] == len(want) and c["bases"] == int(off[-1]) == sum(len(r[1]) for r in want)
    assert c["name_bytes"] == sum(len(r[0]) for r in want)
    assert names == [r[0] for r in want]
    assert np.array_equal(codes, np.concatenate([r[1] for r in want] + [np.zeros(0, dtype=np.uint8)]))
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(r[1]) for r in want])]).astype(np.uint64))
    if want and want[0][2] is not None:
        assert quals == [r[2] for r in want]
    else:
        assert quals is None


def record(rng, fastq, length, name, end, junk=False):
    seq = "".join("ACGTNacgtRYK"[int(x)] for x in rng.integers(0, 12, size=length))
    if junk and length >= 3:
        seq = seq[:1] + "*" + seq[2:]
    if fastq:
        q = "".join(chr(int(x)) for x in rng.integers(33, 127, size=length))
        return ("@%s%s%s%s+%s%s%s" % (name, end, seq, end, end, q, end)).encode()
    cut = int(rng.integers(0, length + 1))
    lines = [s for s in (seq[:cut], seq[cut:]) if s]
    return (">%s%s%s%s" % (name, end, end.join(lines), end)).encode()


def make_name(rng, n, i):
    s = "".join("abXY09_/.:#@>+-\t"[int(x)] for x in rng.integers(0, 16, size=n))
    return s + (" description %d" % i if i % 3 == 0 else "")


@pytest.fixture(scope="module")
def small(tmp_path_factory, gpu_device):
    import ma_amd
    g, reads, names = read_case(gunzip_to(os.path.join(G, "small.case.gz"), str(tmp_path_factory.mktemp("text") / "small.case")))
    idx = ma_amd.Index.build(g)
    idx.set_contig_names(names)
    yield idx, g, reads
    idx.close()


def params(preset="default"):
    import ma_amd
    P = ma_amd.Params.preset(preset)
    P.srand_seed = 1
    return P


def test_strict_texts_on_the_device(tmp_path, small):
    """FASTQ and FASTA, both line ends, with and without the final one, read lengths around the strides, one line of 5 000 and one
    of 70 000 bases (a single line across many workgroups' chunks), names of 0-40 bytes, 1 / 63 / 64 / 65 / 3 001 records: reads(),
    read_text() and read_counts() equal parseHost's arrays, which equal the host reader's"""
    import ma_amd
    rng = np.random.default_rng(20261019)
    texts = []
    for fastq in (True, False):
        for end in ("\n", "\r\n"):
            for final in (True, False):
                t = b"".join(record(rng, fastq, n, make_name(rng, (7 * i) % 41, i), end, junk=i % 4 == 1)
                             for i, n in enumerate(LENGTHS + [5000, 70000]))
                texts.append(t if final else t[:-len(end)])
        for count in (1, 63, 64, 65, 3001):
            texts.append(b"".join(record(rng, fastq, 1 + (i * 7) % 40, make_name(rng, i % 41, i), "\n") for i in range(count)))
    want = host_parse(tmp_path, texts)
    b = ma_amd.Batch(small[0], params(), 4096, 200000)
    for t, w in zip(texts, want):
        assert not isinstance(w, str), w
        check(b, t, w)
    b.close()


@pytest.mark.parametrize("end", ["\n", "\r\n"])
def test_every_alignment_against_the_chunking(tmp_path, small, end):
    """one text of 9 records parsed once per padding of 0 .. 2 x 16 + 1 bytes in the first name (every line break, and with \\r\\n
    the pair itself, at every position of a lane's 16 bytes), once more with the first header's end across a workgroup's 4 096;
    texts of exactly 0, 1, 15, 16 and 17 bytes: all equal parseHost"""
    import ma_amd
    rng = np.random.default_rng(5)
    for fastq in (True, False):
        tail = b"".join(record(rng, fastq, n, "r%d" % i, end) for i, n in enumerate([5, 16, 1, 31, 32, 33, 2, 64]))
        first = record(rng, fastq, 17, "", end)
        texts = [first[:1] + b"p" * p + first[1:] + tail for p in list(range(2 * CHUNK + 2)) + [GROUP - 2, GROUP - 1, GROUP]]
        texts += [b"", first[:1]] + [(">a\n" + "ACGTN" * 4)[:n].encode() for n in (CHUNK - 1, CHUNK, CHUNK + 1)]
        want = host_parse(tmp_path, texts)
        assert sum(isinstance(w, str) for w in want) == 1  # (the text of one byte)
        b = ma_amd.Batch(small[0], params(), 64, 4096)
        for t, w in zip(texts, want):
            check(b, t, w)
        b.close()


def test_refusals(tmp_path, small):
    """the table of tests/emul/text_dev_test.cpp `reasons`: the device's message is parseHost's, byte for byte; of two violations
    the lower line is named whichever workgroup sees it; afterwards the batch holds no reads, aligns like an empty batch, and
    parses and aligns the next valid text"""
    import ma_amd
    idx, g, reads = small
    table = [l.split(" ", 1) for l in subprocess.check_output([build_exe(), "reasons", "print"]).decode().splitlines()]
    assert len(table) >= 11
    rng = np.random.default_rng(9)
    good = [record(rng, True, 40, "r%d" % i, "\n") for i in range(400)]  # ~ 90 bytes each: 9 workgroups
    bad_plus = good[0].replace(b"\n+\n", b"\n-\n")
    bad_qual = good[0][:-2] + b"\n"
    two = [b"".join(good[:150] + [bad_plus] + good[150:390] + [bad_qual]),  # the lower line in an inner workgroup, the other in the last
           b"".join([bad_qual] + good[:390] + [bad_plus]),  # the lower line in the first workgroup
           b"".join(good[:399] + [bad_plus, bad_qual])]  # both in the last one
    want_two = host_parse(tmp_path, two)
    assert [w.split(" ")[2] for w in want_two] == ["603", "4", "1599"]
    valid = b"".join(("@r%d\n%s\n+\n%s\n" % (i, "".join("ACGTN"[int(x)] for x in r), "I" * len(r))).encode() for i, r in enumerate(reads[:16]))
    empty = ma_amd.Batch(idx, params(), 4096, 100000)
    empty.set_reads([])
    empty.align()
    b = ma_amd.Batch(idx, params(), 4096, 100000)
    for text, want in [(bytes.fromhex(h), m) for h, m in table] + list(zip(two, want_two)):
        with pytest.raises(ma_amd.MaError) as e:
            b.set_reads_text(text)
        assert str(e.value) == want and want.startswith("ma_batch_set_reads_text: line ")
        assert b.read_counts() == dict(reads=0, bases=0, name_bytes=0, has_qual=0)
        with pytest.raises(ma_amd.MaError):
            b.read_text()
        b.align()
        assert b.counts() == empty.counts() and b.counts()["alignments"] == 0
    assert b.set_reads_text(valid) == 16
    b.align()
    assert b.counts()["aligned_reads"] > 0 and b.sam(0) > 0
    b.close()
    empty.close()


def test_capacity(small):
    """max_reads + 1 records and max_bases + 1 bases fail with "batch capacity exceeded", max_reads records of max_bases bases
    pass, and so does the next valid call"""
    import ma_amd
    b = ma_amd.Batch(small[0], params(), 8, 64)
    rec = lambda i, n: ("@r%d\n%s\n+\n%s\n" % (i, "ACGT" * (n // 4) + "A" * (n % 4), "I" * n)).encode()
    for text in (b"".join(rec(i, 4) for i in range(9)), b"".join(rec(i, 8) for i in range(7)) + rec(7, 9)):
        with pytest.raises(ma_amd.MaError, match="ma_batch_set_reads_text: batch capacity exceeded"):
            b.set_reads_text(text)
        assert b.read_counts()["reads"] == 0
    assert b.set_reads_text(b"".join(rec(i, 8) for i in range(8))) == 8
    assert b.read_counts()["bases"] == 64
    assert b.set_reads_text(b"") == 0 and b.read_text() == ([], None)
    b.close()


def test_the_references_bytes_from_small24(small):
    """small24.fq as text -> align -> sam(0): the record lines of the file the reference's FileWriter wrote from the reference's
    FileReader's reads (tests/golden/reader/small24.fq.sam.gz)"""
    import ma_amd
    text = open(os.path.join(G, "reader", "small24.fq"), "rb").read()
    want = b"".join(l for l in gzip.open(os.path.join(G, "reader", "small24.fq.sam.gz"), "rb").read().splitlines(True) if not l.startswith(b"@"))
    b = ma_amd.Batch(small[0], params(), 64, 65536)
    assert b.set_reads_text(text) == 24
    b.align()
    assert b.sam(0) == len(want)
    assert b.sam_text()[1] == want
    b.close()


MIXED = dict(seed=41, contig_lens=[300000, 290000], repeat_unit=500, repeat_copies=8, repeat_div=0.01)  # the genome of test_gpu_sam.py


@pytest.mark.parametrize("fastq", [True, False])
def test_text_path_equals_array_path(gpu_device, fastq):
    """1 000 sampled reads as FASTQ / FASTA: set_reads_text + align + sam(bits) == set_reads + set_read_text + align + sam(bits) for
    bits 0 and 31 (bytes and rec_off), and the MappingQuality records are equal"""
    import ma_amd
    g = rand_genome(MIXED["seed"], MIXED["contig_lens"], repeat_unit=MIXED["repeat_unit"], repeat_copies=MIXED["repeat_copies"],
                    repeat_div=MIXED["repeat_div"])
    idx = ma_amd.Index.build(g)
    idx.set_contig_names(["chrA", "chrB"])
    reads = sample_reads(g, 700, 150, 61, sub=0.02) + sample_reads(g, 300, 251, 62, sub=0.03, ins=0.005, dele=0.005, n_rate=0.002)
    rng = np.random.default_rng(63)
    names = ["read%d/%d" % (i, i % 7) for i in range(len(reads))]
    quals = [rng.integers(33, 127, size=len(r), dtype=np.uint8) for r in reads] if fastq else None
    seqs = ["".join("ACGTN"[int(x)] for x in r) for r in reads]
    if fastq:
        text = "".join("@%s\n%s\n+\n%s\n" % (n, s, q.tobytes().decode()) for n, s, q in zip(names, seqs, quals))
    else:
        text = "".join(">%s some description\n%s\n%s\n" % (n, s[:70], s[70:]) for n, s in zip(names, seqs))
    a = ma_amd.Batch(idx, params(), len(reads), sum(len(r) for r in reads) + 64)
    a.set_reads(reads)
    a.set_read_text(names, quals)
    a.align()
    t = ma_amd.Batch(idx, params(), len(reads), sum(len(r) for r in reads) + 64)
    assert t.set_reads_text(text.encode()) == len(reads)
    t.align()
    for x, y in zip(a.mapq_alignments(), t.mapq_alignments()):
        assert len(x) == len(y) and x.tobytes() == y.tobytes()  # (bytes: a mapping quality may be NaN)
    for bits in (0, 31):
        assert a.sam(bits) == t.sam(bits) > 0
        (ao, at), (to, tt) = a.sam_text(), t.sam_text()
        assert at == tt and np.array_equal(ao, to)
    a.close()
    t.close()
    idx.close()


def test_getters_on_the_array_path(small):
    """after set_reads + set_read_text reads() / read_text() return what was set; read_text() without text fails with a message"""
    import ma_amd
    idx, g, reads = small
    b = ma_amd.Batch(idx, params(), len(reads), sum(len(r) for r in reads) + 64)
    b.set_reads(reads[:40])
    with pytest.raises(ma_amd.MaError, match="ma_batch_get_read_text: the reads have no names"):
        b.read_text()
    off, codes = b.reads()
    assert np.array_equal(codes, np.concatenate(reads[:40])) and np.array_equal(np.diff(off.astype(np.int64)), [len(r) for r in reads[:40]])
    names = [("n%d" % i).encode() for i in range(40)]
    b.set_read_text(names, None)
    assert b.read_text() == (names, None)
    quals = [bytes(33 + (i + k) % 90 for k in range(len(r))) for i, r in enumerate(reads[:40])]
    b.set_read_text(names, quals)
    assert b.read_text() == (names, quals)
    assert b.read_counts() == dict(reads=40, bases=int(off[-1]), name_bytes=sum(len(n) for n in names), has_qual=1)
    b.close()


# ---- through the host layer ---------------------------------------------------------------------------------------------------
def build_ma_align():
    exe = os.path.join(ROOT, "examples", "ma_align")
    deps = [exe + ".cpp", os.path.join(ROOT, "ma_amd", "libma_amd.so")] + [os.path.join(ROOT, "ma_amd", "host", h) for h in os.listdir(
        os.path.join(ROOT, "ma_amd", "host")) if h.endswith(".h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        zl = os.path.exists("/usr/include/zlib.h")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall"] + (["-DMA_WITH_ZLIB"] if zl else []) +
                              ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ma_amd", "host"), exe + ".cpp", "-o", exe,
                               "-L" + os.path.join(ROOT, "ma_amd"), "-lma_amd", "-Wl,-rpath," + os.path.join(ROOT, "ma_amd"),
                               "-lpthread"] + (["-lz"] if zl else []))
    return exe


def write_small_case(tmp_path, fastq):
    """small.case as a genome FASTA and a read file (FASTQ with random qualities, or FASTA); the reads"""
    g, reads, names = read_case(gunzip_to(os.path.join(G, "small.case.gz"), str(tmp_path / "small.case")))
    fa = str(tmp_path / "genome.fa")
    with open(fa, "w") as f:
        for nm, c in zip(names, g):
            f.write(">%s\n%s\n" % (nm, "".join("ACGT"[int(b)] for b in c)))
    rng = np.random.default_rng(70)
    rd = str(tmp_path / ("reads.fq" if fastq else "reads.fa"))
    with open(rd, "w") as f:
        for i, r in enumerate(reads):
            seq = "".join("ACGTN"[int(b)] for b in r)
            if fastq:
                f.write("@r%d\n%s\n+\n%s\n" % (i, seq, "".join(chr(int(q)) for q in rng.integers(35, 127, size=len(r)))))
            else:
                f.write(">r%d\n%s\n" % (i, seq))
    return fa, rd, reads


@pytest.mark.parametrize("preset,fastq", [("default", True), ("default", False), ("illumina", True)])
def test_ma_align_text_input_writes_the_same_file(tmp_path, gpu_device, preset, fastq):
    """examples/ma_align --text-input (BatchTextReader + BatchAligner::executeTextSam + one write per batch) on small.case writes,
    byte for byte, the file of plain ma_align (FileReader + executeFlatSam)"""
    exe = build_ma_align()
    fa, rd, reads = write_small_case(tmp_path, fastq)
    dev, text = str(tmp_path / "plain.sam"), str(tmp_path / "text.sam")
    subprocess.check_call([exe, fa, rd, dev, preset])
    subprocess.check_call([exe, "--text-input", fa, rd, text, preset])
    got, want = open(text, "rb").read(), open(dev, "rb").read()
    assert got == want and got.count(b"\n") > len(reads)


def test_ma_align_text_input_refuses_by_line(tmp_path, gpu_device):
    """a multi-line FASTQ ends ma_align --text-input with a non-zero status and the library's message, which names line 3; a .gz
    input is an error that says why"""
    exe = build_ma_align()
    fa, rd, reads = write_small_case(tmp_path, True)
    p = subprocess.run([exe, "--text-input", fa, os.path.join(G, "reader", "reader_multi.fq"), str(tmp_path / "o.sam")], stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"ma_batch_set_reads_text: line 3 (byte 15): " in p.stderr
    p = subprocess.run([exe, "--text-input", fa, os.path.join(G, "reader", "reader_multi.fq.gz"), str(tmp_path / "o.sam")], stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"compressed" in p.stderr
