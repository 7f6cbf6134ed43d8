"""ma_genome_append_text / ma_genome_build_index (ma_amd.Genome, Index.build_text): the genome's FASTA text read on the device.
The yardstick is ma_genome_dev::parseHost, the serial statement of the rules the kernels run, called through the CPU program of
tests/test_genome_text_host.py (which pins it to the reference's files and to FileReader + buildIndex's base loop); the fill is
compared with libc's rand() itself, the index with Index.build on the same bases."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ma_amd
from ma_testlib import ROOT, rand_genome
from test_genome_text_host import build_exe

pytestmark = pytest.mark.gpu
G = os.path.join(ROOT, "tests", "golden", "genome")
SEED = 20261021


def host_results(tmp, texts, seed=1):
    """parseHost's result per text: dict(counts, names, starts, lens, n_holes, hole_starts, hole_lens, codes, filled) or
    dict(refused=message)"""
    paths = []
    for i, t in enumerate(texts):
        p = os.path.join(str(tmp), "t%d.fa" % i)
        with open(p, "wb") as f:
            f.write(t)
        paths.append(p)
    return host_results_of(paths, seed)


def host_results_of(paths, seed=1):
    out = subprocess.check_output([build_exe(), "dump", str(seed)] + paths, timeout=120)
    res = []
    for block in out.split(b"file ")[1:]:
        lines = block.split(b"\n")
        r = dict(names=[], starts=[], lens=[], n_holes=[], hole_starts=[], hole_lens=[])
        for l in lines[1:]:
            k, _, v = l.partition(b" ")
            if k == b"refused":
                r = dict(refused=v.decode())
            elif k == b"counts":
                r["counts"] = dict(zip(("contigs", "bases", "name_bytes", "holes", "hole_bases"), map(int, v.split())))
            elif k == b"contig":
                name, s, n, h = v.rsplit(b" ", 3)
                r["names"].append(name), r["starts"].append(int(s)), r["lens"].append(int(n)), r["n_holes"].append(int(h))
            elif k == b"hole":
                s, n = v.split()
                r["hole_starts"].append(int(s)), r["hole_lens"].append(int(n))
            elif k in (b"codes", b"filled"):
                r[k.decode()] = np.frombuffer(v, dtype=np.uint8) - ord("0")
        res.append(r)
    return res


def check(g, want, filled):
    """every getter of the genome == parseHost's result"""
    assert g.counts() == want["counts"]
    c = g.contigs()
    assert c["names"] == want["names"]
    assert c["starts"].tolist() == want["starts"] and c["lens"].tolist() == want["lens"] and c["n_holes"].tolist() == want["n_holes"]
    st, ln = g.holes()
    assert st.tolist() == want["hole_starts"] and ln.tolist() == want["hole_lens"]
    codes = g.codes()
    assert np.array_equal(codes, want["filled" if filled else "codes"])
    n = want["counts"]["bases"]
    if n > 3:  # a part of the codes, from an odd offset
        assert np.array_equal(g.codes(1, n - 3), codes[1:n - 2])


def append_chunks(g, chunks, complete=True):
    """chunks: (bytes, end_of_file) in order; what a call does not consume goes in front of the next chunk.  Returns the consumed
    counts."""
    rest, got = b"", []
    for data, eof in chunks:
        data = rest + data
        n = g.append_text(data, end_of_file=eof)
        got.append(n)
        rest = data[n:]
    assert rest == b"" or not complete
    return got


def random_cuts(text, rng):
    """the text as up to four chunks cut at random places: a cut inside a line leaves a tail for the next call"""
    cuts = sorted(set(int(x) for x in rng.integers(1, max(len(text), 2), size=int(rng.integers(0, 4)))))
    ends = [0] + [c for c in cuts if c < len(text)] + [len(text)]
    return [(text[a:b], b == len(text)) for a, b in zip(ends, ends[1:])]


def run_case(text, want, chunks, seed=1, max_bases=None):
    g = ma_amd.Genome(max_bases or max(want["counts"]["bases"], 1))
    try:
        append_chunks(g, chunks)
        check(g, want, False)
        idx = g.build_index(seed)
        try:
            check(g, want, True)
            assert idx.sizes()[2] == 2 * want["counts"]["bases"] and idx.sizes()[3] == want["counts"]["contigs"]
        finally:
            idx.close()
    finally:
        g.close()


# ---- 1. fixtures and random genomes ----------------------------------------------------------------------------------------------
def test_fixtures(tmp_path, gpu_device):
    paths = [os.path.join(G, n + ".fa") for n in ("mixed", "crlf", "plain")]
    rng = np.random.default_rng(1)
    for p, want in zip(paths, host_results_of(paths, SEED)):
        text = open(p, "rb").read()
        run_case(text, want, [(text, True)], SEED)
        ends = [i + 1 for i, b in enumerate(text) if b == 10 and i + 1 < len(text)]
        for cut in ends:  # a cut behind every line end
            run_case(text, want, [(text[:cut], False), (text[cut:], True)], SEED)
        run_case(text, want, random_cuts(text, rng), SEED)


@pytest.fixture(scope="module")
def random_genomes(tmp_path_factory):
    d = tmp_path_factory.mktemp("genomes")
    subprocess.check_call([build_exe(), "gen", str(SEED), "200", str(d)], timeout=120)
    paths = [os.path.join(str(d), "g%d.fa" % i) for i in range(200)]
    return [open(p, "rb").read() for p in paths], host_results_of(paths, 7)


@pytest.mark.parametrize("part", range(4))
def test_random_genomes(gpu_device, random_genomes, part):
    """200 of the CPU test's random genomes, 50 per case, through random cuts"""
    texts, wants = random_genomes
    rng = np.random.default_rng(100 + part)
    with_holes = 0
    for text, want in list(zip(texts, wants))[50 * part:50 * part + 50]:
        assert "refused" not in want
        run_case(text, want, random_cuts(text, rng), 7)
        with_holes += 1 if want["counts"]["holes"] else 0
    assert with_holes > 25


# ---- 2. granule and workgroup edges ---------------------------------------------------------------------------------------------------
def bases(rng, n, hole_rate=0.2):
    """n base letters with runs of hole bases"""
    out = []
    while len(out) < n:
        if rng.random() < hole_rate:
            out += list(rng.choice(list(b"NNNNnRYk"), size=int(rng.integers(1, 30))))
        else:
            out += list(rng.choice(list(b"ACGTacgt"), size=int(rng.integers(1, 60))))
    return bytes(out[:n])


def edge_cases():
    rng = np.random.default_rng(5)
    cases = {}
    for off in (15, 16, 17, 4095, 4096, 4097):  # a line feed at this offset of the chunk
        t = b">h\n" + bases(rng, off - 3) + b"\n" + bases(rng, 70) + b"\n" + bases(rng, 5000) + b"\n"
        assert t[off] == 10
        cases["feed at %d" % off] = [(t, True)]
        cases["feed at %d of the second chunk" % off] = [(b">first\nNNACGTNN\n", False), (t[3:], True)]
    name = b">" + b"x" * 150 + b" words that are dropped\n"
    t = b">a\n" + bases(rng, 4096 - 3 - 1 - 60) + b"\n" + name + bases(rng, 100) + b"\n"
    assert t.index(name) < 4096 < t.index(name) + 151
    cases["a header line across byte 4096"] = [(t, True)]
    t = b">a\n" + bases(rng, 4080, 0) + b"N" * 40 + bases(rng, 4096 + 100, 0) + b"NNNN" + b"\n>b\nN\n"
    cases["a hole across byte and base 4096, one at the end, one of a single base"] = [(t, True)]
    t = b">a\n" + bases(rng, 4080, 0) + b"NNNNNNNNNN\nNNNNNNNNNNNNNNNNNNNNNNN\nNNNNNNAC\n"
    cut = t.index(b"\n", 4000) + 1
    cases["a hole across a line end and a chunk border"] = [(t[:cut], False), (t[cut:cut + 24], False), (t[cut + 24:], True)]
    cases["a chunk ends in N, the next starts a contig in N"] = [(b">a\nACNN\n", False), (b">b\nNNAC\n", True)]
    t = b"".join(b">c%d\n" % n + bases(rng, n) + b"\n" for n in (1, 63, 64, 65, 4096))
    cases["contigs of 1, 63, 64, 65 and 4096 bases"] = [(t, True)]
    t = b"".join(b">k%d\n" % i + bases(rng, 1 + i % 7, 0.5) + b"\n" for i in range(65))
    cases["65 contigs of one base line each"] = [(t, True)]
    cases["a chunk that is only a header"] = [(b">a x\nAC\n", False), (b">b\n", False), (b"NNACG\nN", True)]
    cases["a chunk that is only the tail of a line"] = [(b">a\nACGT\nNN", False), (b"AC", False), (b"GT\n", True)]
    return cases


def test_edges(tmp_path, gpu_device):
    cases = edge_cases()
    wants = host_results(tmp_path, [b"".join(c for c, _ in chunks) for chunks in cases.values()], 3)
    for (what, chunks), want in zip(cases.items(), wants):
        assert "refused" not in want, what
        text = b"".join(c for c, _ in chunks)
        if what == "a chunk that is only the tail of a line":
            g = ma_amd.Genome(100)
            assert append_chunks(g, chunks[:2], complete=False) == [8, 0]  # the second call sees "NNAC": no line feed, nothing consumed
            g.close()
        run_case(text, want, chunks, 3)


# ---- 3. the fill ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, SEED])
def test_fill_is_libc_rand(tmp_path, gpu_device, seed):
    rng = np.random.default_rng(9)
    text = b">a\n" + bases(rng, 9000, 0.4) + b"\n>b\n" + bases(rng, 5000, 0.3) + b"\n"
    want = host_results(tmp_path, [text], seed)[0]
    libc = ctypes.CDLL(None)
    libc.srand(ctypes.c_uint(seed))
    hole = want["codes"] == 4
    draws = np.array([libc.rand() & 3 for _ in range(int(hole.sum()))], dtype=np.uint8)
    assert len(draws) > 2000
    built = []
    for _ in range(2):  # the same genome built twice gives the same bytes
        g = ma_amd.Genome(len(text))
        g.append_text(text, end_of_file=True)
        idx = g.build_index(seed)
        codes = g.codes()
        assert np.array_equal(codes[hole], draws) and np.array_equal(codes[~hole], want["codes"][~hole])
        built.append(idx.download())
        idx.close()
        g.close()
    for k in ("bwt", "sa", "pac", "L2"):
        assert np.array_equal(built[0][k], built[1][k])


# ---- 4. / 5. the index, its names and holes --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sixty_kb(gpu_device):
    """about 60 kb, three contigs (two of the same name), holes; the index of the text and the index of Index.build on the same
    bases with names and holes set by hand (holes and draws derived here from the letters, not taken from the genome object)"""
    rng = np.random.default_rng(11)
    contigs = rand_genome(31, [30000, 20000, 10000])
    names = [b"chr1", b"chr1", b"chrX"]
    parts = []
    for name, c in zip(names, contigs):
        s = bytearray(b"ACGT"[int(x)] for x in c)
        for _ in range(6):
            p, n = int(rng.integers(0, len(s) - 300)), int(rng.integers(1, 200))
            s[p:p + n] = b"N" * n
        s[:5] = b"NNNNN"
        parts.append(b">" + name + b" comment\n" + b"\n".join(bytes(s[i:i + 70]) for i in range(0, len(s), 70)) + b"\n")
    text = b"".join(parts)
    seed = 4711
    g = ma_amd.Genome(len(text))
    g.append_text(text, end_of_file=True)
    idx = g.build_index(seed)
    filled, c, holes = g.codes(), g.contigs(), g.holes()
    g.close()
    # the same draws by hand
    libc = ctypes.CDLL(None)
    libc.srand(ctypes.c_uint(seed))
    letters = np.frombuffer(b"".join(l for l in text.split(b"\n") if not l.startswith(b">")), dtype=np.uint8)
    by_hand = np.array([b"ACGT".find(bytes([x])) for x in letters], dtype=np.int8)
    cuts = np.cumsum([0] + [len(x) for x in contigs])
    # the holes by hand, from the letters: a run of letters that are not A C G T inside one contig
    is_hole = (by_hand < 0).tolist()
    starts, lens = [], []
    for k in range(3):
        prev = False
        for i in range(int(cuts[k]), int(cuts[k + 1])):
            if is_hole[i] and prev:
                lens[-1] += 1
            elif is_hole[i]:
                starts.append(i), lens.append(1)
            prev = is_hole[i]
    hand_holes = (np.array(starts, dtype=np.uint64), np.array(lens, dtype=np.uint64))
    for i in np.flatnonzero(by_hand < 0):
        by_hand[i] = libc.rand() & 3
    by_hand = by_hand.astype(np.uint8)
    ref = ma_amd.Index.build([by_hand[cuts[i]:cuts[i + 1]] for i in range(3)])
    ref.set_contig_names(names)
    ref.set_holes(hand_holes[0], hand_holes[1])
    yield dict(idx=idx, ref=ref, filled=filled, by_hand=by_hand, names=names, contigs=c, holes=holes, hand_holes=hand_holes)
    idx.close()
    ref.close()


def test_index_equals_index_build(tmp_path, sixty_kb):
    s = sixty_kb
    assert np.array_equal(s["filled"], s["by_hand"]) and len(s["holes"][0]) >= 18
    assert np.array_equal(s["holes"][0], s["hand_holes"][0]) and np.array_equal(s["holes"][1], s["hand_holes"][1])
    assert s["contigs"]["names"] == s["names"] and s["contigs"]["lens"].tolist() == [30000, 20000, 10000]
    assert s["idx"].sizes() == s["ref"].sizes()
    a, b = s["idx"].download(), s["ref"].download()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    s["idx"].store(str(tmp_path / "a"), names=[n.decode() for n in s["names"]])
    s["ref"].store(str(tmp_path / "b"), names=[n.decode() for n in s["names"]])
    for ext in ("bwt", "sa", "pac", "ann", "amb"):
        assert open(str(tmp_path / "a.") + ext, "rb").read() == open(str(tmp_path / "b.") + ext, "rb").read(), ext


def test_names_and_holes_arrive_on_the_index(sixty_kb):
    s = sixty_kb
    reads = []
    for st, ln in list(zip(*s["hand_holes"]))[:12]:  # reads that touch holes
        a = max(int(st) - 60, 0)
        reads.append(s["filled"][a:a + 150].copy())
    assert len(reads) == 12
    names = ["r%d" % i for i in range(len(reads))]
    texts = []
    for index in (s["idx"], s["ref"]):
        b = ma_amd.Batch(index, ma_amd.Params.preset("default"), len(reads), sum(len(r) for r in reads) + 64)
        b.set_reads(reads)
        b.set_read_text(names, None)
        b.align()
        b.sam(ma_amd.SAM_NGMLR_TAGS | ma_amd.SAM_SOFT_CLIP)
        single = b.sam_text()[1]
        b.pair()
        b.pair_sam(0)
        texts.append((bytes(single), bytes(b.pair_sam_text()[1])))
        b.close()
    assert texts[0][0].count(b"\n") >= 12 and b"\tchr1\t" in texts[0][0] and b"\tchr1\t" in texts[0][1] and b"NM:i:" in texts[0][0]
    assert texts[0] == texts[1]


def test_build_text(gpu_device):
    text = open(os.path.join(G, "mixed.fa"), "rb").read()
    idx = ma_amd.Index.build_text(text, seed=5)
    assert idx.sizes()[2:] == (2 * 179, 3)
    idx.close()


# ---- 6. refusals and capacity --------------------------------------------------------------------------------------------------------------
def test_refusals_and_capacity(gpu_device):
    reason = {"cr": "a carriage return that is not followed by a line feed", "empty": "an empty line where bases are expected",
              "start": "a sequence line must not start with a blank or '@' (FASTQ: nor with '+')", "nobases": "a FASTA record without bases",
              "kind": "the text starts with neither '@' (FASTQ) nor '>' (FASTA)"}
    first = b">a x\nACGTN\n"  # 11 bytes, 2 lines
    g = ma_amd.Genome(1000)
    before = g.counts()

    def refused(data, eof, message):
        state = (g.counts(), g.contigs()["lens"].tolist(), g.holes()[0].tolist(), g.holes()[1].tolist())
        with pytest.raises(ma_amd.MaError) as e:
            g.append_text(data, end_of_file=eof)
        assert str(e.value) == "ma_genome_append_text: " + message
        assert (g.counts(), g.contigs()["lens"].tolist(), g.holes()[0].tolist(), g.holes()[1].tolist()) == state

    with pytest.raises(ma_amd.MaError, match="^ma_genome_build_index: the genome has no contigs$"):
        g.build_index()
    refused(b"ACGT\n", True, "line 1 (byte 0): " + reason["kind"])
    refused(b"@r\nACGT\n+\nIIII\n", True, "a genome is FASTA")
    refused(b">a\nAC\rGT\n", True, "line 2 (byte 3): " + reason["cr"])
    refused(b">a\nACGT\n\nAC\n", True, "line 3 (byte 8): " + reason["empty"])
    refused(b">a\nACGT\n AC\n", True, "line 3 (byte 8): " + reason["start"])
    refused(b">a\n>b\nAC\n", True, "line 1 (byte 0): " + reason["nobases"])
    refused(b">a\nAC\n>b", True, "line 3 (byte 6): " + reason["nobases"])
    assert g.counts() == before
    assert g.append_text(first + b"AC") == 11
    # in a second chunk line and byte count over both
    refused(b"AC\rGT\n", False, "line 3 (byte 11): " + reason["cr"])
    refused(b"AC\n\n", False, "line 4 (byte 14): " + reason["empty"])
    refused(b"@AC\n", False, "line 3 (byte 11): " + reason["start"])
    refused(b"AC\n>b\n>c\nAC\n", False, "line 4 (byte 14): " + reason["nobases"])
    refused(b"AC\n>b\n", True, "line 4 (byte 14): " + reason["nobases"])
    assert g.append_text(b"NNAC\n>b\n") == 8  # a header ends a chunk that is not the file's end
    with pytest.raises(ma_amd.MaError, match="^ma_genome_build_index: the last contig is still open without bases$"):
        g.build_index()
    refused(b">c\nAC\n", False, "line 4 (byte 16): " + reason["nobases"])
    refused(b"", True, "line 4 (byte 16): " + reason["nobases"])
    assert g.append_text(b"GT\n", end_of_file=True) == 3
    refused(b"ACGT\n", False, "line 6 (byte 22): " + reason["kind"])
    assert g.counts() == dict(contigs=2, bases=11, name_bytes=2, holes=1, hole_bases=3) and g.holes()[1].tolist() == [3]
    idx = g.build_index()
    with pytest.raises(ma_amd.MaError, match="^ma_genome_build_index: the index was already built$"):
        g.build_index()
    refused(b">c\nAC\n", True, "the index was already built")
    idx.close()
    g.close()
    # n_bytes of 2 GiB: refused on the number alone, before a byte of the chunk is looked at (the buffer holds 16 bytes)
    g = ma_amd.Genome(100)
    assert g.append_text(b">a\nAC\n") == 6
    before = g.counts()
    small = np.frombuffer(b"ACGT\nACGT\nACGT\n\0", dtype=np.uint8)
    for eof in (1, 0):
        consumed = ctypes.c_uint64(99)
        rc = ma_amd.lib().ma_genome_append_text(g.h, small.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(2 ** 31), ctypes.c_int32(eof),
                                                ctypes.byref(consumed))
        assert rc != 0 and ma_amd.lib().ma_last_error() == b"ma_genome_append_text: too large"
        assert consumed.value == 0 and g.counts() == before
    assert g.append_text(b"GT\n", end_of_file=True) == 3 and g.counts()["bases"] == 4 and g.codes().tolist() == [0, 1, 2, 3]
    # compressed bytes where a header is due are named
    with pytest.raises(ma_amd.MaError) as e:
        g.append_text(b"\x1f\x8b\x08\x04more\n")
    assert str(e.value) == "ma_genome_append_text: a genome as BGZF or gzip is not served (plain FASTA text only)" and g.counts()["bases"] == 4
    with pytest.raises(ma_amd.MaError, match="a genome as BGZF or gzip is not served"):
        ma_amd.Index.build_text(b"\x1f\x8b\x08\x00" + bytes(30))
    g.close()
    # exactly max_bases bases pass, one more is refused
    g = ma_amd.Genome(6)
    assert g.append_text(b">a\nACGT\n") == 8
    with pytest.raises(ma_amd.MaError) as e:
        g.append_text(b"ACG\n")
    assert str(e.value) == "ma_genome_append_text: genome capacity exceeded (7 bases)" and g.counts()["bases"] == 4
    assert g.append_text(b"AN\n", end_of_file=True) == 3 and g.counts()["bases"] == 6
    assert g.codes().tolist() == [0, 1, 2, 3, 0, 4]
    g.close()


# ---- 7. the host layer ---------------------------------------------------------------------------------------------------------------------
def build_store_test():
    exe = os.path.join(ROOT, "tests", "emul", "genome_store_test")
    deps = [exe + ".cpp", os.path.join(ROOT, "ma_amd", "libma_amd.so")] + [os.path.join(ROOT, "ma_amd", "host", h) for h in os.listdir(
        os.path.join(ROOT, "ma_amd", "host")) if h.endswith(".h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ma_amd", "host"),
                               exe + ".cpp", "-o", exe, "-L" + os.path.join(ROOT, "ma_amd"), "-lma_amd", "-Wl,-rpath," + os.path.join(ROOT, "ma_amd"),
                               "-lpthread"])
    return exe


def genome_file(path, seed, lens):
    """a FASTA genome with holes; returns its text"""
    rng = np.random.default_rng(seed)
    parts = []
    for i, n in enumerate(lens):
        s = bases(rng, n, 0.03)
        parts.append(b">chr%d some words\n" % (i + 1) + b"\n".join(s[k:k + 60] for k in range(0, len(s), 60)) + b"\n")
    text = b"".join(parts)
    with open(path, "wb") as f:
        f.write(text)
    return text


def test_host_layer_stores_the_same_files(tmp_path, gpu_device):
    """buildIndexFromFastaText in chunks of 4 096 bytes (and of 50: lines longer than the buffer) and buildIndexFromFasta after
    srand(seed): storeIndex writes the same five files"""
    fa = str(tmp_path / "genome.fa")
    text = genome_file(fa, 21, [20000, 9000, 7000])
    assert len(text) > 8 * 4096 and sum(text.count(c) for c in (b"N", b"n", b"R", b"Y", b"k")) > 300
    for chunk in (4096, 50):
        a, b = str(tmp_path / ("host%d" % chunk)), str(tmp_path / ("text%d" % chunk))
        out = subprocess.check_output([build_store_test(), fa, a, b, "1", str(chunk)], timeout=120)
        assert out.startswith(b"stored ok: 3 contigs"), out
        for ext in ("bwt", "sa", "pac", "ann", "amb"):
            assert open(a + "." + ext, "rb").read() == open(b + "." + ext, "rb").read(), ext
    assert open(a + ".amb", "rb").read().count(b"\n") > 20


@pytest.mark.parametrize("tags", [False, True])
def test_ma_align_genome_text_writes_the_same_file(tmp_path, gpu_device, tags):
    """examples/ma_align --genome-text genome.fa reads.fq out.sam writes the bytes of ma_align genome.fa reads.fq out.sam, with and
    without --ngmlr-tags; reads that touch holes among them"""
    from test_gpu_reads_text import build_ma_align
    exe = build_ma_align()
    fa = str(tmp_path / "genome.fa")
    text = genome_file(fa, 22, [40000, 15000])
    letters = b"".join(l for l in text.split(b"\n") if not l.startswith(b">"))
    rng = np.random.default_rng(23)
    fq = str(tmp_path / "reads.fq")
    with open(fq, "wb") as f:
        for i in range(60):
            p = int(rng.integers(0, len(letters) - 150))
            seq = letters[p:p + 150].upper().replace(b"R", b"N").replace(b"Y", b"N").replace(b"K", b"N")
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, seq, b"I" * len(seq)))
    outs = []
    for flag in ([], ["--genome-text"]):
        out = str(tmp_path / ("out%d.sam" % len(flag)))
        subprocess.check_call([exe] + flag + (["--ngmlr-tags"] if tags else []) + [fa, fq, out], timeout=120)
        outs.append(open(out, "rb").read())
    assert outs[0].count(b"\n") > 60 and outs[0] == outs[1]
