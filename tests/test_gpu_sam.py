"""ma_sam_batch: the single-end SAM records of a batch formatted on the device (ma_amd/csrc/stage_sam.h), through the C ABI /
ma_amd.api.  Every case compares the device's bytes and rec_off with a yardstick: the SAM goldens the compiled reference
wrote, or ma_amd's FileWriter (ma_amd/host/ma_sam.h) run by tests/emul/sam_dev_test.cpp (mode `dump`) on the records the
device itself reports."""
import ctypes as C
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

from ma_testlib import gunzip_to, rand_genome, read_case, revcomp, sample_reads
from test_sam_dev_host import build_exe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
LENGTHS = [1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257]
ALL_BITS = [0, 1, 2, 4, 8, 16, 31]


def make_quals(reads, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(33, 127, size=len(r), dtype=np.uint8) for r in reads]


def yardstick(tmp, contig_names, starts, lens, names, reads, quals, off, alns, ops, options):
    """FileWriter's (rec_off, text) for the records given; a formatter exception comes back as its text (str)"""
    path = os.path.join(str(tmp), "sam.dump")
    with open(path, "wb") as f:
        f.write(b"MASAMD01" + struct.pack("<I", len(contig_names)))
        for nm, s, l in zip(contig_names, starts, lens):
            f.write(struct.pack("<I", len(nm)) + nm.encode() + struct.pack("<QQ", int(s), int(l)))
        f.write(struct.pack("<II", len(reads), 1 if quals is not None else 0))
        for i, r in enumerate(reads):
            f.write(struct.pack("<I", len(names[i])) + names[i].encode() + struct.pack("<I", len(r)))
            f.write(np.asarray(r, dtype=np.uint8).tobytes())
            if quals is not None:
                f.write(np.asarray(quals[i], dtype=np.uint8).tobytes())
        f.write(np.asarray(off, dtype=np.uint64).tobytes())
        f.write(np.ascontiguousarray(alns).tobytes())
        n_ops = int(sum(int(a["n_ops"]) for a in alns))
        f.write(struct.pack("<Q", n_ops) + np.asarray(ops[:2 * n_ops], dtype=np.uint64).tobytes())
    out = os.path.join(str(tmp), "yard.sam")
    p = subprocess.run([build_exe(), "dump", path, out, str(options)], stdout=subprocess.PIPE)
    if p.returncode == 3:
        text = p.stdout.decode().strip()
        assert text.startswith("ERROR: ")
        return text[len("ERROR: "):]
    assert p.returncode == 0
    return np.fromfile(out + ".off", dtype=np.uint64), open(out, "rb").read()


class Ctx:
    """an index with contig names, and what the yardstick needs of it"""

    def __init__(self, g, contig_names):
        import ma_amd
        self.g, self.contig_names = g, contig_names
        self.idx = ma_amd.Index.build(g)
        self.idx.set_contig_names(contig_names)
        self.lens = [len(c) for c in g]
        self.starts = [int(x) for x in np.concatenate([[0], np.cumsum(self.lens)[:-1]])]
        self.F = sum(self.lens)

    def batch(self, P, reads, names, quals):
        import ma_amd
        b = ma_amd.Batch(self.idx, P, max(len(reads), 1), sum(len(r) for r in reads) + 64)
        b.set_reads(reads)
        b.set_read_text(names, quals)
        return b

    def check(self, tmp, b, reads, names, quals, options):
        """device text and offsets == the yardstick's on the device's own MappingQuality records; returns those records"""
        off, alns, ops = b.mapq_alignments()
        for opt in options:
            nb = b.sam(opt)
            roff, text = b.sam_text()
            woff, want = yardstick(tmp, self.contig_names, self.starts, self.lens, names, reads, quals, off, alns, ops, opt)
            assert text == want, "options %d: first difference at byte %d" % (
                opt, next((i for i, (x, y) in enumerate(zip(text, want)) if x != y), min(len(text), len(want))))
            assert np.array_equal(roff, woff) and nb == len(want) == int(roff[-1])
        return off, alns, ops


def params(preset="default", **changed):
    import ma_amd
    P = ma_amd.Params.preset(preset)
    P.srand_seed = 1
    for k, v in changed.items():
        setattr(P, k, v)
    return P


@pytest.fixture(scope="module")
def small(tmp_path_factory, gpu_device):
    g, reads, names = read_case(gunzip_to(os.path.join(G, "small.case.gz"), str(tmp_path_factory.mktemp("sam") / "small.case")))
    ctx = Ctx(g, names)
    yield ctx, reads
    ctx.idx.close()


@pytest.mark.parametrize("preset,opt", [("default", 0), ("default", 1), ("default", 2), ("default", 3), ("illumina", 0)])
def test_small_case_against_the_reference_goldens(small, preset, opt):
    """small.case aligned and printed on the device: the record lines of the text the reference's FileWriter wrote"""
    ctx, reads = small
    want = b"".join(l for l in gzip.open(os.path.join(G, "small_ref.%s.opt%d.sam.gz" % (preset, opt)), "rb").read().splitlines(True)
                    if not l.startswith(b"@"))
    b = ctx.batch(params(preset), reads, ["r%d" % i for i in range(len(reads))], None)
    b.align()
    assert b.sam(opt) == len(want)
    off, text = b.sam_text()
    assert text == want
    # rec_off cuts the text at record boundaries, one range per read, every range starting with the read's name
    assert int(off[0]) == 0 and int(off[-1]) == len(want) and np.all(np.diff(off.astype(np.int64)) > 0)
    for r in (0, 1, len(reads) - 1):
        assert text[int(off[r]):int(off[r + 1])].startswith(b"r%d\t" % r) and text[int(off[r + 1]) - 1:int(off[r + 1])] == b"\n"
    b.close()


# ---- a random genome: two contigs of 300 kb with a repeat family ----------------------------------------------------------
MIXED = dict(seed=41, contig_lens=[300000, 290000], repeat_unit=500, repeat_copies=8, repeat_div=0.01)


def mixed_genome():
    return rand_genome(MIXED["seed"], MIXED["contig_lens"], repeat_unit=MIXED["repeat_unit"], repeat_copies=MIXED["repeat_copies"],
                       repeat_div=MIXED["repeat_div"])


def chimeric_reads(g, n, seed):
    """2 kb reads of two 1 kb pieces from different places, the second on the other strand: a primary and a supplementary"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        p, q = int(rng.integers(0, len(g[0]) - 1000)), int(rng.integers(0, len(g[1]) - 1000))
        a, c = g[0][p:p + 1000], g[1][q:q + 1000]
        rd = np.concatenate([a, revcomp(c)])
        out.append(revcomp(rd) if i % 2 else rd)
    return out


@pytest.fixture(scope="module")
def mixed(gpu_device):
    g = mixed_genome()
    ctx = Ctx(g, ["ctgA", "ctgB"])
    yield ctx
    ctx.idx.close()


def record_stats(off, alns, F):
    n = len(off) - 1
    per_read = np.diff(off.astype(np.int64))
    return dict(records=len(alns), reverse=int(np.sum(alns["begin_ref"] >= F)), secondary=int(np.sum(alns["secondary"] != 0)),
                supplementary=int(np.sum(alns["supplementary"] != 0)), unaligned=int(np.sum(per_read == 0)),
                aligned=int(np.sum(per_read > 0)), reads=n)


def test_random_genome_every_option_bit(tmp_path, mixed):
    """~400 reads -- 150 bp on both strands, some with N, 20 random ones, 12 chimeric 2 kb reads under pacbio, a run with
    report_n_best 3 -- with and without qualities under every option bit, against FileWriter on the device's records; the
    records hold what makes the comparison mean something"""
    ctx = mixed
    short = (sample_reads(ctx.g, 300, 150, 42, sub=0.01) + sample_reads(ctx.g, 60, 150, 43, sub=0.04, n_rate=0.02)
             + sample_reads(ctx.g, 20, 150, 44, random_frac=1.0))
    # reads out of the repeat family (the unit sits in the genome 8 times): secondaries under report_n_best
    unit_at = find_repeat(ctx.g)
    rep = [ctx.g[c][p + 20 * i:p + 20 * i + 150].copy() for i, (c, p) in enumerate(unit_at * 2)][:16]
    runs = [("default", params("default"), short, True), ("default, no qualities", params("default"), short[:120], False),
            ("pacbio", params("pacbio"), chimeric_reads(ctx.g, 12, 47), True),
            ("n best 3", params("default", report_n_best=3), rep + short[:40], True)]
    total = dict(records=0, reverse=0, secondary=0, supplementary=0, unaligned=0, aligned=0, reads=0)
    for name, P, reads, with_q in runs:
        names = ["%s:%d" % (name.split(",")[0].replace(" ", "_"), i) for i in range(len(reads))]
        quals = make_quals(reads, 48) if with_q else None
        b = ctx.batch(P, reads, names, quals)
        b.align()
        off, alns, _ = ctx.check(tmp_path, b, reads, names, quals, ALL_BITS)
        st = record_stats(off, alns, ctx.F)
        print(name, st)
        for k in total:
            total[k] += st[k]
        b.close()
    print("total", total)
    assert total["reads"] >= 400
    assert total["reverse"] >= 0.3 * total["records"]
    assert total["secondary"] >= 5 and total["supplementary"] >= 5 and total["unaligned"] >= 5
    assert total["aligned"] >= 0.8 * total["reads"]


def find_repeat(g):
    """(contig, position) of the copies of the repeat unit: the draws of rand_genome replayed (no search through the genome)"""
    rng = np.random.default_rng(MIXED["seed"])
    for l in MIXED["contig_lens"]:
        rng.integers(0, 4, size=int(l), dtype=np.uint8)
    u = MIXED["repeat_unit"]
    unit = rng.integers(0, 4, size=u, dtype=np.uint8)
    at = []
    for _ in range(MIXED["repeat_copies"]):
        c = int(rng.integers(0, len(MIXED["contig_lens"])))
        at.append((c, int(rng.integers(0, MIXED["contig_lens"][c] - u))))
        mut = rng.random(u) < MIXED["repeat_div"]
        rng.integers(1, 4, size=int(mut.sum()), dtype=np.uint8)
    at = sorted(cp for cp in at if np.mean(g[cp[0]][cp[1]:cp[1] + u] == unit) > 0.9)  # (a later copy may overlap an earlier one)
    assert len(at) >= 4, "the replay does not find the repeat family of the genome"
    return at


def test_every_read_length_in_one_batch(tmp_path, mixed):
    """error-free reads of every length around the wavefront's stride of 64, both strands, in one batch: the cooperative SEQ /
    QUAL copy meets every tail and, behind names of varying length, every misaligned output offset"""
    ctx = mixed
    rng = np.random.default_rng(50)
    reads = []
    for rep in range(6):
        for L in LENGTHS:
            c = ctx.g[rep % 2]
            p = int(rng.integers(0, len(c) - L))
            rd = c[p:p + L].copy()
            reads.append(revcomp(rd) if (rep + L) % 2 else rd)
    names = ["q" * (1 + i % 7) + str(i) for i in range(len(reads))]
    quals = make_quals(reads, 51)
    b = ctx.batch(params("default"), reads, names, quals)
    b.align()
    off, alns, _ = ctx.check(tmp_path, b, reads, names, quals, [0, 1, 2])
    st = record_stats(off, alns, ctx.F)
    print(st)
    assert st["aligned"] >= 6 * 7 and st["unaligned"] >= 6 * 4 and st["reverse"] >= 10  # 63 bases and more align, 5 and fewer do not
    b.close()


# ---- injected alignments ----------------------------------------------------------------------------------------------------
def single_base_ops(n):
    t = np.array([(3 if j % 8 == 3 else 4) if j % 4 == 3 else j % 4 for j in range(n)], dtype=np.uint64)
    ops = np.empty(2 * n, dtype=np.uint64)
    ops[0::2], ops[1::2] = t, 1
    return ops, int(np.sum(t != 4)), int(np.sum(t != 3))


def one_alignment(begin_ref, rlen, begin_q, end_q, n_ops, score=5000):
    import ma_amd
    a = np.zeros(1, dtype=ma_amd.ALIGNMENT_DT)
    a["begin_ref"], a["end_ref"], a["begin_q"], a["end_q"], a["score"], a["n_ops"] = begin_ref, begin_ref + rlen, begin_q, end_q, score, n_ops
    return a


@pytest.mark.parametrize("n_ops", [65535, 65536])
@pytest.mark.parametrize("rev", [False, True], ids=["forward", "reverse"])
def test_long_cigar_and_cg_tag(tmp_path, mixed, n_ops, rev):
    """one 70 kb read with 65 535 / 65 536 single-base ops through ma_batch_set_alignments: the CG:B:I tag appears from 0x10000 ops
    on and MA_SAM_NO_CG_TAG switches it off"""
    ctx = mixed
    ops, qlen, rlen = single_base_ops(n_ops)
    read = np.resize(ctx.g[0][1000:71000], 70000).copy()
    begin_ref = 2 * ctx.F - (5000 + rlen) if rev else 5000
    b = ctx.batch(params("default"), [read], ["long"], make_quals([read], 52))
    b.set_alignments([0, 1], one_alignment(begin_ref, rlen, 100, 100 + qlen, n_ops), ops)
    ctx.check(tmp_path, b, [read], ["long"], make_quals([read], 52), [0, 16, 2, 19])
    b.sam(0)
    assert (b"\tCG:B:I," in b.sam_text()[1]) == (n_ops >= 0x10000)
    b.sam(16)
    assert b"\tCG:B:I," not in b.sam_text()[1]
    b.close()


def test_zero_length_alignments_and_a_record_beyond_its_read(tmp_path, mixed):
    """a list of zero-length alignments only prints the unmapped record with MAPQ 0; a record whose end_q lies beyond the read fails
    the call with the host formatter's text -- on either strand -- and the next call on the object works"""
    import ma_amd
    ctx = mixed
    reads = [ctx.g[0][2000:2150].copy(), ctx.g[1][3000:3150].copy()]
    names, quals = ["z", "ok"], make_quals(reads, 53)
    b = ctx.batch(params("default"), reads, names, quals)
    alns = np.concatenate([one_alignment(2000, 0, 10, 10, 2), one_alignment(9000, 0, 0, 0, 0), one_alignment(ctx.lens[0] + 3000, 150, 0, 150, 1)])
    alns["ops_off"] = [0, 2, 2]
    ops = np.array([0, 0, 4, 0, 0, 150], dtype=np.uint64)
    b.set_alignments([0, 2, 3], alns, ops)
    ctx.check(tmp_path, b, reads, names, quals, [0, 1, 12])
    b.sam(0)
    text = b.sam_text()[1]
    assert text.startswith(b"z\t4\t*\t0\t0\t*\t*\t0\t0\t") and text.count(b"\n") == 2
    for rev in (False, True):
        bad = one_alignment(2 * ctx.F - 2150 if rev else 2000, 150, 120, 153, 1)
        b.set_alignments([0, 1, 1], bad, np.array([0, 33], dtype=np.uint64))
        off, malns, mops = b.mapq_alignments()
        assert len(malns) == 1 and int(malns[0]["end_q"]) == 153
        want = yardstick(tmp_path, ctx.contig_names, ctx.starts, ctx.lens, names, reads, quals, off, malns, mops, 0)
        assert want == ("Index out of range (compCharAt)" if rev else "Query length is off by -3.")
        with pytest.raises(ma_amd.MaError) as e:
            b.sam(0)
        assert str(e.value) == want
        with pytest.raises(ma_amd.MaError, match="run ma_sam_batch first"):
            b.sam_text()
        ctx.check(tmp_path, b, reads, names, quals, [1])  # soft clipping prints the whole read: no error, on the same object
    b.set_alignments([0, 2, 3], alns, ops)
    ctx.check(tmp_path, b, reads, names, quals, [0])
    b.close()


def test_empty_and_unaligned_batches(tmp_path, mixed):
    """an empty batch yields an empty text; reads without any alignment yield one unmapped record each (MAPQ text 255)"""
    import ma_amd
    ctx = mixed
    b = ma_amd.Batch(ctx.idx, params("default"), 8, 1024)  # (room for the reads set further down)
    b.set_reads([])
    b.set_read_text([], None)
    b.align()
    assert b.sam(0) == 0
    off, text = b.sam_text()
    assert text == b"" and list(off) == [0]
    rng = np.random.default_rng(54)
    reads = [rng.integers(0, 4, size=L, dtype=np.uint8) for L in (150, 1, 64, 65, 150)]
    names = ["u%d" % i for i in range(len(reads))]
    b.set_reads(reads)
    with pytest.raises(ma_amd.MaError, match="ma_batch_set_read_text"):  # setting reads dropped the text
        b.align()
        b.sam(0)
    for quals in (None, make_quals(reads, 55)):
        b.set_read_text(names, quals)
        off, alns, _ = ctx.check(tmp_path, b, reads, names, quals, [0, 1])
        assert len(alns) == 0
    assert b.sam_text()[1].count(b"\t4\t*\t0\t255\t") == len(reads)
    b.close()


def test_set_read_text_refuses_quality_strings_that_do_not_fit_their_reads(mixed):
    """the library copies one quality character per base: a string shorter or longer than its read is refused before the call"""
    import ma_amd
    ctx = mixed
    reads = [ctx.g[0][100:250].copy(), ctx.g[0][400:550].copy(), ctx.g[1][10:74].copy()]
    b = ma_amd.Batch(ctx.idx, params("default"), 3, 1024)
    b.set_reads(reads)
    quals = make_quals(reads, 56)
    for bad, n in ((quals[1][:-1], 149), (np.concatenate([quals[1], quals[1][:1]]), 151)):
        with pytest.raises(ma_amd.MaError, match="quality string 1 has %d characters, its read 150 bases" % n):
            b.set_read_text(["a", "b", "c"], [quals[0], bad, quals[2]])
    with pytest.raises(ma_amd.MaError, match="2 quality strings for 3 reads"):
        b.set_read_text(["a", "b", "c"], quals[:2])
    b.set_read_text(["a", "b", "c"], quals)
    b.close()


def test_downloads_and_two_batches_in_flight(tmp_path, mixed):
    """start_sam_download + finish_download == sam_text(); two batch objects on their own streams print what each prints alone;
    the MappingQuality records are the same before and after sam()"""
    import ma_amd
    ctx = mixed
    sets = [sample_reads(ctx.g, 200, 150, 60 + i, sub=0.02) for i in range(2)]
    alone = []
    for reads in sets:
        names = ["s%d" % i for i in range(len(reads))]
        b = ctx.batch(params("default"), reads, names, make_quals(reads, 62))
        b.align()
        before = b.mapq_alignments()
        b.sam(1)
        alone.append(b.sam_text())
        after = b.mapq_alignments()
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        harr = [ma_amd.HostArray(len(reads) + 1, np.uint64), ma_amd.HostArray(b.sam_bytes(), np.uint8)]
        assert b.start_sam_download(*harr) == len(alone[-1][1])
        b.finish_download()
        assert np.array_equal(harr[0].a, alone[-1][0]) and harr[1].a.tobytes() == alone[-1][1]
        for h in harr:
            h.close()
        b.close()
    streams, batches = [], []
    for reads in sets:
        s = C.c_void_p()
        assert ma_amd.lib().ma_stream_create(ctx.idx.h, C.byref(s)) == 0
        streams.append(s)
        b = ma_amd.Batch(ctx.idx, params("default"), len(reads), sum(len(r) for r in reads) + 64)
        b.set_stream(s.value)
        b.set_reads(reads)
        b.set_read_text(["s%d" % i for i in range(len(reads))], make_quals(reads, 62))
        batches.append(b)
    for b in batches:
        b.align()
    for b in batches:
        b.sam(1)
    for b, want in zip(batches, alone):
        off, text = b.sam_text()
        assert text == want[1] and np.array_equal(off, want[0])
    for b, s in zip(batches, streams):
        b.close()
        assert ma_amd.lib().ma_stream_destroy(ctx.idx.h, s) == 0


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


@pytest.mark.parametrize("fastq,bits,mix", [(True, 0, False), (False, 3, False), (True, 31, False), (True, 1, True)])
def test_execute_flat_sam_of_both_aligners_against_the_host_writer(tmp_path, gpu_device, fastq, bits, mix):
    """small.case in device batches of 37 reads, two in flight: BatchAligner::executeFlatSam and MultiDeviceAligner::executeFlatSam
    (two replicas on one device, second run) + BatchFileWriter::write give the file of executeFlat + the host formatter, in input
    order; every batch comes back as device text, except the one that mixes reads with and without qualities, which comes
    back as records; an executeFlat behind the SAM runs still yields its records"""
    exe = os.path.join(ROOT, "tests", "emul", "sam_graph_test")
    deps = [exe + ".cpp", os.path.join(ROOT, "ma_amd", "libma_amd.so")] + [os.path.join(ROOT, "ma_amd", "host", h) for h in os.listdir(
        os.path.join(ROOT, "ma_amd", "host")) if h.endswith(".h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "ma_amd", "host"), exe + ".cpp", "-o", exe, "-L" + os.path.join(ROOT, "ma_amd"),
                               "-lma_amd", "-Wl,-rpath," + os.path.join(ROOT, "ma_amd"), "-lpthread"])
    fa, rd, reads = write_small_case(tmp_path, fastq)
    out = str(tmp_path / "g")
    stats = subprocess.check_output([exe, fa, rd, out, "default", "37", "2", str(bits)] + (["mix"] if mix else [])).decode()
    n_batches = (len(reads) + 36) // 37
    assert n_batches >= 3
    assert '"reads": %d,' % len(reads) in stats and '"shards_used": 2' in stats
    # reads 0 .. 49 without qualities: batch 0 has none (served), batch 1 mixes (records), the others have them all
    assert '"text_batches": %d, "record_batches": %d' % ((n_batches - 1, 1) if mix else (n_batches, 0)) in stats
    want = open(out + ".flat.sam", "rb").read()
    assert want.count(b"\n") > len(reads)
    for leg in ("dev", "multi", "again"):
        assert open(out + ".%s.sam" % leg, "rb").read() == want, leg


@pytest.mark.parametrize("preset,fastq", [("default", True), ("default", False), ("illumina", True)])
def test_ma_align_writes_the_same_file_with_and_without_the_device_path(tmp_path, gpu_device, preset, fastq):
    """examples/ma_align on small.case (FASTQ: qualities, FASTA: none): the file written through BatchAligner::executeFlatSam +
    BatchFileWriter's one write per batch is, byte for byte, the file of --host-sam (BatchAligner::execute + FileWriter); its
    record lines are the reference's golden but for the quality column the golden's reads do not have"""
    exe = build_ma_align()
    fa, rd, reads = write_small_case(tmp_path, fastq)
    dev, host = str(tmp_path / "device.sam"), str(tmp_path / "host.sam")
    subprocess.check_call([exe, fa, rd, dev, preset])
    subprocess.check_call([exe, "--host-sam", fa, rd, host, preset])
    got, want = open(dev, "rb").read(), open(host, "rb").read()
    assert got == want and got.count(b"\n") > len(reads)
    golden = [l.split(b"\t") for l in gzip.open(os.path.join(G, "small_ref.%s.opt0.sam.gz" % preset), "rb").read().splitlines()
              if not l.startswith(b"@")]
    lines = [l.split(b"\t") for l in got.splitlines() if not l.startswith(b"@")]
    assert [l[:10] + l[11:] for l in lines] == [l[:10] + l[11:] for l in golden]
    assert all((l[10] != b"*") == fastq for l in lines if l[9] != b"*")
