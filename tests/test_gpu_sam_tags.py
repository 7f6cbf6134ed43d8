"""ma_sam_batch with MA_SAM_NGMLR_TAGS: the single-end SAM records of a batch with the NGMLR tag emulation (MD SV AS NM XI XE XR
CV SA QS QE) formatted on the device (ma_amd/csrc/stage_sam.h, k_sam_size<true> / k_sam_write<true>), through the C ABI /
ma_amd.api.  Every case compares the device's bytes and rec_off with a yardstick: the SAM goldens the compiled reference wrote
with the option on, or ma_amd's FileWriter with bEmulateNgmlrTags (ma_amd/host/ma_sam.h) run by
tests/emul/sam_tags_dev_test.cpp (mode `dump`) on the records the device itself reports, with the genome's bases and holes."""
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from ma_testlib import gunzip_to, read_case, revcomp
from test_gpu_sam import Ctx, LENGTHS, build_ma_align, chimeric_reads, make_quals, mixed_genome, params, write_small_case
from test_sam_tags_dev_host import build_exe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
TAGS = 32
TAG_BITS = [32, 33, 34, 36, 40, 48, 63]


def write_dump(path, ctx, names, reads, quals, off, alns, ops):
    """the records given, the genome's bases and the holes in the format sam_tags_dev_test reads"""
    with open(path, "wb") as f:
        f.write(b"MASAMT01" + struct.pack("<I", len(ctx.contig_names)))
        for nm, s, l in zip(ctx.contig_names, ctx.starts, ctx.lens):
            f.write(struct.pack("<I", len(nm)) + nm.encode() + struct.pack("<QQ", int(s), int(l)))
        f.write(struct.pack("<Q", ctx.F) + np.concatenate(ctx.g).astype(np.uint8).tobytes())
        f.write(struct.pack("<Q", len(ctx.holes)))
        for s, l in ctx.holes:
            f.write(struct.pack("<QQ", int(s), int(l)))
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
    return path


def read_dump(path):
    """a dump of `sam_tags_dev_test case`: (contig names, contigs, holes, read names, reads, quals, off, alns, ops)"""
    import ma_amd
    d = open(path, "rb").read()
    assert d[:8] == b"MASAMT01"
    at = [8]

    def take(fmt):
        v = struct.unpack_from("<" + fmt, d, at[0])
        at[0] += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def raw(n):
        at[0] += n
        return d[at[0] - n:at[0]]

    cnames, cstarts, clens = [], [], []
    for _ in range(take("I")):
        cnames.append(raw(take("I")).decode())
        s, l = take("QQ")
        cstarts.append(s), clens.append(l)
    genome = np.frombuffer(raw(take("Q")), dtype=np.uint8)
    holes = [take("QQ") for _ in range(take("Q"))]
    n, has_q = take("II")
    names, reads, quals = [], [], []
    for _ in range(n):
        names.append(raw(take("I")).decode())
        L = take("I")
        reads.append(np.frombuffer(raw(L), dtype=np.uint8).copy())
        if has_q:
            quals.append(np.frombuffer(raw(L), dtype=np.uint8).copy())
    off = np.frombuffer(raw(8 * (n + 1)), dtype=np.uint64).copy()
    alns = np.frombuffer(raw(int(off[-1]) * ma_amd.ALIGNMENT_DT.itemsize), dtype=ma_amd.ALIGNMENT_DT).copy()
    ops = np.frombuffer(raw(16 * take("Q")), dtype=np.uint64).copy()
    g = [genome[s:s + l].copy() for s, l in zip(cstarts, clens)]
    return cnames, g, holes, names, reads, quals if has_q else None, off, alns, ops


def yardstick(tmp, ctx, names, reads, quals, off, alns, ops, options):
    """FileWriter's (rec_off, text) per option for the records given; an exception comes back as its text (str)"""
    path = write_dump(os.path.join(str(tmp), "tags.dump"), ctx, names, reads, quals, off, alns, ops)
    res = []
    for opt in options:
        out = os.path.join(str(tmp), "yard.%d.sam" % opt)
        p = subprocess.run([build_exe(), "dump", path, out, str(opt)], stdout=subprocess.PIPE)
        if p.returncode == 3:
            text = p.stdout.decode().strip()
            assert text.startswith("ERROR: ")
            res.append(text[len("ERROR: "):])
            continue
        assert p.returncode == 0
        res.append((np.fromfile(out + ".off", dtype=np.uint64), open(out, "rb").read()))
    return res


class TagCtx(Ctx):
    """an index with contig names and holes"""

    def __init__(self, g, contig_names, holes):
        Ctx.__init__(self, g, contig_names)
        self.holes = [(int(s), int(l)) for s, l in holes]
        self.idx.set_holes([s for s, _ in self.holes], [l for _, l in self.holes])

    def check_tags(self, tmp, b, reads, names, quals, options):
        """device text and offsets == FileWriter's on the device's own MappingQuality records; returns the texts"""
        off, alns, ops = b.mapq_alignments()
        texts = []
        for opt, (woff, want) in zip(options, yardstick(tmp, self, names, reads, quals, off, alns, ops, options)):
            nb = b.sam(opt)
            roff, text = b.sam_text()
            assert text == want, "options %d: first difference at byte %d" % (
                opt, next((i for i, (x, y) in enumerate(zip(text, want)) if x != y), min(len(text), len(want))))
            assert np.array_equal(roff, woff) and nb == len(want) == int(roff[-1])
            texts.append(text)
        return texts


def text_census(text):
    lines = [l.split(b"\t") for l in text.splitlines()]
    mapped = [l for l in lines if not int(l[1]) & 4]
    return dict(records=len(mapped), reverse=sum(1 for l in mapped if int(l[1]) & 16), sa=text.count(b"\tSA:Z:"),
                md_deletion=sum(1 for l in mapped for t in l[11:] if t.startswith(b"MD:Z:") and b"^" in t),
                nm_above_0=sum(1 for l in mapped for t in l[11:] if t.startswith(b"NM:i:") and int(t[5:]) > 0),
                sv=sorted(set(int(m) for m in re.findall(rb"\tSV:i:(\d)", text))))


# ---- small.case against the goldens the reference wrote with the option on ----------------------------------------------------
@pytest.fixture(scope="module")
def small(tmp_path_factory, gpu_device):
    g, reads, names = read_case(gunzip_to(os.path.join(G, "small.case.gz"), str(tmp_path_factory.mktemp("samtags") / "small.case")))
    ctx = TagCtx(g, names, [])
    yield ctx, reads
    ctx.idx.close()


@pytest.mark.parametrize("preset,bits,opt", [("default", 32, 4), ("default", 33, 5), ("illumina", 32, 4)])
def test_small_case_with_tags_against_the_reference_goldens(small, preset, bits, opt):
    """small.case aligned and printed on the device with MA_SAM_NGMLR_TAGS: the record lines of the text the reference's
    FileWriter wrote under "Emulate NGMLR's tag output" """
    ctx, reads = small
    want = b"".join(l for l in gzip.open(os.path.join(G, "small_ref.%s.opt%d.sam.gz" % (preset, opt)), "rb").read().splitlines(True)
                    if not l.startswith(b"@"))
    b = ctx.batch(params(preset), reads, ["r%d" % i for i in range(len(reads))], None)
    b.align()
    assert b.sam(bits) == len(want)
    off, text = b.sam_text()
    assert text == want
    assert int(off[0]) == 0 and int(off[-1]) == len(want) and np.all(np.diff(off.astype(np.int64)) > 0)
    assert b"\tMD:Z:" in text and b"\tQE:i:" in text
    b.close()


# ---- aligned reads on a genome with holes -----------------------------------------------------------------------------------------
NOISY_AT = [(0, 50000, 2000), (0, 80000, 2000)]  # (contig, start, length) of the first two noisy reads: holes sit next to / in them


def noisy_reads(g, n, seed):
    """reads of 1 - 3 kb with 3 % substitutions, 2 % insertions and 2 % deletions, every other one on the reverse strand"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        c, p, L = NOISY_AT[i] if i < len(NOISY_AT) else (None, None, int(rng.integers(1000, 3001)))
        if c is None:
            c = int(rng.integers(0, len(g)))
            p = int(rng.integers(0, len(g[c]) - L))
        src = g[c][p:p + L].copy()
        sub = rng.random(L) < 0.03
        src[sub] = (src[sub] + rng.integers(1, 4, size=int(sub.sum()))) % 4
        keep = rng.random(L) >= 0.02
        ins = rng.random(L) < 0.02
        pieces = []
        for j in np.flatnonzero(ins | ~keep):  # (the few places that change the length)
            pieces.append(j)
        rd, last = [], 0
        for j in pieces:
            rd.append(src[last:j])
            if ins[j]:
                rd.append(rng.integers(0, 4, size=1, dtype=np.uint8))
            if keep[j]:
                rd.append(src[j:j + 1])
            last = j + 1
        rd.append(src[last:])
        rd = np.concatenate(rd).astype(np.uint8)
        out.append(revcomp(rd) if i % 2 else rd)
    return out


@pytest.fixture(scope="module")
def holey(gpu_device):
    g = mixed_genome()
    l0 = len(g[0])
    holes = [(40, 150), (NOISY_AT[0][1] - 120, 120), (NOISY_AT[1][1] + 500, 30), (l0 - 60, 60)]
    ctx = TagCtx(g, ["ctgA", "ctgB"], holes)
    yield ctx
    ctx.idx.close()


def length_reads(g):
    rng = np.random.default_rng(50)
    reads = []
    for rep in range(6):
        for L in LENGTHS:
            c = g[rep % 2]
            p = int(rng.integers(0, len(c) - L))
            rd = c[p:p + L].copy()
            reads.append(revcomp(rd) if (rep + L) % 2 else rd)
    return reads


@pytest.mark.parametrize("with_q", [True, False], ids=["qualities", "no_qualities"])
@pytest.mark.parametrize("kind", ["lengths", "chimeric", "noisy"])
def test_aligned_reads_with_tags_under_every_option_bit(tmp_path, holey, kind, with_q):
    """reads of 1 .. 257 bases on both strands (default), 64 chimeric 2 kb reads with a primary and a supplementary on opposite
    strands and 64 reads of 1 - 3 kb with substitutions, insertions and deletions (pacbio), on a genome with four holes: the
    device's text with tags under every option bit is FileWriter's on the device's own records; afterwards sam(0) on the same
    batch gives today's text"""
    ctx = holey
    if kind == "lengths":
        P, reads = params("default"), length_reads(ctx.g)
    elif kind == "chimeric":
        P, reads = params("pacbio"), chimeric_reads(ctx.g, 64, 47)
    else:
        P, reads = params("pacbio"), noisy_reads(ctx.g, 64, 48)
    names = ["%s:%d" % (kind, i) for i in range(len(reads))]
    quals = make_quals(reads, 49) if with_q else None
    b = ctx.batch(P, reads, names, quals)
    b.align()
    before = b.mapq_alignments()
    texts = ctx.check_tags(tmp_path, b, reads, names, quals, TAG_BITS)
    st = text_census(texts[0])
    print(kind, st)
    assert st["records"] >= 0.5 * len(reads)
    assert st["reverse"] >= 20 and st["records"] - st["reverse"] >= 20  # both strands
    if kind == "chimeric":
        assert st["sa"] >= 16
    if kind == "noisy":
        assert st["md_deletion"] >= 32 and st["nm_above_0"] >= 32
    after = b.mapq_alignments()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))  # the swap of insertions and deletions is a view
    ctx.check(tmp_path, b, reads, names, quals, [0])  # the yardstick without tags of test_gpu_sam.py
    b.close()


# ---- injected records: the deterministic cases of sam_tags_dev_test.cpp ---------------------------------------------------------
@pytest.fixture(scope="module")
def case_ctx(gpu_device):
    made = {}

    def get(cnames, g, holes):
        key = (len(g[0]), len(g[1]))
        if key not in made:
            made[key] = TagCtx(g, cnames, holes)
        assert all(np.array_equal(x, y) for x, y in zip(made[key].g, g))
        return made[key]
    yield get
    for c in made.values():
        c.idx.close()


def injected(tmp_path, case_ctx, name):
    path = str(tmp_path / (name + ".case.dump"))
    subprocess.check_call([build_exe(), "case", name, path])
    cnames, g, holes, names, reads, quals, off, alns, ops = read_dump(path)
    ctx = case_ctx(cnames, g, holes)
    # MappingQuality sorts a read's records by score: the case's order is kept by scores that fall along it
    for r in range(len(reads)):
        for i, k in enumerate(range(int(off[r]), int(off[r + 1]))):
            alns["score"][k] = 100000 - 1000 * i
    b = ctx.batch(params("pacbio"), reads, names, quals)
    b.set_alignments(off, alns, ops)
    return ctx, b, names, reads, quals, alns


@pytest.mark.parametrize("name,options", [("runs", [32, 33, 34]), ("sisters", [32, 33, 36, 40, 44]), ("span0", [32, 33]), ("edges", [32, 33]),
                                          ("long", [32, 48, 33])])
def test_injected_records_with_tags(tmp_path, case_ctx, name, options):
    """the deterministic cases through ma_batch_set_alignments: the four I/D runs on both strands, three-sister lists in which
    the swap shows in the sisters before a record only, records without reference / query bases (XI:f:-nan), records of 0x10000
    ops with and without MA_SAM_NO_CG_TAG, a record at begin_ref 10 and records around the holes"""
    ctx, b, names, reads, quals, alns = injected(tmp_path, case_ctx, name)
    moff, malns, _ = b.mapq_alignments()
    assert len(malns) == len(alns), "MappingQuality dropped records of the case"
    texts = ctx.check_tags(tmp_path, b, reads, names, quals, options)
    st = text_census(texts[0])
    print(name, st)
    if name == "runs":
        assert st["reverse"] == 6 and st["records"] == 12
    if name == "sisters":
        assert st["sa"] >= 3
    if name == "span0":
        assert b"\tXI:f:-nan\t" in texts[0]
    if name == "edges":
        assert {0, 1, 3} <= set(st["sv"]) or {0, 1, 2} <= set(st["sv"])
    if name == "long":
        assert texts[0].count(b"\tCG:B:I,") == 2 and b"\tCG:B:I," not in texts[1]
    b.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_records_the_tags_cannot_print_fail_the_call_and_leave_the_batch_usable(tmp_path, case_ctx):
    """a record across the two strands fails with the reference's text; ops that cover one reference base too many, or one too
    few, fail with the library's message naming the record; after each failure sam(32) on corrected records works on the same
    object, the MappingQuality records are what they were, and pair_sam(0) still works on a batch that has just served sam(32)"""
    import ma_amd
    ctx, b, names, reads, quals, alns = injected(tmp_path, case_ctx, "runs")
    n = len(reads)
    assert n % 2 == 0
    off = np.arange(n + 1, dtype=np.uint64)
    good = np.zeros(n, dtype=ma_amd.ALIGNMENT_DT)
    good["begin_ref"] = 300 + 10 * np.arange(n)
    good["end_ref"] = good["begin_ref"] + 30
    good["end_q"], good["score"], good["n_ops"], good["ops_off"] = 30, 5000, 1, np.arange(n)
    ops = np.tile(np.array([1, 30], dtype=np.uint64), n)
    F = ctx.F
    cases = []
    bad = good.copy()
    bad["begin_ref"][3], bad["end_ref"][3] = F - 10, F + 20
    cases.append((bad, ops, r"^\(vExtractSubsection\) Try to extract bridging sequence\. This is impossible\.$"))
    bad = good.copy()
    bad["end_ref"][5] -= 1  # the ops cover one reference base too many
    cases.append((bad, ops, r"record 0 of read 5: the ops do not cover"))
    bad = good.copy()
    bad["end_ref"][6] += 1  # one too few
    cases.append((bad, ops, r"record 0 of read 6: the ops do not cover"))
    for bad, bops, msg in cases:
        b.set_alignments(off, bad, bops)
        before = b.mapq_alignments()
        with pytest.raises(ma_amd.MaError, match=msg):
            b.sam(TAGS)
        with pytest.raises(ma_amd.MaError, match="run ma_sam_batch first"):
            b.sam_text()
        after = b.mapq_alignments()
        assert all(np.array_equal(x, y) for x, y in zip(before, after))
        b.set_alignments(off, good, ops)
        ctx.check_tags(tmp_path, b, reads, names, quals, [TAGS])
    with pytest.raises(ma_amd.MaError, match="sorted, not overlapping"):
        ctx.idx.set_holes([100, 90], [20, 5])
    with pytest.raises(ma_amd.MaError, match="not inside the forward strand"):
        ctx.idx.set_holes([F - 5], [6])
    ctx.idx.set_holes([s for s, _ in ctx.holes], [l for _, l in ctx.holes])
    b.pair()
    assert b.pair_sam(0) > 0
    b.close()


# ---- the float arithmetic and the %f formatter of XI / CV on the device -----------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1], ids=["XI", "CV"])
def test_xi_and_cv_texts_of_the_device(gpu_device, kind):
    """ma_debug_ngmlr_floats over 1 M seeded (num, den) pairs and all num <= den <= 4096: the device's text is '%f' of the same
    arithmetic in numpy.float32 (u64 -> float, one multiplication by 100 for CV, one division)"""
    import ma_amd
    rng = np.random.default_rng(90 + kind)
    den = np.repeat(np.arange(1, 4097, dtype=np.uint64), np.arange(2, 4098))
    num = np.concatenate([np.arange(0, d + 1, dtype=np.uint64) for d in range(1, 4097)])
    n = 1000000
    # read-like magnitudes, mostly num <= den; one in eight pairs of any 40 bits
    rden = rng.integers(1, 1 << 20, size=n).astype(np.uint64)
    rnum = (rng.random(n) * (rden + 1)).astype(np.uint64)
    wild = rng.random(n) < 0.125
    rden[wild] = rng.integers(1, 1 << 40, size=int(wild.sum())).astype(np.uint64)
    rnum[wild] = rng.integers(0, 1 << 40, size=int(wild.sum())).astype(np.uint64)
    num, den = np.concatenate([num, rnum]), np.concatenate([den, rden])
    got = ma_amd.debug_ngmlr_floats(kind, num, den)
    fnum = num.astype(np.float32)
    if kind:
        fnum = np.float32(100.0) * fnum
    want = fnum / den.astype(np.float32)
    assert want.dtype == np.float32
    fits = want < 1e8  # (a slot holds 15 characters)
    wtext = np.char.mod("%f", want.astype(np.float64)).astype("S16")
    bad = np.flatnonzero((got != wtext) & fits)
    assert len(bad) == 0, "%d differ, first: %d / %d -> %r, want %r" % (len(bad), num[bad[0]], den[bad[0]], got[bad[0]], wtext[bad[0]])
    assert np.all(got[~fits] == b"") and fits.sum() > 0.99 * len(fits)
    assert ma_amd.debug_ngmlr_floats(kind, [0, 5], [0, 0]).tolist() == [b"-nan", b"inf"]


# ---- through the host layer ---------------------------------------------------------------------------------------------------
def build_graph_exe():
    exe = os.path.join(ROOT, "tests", "emul", "sam_tags_graph_test")
    deps = [exe + ".cpp", os.path.join(ROOT, "ma_amd", "libma_amd.so")] + [os.path.join(ROOT, "ma_amd", "host", h) for h in os.listdir(
        os.path.join(ROOT, "ma_amd", "host")) if h.endswith(".h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "ma_amd", "host"), exe + ".cpp", "-o", exe, "-L" + os.path.join(ROOT, "ma_amd"),
                               "-lma_amd", "-Wl,-rpath," + os.path.join(ROOT, "ma_amd"), "-lpthread"])
    return exe


@pytest.mark.parametrize("bits", [32, 63 - 12])
def test_execute_flat_sam_of_both_aligners_with_tags_against_the_host_writer(tmp_path, gpu_device, bits):
    """the reads of the aligned-reads test (pacbio) in device batches of 70, two in flight, on a pack with the four holes:
    BatchAligner::executeFlatSam and MultiDeviceAligner::executeFlatSam (two replicas on one device, second run) +
    BatchFileWriter::write give the file FileWriter writes from execute( )'s containers; every batch comes back as device text
    made with the tag bit, and a writer without the option refuses it"""
    g = mixed_genome()
    holes = [(40, 150), (NOISY_AT[0][1] - 120, 120), (NOISY_AT[1][1] + 500, 30), (len(g[0]) - 60, 60)]
    reads = length_reads(g) + chimeric_reads(g, 64, 47) + noisy_reads(g, 64, 48)
    quals = make_quals(reads, 49)
    fa, fq = str(tmp_path / "genome.fa"), str(tmp_path / "reads.fq")
    with open(fa, "w") as f:
        for nm, c in zip(["ctgA", "ctgB"], g):
            f.write(">%s\n%s\n" % (nm, "".join("ACGT"[int(x)] for x in c)))
    with open(fq, "w") as f:
        for i, (r, q) in enumerate(zip(reads, quals)):
            f.write("@q%d\n%s\n+\n%s\n" % (i, "".join("ACGT"[int(x)] for x in r), q.tobytes().decode()))
    out = str(tmp_path / "g")
    stats = subprocess.check_output([build_graph_exe(), fa, fq, out, "pacbio", "70", "2", str(bits)] +
                                    [str(v) for h in holes for v in h]).decode()
    n_batches = (len(reads) + 69) // 70
    assert n_batches >= 3
    assert '"reads": %d,' % len(reads) in stats and '"shards_used": 2' in stats
    assert '"text_batches": %d, "record_batches": 0' % (2 * n_batches) in stats
    want = open(out + ".host.sam", "rb").read()
    assert want.count(b"\n") > len(reads) and b"\tSA:Z:" in want and b"\tMD:Z:" in want
    for leg in ("dev", "multi"):
        assert open(out + ".%s.sam" % leg, "rb").read() == want, leg


def test_ma_align_with_ngmlr_tags_writes_the_golden(tmp_path, gpu_device):
    """examples/ma_align --ngmlr-tags on small.case (FASTA reads): the device path writes the file the reference wrote with
    "Emulate NGMLR's tag output", header included, and --host-sam (BatchAligner::execute + FileWriter) the same bytes.  (The
    golden came from the reference's stream constructor, which separates SN and LN of an @SQ line by a blank; ma_align opens
    its file by name, and that constructor writes a tab there (sic, fileWriter.h:385-422): the one difference allowed for.)"""
    exe = build_ma_align()
    fa, rd, reads = write_small_case(tmp_path, False)
    dev, host = str(tmp_path / "device.sam"), str(tmp_path / "host.sam")
    subprocess.check_call([exe, "--ngmlr-tags", fa, rd, dev, "default"])
    subprocess.check_call([exe, "--ngmlr-tags", "--host-sam", fa, rd, host, "default"])
    want = gzip.open(os.path.join(G, "small_ref.default.opt4.sam.gz"), "rb").read()
    want = b"".join(l.replace(b" LN:", b"\tLN:") if l.startswith(b"@SQ") else l for l in want.splitlines(True))
    assert want.startswith(b"@SQ\tSN:") and open(dev, "rb").read() == want
    assert open(host, "rb").read() == want
