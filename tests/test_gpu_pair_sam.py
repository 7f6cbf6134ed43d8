"""ma_pair_sam_batch: the paired-end SAM records of a batch formatted on the device (ma_amd/csrc/stage_pair_sam.h), through the
C ABI / ma_amd.api.  Every case compares the device's bytes and pair_off with a yardstick: the SAM golden the compiled reference's
PairedFileWriter wrote, or ma_amd's PairedFileWriter (ma_amd/host/ma_sam.h) run by tests/emul/sam_pair_dev_test.cpp (mode `dump`) on
the pair records the device itself reports (pairs())."""
import ctypes as C
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

from ma_testlib import gunzip_to, rand_genome, read_case, revcomp, sample_pairs, write_case
from test_gpu_sam import ALL_BITS, LENGTHS, MIXED, Ctx, make_quals, one_alignment, params, single_base_ops
from test_sam_pair_dev_host import PAIR_GOLDEN, build_exe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
# the genome of test_gpu_sam.py with a repeat family long enough (700, exact copies) to hold both mates of a pair
PAIRED = dict(MIXED, repeat_unit=700, repeat_div=0.0)
SEEDS = dict(pairs=77, random_mates=78, quals=79)


def yardstick(tmp, ctx, names, reads, quals, res, options):
    """PairedFileWriter's (pair_off, text) for the arrays of pairs(); a formatter exception comes back as its text (str)"""
    off, alns, ops, mate, other = res
    path = os.path.join(str(tmp), "pair_sam.dump")
    with open(path, "wb") as f:
        f.write(b"MASAMP01" + struct.pack("<I", len(ctx.contig_names)))
        for nm, s, l in zip(ctx.contig_names, ctx.starts, ctx.lens):
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
        f.write(np.asarray(mate, dtype=np.int32).tobytes() + np.asarray(other, dtype=np.int32).tobytes())
    out = os.path.join(str(tmp), "yard.sam")
    p = subprocess.run([build_exe(), "dump", path, out, str(options)], stdout=subprocess.PIPE)
    if p.returncode == 3:
        text = p.stdout.decode().strip()
        assert text.startswith("ERROR: ")
        return text[len("ERROR: "):]
    assert p.returncode == 0
    return np.fromfile(out + ".off", dtype=np.uint64), open(out, "rb").read()


def check(tmp, ctx, b, reads, names, quals, options):
    """device text and offsets == the yardstick's on the device's own pair records; returns the text of the last option set"""
    res = b.pairs()
    text = b""
    for opt in options:
        nb = b.pair_sam(opt)
        poff, text = b.pair_sam_text()
        woff, want = yardstick(tmp, ctx, names, reads, quals, res, opt)
        assert text == want, "options %d: first difference at byte %d" % (
            opt, next((i for i, (x, y) in enumerate(zip(text, want)) if x != y), min(len(text), len(want))))
        assert np.array_equal(poff, woff) and nb == len(want) == int(poff[-1]) == b.pair_sam_bytes()
    return text


def paired_batch(ctx, P, reads, names, quals):
    b = ctx.batch(P, reads, names, quals)
    b.align()
    b.pair()
    return b


def text_stats(poff, text):
    """what the text of option set 0 holds, per pair and per record"""
    st = dict(pairs=len(poff) - 1, two_records=0, one_unaligned=0, both_unaligned=0, mate_reverse=0, rnext_named=0, rnext_same=0)
    for k in range(len(poff) - 1):
        lines = [l.split(b"\t") for l in text[int(poff[k]):int(poff[k + 1])].splitlines()]
        flags = [int(l[1]) for l in lines]
        unaligned = sum(1 for f in flags if f & 4)
        assert len(lines) >= 2 and unaligned <= 2
        st[("two_records", "one_unaligned", "both_unaligned")[unaligned]] += 1
        st["mate_reverse"] += sum(1 for f in flags if f & 0x20)
        st["rnext_named"] += sum(1 for l in lines if l[6] not in (b"=", b"*"))
        st["rnext_same"] += sum(1 for l in lines if l[6] == b"=")
    return st


# ---- 1. the golden -----------------------------------------------------------------------------------------------------------
def test_golden_case_against_the_reference_golden(tmp_path, gpu_device):
    """f4.case as one batch under illumina, options 3: the record lines of the text the reference's PairedFileWriter wrote;
    pair_off cuts it at pair boundaries"""
    g, reads, names = read_case(gunzip_to(os.path.join(G, "f4.case.gz"), str(tmp_path / "f4.case")))
    reads = reads[:len(reads) // 2 * 2]
    want = b"".join(l for l in gzip.open(os.path.join(G, PAIR_GOLDEN + ".sam.gz"), "rb").read().splitlines(True) if not l.startswith(b"@"))
    ctx = Ctx(g, names)
    b = paired_batch(ctx, params("illumina"), reads, ["r%d" % i for i in range(len(reads))], None)
    assert b.pair_sam(3) == len(want)
    off, text = b.pair_sam_text()
    assert text == want
    assert len(off) == len(reads) // 2 + 1 and int(off[0]) == 0 and int(off[-1]) == len(want) and np.all(np.diff(off.astype(np.int64)) > 0)
    for k in range(len(reads) // 2):
        lines = text[int(off[k]):int(off[k + 1])].splitlines(True)
        assert len(lines) >= 2 and all(l.endswith(b"\n") and l.split(b"\t")[0] in (b"r%d" % (2 * k), b"r%d" % (2 * k + 1)) for l in lines)
    b.close()
    ctx.idx.close()


# ---- 2. every shape and option bit -------------------------------------------------------------------------------------------
def find_repeat(g):
    """(contig, position) of the copies of the repeat unit: the draws of rand_genome replayed (no search through the genome)"""
    rng = np.random.default_rng(PAIRED["seed"])
    for l in PAIRED["contig_lens"]:
        rng.integers(0, 4, size=int(l), dtype=np.uint8)
    u = PAIRED["repeat_unit"]
    unit = rng.integers(0, 4, size=u, dtype=np.uint8)
    at = []
    for _ in range(PAIRED["repeat_copies"]):
        c = int(rng.integers(0, len(PAIRED["contig_lens"])))
        at.append((c, int(rng.integers(0, PAIRED["contig_lens"][c] - u))))
        mut = rng.random(u) < PAIRED["repeat_div"]
        rng.integers(1, 4, size=int(mut.sum()), dtype=np.uint8)
    at = sorted(cp for cp in at if np.array_equal(g[cp[0]][cp[1]:cp[1] + u], unit))  # (a later copy may overlap an earlier one)
    assert len(at) >= 4, "the replay does not find the repeat family of the genome"
    return at


def shapes_input():
    """the genome and the two runs of test 2: (name, changed parameters, reads)"""
    g = rand_genome(PAIRED["seed"], PAIRED["contig_lens"], repeat_unit=PAIRED["repeat_unit"], repeat_copies=PAIRED["repeat_copies"],
                    repeat_div=PAIRED["repeat_div"])
    pairs = sample_pairs(g, 600, 150, SEEDS["pairs"], far_frac=0.1, same_strand_frac=0.05, random_mate_frac=0.08)
    rng = np.random.default_rng(SEEDS["random_mates"])
    rand = [rng.integers(0, 4, size=150, dtype=np.uint8) for _ in range(16)]
    rep = []
    # 8 pairs with both mates inside one copy of the unit, on opposite strands (the copies are exact and lie on both contigs:
    # the proper candidates tie); 8 pairs on ONE strand -- no candidate is proper -- whose second mate reaches out of its copy
    # into the flank and so has one best place, while the first mate's best places tie: partners on different contigs
    for i, (c, p) in enumerate((find_repeat(g) * 2)[:16]):
        m1 = g[c][p + 10 * i:p + 10 * i + 150].copy()
        m2 = revcomp(g[c][p + 10 * i + 250:p + 10 * i + 400]) if i < 8 else g[c][p + 625:p + 775].copy()
        rep += [m1, m2] if i % 2 == 0 else [revcomp(m2), revcomp(m1)]
    return g, [("paired", {}, pairs + rand), ("n_best_3", dict(report_n_best=3), rep)]


@pytest.fixture(scope="module")
def shapes(gpu_device):
    g, runs = shapes_input()
    ctxs = {"two_names": Ctx(g, ["ctgA", "ctgB"]), "same_name": Ctx(g, ["ctg", "ctg"])}
    yield ctxs, runs
    for c in ctxs.values():
        c.idx.close()


@pytest.mark.parametrize("index", ["two_names", "same_name"])
@pytest.mark.parametrize("with_quals", [True, False], ids=["qualities", "no-qualities"])
def test_every_record_shape_and_option_bit(tmp_path, shapes, index, with_quals):
    """600 sampled pairs (far, same-strand and random mates among them), 8 pairs of two random mates, 16 pairs out of the repeat
    family under report_n_best 3, names of varying length, under every option bit against PairedFileWriter on the device's
    pair records; the text holds what makes the comparison mean something.  On the index whose two contigs share a name every
    RNEXT is "=" (the names are compared, not the ids)."""
    ctxs, runs = shapes
    ctx = ctxs[index]
    total = None
    for name, changed, reads in runs:
        names = ["q" * (1 + i % 7) + "%s:%d" % (name, i) for i in range(len(reads))]
        quals = make_quals(reads, SEEDS["quals"]) if with_quals else None
        b = paired_batch(ctx, params("illuminapaired", **changed), reads, names, quals)
        check(tmp_path, ctx, b, reads, names, quals, ALL_BITS)
        b.pair_sam(0)
        st = text_stats(*b.pair_sam_text())
        print(index, name, st)
        total = st if total is None else {k: total[k] + st[k] for k in st}
        b.close()
    print(index, "total", total)
    assert total["pairs"] >= 600
    assert total["two_records"] >= 5 and total["one_unaligned"] >= 5 and total["both_unaligned"] >= 5 and total["mate_reverse"] >= 5
    if index == "two_names":
        assert total["rnext_named"] >= 5
    else:
        assert total["rnext_named"] == 0 and total["rnext_same"] >= 5


# ---- 3. wavefront edges --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(gpu_device):
    g = rand_genome(PAIRED["seed"], PAIRED["contig_lens"], repeat_unit=PAIRED["repeat_unit"], repeat_copies=PAIRED["repeat_copies"],
                    repeat_div=PAIRED["repeat_div"])
    ctx = Ctx(g, ["ctgA", "ctgB"])
    yield ctx
    ctx.idx.close()


def edge_pairs(g, n):
    """error-free pairs, mate lengths LENGTHS[i] / another one, outer distance 600, both arrangements"""
    rng = np.random.default_rng(90)
    reads = []
    for i in range(n):
        l1 = LENGTHS[i % len(LENGTHS)]
        l2 = LENGTHS[(i + 1 + (i // len(LENGTHS)) % (len(LENGTHS) - 1)) % len(LENGTHS)]
        assert l1 != l2
        c = g[i % 2]
        p = int(rng.integers(0, len(c) - 600))
        m1, m2 = c[p:p + l1].copy(), revcomp(c[p + 600 - l2:p + 600])
        reads += [m1, m2] if i % 4 < 2 else [revcomp(m2), revcomp(m1)]
    return reads


@pytest.mark.parametrize("n_pairs", [1, 63, 64, 65, 129])
def test_wavefront_edges(tmp_path, mixed, n_pairs):
    """error-free pairs of every mate length around the stride of 64, the two mates of a pair of different lengths, both strand
    arrangements, in batches that end before, at and behind a wavefront's 64 pairs"""
    ctx = mixed
    reads = edge_pairs(ctx.g, 129)[:2 * n_pairs]
    names = ["e" * (1 + i % 5) + str(i) for i in range(len(reads))]
    quals = make_quals(reads, 91)
    b = paired_batch(ctx, params("illuminapaired"), reads, names, quals)
    check(tmp_path, ctx, b, reads, names, quals, [0, 1, 2])
    b.pair_sam(0)
    st = text_stats(*b.pair_sam_text())
    print(st)
    assert st["pairs"] == n_pairs
    if n_pairs >= 63:
        assert st["two_records"] >= 10 and st["one_unaligned"] + st["both_unaligned"] >= 10  # short mates do not align
    b.close()


def test_empty_batch(mixed):
    """an empty batch: empty text, pair_off == [0]"""
    import ma_amd
    ctx = mixed
    b = ma_amd.Batch(ctx.idx, params("illuminapaired"), 8, 1024)
    b.set_reads([])
    b.set_read_text([], None)
    b.align()
    b.pair()
    assert b.pair_sam(0) == 0
    off, text = b.pair_sam_text()
    assert text == b"" and list(off) == [0]
    b.close()


def test_pairs_without_any_seed(tmp_path, mixed):
    """a batch none of whose reads has a harmonized set (ma_pair_batch launches nothing then): two unaligned records per pair;
    also with empty mates, first or second, beside a mate that has bases and qualities"""
    ctx = mixed
    rng = np.random.default_rng(92)
    names = ["u%d" % i for i in range(6)]
    # (a mate of length 0 has no SEQ and no QUAL to copy; the other mate's QUAL is printed all the same)
    for lens, with_quals in (((150, 1, 64, 65, 3, 150), False), ((150, 1, 64, 65, 3, 150), True), ((1, 3, 4, 5, 3, 1), True),
                             ((0, 150, 65, 0, 0, 0), True), ((0, 150, 65, 0, 0, 0), False), ((0, 3, 4, 0, 1, 5), True)):
        reads = [rng.integers(0, 4, size=L, dtype=np.uint8) for L in lens]
        quals = make_quals(reads, 93) if with_quals else None
        b = paired_batch(ctx, params("illuminapaired"), reads, names, quals)
        assert len(b.pairs()[1]) == 0
        text = check(tmp_path, ctx, b, reads, names, quals, [1, 0])
        assert text.count(b"\n") == 6 and text.startswith(b"u0\t77\t*\t0\t0\t*\t*\t0\t0\t")
        if with_quals:  # every non-empty mate's qualities are in the text
            for r, q in zip(reads, quals):
                assert len(r) == 0 or bytes(q) in text
        b.close()


# ---- 4. injected alignments -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rev", [False, True], ids=["forward", "reverse"])
def test_record_beyond_its_own_mate(tmp_path, mixed, rev):
    """a pair whose second mate's record ends beyond that mate (the first mate is longer: only the own length tells): pair_sam(0)
    fails with the host formatter's text, pair_sam(1) -- soft clipping prints the whole read -- succeeds on the same object"""
    import ma_amd
    ctx = mixed
    reads = [ctx.g[0][2000:2400].copy(), ctx.g[0][2500:2650].copy()]
    names, quals = ["first", "second"], make_quals(reads, 94)
    b = ctx.batch(params("illuminapaired"), reads, names, quals)
    alns = np.concatenate([one_alignment(2 * ctx.F - 2400 if not rev else 2000, 400, 0, 400, 1),
                           one_alignment(2 * ctx.F - 2650 if rev else 2500, 150, 120, 153, 1)])
    alns["ops_off"] = [0, 1]
    b.set_alignments([0, 1, 2], alns, np.array([0, 400, 0, 33], dtype=np.uint64))
    b.pair()
    res = b.pairs()
    assert len(res[1]) == 2 and int(res[1][1]["end_q"]) == 153 and list(res[3]) == [1, 0] and list(res[4]) == [1, 0]
    want = yardstick(tmp_path, ctx, names, reads, quals, res, 0)
    assert want == ("Index out of range (compCharAt)" if rev else "Query length is off by -3.")
    with pytest.raises(ma_amd.MaError) as e:
        b.pair_sam(0)
    assert str(e.value) == want
    with pytest.raises(ma_amd.MaError, match="run ma_pair_sam_batch first"):
        b.pair_sam_text()
    check(tmp_path, ctx, b, reads, names, quals, [1])
    b.close()


def test_cg_tag_inside_a_pair(tmp_path, mixed):
    """a 65 536-op record as the first mate of a pair: the CG:B:I tag appears, MA_SAM_NO_CG_TAG switches it off"""
    ctx = mixed
    ops, qlen, rlen = single_base_ops(65536)
    reads = [np.resize(ctx.g[0][1000:71000], 70000).copy(), ctx.g[0][80000:80150].copy()]
    names, quals = ["long", "short"], make_quals(reads, 95)
    b = ctx.batch(params("illuminapaired"), reads, names, quals)
    alns = np.concatenate([one_alignment(5000, rlen, 100, 100 + qlen, 65536), one_alignment(2 * ctx.F - 80150, 150, 0, 150, 1)])
    alns["ops_off"] = [0, 65536]
    b.set_alignments([0, 1, 2], alns, np.concatenate([ops, np.array([0, 150], dtype=np.uint64)]))
    b.pair()
    assert len(b.pairs()[1]) == 2
    check(tmp_path, ctx, b, reads, names, quals, [0, 16, 2, 19])
    b.pair_sam(0)
    assert b.pair_sam_text()[1].count(b"\tCG:B:I,") == 1
    b.pair_sam(16)
    assert b"\tCG:B:I," not in b.pair_sam_text()[1]
    b.close()


# ---- 5. order of calls ----------------------------------------------------------------------------------------------------------
def test_order_of_calls(tmp_path, mixed):
    """pair_sam before pair(), without read text, without contig names, with unknown option bits: a message each, no text
    afterwards, and the object works once the missing call was made.  (That no kernel ran cannot be seen through the API and is
    not checked here: the launcher returns before it binds the device in all four cases.)"""
    import ma_amd
    ctx = mixed
    reads = edge_pairs(ctx.g, 8)
    names = ["o%d" % i for i in range(len(reads))]
    b = ma_amd.Batch(ctx.idx, params("illuminapaired"), len(reads), sum(len(r) for r in reads) + 64)
    b.set_reads(reads)
    b.align()
    with pytest.raises(ma_amd.MaError, match="run ma_pair_batch first"):
        b.pair_sam(0)
    b.pair()
    with pytest.raises(ma_amd.MaError, match="ma_batch_set_read_text"):
        b.pair_sam(0)
    b.set_read_text(names, None)
    with pytest.raises(ma_amd.MaError, match="unknown option bits 32"):
        b.pair_sam(32)
    with pytest.raises(ma_amd.MaError, match="run ma_pair_sam_batch first"):
        b.pair_sam_text()
    with pytest.raises(ma_amd.MaError, match="run ma_pair_sam_batch first"):
        b.pair_sam_bytes()
    check(tmp_path, ctx, b, reads, names, None, [0])
    b.close()
    bare = ma_amd.Index.build([ctx.g[0][:60000]])
    rd = [ctx.g[0][100:250].copy(), revcomp(ctx.g[0][400:550])]
    b = ma_amd.Batch(bare, params("illuminapaired"), 2, 1024)
    b.set_reads(rd)
    b.set_read_text(["a", "b"], None)
    b.align()
    b.pair()
    with pytest.raises(ma_amd.MaError, match="ma_index_set_contig_names"):
        b.pair_sam(0)
    b.close()
    bare.close()


# ---- 6. existing calls undisturbed --------------------------------------------------------------------------------------------
def test_existing_calls_undisturbed(tmp_path, mixed):
    """pairs() and mapq_alignments() are the same before and after pair_sam; the single-end text of the same object is the
    single-end text -- printed before pair_sam and fetched after it, and printed after it"""
    ctx = mixed
    reads = sample_pairs(ctx.g, 100, 150, 96)
    names = ["x%d" % i for i in range(len(reads))]
    quals = make_quals(reads, 97)
    single = ctx.batch(params("illuminapaired"), reads, names, quals)
    single.align()
    single.sam(1)
    want_single = single.sam_text()
    single.close()
    b = ctx.batch(params("illuminapaired"), reads, names, quals)
    b.align()
    b.sam(1)
    b.pair()
    before = b.pairs(), b.mapq_alignments()
    text = check(tmp_path, ctx, b, reads, names, quals, [0, 1])
    after = b.pairs(), b.mapq_alignments()
    for x, y in zip(before, after):
        assert all(np.array_equal(u, v) for u, v in zip(x, y))
    off, got = b.sam_text()  # (printed before pair_sam)
    assert got == want_single[1] and np.array_equal(off, want_single[0]) and got != text
    b.sam(1)
    off, got = b.sam_text()
    assert got == want_single[1] and np.array_equal(off, want_single[0])
    assert b.pair_sam_text()[1] == text  # and the pair text is still the pair text
    b.close()


# ---- 7. downloads and two batches in flight -------------------------------------------------------------------------------------
def test_downloads_and_two_batches_in_flight(tmp_path, mixed):
    """start_pair_sam_download + finish_download == pair_sam_text(); two batch objects on their own streams print what each
    prints alone"""
    import ma_amd
    ctx = mixed
    sets = [sample_pairs(ctx.g, 100, 150, 98 + i) for i in range(2)]
    alone = []
    for reads in sets:
        names = ["s%d" % i for i in range(len(reads))]
        b = paired_batch(ctx, params("illuminapaired"), reads, names, make_quals(reads, 62))
        b.pair_sam(1)
        alone.append(b.pair_sam_text())
        harr = [ma_amd.HostArray(len(reads) // 2 + 1, np.uint64), ma_amd.HostArray(b.pair_sam_bytes(), np.uint8)]
        assert b.start_pair_sam_download(*harr) == len(alone[-1][1])
        b.finish_download()
        assert np.array_equal(harr[0].a, alone[-1][0]) and harr[1].a.tobytes() == alone[-1][1]
        for h in harr:
            h.close()
        b.close()
    assert alone[0][1] != alone[1][1]
    streams, batches = [], []
    for reads in sets:
        s = C.c_void_p()
        assert ma_amd.lib().ma_stream_create(ctx.idx.h, C.byref(s)) == 0
        streams.append(s)
        b = ma_amd.Batch(ctx.idx, params("illuminapaired"), len(reads), sum(len(r) for r in reads) + 64)
        b.set_stream(s.value)
        b.set_reads(reads)
        b.set_read_text(["s%d" % i for i in range(len(reads))], make_quals(reads, 62))
        batches.append(b)
    for b in batches:
        b.align()
    for b in batches:
        b.pair()
    for b in batches:
        b.pair_sam(1)
    for b, want in zip(batches, alone):
        off, text = b.pair_sam_text()
        assert text == want[1] and np.array_equal(off, want[0])
    for b, s in zip(batches, streams):
        b.close()
        assert ma_amd.lib().ma_stream_destroy(ctx.idx.h, s) == 0


# ---- 8. through the host layer ---------------------------------------------------------------------------------------------------
def host_deps():
    return [os.path.join(ROOT, "ma_amd", "libma_amd.so"), os.path.join(ROOT, "include", "ma_amd.h")] + [
        os.path.join(ROOT, "ma_amd", "host", h) for h in os.listdir(os.path.join(ROOT, "ma_amd", "host")) if h.endswith(".h")]


def build_driver():
    exe = os.path.join(ROOT, "tests", "emul", "pair_sam_graph_test")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in [exe + ".cpp"] + host_deps()):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "ma_amd", "host"), exe + ".cpp", "-o", exe, "-L" + os.path.join(ROOT, "ma_amd"),
                               "-lma_amd", "-Wl,-rpath," + os.path.join(ROOT, "ma_amd"), "-lpthread"])
    return exe


@pytest.fixture(scope="module")
def x8_case(tmp_path_factory):
    """4001 pairs of the eight-copy genome of test_gpu_pairs.py (sample_pairs draws pair by pair: its first 4001 pairs)"""
    g = rand_genome(6, [500000, 300000, 200000], repeat_unit=700, repeat_copies=8, repeat_div=0.0)
    reads = sample_pairs(g, 4001, 150, 77, far_frac=0.1, same_strand_frac=0.05, random_mate_frac=0.08)
    path = str(tmp_path_factory.mktemp("pair_sam") / "x8.case")
    write_case(path, g, reads)
    return path


@pytest.mark.parametrize("quals", ["quals", "mix"])
def test_execute_paired_flat_sam_of_both_aligners_against_the_host_writer(tmp_path, gpu_device, x8_case, quals):
    """4001 pairs in device batches of 1001 (-> 1002) reads, two in flight: BatchAligner::executePairedFlatSam and
    MultiDeviceAligner::executePairedFlatSam (two replicas of one device, second run) + BatchPairedFileWriter give the file of
    executePairedFlat + BatchPairedFileWriter; every batch comes back as device text, except the one that mixes reads with and
    without qualities, which comes back as pair records"""
    out = str(tmp_path / "g")
    stats = subprocess.check_output([build_driver(), x8_case, "4001", "1001", "2", out, "illuminapaired", "0", quals]).decode()
    print(stats)
    assert '"pairs": 4001,' in stats and '"shards_used": 2' in stats
    assert '"text_batches": %d, "record_batches": %d' % ((7, 1) if quals == "mix" else (8, 0)) in stats
    want = open(out + ".flat.sam", "rb").read()
    assert want.count(b"\n") > 8002
    for leg in ("dev", "multi"):
        assert open(out + ".%s.sam" % leg, "rb").read() == want, leg


def test_golden_through_the_host_layer(tmp_path, gpu_device):
    """f4.case under illumina, options 3, through executePairedFlatSam + BatchPairedFileWriter: the reference's file, header
    included"""
    case = gunzip_to(os.path.join(G, "f4.case.gz"), str(tmp_path / "f4.case"))
    out = str(tmp_path / "g")
    stats = subprocess.check_output([build_driver(), case, "0", "1000000", "1", out, "illumina", "3"]).decode()
    assert '"text_batches": 1, "record_batches": 0' in stats
    want = gzip.open(os.path.join(G, PAIR_GOLDEN + ".sam.gz"), "rb").read()
    for leg in ("flat", "dev", "multi"):
        assert open(out + ".%s.sam" % leg, "rb").read() == want, leg


def test_ma_align_writes_the_same_paired_file_with_and_without_the_device_path(tmp_path, gpu_device):
    """examples/ma_align on paired FASTQ: the file written through executePairedFlatSam is, byte for byte, the file of
    --host-sam (executePairedFlat + the host formatter), qualities included"""
    from test_gpu_sam import build_ma_align
    exe = build_ma_align()
    g = rand_genome(PAIRED["seed"], PAIRED["contig_lens"], repeat_unit=PAIRED["repeat_unit"], repeat_copies=PAIRED["repeat_copies"],
                    repeat_div=PAIRED["repeat_div"])
    reads = sample_pairs(g, 300, 150, 100)
    fa = str(tmp_path / "genome.fa")
    with open(fa, "w") as f:
        for nm, c in zip(("ctgA", "ctgB"), g):
            f.write(">%s\n%s\n" % (nm, "".join("ACGT"[int(b)] for b in c)))
    rng = np.random.default_rng(101)
    files = [str(tmp_path / "reads_1.fq"), str(tmp_path / "reads_2.fq")]
    for m in (0, 1):
        with open(files[m], "w") as f:
            for k in range(len(reads) // 2):
                r = reads[2 * k + m]
                f.write("@p%d/%d\n%s\n+\n%s\n" % (k, m + 1, "".join("ACGTN"[int(b)] for b in r),
                                                  "".join(chr(int(q)) for q in rng.integers(35, 127, size=len(r)))))
    dev, host = str(tmp_path / "device.sam"), str(tmp_path / "host.sam")
    subprocess.check_call([exe, fa, files[0], dev, "illuminapaired", files[1]])
    subprocess.check_call([exe, "--host-sam", fa, files[0], host, "illuminapaired", files[1]])
    got, want = open(dev, "rb").read(), open(host, "rb").read()
    assert got == want
    lines = [l.split(b"\t") for l in got.splitlines() if not l.startswith(b"@")]
    assert len(lines) >= 600 and sum(1 for l in lines if l[10] != b"*") >= 500 and sum(1 for l in lines if l[6] == b"=") >= 400
