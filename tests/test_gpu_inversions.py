"""ma_inversions_batch: SmallInversions::execute (smallInversions.h:22-221) on the device (ma_amd/csrc/stage_inv.h), through the
C ABI / ma_amd.api and through the flat paths of the host layer.  The yardsticks: the dumps and SAM texts the compiled
reference wrote (tests/golden/inv.*, made by tests/golden/make_inv_golden.py; f4.default.inv1.pair1.zd100.opt0), and the host
module ma_amd::SmallInversions (ma_amd/host/ma_modules.h) run by tests/emul/inv_graph_test.cpp on the same lists."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from ma_testlib import gunzip_to, rand_genome, read_case, revcomp, write_case
from test_gpu_pairs import p_lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
# (golden, paired, Z Drop Inversions, SAM options, inversion records in it: what tests/golden/make_inv_golden.py printed)
SINGLE = [("inv.default.pair0.zd40.opt3", 40, 3, 26), ("inv.default.pair0.zd100.opt0", 100, 0, 14)]
PAIRED = ("inv.default.pair1.zd40.opt1", 40, 1, 26)
SEED, MATCH, MISMATCH, INSERTION, DELETION = range(5)


def f_lines(off, alns, ops, r):
    """read r's records as the 'f' lines of a single-end f4 dump (%.17g round-trips a double: equal text is equal mapq bits)"""
    out = []
    for i in range(int(off[r]), int(off[r + 1])):
        a = alns[i]
        o = ops[2 * int(a["ops_off"]):2 * (int(a["ops_off"]) + int(a["n_ops"]))]
        out.append("f 0 -1 %d %d %d %d %d %d %d %d %.17g %d%s" % (
            a["begin_ref"], a["end_ref"], a["begin_q"], a["end_q"], a["score"], a["soc_index"], a["secondary"], a["supplementary"],
            a["mapq"], a["n_ops"], "".join(" %d:%d" % (o[2 * j], o[2 * j + 1]) for j in range(len(o) // 2))))
    return out


def golden_lists(text):
    """the FIN lists of an f4 dump in file order (single-end: one per read; paired: mate 1, mate 2 of every pair), their 'f'
    lines with first / other set to 0 / -1 as f_lines prints them"""
    lists = []
    for line in text.split("\n"):
        if line.startswith("FIN"):
            lists.append([])
        elif line.startswith("f "):
            t = line.split()
            lists[-1].append(" ".join(["f", "0", "-1"] + t[3:]))
    return lists


def sam_records(name):
    return b"".join(l for l in gzip.open(os.path.join(G, name + ".sam.gz"), "rb").read().splitlines(True) if not l.startswith(b"@"))


@pytest.fixture(scope="module")
def inv_case(tmp_path_factory, gpu_device):
    import ma_amd
    path = gunzip_to(os.path.join(G, "inv.case.gz"), str(tmp_path_factory.mktemp("inv") / "inv.case"))
    g, reads, names = read_case(path)
    idx = ma_amd.Index.build(g)
    idx.set_contig_names(names)
    yield dict(path=path, g=g, reads=reads, idx=idx)
    idx.close()


def aligned(case, zd, reads=None):
    import ma_amd
    reads = case["reads"] if reads is None else reads
    P = ma_amd.Params.preset("default")
    P.search_inversions, P.zdrop_inversion = 1, zd
    b = ma_amd.Batch(case["idx"], P, len(reads), sum(len(r) for r in reads) + 64)
    b.set_reads(reads)
    b.set_read_text(["r%d" % i for i in range(len(reads))], None)
    b.align()
    return b


# ---- 1. aligned reads against the reference's goldens ------------------------------------------------------------------------
@pytest.mark.parametrize("golden", SINGLE, ids=[g[0] for g in SINGLE])
def test_aligned_single_end(inv_case, golden):
    """inv.case under the golden's parameters: the final lists record by record (ops and mapq bits), the counts, the SAM text"""
    name, zd, opt, n_inv = golden
    want = golden_lists(gzip.open(os.path.join(G, name + ".f4.gz"), "rt").read())
    b = aligned(inv_case, zd)
    before = int(b.mapq_alignments()[0][-1])
    b.inversions()
    c = b.inversion_counts()
    print(name, c)
    off, alns, ops = b.mapq_alignments()
    assert len(want) == len(inv_case["reads"]) == 80
    for r in range(80):
        assert f_lines(off, alns, ops, r) == want[r], "read %d" % r
    assert c["records"] == n_inv == int(off[-1]) - before and c["candidates"] >= c["jobs"] >= c["records"]
    assert b.counts()["alignments"] >= int(off[-1])
    wsam = sam_records(name)
    assert b.sam(opt) == len(wsam)
    assert b.sam_text()[1] == wsam
    # twice gives the same lists; the lists NeedlemanWunsch left are served as before
    b.inversions()
    again = b.mapq_alignments()
    assert b.inversion_counts() == c and all(np.array_equal(x, y) for x, y in zip(again, (off, alns, ops)))
    assert int(b.alignments()[0][-1]) == b.counts()["hsets"]
    b.close()


def test_aligned_paired(inv_case):
    """the same with pair() and pair_sam(): the PAIR lines and the SAM bytes of the paired golden (its FIN lines were printed
    after PairedReads had changed the records it picked: the lists before pairing are those of the single-end golden)"""
    name, zd, opt, n_inv = PAIRED
    text = gzip.open(os.path.join(G, name + ".f4.gz"), "rt").read()
    want_lists = golden_lists(gzip.open(os.path.join(G, SINGLE[0][0] + ".f4.gz"), "rt").read())
    want_pairs = [l for l in text.split("\n") if l.startswith(("P ", "PAIR", "p "))]
    reads = inv_case["reads"]
    b = aligned(inv_case, zd)
    b.inversions()
    assert b.inversion_counts()["records"] == n_inv
    off, alns, ops = b.mapq_alignments()
    for r in range(len(reads)):
        assert f_lines(off, alns, ops, r) == want_lists[r], "read %d" % r
    b.pair()
    res = b.pairs()
    got = []
    for k in range(len(reads) // 2):
        lines = p_lines(*res, k)
        got += ["P %d %d %d" % (k, len(reads[2 * k]), len(reads[2 * k + 1])), "PAIR %d" % len(lines)] + lines
    assert got == want_pairs
    wsam = sam_records(name)
    assert b.pair_sam(opt) == len(wsam)
    assert b.pair_sam_text()[1] == wsam
    b.close()


def test_f4_case_paired(tmp_path, gpu_device):
    """f4.case under ("default", inv 1, paired, zd 100, opt 0): the P / PAIR / p lines and the SAM bytes of the existing golden"""
    import ma_amd
    g, reads, names = read_case(gunzip_to(os.path.join(G, "f4.case.gz"), str(tmp_path / "f4.case")))
    reads = reads[:len(reads) // 2 * 2]
    name = "f4.default.inv1.pair1.zd100.opt0"
    want = [l for l in gzip.open(os.path.join(G, name + ".f4.gz"), "rt").read().split("\n") if l.startswith(("P ", "PAIR", "p "))]
    idx = ma_amd.Index.build(g)
    idx.set_contig_names(names)
    b = aligned(dict(idx=idx, reads=reads), 100)
    b.inversions()
    assert b.inversion_counts()["records"] == 5
    b.pair()
    res = b.pairs()
    got = []
    for k in range(len(reads) // 2):
        lines = p_lines(*res, k)
        got += ["P %d %d %d" % (k, len(reads[2 * k]), len(reads[2 * k + 1])), "PAIR %d" % len(lines)] + lines
    assert got == want
    wsam = sam_records(name)
    assert b.pair_sam(0) == len(wsam) and b.pair_sam_text()[1] == wsam
    b.close()
    idx.close()


# ---- 2. small hand-made lists through ma_batch_set_alignments ----------------------------------------------------------------
def build_driver():
    exe = os.path.join(ROOT, "tests", "emul", "inv_graph_test")
    src = exe + ".cpp"
    deps = [src, os.path.join(ROOT, "tests", "emul", "inv_common.h"), os.path.join(ROOT, "tests", "emul", "sam_dev_common.h"),
            os.path.join(ROOT, "include", "ma_amd.h"), os.path.join(ROOT, "ma_amd", "libma_amd.so")] + [
        os.path.join(ROOT, "ma_amd", "host", h) for h in ("ma_sam.h", "ma_modules.h", "ms_graph.h", "ma_pair_flat.h", "ma_flat_sam.h",
                                                          "ma_sam_dev.h", "ma_batch_nodes.h", "ma_engine.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "ma_amd", "host"), src, "-o", exe, "-L" + os.path.join(ROOT, "ma_amd"),
                               "-lma_amd", "-Wl,-rpath," + os.path.join(ROOT, "ma_amd"), "-lpthread"])
    return exe


class HandMade:
    """One contig of 6000 bases; every read is a piece of it with stretches reverse-complemented in place, every record a
    hand-written op list over it.  A mismatch run of w bases behind a seed is a drop of 2 w (default scores); two deletion
    (insertion) runs of 10 and 40 behind a seed a drop of 8: "Z Drop Inversions" is 8 in these tests."""
    F = 6000

    def __init__(self):
        self.g = rand_genome(31, [self.F])
        self.reads, self.lists = [], []

    def read(self, p, length, inverted=(), reverse=False):
        # (the window of a stretch is the reverse-strand position of its begin AND of its end, pack.h:924-927: one base further;
        # the inverted bases are taken from there, so that query and window of a stretch are equal base by base)
        rd, shift = np.array(self.g[0][p:p + length], dtype=np.uint8), -1 if reverse else 1
        for a, w in inverted:
            rd[a:a + w] = revcomp(self.g[0][p + a + shift:p + a + w + shift])
        self.reads.append(revcomp(rd) if reverse else rd)
        self.lists.append([])
        return len(self.reads) - 1

    def record(self, r, begin_q, begin_ref, ops):
        self.lists[r].append((begin_q, begin_ref, ops))

    def plain(self, p):  # a read with one record of one seed: nothing to find
        self.record(self.read(p, 120), 0, p, [(SEED, 120)])

    def arrays(self):
        import ma_amd
        n = sum(len(l) for l in self.lists)
        off, alns, ops = np.zeros(len(self.reads) + 1, dtype=np.uint64), np.zeros(n, dtype=ma_amd.ALIGNMENT_DT), []
        i = 0
        for r, l in enumerate(self.lists):
            for bq, br, o in l:
                a = alns[i]
                a["begin_q"], a["begin_ref"], a["ops_off"], a["n_ops"], a["soc_index"] = bq, br, len(ops) // 2, len(o), i % 3
                a["end_q"] = bq + sum(x[1] for x in o if x[0] != DELETION)
                a["end_ref"] = br + sum(x[1] for x in o if x[0] != INSERTION)
                a["score"] = sum({SEED: 2 * x[1], MATCH: 2 * x[1], MISMATCH: -4 * x[1]}.get(x[0], -(4 + 2 * x[1])) for x in o)
                for x in o:
                    ops += [x[0], x[1]]
                i += 1
            off[r + 1] = i
        return off, alns, np.array(ops, dtype=np.uint64)


def base_shapes(h):
    h.record(h.read(100, 300, [(120, 40)]), 0, 100, [(MATCH, 120), (MISMATCH, 40), (MATCH, 140)])  # no seed op at all
    h.record(h.read(500, 300, [(200, 40)]), 0, 500, [(SEED, 190), (MATCH, 10), (MISMATCH, 40), (MATCH, 60)])  # only behind the last seed
    h.record(h.read(900, 300, [(10, 60)]), 0, 900, [(MATCH, 10), (MISMATCH, 60), (SEED, 230)])  # before the first seed
    h.record(h.read(1300, 400, [(100, 40), (250, 60)]), 0, 1300,
             [(SEED, 100), (MISMATCH, 40), (SEED, 110), (MISMATCH, 60), (SEED, 90)])  # two stretches in one record
    h.record(h.read(1800, 200), 0, 1800, [(SEED, 100), (DELETION, 10), (DELETION, 40), (SEED, 100)])  # qlen 0
    h.record(h.read(2100, 250), 0, 2100, [(SEED, 100), (INSERTION, 10), (INSERTION, 40), (SEED, 100)])  # tlen 0
    h.record(h.read(2500, 218, [(100, 18)]), 0, 2500, [(SEED, 100), (MISMATCH, 18), (SEED, 100)])  # window score 36: dropped
    h.record(h.read(2800, 219, [(100, 19)]), 0, 2800, [(SEED, 100), (MISMATCH, 19), (SEED, 100)])  # 38: kept
    r = h.read(3200, 300, [(100, 50)], reverse=True)  # a parent on the reverse strand: its window lies on the forward strand
    h.record(r, 0, 2 * h.F - 3500, [(SEED, 150), (MISMATCH, 50), (SEED, 100)])
    h.read(3600, 150)  # a read with an empty list
    r = h.read(3800, 300, [(100, 40)])  # two records in one list, the second one with the candidate
    h.record(r, 0, 3800, [(SEED, 300)])
    h.record(r, 0, 3800, [(SEED, 100), (MISMATCH, 40), (SEED, 160)])


def run_lists(tmp, h, zd, heur_off):
    """the device's final lists of the hand-made batch, and the lists before the call"""
    import ma_amd
    idx = ma_amd.Index.build(h.g)
    P = ma_amd.Params.preset("default")
    P.zdrop_inversion, P.disable_heuristics = zd, heur_off
    b = ma_amd.Batch(idx, P, len(h.reads), sum(len(r) for r in h.reads) + 64)
    b.set_reads(h.reads)
    b.set_alignments(*h.arrays())
    before = b.mapq_alignments()
    b.inversions()
    return idx, b, before


def host_lists(tmp, h, before, zd, heur_off):
    """SmallInversions::executeBatch of the host module on the lists `before`"""
    case, lists, out = str(tmp / "hand.case"), str(tmp / "hand.lists"), str(tmp / "hand.out")
    write_case(case, h.g, h.reads)
    with open(lists, "w") as f:
        for r in range(len(h.reads)):
            l = f_lines(*before, r)
            f.write("R %d %d\nFIN 0 %d\n%s" % (r, len(h.reads[r]), len(l), "".join(x + "\n" for x in l)))
    subprocess.check_call([build_driver(), "lists", case, lists, str(zd), str(heur_off), out])
    return golden_lists(open(out).read())


@pytest.mark.parametrize("total,heur_off", [(0, 0), (0, 1), (65, 0), (257, 0)], ids=["base", "no-heuristics", "65-records", "257-records"])
def test_hand_made_lists(tmp_path, gpu_device, total, heur_off):
    """the hand-made records of the CPU test and lists with empty reads; with `total` the batch is filled with plain records
    to 65 / 257 records, one past the wavefront / the block, and its LAST record -- the last record of the last read -- holds a
    candidate; against the host module on the same lists; then with a threshold nothing reaches"""
    h = HandMade()
    base_shapes(h)
    if total:
        n = sum(len(l) for l in h.lists)
        for i in range(total - n - 1):
            h.plain(4200 + 3 * i)
        h.record(h.read(5500, 300, [(100, 40)]), 0, 5500, [(SEED, 100), (MISMATCH, 40), (SEED, 160)])
        assert sum(len(l) for l in h.lists) == total
    idx, b, before = run_lists(tmp_path, h, 8, heur_off)
    c = b.inversion_counts()
    print(c)
    got = b.mapq_alignments()
    want = host_lists(tmp_path, h, before, 8, heur_off)
    for r in range(len(h.reads)):
        assert f_lines(*got, r) == want[r], "read %d" % r
    n_want = sum(len(l) for l in want) - int(before[0][-1])
    # candidates: 1 before the first seed, 2 of the two stretches, 1 + 1 with an empty side, 2 at the score threshold, 1 on the
    # reverse strand, 1 in the second record of a list (+ 1 in the batch's last record); the jobs are those with both sides
    assert c == dict(candidates=9 + (1 if total else 0), jobs=7 + (1 if total else 0), records=n_want)
    # kept: all but the two with an empty side and the one at the threshold, which only disable_heuristics keeps
    assert n_want == (9 if heur_off else 6) + (1 if total else 0)
    if total:
        assert f_lines(*got, len(h.reads) - 1)[-1].split()[10] == "1"  # the batch's last record is an inversion record
    # nothing reaches a threshold of 100000: no candidate, the download is what it was, and twice is the same
    b.close()
    idx.close()
    idx, b, before = run_lists(tmp_path, h, 100000, heur_off)
    assert b.inversion_counts() == dict(candidates=0, jobs=0, records=0)
    after = b.mapq_alignments()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))
    b.inversions()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, b.mapq_alignments()))
    b.close()
    idx.close()


def test_batch_without_any_harmonized_set(gpu_device):
    import ma_amd
    h = HandMade()
    for p in (100, 400, 700):
        h.read(p, 150)
    idx = ma_amd.Index.build(h.g)
    b = ma_amd.Batch(idx, ma_amd.Params.preset("default"), 3, 600)
    b.set_reads(h.reads)
    b.set_alignments(*h.arrays())
    b.inversions()
    assert b.inversion_counts() == dict(candidates=0, jobs=0, records=0)
    off, alns, _ = b.mapq_alignments()
    assert list(off) == [0, 0, 0, 0] and len(alns) == 0
    b.close()
    idx.close()


# ---- 3. invalid lists and state ----------------------------------------------------------------------------------------------
def test_stretch_beyond_its_read_fails_and_the_object_stays_usable(gpu_device):
    """a record whose stretch ends beyond its read (only ma_batch_set_alignments can hand one in) fails the call with a
    message that names read and record; nothing beyond the read is read; the next valid lists on the same object succeed"""
    import ma_amd
    h = HandMade()
    h.plain(100)
    r = h.read(1000, 150)
    h.record(r, 0, 1000, [(SEED, 150)])
    h.record(r, 0, 1000, [(SEED, 100), (MISMATCH, 60), (SEED, 100)])  # the stretch [100, 160) of a read of 150 bases
    idx = ma_amd.Index.build(h.g)
    P = ma_amd.Params.preset("default")
    P.zdrop_inversion = 8
    b = ma_amd.Batch(idx, P, 8, 4096)
    b.set_reads(h.reads)
    b.set_alignments(*h.arrays())
    before = b.mapq_alignments()
    k = [l.split()[13:] for l in f_lines(*before, 1)].index(["0:100", "2:60", "0:100"])
    with pytest.raises(ma_amd.MaError, match="record %d of read 1: a stretch between two seeds ends beyond the read" % k):
        b.inversions()
    with pytest.raises(ma_amd.MaError, match="run ma_inversions_batch first"):
        b.inversion_counts()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, b.mapq_alignments()))
    good = HandMade()
    good.record(good.read(2800, 219, [(100, 19)]), 0, 2800, [(SEED, 100), (MISMATCH, 19), (SEED, 100)])
    b.set_reads(good.reads)
    b.set_alignments(*good.arrays())
    b.inversions()
    assert b.inversion_counts() == dict(candidates=1, jobs=1, records=1)
    assert int(b.mapq_alignments()[0][-1]) == 2
    b.close()
    idx.close()


def test_state(inv_case):
    """before the DP stage the call fails; after pair() it drops the pairs; setting reads puts the MappingQuality lists back"""
    import ma_amd
    reads = inv_case["reads"][48:64]  # the reads with two inverted stretches
    P = ma_amd.Params.preset("default")
    P.zdrop_inversion = 40
    b = ma_amd.Batch(inv_case["idx"], P, len(reads), sum(len(r) for r in reads) + 64)
    b.set_reads(reads)
    b.seed()
    b.extract()
    b.chain()
    with pytest.raises(ma_amd.MaError, match="ma_inversions_batch: no MappingQuality output"):
        b.inversions()
    b.dp()
    plain = b.mapq_alignments()
    b.pair()
    assert b.pair_counts()["records"] > 0
    b.inversions()
    assert b.inversion_counts()["records"] > 0
    with pytest.raises(ma_amd.MaError, match="run ma_pair_batch first"):
        b.pairs()
    final = b.mapq_alignments()
    assert int(final[0][-1]) == int(plain[0][-1]) + b.inversion_counts()["records"]
    b.pair()
    assert b.pair_counts()["records"] > 0
    b.set_reads(reads)
    with pytest.raises(ma_amd.MaError, match="run ma_inversions_batch first"):
        b.inversion_counts()
    b.align()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(plain, b.mapq_alignments()))
    b.close()


# ---- 4. the host layer -------------------------------------------------------------------------------------------------------
LAYER = [("inv.default.pair0.zd40.opt3", 0, 40, 3), ("inv.default.pair0.zd100.opt0", 0, 100, 0), ("inv.default.pair1.zd40.opt1", 1, 40, 1)]


@pytest.mark.parametrize("golden", LAYER, ids=[g[0] for g in LAYER])
def test_flat_paths_of_the_host_layer(tmp_path, inv_case, golden):
    """inv.case with search_inversions in batches of 32 reads: executeFlat + BatchFileWriter, executeFlatSam (paired:
    executePairedFlat + BatchPairedFileWriter, executePairedFlatSam) and the MultiDeviceAligner forms over two replicas give
    the golden's SAM bytes, and those of execute / executePaired + the per-read writers (the host module) from the same binary"""
    name, paired, zd, opt = golden
    out = str(tmp_path / "o")
    subprocess.check_call([build_driver(), "layer", inv_case["path"], str(zd), str(opt), str(paired), "32", out])
    want = gzip.open(os.path.join(G, name + ".sam.gz"), "rb").read()
    for kind in ("cont", "flat", "dev", "multi.flat", "multi.dev"):
        assert open("%s.%s.sam" % (out, kind), "rb").read() == want, kind
