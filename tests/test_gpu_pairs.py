"""ma_pair_batch: PairedReads::execute (pairedReads.cpp:14-131) on the device, through the C ABI / ma_amd.api, against the golden
the compiled reference wrote and against the oracle's f4 dump on inputs chosen (with the oracle, on the CPU) to hold ties,
improper winners, empty mates and pairs the kernel leaves to the host."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from ma_testlib import OrIndex, gunzip_to, or_params, rand_genome, read_case, sample_pairs, write_case
from pairs_testlib import oracle_pairs, pair_stats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
TIE_CAP = 32  # PAIR_TIE_CAP of ma_amd/csrc/stage_pair.h: tied candidates a lane sorts on chip


def p_lines(pair_off, alns, ops, mate, other, k):
    """pair k's records as the 'p' lines of an f4 dump (oracle/ma_oracle_api.inc dumpF4Line; %.17g round-trips a double,
    so equal text is equal mapq bits)"""
    out = []
    for i in range(int(pair_off[k]), int(pair_off[k + 1])):
        a = alns[i]
        o = ops[2 * int(a["ops_off"]):2 * (int(a["ops_off"]) + int(a["n_ops"]))]
        out.append("p %d %d %d %d %d %d %d %d %d %d %.17g %d%s" % (
            mate[i], other[i], a["begin_ref"], a["end_ref"], a["begin_q"], a["end_q"], a["score"], a["soc_index"], a["secondary"],
            a["supplementary"], a["mapq"], a["n_ops"], "".join(" %d:%d" % (o[2 * j], o[2 * j + 1]) for j in range(len(o) // 2))))
    return out


def paired_batch(idx, P, reads):
    import ma_amd
    b = ma_amd.Batch(idx, P, len(reads), sum(len(r) for r in reads) + 64)
    b.set_reads(reads)
    b.align()
    b.pair()
    return b


def test_golden_case_on_the_device(tmp_path, gpu_device):
    """f4.case as one batch under ("illumina", inv 0, paired, opt 3): the P / PAIR / p lines of the reference's dump."""
    import ma_amd
    g, reads, _ = read_case(gunzip_to(os.path.join(G, "f4.case.gz"), str(tmp_path / "f4.case")))
    want = [l for l in gzip.open(os.path.join(G, "f4.illumina.inv0.pair1.zd100.opt3.f4.gz"), "rt").read().split("\n")
            if l.startswith(("P ", "PAIR", "p "))]
    idx = ma_amd.Index.build(g)
    b = paired_batch(idx, ma_amd.Params.preset("illumina"), reads)
    res = b.pairs()
    got = []
    for k in range(len(reads) // 2):
        lines = p_lines(*res, k)
        got += ["P %d %d %d" % (k, len(reads[2 * k]), len(reads[2 * k + 1])), "PAIR %d" % len(lines)] + lines
    assert sum(l.startswith("p ") for l in want) > 100
    for i, (x, y) in enumerate(zip(got, want)):
        assert x == y, "line %d" % i
    assert len(got) == len(want)
    assert b.pair_counts()["host_pairs"] == 0
    b.close()
    idx.close()


# Two genomes with one repeat family each, long enough (700) to hold both mates of a pair: three exact copies keep every pair
# below TIE_CAP candidates, eight copies with the lists cut to the 7 / 5 best give tied pairs of up to 49 / 25 of them.
# (report_n_best only ever shortens a MappingQuality list, mappingQuality.cpp:118-124: what makes the lists long is the
# number of copies, so the settings with report_n_best > 0 run on the genome with more of them.)
GENOMES = {"x3": dict(seed=5, copies=3), "x8": dict(seed=6, copies=8)}
SETTINGS = [
    # name, genome, changed parameters, pairs left to the host expected
    ("illuminapaired", "x3", {}, False),
    ("narrow", "x3", dict(mean_paired_dist=300.0, std_paired_dist=40.0, paired_bonus=1.5), False),
    ("nbest7", "x8", dict(mean_paired_dist=450.5, std_paired_dist=200.0, paired_bonus=1.0, report_n_best=7), True),
    ("nbest5", "x8", dict(mean_paired_dist=380.0, std_paired_dist=100.0, paired_bonus=1.3, report_n_best=5), None),
]
N_PAIRS = 20000


@pytest.fixture(scope="module")
def genomes(gpu_device):
    import ma_amd
    out = {}
    for name, d in GENOMES.items():
        g = rand_genome(d["seed"], [500000, 300000, 200000], repeat_unit=700, repeat_copies=d["copies"], repeat_div=0.0)
        reads = sample_pairs(g, N_PAIRS, 150, 77, far_frac=0.1, same_strand_frac=0.05, random_mate_frac=0.08)
        idx = ma_amd.Index.build(g)
        out[name] = dict(g=g, reads=reads, idx=idx, oidx=OrIndex.from_parts(idx.download()))
    yield out
    for d in out.values():
        d["idx"].close()


@pytest.mark.parametrize("setting", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_parity_with_the_oracle_at_size(tmp_path, genomes, setting):
    """20 000 pairs (far, same-strand and random mates among them): every field of every record, mate and other, mapq as
    bits, against the oracle's PairedReads on the same input; the input holds what makes the comparison mean something."""
    import ma_amd
    name, gname, changed, want_host_pairs = setting
    d = genomes[gname]
    P, op = ma_amd.Params.preset("illuminapaired"), or_params("illuminapaired", 1)
    op.use_paired_reads = 1
    for k, v in changed.items():
        setattr(P, k, v)
        setattr(op, k, v)
    want = oracle_pairs(d["oidx"], d["reads"], op, str(tmp_path / "or"))
    assert len(want) == N_PAIRS
    st = pair_stats(want, op, 2 * sum(len(c) for c in d["g"]), TIE_CAP)
    print(name, st)
    assert st["tied"] > 100 and st["improper_winner"] > 100 and st["one_empty"] > 100 and st["both_empty"] > 50
    assert st["mapq_set"] > 1000
    b = paired_batch(d["idx"], P, d["reads"])
    c = b.pair_counts()
    print(name, c)
    assert c["pairs"] == N_PAIRS
    # the pairs the library finished on the host are exactly the tied ones beyond the kernel's limit
    assert c["host_pairs"] == st["over_cap"]
    if want_host_pairs is True:
        assert c["host_pairs"] > 0
    elif want_host_pairs is False:
        assert c["host_pairs"] == 0
    res = b.pairs()
    assert int(res[0][-1]) == c["records"] == sum(len(p["pair"]) for p in want)
    for k, p in enumerate(want):
        assert p_lines(*res, k) == ["p " + r["text"] for r in p["pair"]], "pair %d" % k
    # the MappingQuality records are still the unpaired ones
    off, alns, _ = b.mapq_alignments()
    assert [int(off[i + 1] - off[i]) for i in range(64)] == [len(p["fin"][m]) for p in want[:32] for m in (0, 1)]
    # the asynchronous form delivers the same arrays
    arrs = [ma_amd.HostArray(c["pairs"] + 1, np.uint64), ma_amd.HostArray(c["records"], ma_amd.ALIGNMENT_DT),
            ma_amd.HostArray(2 * c["ops"], np.uint64), ma_amd.HostArray(c["records"], np.int32),
            ma_amd.HostArray(c["records"], np.int32)]
    assert b.start_pair_download(*arrs) == c
    b.finish_download()
    for got_a, want_a in zip(arrs, res):
        assert np.array_equal(got_a.a, want_a[:got_a.n])
    for a in arrs:
        a.close()
    b.close()


def test_error_paths_launch_nothing(genomes):
    """an odd number of reads, and pairing before the DP stage: a status and a message each"""
    import ma_amd
    d = genomes["x3"]
    P = ma_amd.Params.preset("illuminapaired")
    reads = d["reads"][:7]
    b = ma_amd.Batch(d["idx"], P, len(reads), sum(len(r) for r in reads) + 64)
    b.set_reads(reads)
    b.seed()
    b.extract()
    b.chain()
    with pytest.raises(ma_amd.MaError, match="no MappingQuality output"):
        b.pair()
    b.dp()
    with pytest.raises(ma_amd.MaError, match="odd number of reads"):
        b.pair()
    with pytest.raises(ma_amd.MaError, match="run ma_pair_batch first"):
        b.pairs()
    b.set_reads(reads[:6])
    b.align()
    b.pair()
    assert b.pair_counts()["pairs"] == 3
    b.close()


def build_driver():
    exe = os.path.join(ROOT, "tests", "emul", "pair_graph_test")
    src = exe + ".cpp"
    deps = [src, os.path.join(ROOT, "include", "ma_amd.h"), os.path.join(ROOT, "ma_amd", "libma_amd.so")] + [
        os.path.join(ROOT, "ma_amd", "host", h) for h in ("ma_sam.h", "ma_modules.h", "ms_graph.h", "ma_pair_flat.h", "ma_flat_sam.h",
                                                          "ma_sam_dev.h", "ma_batch_nodes.h", "ma_engine.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "ma_amd", "host"), src, "-o", exe, "-L" + os.path.join(ROOT, "ma_amd"),
                               "-lma_amd", "-Wl,-rpath," + os.path.join(ROOT, "ma_amd"), "-lpthread"])
    return exe


def test_golden_sam_through_the_flat_paired_path(tmp_path, gpu_device):
    """f4.case under ("illumina", inv 0, paired, opt 3) through BatchAligner::executePairedFlat + the flat pair writer: the
    reference's SAM byte for byte (and the container path's, from the same binary)."""
    exe = build_driver()
    case = gunzip_to(os.path.join(G, "f4.case.gz"), str(tmp_path / "f4.case"))
    subprocess.check_call([exe, case, "illumina", "0", "3", "1000000", "1", str(tmp_path / "flat.sam"), str(tmp_path / "cont.sam")])
    want = gzip.open(os.path.join(G, "f4.illumina.inv0.pair1.zd100.opt3.sam.gz"), "rb").read()
    assert open(str(tmp_path / "flat.sam"), "rb").read() == want
    assert open(str(tmp_path / "cont.sam"), "rb").read() == want


@pytest.mark.parametrize("inv", [1])
def test_flat_paired_path_with_small_inversions_takes_the_container_path(tmp_path, gpu_device, inv):
    """With "Detect Small Inversions" executePairedFlat goes through containers and flattens: the golden of
    ("default", inv 1, paired, zd 100, opt 0)."""
    exe = build_driver()
    case = gunzip_to(os.path.join(G, "f4.case.gz"), str(tmp_path / "f4.case"))
    subprocess.check_call([exe, case, "default", "1", "0", "1000000", "1", str(tmp_path / "flat.sam"), str(tmp_path / "cont.sam")])
    want = gzip.open(os.path.join(G, "f4.default.inv1.pair1.zd100.opt0.sam.gz"), "rb").read()
    assert open(str(tmp_path / "flat.sam"), "rb").read() == want


@pytest.mark.parametrize("inflight,shards", [(1, 0), (3, 0), (2, 2)], ids=["1-in-flight", "3-in-flight", "2-replicas"])
def test_flat_path_equals_container_path(tmp_path, genomes, inflight, shards):
    """4001 pairs of the eight-copy genome in batches of 1001 reads (odd: a boundary there would split a pair; the driver
    fails if a batch holds an odd number of reads) under illuminapaired: executePairedFlat + the flat writer give the SAM
    bytes of executePaired + PairedFileWriter; also through MultiDeviceAligner over two replicas."""
    exe = build_driver()
    d = genomes["x8"]
    case = str(tmp_path / "x8.case")
    write_case(case, d["g"], d["reads"][:8002])
    out = subprocess.check_output([exe, case, "illuminapaired", "0", "0", "1001", str(inflight), str(tmp_path / "flat.sam"),
                                   str(tmp_path / "cont.sam"), str(shards)]).decode()
    print(out)
    assert int(out.split()[1]) == 8  # 8002 reads in batches of 1002
    flat, cont = open(str(tmp_path / "flat.sam"), "rb").read(), open(str(tmp_path / "cont.sam"), "rb").read()
    assert flat.count(b"\n") > 8002
    assert flat == cont
