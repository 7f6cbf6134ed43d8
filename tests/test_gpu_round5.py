"""Round 5: full-size NOISY-read parity inside `pytest -m gpu`: the GRCh38-size index of bench.py, reads
with the error profiles of BASELINE.json's configs, every alignment op and the mapq bits against the oracle, under the
Default, PacBio and Nanopore parameter sets (parameter.h:1081-1104); the presets of the C ABI; SMEM seeding of long reads
on the 16-byte list entries."""
import ctypes as C
import os

import numpy as np
import pytest

from ma_testlib import OrIndex, or_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRCH38 = [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717,
          133797422, 135086622, 133275309, 114364328, 107043718, 101991189, 90338345, 83257441, 80373285, 58617616,
          64444167, 46709983, 50818468, 156040895, 57227415]


@pytest.fixture(scope="module")
def gpu_device():
    import ma_amd
    if ma_amd.device_count() < 1:
        pytest.skip("no HIP device")
    ma_amd.set_device(0)
    return 0


@pytest.fixture(scope="module")
def grch38(gpu_device):
    """bench.py's genome (24 contigs of GRCh38's lengths, seed 2, planted repeat families), its index on the device and the
    same index bytes in the oracle."""
    import torch
    import ma_amd
    L = ma_amd.lib()
    lens = np.array(GRCH38, dtype=np.uint64)
    F = int(lens.sum())
    g = torch.empty(F, dtype=torch.uint8, device="cuda")
    assert L.ma_synth_genome_device(C.c_uint64(2), C.c_uint64(F), C.c_int32(1), C.c_void_p(g.data_ptr())) == 0
    idx = ma_amd.Index.build_device(lens, g.data_ptr())
    del g
    torch.cuda.empty_cache()
    oidx = OrIndex.from_parts(idx.download())
    yield idx, oidx
    idx.close()


def synth_reads(idx, seed, n, rl, sub=0.0, ins=0.0, dele=0.0):
    import torch
    import ma_amd
    L = ma_amd.lib()
    cap = int(n * (rl * (1 + 2 * ins) + 8)) + 1024
    codes = torch.empty(cap, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    nb = C.c_uint64()
    assert L.ma_synth_reads_device(idx.h, C.c_uint64(seed), C.c_uint64(n), C.c_uint32(rl), C.c_double(sub), C.c_double(ins),
                                   C.c_double(dele), C.c_uint64(0), C.c_void_p(codes.data_ptr()), C.c_void_p(offs.data_ptr()),
                                   C.c_uint64(cap), C.byref(nb)) == 0
    return codes, offs, int(nb.value)


def assert_same_as_oracle(bt, res, n, what):
    """every NeedlemanWunsch alignment (positions, score, SoC index, every op) and every MappingQuality record (flags, the bits
    of the mapq double) of the first n reads"""
    goff, galn, gops = bt.alignments()
    moff, mq, _ = bt.mapq_alignments()
    na, nm = int(res["aln_off"][n]), int(res["mq_off"][n])
    assert np.array_equal(goff[:n + 1], res["aln_off"][:n + 1]), what + ": alignments per read"
    nops = int(res["alns"]["ops_off"][na - 1] + res["alns"]["n_ops"][na - 1]) if na else 0
    if galn[:na].tobytes() != res["alns"][:na].tobytes():
        for f in res["alns"].dtype.names:
            bad = np.nonzero(galn[f][:na] != res["alns"][f][:na])[0]
            assert len(bad) == 0, "%s: alignment field %s differs first at alignment %d" % (what, f, int(bad[0]))
    assert np.array_equal(gops[:2 * nops], res["ops"][:2 * nops]), what + ": alignment ops"
    assert np.array_equal(moff[:n + 1], res["mq_off"][:n + 1]), what + ": mapq records per read"
    for f in ("begin_ref", "end_ref", "begin_q", "end_q", "score", "soc_index", "n_ops", "secondary", "supplementary"):
        assert np.array_equal(mq[f][:nm], res["mq"][f][:nm]), what + ": mapq record field " + f
    assert mq["mapq"][:nm].tobytes() == res["mq"]["mapq"][:nm].tobytes(), what + ": mapq bits"
    return na, nops, nm


# (workload, reads, read length, sub / ins / del rates of BASELINE.json's configs, read seed, presets)
SCALE_CASES = [
    ("150bp", 100000, 150, 0.005, 0.0, 0.0, 11, ("default", "illumina")),
    ("10kb", 2000, 10000, 0.004, 0.003, 0.003, 12, ("default", "pacbio", "nanopore")),
    ("50kb", 256, 50000, 0.03, 0.03, 0.04, 13, ("default", "pacbio", "nanopore")),
]


@pytest.mark.parametrize("case", SCALE_CASES, ids=[c[0] for c in SCALE_CASES])
def test_noisy_reads_at_grch38_scale_vs_oracle(grch38, case):
    """configs[1] / [2] / [4] at the genome size they are quoted on: noisy synthetic reads against the 6.2 Gnt index (positions
    above 2^32, drop-all heuristic and SoC score threshold ON, the repeat families' ambiguity), compared with the oracle record
    by record.  The oracle runs on the index bytes the GPU builder produced (pinned at this scale by
    test_gpu_round4.py::test_index_pinned_at_grch38_scale)."""
    import ma_amd
    idx, oidx = grch38
    name, n, rl, sub, ins, dele, seed, presets = case
    codes, offs, nb = synth_reads(idx, seed, n, rl, sub, ins, dele)
    oh = offs.cpu().numpy()
    ch = codes[:nb].cpu().numpy()
    reads = [ch[int(oh[i]):int(oh[i + 1])] for i in range(n)]
    threads = min(16, os.cpu_count() or 1)
    for preset in presets:
        bt = ma_amd.Batch(idx, ma_amd.Params.preset(preset), n, nb + 64)
        bt.set_reads_device(codes.data_ptr(), offs.data_ptr(), n, nb)
        bt.align()
        bt.sync()
        res = oidx.align(reads, or_params(preset, 1), threads=threads)
        na, nops, nm = assert_same_as_oracle(bt, res, n, "%s/%s" % (name, preset))
        aligned = bt.counts()["aligned_reads"]
        assert aligned == res["n_aligned"] and aligned >= 0.97 * n, (name, preset, aligned)
        assert na >= n * 0.97 and nops > na
        if preset in ("pacbio", "nanopore"):
            # xMaxSupplementaryPerPrim = 100 (parameter.h:1097,1103): the selection differs from the Default set's
            assert ma_amd.Params.preset(preset).max_supplementary == 100
        print("%s %s: %d reads, %d alignments, %d ops, %d mapq records identical" % (name, preset, n, na, nops, nm))
        bt.close()


def test_presets_of_the_c_abi(gpu_device):
    """ma_params_preset = ParameterSetManager::setSelected over the sets of parameter.h:1081-1104; unknown keys fail with the
    reference's text, the sv-* sets (non-rectangular SoC) are refused."""
    import ma_amd
    d, i, ip, pb, on = (ma_amd.Params.preset(k) for k in ("default", "Illumina", "illuminapaired", "pacbio", "NANOPORE"))
    assert (d.seeding_technique, d.max_ambiguity, d.min_num_soc, d.max_num_soc, d.max_supplementary) == (0, 100, 1, 30, 1)
    assert (i.seeding_technique, i.max_ambiguity, i.min_num_soc, i.max_num_soc, i.use_paired_reads) == (1, 500, 10, 20, 0)
    assert (ip.seeding_technique, ip.max_ambiguity, ip.min_num_soc, ip.max_num_soc, ip.use_paired_reads) == (1, 500, 10, 20, 1)
    assert (pb.seeding_technique, pb.max_supplementary, pb.min_num_soc, pb.max_num_soc) == (0, 100, 5, 30)
    assert (on.seeding_technique, on.max_supplementary, on.min_num_soc, on.max_ambiguity) == (1, 100, 5, 100)
    with pytest.raises(RuntimeError, match="can not be found"):
        ma_amd.Params.preset("no-such-set")
    with pytest.raises(RuntimeError, match="not implemented"):
        ma_amd.Params.preset("sv-pacbio")


def test_smem_seeding_of_long_reads_on_compact_entries(gpu_device):
    """Nanopore preset = SMEM seeding of long reads (parameter.h:1101-1104).  The pending lists of binarySeeding.h:296-433 are
    16-byte entries for reads below 2^22 bases (one 22-bit length; the start is shared by a list's entries); MA_SMEM_COMPACT=0
    keeps the 40-byte records.  Both give the oracle's segments, also with uiMinAmbiguity > 0 (no twin merging) and Ns."""
    import ma_amd
    from ma_testlib import rand_genome, sample_reads
    g = rand_genome(55, [400000, 250000], repeat_unit=300, repeat_copies=60, repeat_div=0.08)
    idx = ma_amd.Index.build(g)
    oidx = OrIndex.from_parts(idx.download())
    reads = (sample_reads(g, 40, 2047, 3, sub=0.03, ins=0.03, dele=0.04) + sample_reads(g, 40, 2048, 4, sub=0.03, ins=0.02, dele=0.02)
             + sample_reads(g, 24, 12000, 5, sub=0.03, ins=0.03, dele=0.04, n_rate=0.002) + sample_reads(g, 6, 60000, 6, sub=0.02, ins=0.02, dele=0.02))
    nb = sum(len(r) for r in reads)
    for min_amb in (0, 2):
        op = or_params("nanopore", 1)
        op.min_ambiguity = min_amb
        res = oidx.align(reads, op, threads=8)
        for compact in ("1", "0"):
            os.environ["MA_SMEM_COMPACT"] = compact
            try:
                P = ma_amd.Params.preset("nanopore")
                P.min_ambiguity = min_amb
                bt = ma_amd.Batch(idx, P, len(reads), nb + 64)
                bt.set_reads(reads)
                bt.align()
                bt.sync()
                soff, segs = bt.segments()
                assert np.array_equal(soff, res["seg_off"]), (min_amb, compact)
                assert segs.tobytes() == res["segs"].tobytes(), (min_amb, compact)
                assert_same_as_oracle(bt, res, len(reads), "nanopore min_amb=%d compact=%s" % (min_amb, compact))
                bt.close()
            finally:
                del os.environ["MA_SMEM_COMPACT"]
    idx.close()


def test_bench_cross_leg_parity_and_line_hygiene(gpu_device):
    """ADVICE r4 (medium) + VERDICT r4 item 8: the records of the overlapped and host-to-host legs are compared, byte for byte,
    with the same steps run alone (cross_leg_parity, top-level parity_150bp_h2h / _overlapped); the top-level roofline is the
    single-stream leg's (avg_launch_ms <= that leg's ms_per_step) and quotes the chip's issue peak with the mix ceiling second."""
    from test_gpu_round2 import _bench
    line = _bench(["--workload", "150bp", "--genome-scale", "0.01", "--steps", "4", "--warmup", "1", "--reads-per-step", "40000",
                   "--cpu-sample", "0", "--boundary-reads", "0", "--gpus", "1"])
    w = line["config"]["workloads"][0]
    for leg in ("overlapped", "host_to_host"):
        xp = w[leg]["cross_leg_parity"]
        assert xp["steps_compared"] == 3 and xp["mismatching_steps"] == 0 and xp["alignments"] > 3 * 40000 * 0.95, (leg, xp)
    assert line["parity_150bp_h2h"].startswith("0 mismatching of 3 steps")
    assert line["parity_150bp_overlapped"].startswith("0 mismatching of 3 steps")
    assert abs(line["h2h_over_device_resident_150bp"] - line["value_150bp"] / line["value_150bp_device_resident"]) < 2e-3
    rf = line["roofline"]
    assert rf["avg_launch_ms"] <= w["ms_per_step"] and "one batch at a time" in rf["leg"]
    if rf["bound"] == "valu":
        assert rf["peak"] == 1228.8 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 2e-3 and rf["mix_ceiling"]["peak"] < rf["peak"]


def test_ranks_share_one_device_without_starving_the_host(gpu_device):
    """bench.py with 4 ranks x 5 batches in flight = 20 waiting host threads.  Under the pool's 16-core
    CFS quota spinning stream waits would throttle the whole process group, so bench.py switches the batches to blocking
    (event) waits when ranks x batches exceeds the cores the quota grants.  All 4 ranks run on GPU 0 here (MA_BENCH_ONE_DEVICE,
    gloo; with this process and the launcher, at most six processes have the device open); they share one GPU, so the AGGREGATE
    rate is what must hold: at least 1 / 1.2 of one rank's."""
    from test_gpu_round2 import _bench
    R, NB = 4, 5
    common = ["--workload", "150bp", "--genome-scale", "0.01", "--steps", "6", "--warmup", "1", "--reads-per-step", "100000",
              "--cpu-sample", "0", "--boundary-reads", "0", "--overlap", str(NB)]
    one = _bench(common + ["--gpus", "1"])
    many = _bench(common + ["--gpus", str(R)], nproc=R, env={"MA_BENCH_ONE_DEVICE": "1"}, self_launch=True)
    assert many["n_gpus"] == R
    wr = many["config"]["workloads"][0]
    assert wr["host_to_host"]["aligned_reads"] > 0.95 * R * 6 * 100000
    quota = wr["host_cores"]
    assert wr["host_to_host"]["stream_waits"].startswith("blocking" if R * NB > quota else "spinning"), (quota, wr["host_to_host"]["stream_waits"])
    print("1 rank: %.0f reads/s host to host; %d ranks on one device: %.0f reads/s, waits %s, cfs throttled %s" % (
        one["value"], R, many["value"], wr["host_to_host"]["stream_waits"], many.get("cfs_throttled_150bp")))
    assert many["value"] >= one["value"] / 1.2, (one["value"], many["value"])
    assert many["parity_150bp_h2h"].startswith("0 mismatching")


def short_extension_cases(n, seed):
    """Extension jobs as the pipeline emits them for read ends and dual extensions (needlemanWunsch.cpp:239-622): queries of
    1..64 bases (the kernel that runs several jobs per wavefront, ksw_grp.h, takes qlen <= 64), targets from shorter than the
    query to query + 1000 padded bases, band 512, z-drop 200 (or small: it must fire), left-aligned or right-aligned with a
    reversed cigar; the query is a noisy copy of the target's head, a copy with a gap, junk, a tandem repeat, or holds Ns."""
    from ma_testlib import KSW_EXTZ, KSW_REV, KSW_RIGHT
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(n):
        ql = int(rng.choice([1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64])) if rng.random() < 0.3 else int(rng.integers(1, 65))
        kind = rng.random()
        tl = int(rng.choice([1, 2, ql, ql + 1, max(1, ql - 3), ql + 40, ql + 500, ql + 1000]))
        t = rng.integers(0, 4, size=tl, dtype=np.uint8)
        if kind < 0.12:  # tandem repeat: late maxima are plausible
            unit = rng.integers(0, 4, size=int(rng.integers(1, 7)), dtype=np.uint8)
            t = np.tile(unit, tl // len(unit) + 1)[:tl].copy()
        if kind < 0.75:
            q = np.resize(t, ql).copy() if tl < ql else t[:ql].copy()
            er = rng.choice([0.0, 0.02, 0.08, 0.2, 0.4])
            mut = rng.random(ql) < er
            q[mut] = (q[mut] + rng.integers(1, 4, size=int(mut.sum()), dtype=np.uint8)) % 4
            if rng.random() < 0.4 and ql > 8:  # an indel
                p = int(rng.integers(2, ql - 2))
                g = int(rng.integers(1, 12))
                q = np.concatenate([q[:p], q[p + g:]]) if rng.random() < 0.5 else np.concatenate([q[:p], rng.integers(0, 4, size=g, dtype=np.uint8), q[p:]])
                q = q[:64] if len(q) else t[:1].copy()
            if rng.random() < 0.3:  # the match starts after a bad first base (a seed ended there)
                q[0] = (q[0] + 1) % 4
        else:
            q = rng.integers(0, 4, size=ql, dtype=np.uint8)  # junk: lives until the early stop proves it dead
        if rng.random() < 0.1:
            q = q.copy()
            q[rng.random(len(q)) < 0.2] = 4  # N
        zd = int(rng.choice([200, 200, 200, 30, 10, 3]))
        fl = KSW_EXTZ if rng.random() < 0.5 else (KSW_EXTZ | KSW_RIGHT | KSW_REV)
        cases.append((np.ascontiguousarray(q, dtype=np.uint8), np.ascontiguousarray(t, dtype=np.uint8), 512, zd, fl))
    return cases


@pytest.mark.parametrize("scoring", [None, (3, 5, 6, 3, 30, 2), (1, 3, 5, 2, 24, 1), (2, 4, 12, 1, 6, 3)])
def test_short_extensions_that_share_a_wavefront(gpu_device, scoring, monkeypatch):
    """ksw_grp.h: 2 or 4 short extension jobs per wavefront.  What the callers read -- max, max_q, max_t
    and the cigar (needlemanWunsch.cpp:239-622) -- against the oracle's kswcpp (every diagonal, kswcpp_core.h:308-879) and
    against the one-job-per-wavefront kernels (MA_KSW_GRP=0), incl. z-drops, Ns, ragged last sets and a swapped gap model."""
    import ma_amd
    from ma_testlib import or_ksw
    P = ma_amd.Params.preset("default")
    op = or_params("default", 1)
    if scoring is not None:
        for prm in (P, op):
            prm.match, prm.mismatch, prm.gap, prm.extend, prm.gap2, prm.extend2 = scoring
    for n, seed in ((3001, 5), (7, 6), (1, 7), (2, 8)):
        cases = short_extension_cases(n, seed + (0 if scoring is None else scoring[0]))
        long_cases = [(np.concatenate([q, q[::-1], q])[:int(65 + (i * 7) % 64)], t, w, zd, fl) for i, (q, t, w, zd, fl) in enumerate(cases[:400]) if len(q) >= 33]
        monkeypatch.setenv("MA_KSW_GRP", "1")
        ez, cigs = ma_amd.ksw_batch(P, cases, pipeline_semantics=True)
        monkeypatch.setenv("MA_KSW_GRP", "2")  # reads as 1: the 65..128-base cases run on k_ksw_ext
        ez2, cigs2 = ma_amd.ksw_batch(P, cases + long_cases, pipeline_semantics=True)
        monkeypatch.setenv("MA_KSW_GRP", "0")
        ez0, cigs0 = ma_amd.ksw_batch(P, cases, pipeline_semantics=True)
        for i, (q, t, w, zd, fl) in enumerate(cases):
            oez, ocig = or_ksw(op, q, t, w, zd, fl)
            what = "case %d (qlen %d tlen %d zdrop %d flag %#x)" % (i, len(q), len(t), zd, fl)
            for f in ("max", "max_q", "max_t"):
                assert int(ez[f][i]) == int(oez[f]), "%s: %s = %d, oracle %d, one job per wave %d" % (what, f, int(ez[f][i]), int(oez[f]), int(ez0[f][i]))
                assert int(ez0[f][i]) == int(oez[f]), what
            assert np.array_equal(cigs[i], ocig), "%s: cigar %s, oracle %s" % (what, cigs[i].tolist(), ocig.tolist())
            assert np.array_equal(cigs0[i], ocig), what
            assert all(int(ez2[f][i]) == int(oez[f]) for f in ("max", "max_q", "max_t")) and np.array_equal(cigs2[i], ocig), what + " (MA_KSW_GRP=2)"
        for k, (q, t, w, zd, fl) in enumerate(long_cases):
            i = len(cases) + k
            oez, ocig = or_ksw(op, q, t, w, zd, fl)
            assert all(int(ez2[f][i]) == int(oez[f]) for f in ("max", "max_q", "max_t")) and np.array_equal(cigs2[i], ocig), (
                "four rows per lane, qlen %d tlen %d flag %#x" % (len(q), len(t), fl))
    monkeypatch.delenv("MA_KSW_GRP")


@pytest.mark.parametrize("slots", [1, 2, 3, 5])
def test_a_late_n_switches_the_score_profile_of_the_exact_kernel(gpu_device, slots):
    """ksw_pk.h scores with three instructions per slot while neither sequence holds an N and re-checks the
    target bases whenever a ring slot is recycled (hasN).  Deterministic cases for the LATE flip: exactly one N in the target
    beyond the first ring (R x 128 cells), exactly one N in the query's tail, an N at the very last base of either -- for every
    ring size of k_ksw_pk<1|2|3|5>, left- and right-aligned: every ez field and the cigar against the oracle."""
    import ma_amd
    from ma_testlib import KSW_EXTZ, KSW_REV, KSW_RIGHT, or_ksw
    P = ma_amd.Params.preset("default")
    op = or_params("default", 1)
    rng = np.random.default_rng(900 + slots)
    m = {1: 90, 2: 200, 3: 330, 5: 560}[slots]  # ksw_pk_slots = ceil((min(qlen, tlen, w + 1) + 30) / 128)
    ring = 128 * slots
    cases = []
    for fl in (KSW_EXTZ, KSW_EXTZ | KSW_RIGHT | KSW_REV, 0):
        for where in ("target_beyond_ring", "query_tail", "target_last", "query_last", "none"):
            tl = ring + 300 + int(rng.integers(0, 40))
            t = rng.integers(0, 4, size=tl, dtype=np.uint8)
            ql = m if fl else tl - int(rng.integers(0, 6))  # global jobs: near-square (the band must reach the corner)
            q = t[:ql].copy() if ql <= tl else np.resize(t, ql).copy()
            mut = rng.random(ql) < 0.03
            q[mut] = (q[mut] + rng.integers(1, 4, size=int(mut.sum()), dtype=np.uint8)) % 4
            if where == "target_beyond_ring":
                t[ring + 17] = 4
            elif where == "query_tail":
                q[ql - 7] = 4
            elif where == "target_last":
                t[tl - 1] = 4
            elif where == "query_last":
                q[ql - 1] = 4
            w = 512 if fl else max(20, abs(tl - ql) + 10)
            cases.append((q, t, w, 200 if fl else -1, fl))
    ez, cigs = ma_amd.ksw_batch(P, cases)
    for i, (q, t, w, zd, fl) in enumerate(cases):
        oez, ocig = or_ksw(op, q, t, w, zd, fl)
        for f in oez.dtype.names:
            assert int(ez[f][i]) == int(oez[f]), "case %d (qlen %d tlen %d w %d flag %#x) field %s: %d vs oracle %d" % (
                i, len(q), len(t), w, fl, f, int(ez[f][i]), int(oez[f]))
        assert np.array_equal(cigs[i], ocig), "case %d cigar" % i


def test_one_by_one_gap_fills_are_answered_by_the_enumeration(gpu_device, monkeypatch):
    """A single mismatch between two seeds is a 1 x 1 global kswcpp call (NeedlemanWunsch::ksw, needlemanWunsch.cpp:82-169; 30 % of
    the DP calls of a 150 bp batch).  k_dp_enum writes its result itself -- one M, whatever the bases, as long as the worst
    score cannot lose to a gap (stage_dp.h) -- and lists no job.  Same alignments, ops, mapq bits and counters as with the
    shortcut off (MA_DP_1X1=0) and as the oracle, reads with Ns in the gap included; under a scoring where a gap CAN win the
    shortcut must switch itself off."""
    import ma_amd
    from ma_testlib import rand_genome
    g = rand_genome(31, [300000, 150000], repeat_unit=200, repeat_copies=30, repeat_div=0.06)
    rng = np.random.default_rng(5)
    reads = []
    for i in range(4000):  # 150 bp reads with 1..3 isolated substitutions (or Ns) far from the ends: 1 x 1 gaps between seeds
        c = g[i % 2]
        p = int(rng.integers(0, len(c) - 150))
        r = c[p:p + 150].copy()
        for pos in rng.choice(np.arange(25, 125), size=int(rng.integers(1, 4)), replace=False):
            r[pos] = 4 if rng.random() < 0.1 else (r[pos] + int(rng.integers(1, 4))) % 4
        reads.append(r if i % 3 else (3 - r[::-1]).astype(np.uint8) if r.max() < 4 else r)
    idx = ma_amd.Index.build(g)
    oidx = OrIndex.from_parts(idx.download())
    nb = sum(len(r) for r in reads)
    for scoring in (None, (2, 13, 4, 2, 24, 1)):  # the second: a mismatch costs more than two gap openings -- kswcpp returns at once (kswcpp_core.h:340-341)
        P = ma_amd.Params.preset("default")
        op = or_params("default", 1)
        if scoring is not None:
            for prm in (P, op):
                prm.match, prm.mismatch, prm.gap, prm.extend, prm.gap2, prm.extend2 = scoring
        res = oidx.align(reads, op, threads=8)
        out = {}
        for on in ("1", "0"):
            monkeypatch.setenv("MA_DP_1X1", on)
            bt = ma_amd.Batch(idx, P, len(reads), nb + 64)
            bt.set_reads(reads)
            bt.align()
            bt.sync()
            assert_same_as_oracle(bt, res, len(reads), "1x1 shortcut %s, scoring %s" % (on, scoring))
            jobs = bt.dp_jobs()
            out[on] = (bt.counters().copy(), int(((jobs[:, 0] == 1) & (jobs[:, 1] == 1) & (jobs[:, 4] == 0)).sum()))
            bt.close()
        assert np.array_equal(out["1"][0], out["0"][0]), "work counters must not depend on who answers the 1 x 1 jobs"
        assert int(out["1"][0][5]) == int(res["counters"][5])  # ksw calls as the oracle counts them
        if scoring is None:
            assert out["1"][1] > 2000  # there ARE such jobs in this read set
    monkeypatch.delenv("MA_DP_1X1")
    idx.close()


def test_double_buffered_io_of_a_batch_object(gpu_device):
    """ma_batch_stage_reads / _use_staged_reads / _start_mapq_download / _finish_download: five different batches of reads go
    through ONE batch object with the upload of the next reads and the download of the last results running beside the kernels;
    every step's host arrays hold the bytes the serial calls (ma_batch_set_reads + ma_batch_get_mapq_alignments) return for the
    same reads.  Misuse (two staged uploads, taking reads that were never staged, two pending downloads) fails with a message."""
    import torch
    import ma_amd
    L = ma_amd.lib()
    lens = np.array([300000, 200000, 150000], dtype=np.uint64)
    F = int(lens.sum())
    g = torch.empty(F, dtype=torch.uint8, device="cuda")
    assert L.ma_synth_genome_device(C.c_uint64(7), C.c_uint64(F), C.c_int32(1), C.c_void_p(g.data_ptr())) == 0
    idx = ma_amd.Index.build_device(lens, g.data_ptr())
    P = ma_amd.Params.preset("default")
    n, steps = 6000, 5
    host = []
    for k in range(steps):  # different read lengths and error rates per step: the buffers change size from step to step
        rl = (150, 250, 100, 400, 150)[k]
        codes, offs, nb = synth_reads(idx, 100 + k, n, rl, sub=0.01, ins=0.002, dele=0.002)
        hc, ho = ma_amd.HostArray(nb + 64, np.uint8), ma_amd.HostArray(n + 1, np.uint64)
        hc.a[:nb] = codes[:nb].cpu().numpy()
        ho.a[:] = offs.cpu().numpy().astype(np.uint64)
        host.append((hc, ho, nb))
    cap = max(h[2] for h in host) + 64
    # ---- serial reference: one object, set_reads + align + get
    want = []
    bt = ma_amd.Batch(idx, P, n, cap)
    for hc, ho, nb in host:
        bt.set_reads_flat(hc.ptr, ho.ptr, n)
        bt.align()
        bt.sync()
        off, al, ops = bt.mapq_alignments()
        na = int(off[n])
        nops = int(al["ops_off"][na - 1] + al["n_ops"][na - 1]) if na else 0
        want.append((off.copy(), al[:na].copy(), ops[:2 * nops].copy()))
    bt.close()
    # ---- double-buffered, on a stream of its own
    st = torch.cuda.Stream()
    bt = ma_amd.Batch(idx, P, n, cap)
    bt.set_stream(st.cuda_stream)
    with pytest.raises(RuntimeError, match="no reads staged"):
        bt.use_staged_reads()
    out = [(ma_amd.HostArray(n + 1, np.uint64), ma_amd.HostArray(4 * n, ma_amd.ALIGNMENT_DT), ma_amd.HostArray(200 * n, np.uint64))
           for _ in range(2)]
    bt.stage_reads_flat(host[0][0].ptr, host[0][1].ptr, n)
    with pytest.raises(RuntimeError, match="not taken"):
        bt.stage_reads_flat(host[1][0].ptr, host[1][1].ptr, n)
    got = []
    for k in range(steps):
        bt.use_staged_reads()
        if k + 1 < steps:
            bt.stage_reads_flat(host[k + 1][0].ptr, host[k + 1][1].ptr, n)  # beside this step's kernels
        bt.align()
        bt.sync()
        o = out[k & 1]
        assert bt.start_mapq_download(*o) is not None
        if k == 0:
            with pytest.raises(RuntimeError, match="not finished"):
                bt.start_mapq_download(*out[1])
        if k > 0:  # the download of step k runs while step k - 1's arrays are read here
            po = out[(k - 1) & 1]
            got.append(tuple(x.a.copy() for x in po))
        bt.finish_download()
    got.append(tuple(x.a.copy() for x in out[(steps - 1) & 1]))
    # (the arrays of step k - 1 were complete: finish_download of step k - 1 ran before they were copied)
    for k, ((woff, wal, wops), (goff, gal, gops)) in enumerate(zip(want, got)):
        na = int(woff[n])
        assert np.array_equal(goff[:n + 1], woff), k
        assert gal[:na].tobytes() == wal.tobytes(), k
        assert np.array_equal(gops[:len(wops)], wops), k
        assert na > 0.9 * n
    # the serial calls still work on the same object afterwards, and wait for nothing that is not pending
    bt.set_reads_flat(host[2][0].ptr, host[2][1].ptr, n)
    bt.align()
    bt.sync()
    off, al, ops = bt.mapq_alignments()
    assert np.array_equal(off, want[2][0]) and al[:int(off[n])].tobytes() == want[2][1].tobytes()
    bt.finish_download()
    bt.close()
    for hc, ho, _ in host:
        hc.close()
        ho.close()
    for o in out:
        for x in o:
            x.close()
    idx.close()


def band_stats():
    import ma_amd
    out = (C.c_ulonglong * 8)()
    assert ma_amd.lib().ma_debug_band_stats(out) == 0
    return np.array(list(out), dtype=np.int64)


def band_extension_cases(n, seed, qmin=65, qmax=254):
    """Extension jobs of qmin..qmax query bases as the pipeline emits them (band 512, z-drop 200, target = query + up to 1000 padded
    bases): a noisy copy of the target's head that starts with a mismatch (a seed ended there), 0..12 % errors incl. indels of up
    to 30 bases, tandem repeats and low-complexity stretches (where the alignment may wander), junk, Ns."""
    from ma_testlib import KSW_EXTZ, KSW_REV, KSW_RIGHT
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(n):
        ql = int(rng.integers(qmin, qmax + 1))
        tl = int(rng.choice([ql + 1000, ql + 1000, ql + 300, ql + 40, ql, max(1, ql - 20), ql // 2 + 1]))
        t = rng.integers(0, 4, size=tl + 64, dtype=np.uint8)
        kind = rng.random()
        if kind < 0.25:  # repeats: several alignments of about the same score
            unit = rng.integers(0, 4, size=int(rng.integers(1, 12)), dtype=np.uint8)
            s0, L = int(rng.integers(0, max(1, tl // 2))), int(rng.integers(10, 200))
            L = min(L, len(t) - s0)
            t[s0:s0 + L] = np.resize(unit, L)
        er_sub, er_indel = rng.choice([0.0, 0.005, 0.02, 0.05, 0.12]), rng.choice([0.0, 0.0, 0.003, 0.02])
        out, i = [], 0
        while len(out) < ql and i < len(t) - 31:
            u = rng.random()
            if len(out) == 0 and rng.random() < 0.7:
                out.append((int(t[i]) + 1 + int(rng.integers(0, 3))) % 4); i += 1
            elif u < er_sub:
                out.append((int(t[i]) + 1 + int(rng.integers(0, 3))) % 4); i += 1
            elif u < er_sub + er_indel:
                g = int(rng.integers(1, 31))
                if rng.random() < 0.5:
                    out.extend(int(x) for x in rng.integers(0, 4, size=g))
                else:
                    i += g
            else:
                out.append(int(t[i])); i += 1
        q = np.array((out + [0] * ql)[:ql], dtype=np.uint8)
        if kind > 0.93:
            q = rng.integers(0, 4, size=ql, dtype=np.uint8)  # junk
        if rng.random() < 0.05:
            q[rng.random(ql) < 0.1] = 4  # N
        # small z-drops: the reference's test is armed from diagonal 0 (ez.max = 0, max_t = max_q = -1: kswcpp_core.h:22-44), so a
        # first-base mismatch z-drops at r = 0 when zdrop < |mismatch|
        zd = int(rng.choice([200, 200, 200, 100, 30, 10, 3, 0]))
        fl = KSW_EXTZ if rng.random() < 0.5 else (KSW_EXTZ | KSW_RIGHT | KSW_REV)
        cases.append((q, np.ascontiguousarray(t[:tl]), 512, zd, fl))
    return cases


@pytest.mark.parametrize("scoring", [None, (3, 5, 6, 3, 30, 2), (2, 4, 12, 1, 6, 3)])
def test_banded_extensions_are_the_wide_bands_or_handed_back(gpu_device, scoring, monkeypatch):
    """ksw_band.h (MA_KSW_GRP=3): extension jobs on a band of 24 cells, four per wavefront, each one PROVEN after the fact to be
    the wide band's result or handed back to the exact kernel.  Every job's max, max_q, max_t and cigar against the oracle's
    kswcpp at the full band (kswcpp_core.h:308-879); a healthy share of the jobs must be proved (else the test tests nothing)."""
    import ma_amd
    from ma_testlib import or_ksw
    P = ma_amd.Params.preset("default")
    op = or_params("default", 1)
    if scoring is not None:
        for prm in (P, op):
            prm.match, prm.mismatch, prm.gap, prm.extend, prm.gap2, prm.extend2 = scoring
    monkeypatch.setenv("MA_KSW_GRP", "3")
    # every eligible job is tried (MA_KSW_BAND_ALL: no pre-filter), then only those whose query follows the target's main diagonal
    for n, seed, qmin, every in ((6000, 21, 65, True), (1500, 22, 33, True), (3, 23, 65, True), (6000, 24, 65, False)):
        monkeypatch.setenv("MA_KSW_GRP", str(1000 + qmin))  # (33: also the queries of 33..64 bases)
        if every:
            monkeypatch.setenv("MA_KSW_BAND_ALL", "1")
        else:
            monkeypatch.delenv("MA_KSW_BAND_ALL", raising=False)
        cases = band_extension_cases(n, seed + (0 if scoring is None else 10 * scoring[0]), qmin=qmin)
        s0 = band_stats()
        ez, cigs = ma_amd.ksw_batch(P, cases, pipeline_semantics=True)
        s1 = band_stats() - s0
        bad = 0
        for i, (q, t, w, zd, fl) in enumerate(cases):
            oez, ocig = or_ksw(op, q, t, w, zd, fl)
            same = all(int(ez[f][i]) == int(oez[f]) for f in ("max", "max_q", "max_t")) and np.array_equal(cigs[i], ocig)
            if not same and bad < 5:
                print("case %d (qlen %d tlen %d zdrop %d flag %#x): got %s %s, oracle %s %s" % (
                    i, len(q), len(t), zd, fl, [int(ez[f][i]) for f in ("max", "max_q", "max_t")], cigs[i].tolist()[:12],
                    [int(oez[f]) for f in ("max", "max_q", "max_t")], ocig.tolist()[:12]))
            bad += 0 if same else 1
        print("band: %d jobs tried, %d proved, failed checks %s, handed back otherwise %d, %.1f diagonals per job" % (
            s1[0], s1[1], s1[2:6].tolist(), s1[6], s1[7] / max(s1[0], 1)))
        assert bad == 0, "%d of %d jobs differ from the oracle" % (bad, len(cases))
        if every:
            assert s1[0] <= len(cases) and ( n < 100 or s1[0] > 0.5 * len(cases) )  # (a scoring scheme may take some shapes out of the extension kernels' regime)
            assert n < 100 or s1[1] > 0.1 * s1[0], s1  # (the cases are hard on purpose: most of them must FAIL a check)
        else:
            assert 0.05 * len(cases) < s1[0] < len(cases) and s1[1] > 0.3 * s1[0], s1  # (the filter admits up to 5 mismatches; many of the cases have an indel behind them; three eighths run under a z-drop of 10 or less, which check 4 refuses)
    monkeypatch.delenv("MA_KSW_GRP")
    monkeypatch.delenv("MA_KSW_BAND_ALL", raising=False)


def test_host_threads_are_pinned_next_to_the_gpu(gpu_device):
    """ma_host_bind_thread: the calling thread's CPU mask becomes the local_cpulist of the GPU's PCI function (mode 0), its
    complement (mode 1: the A/B experiment of DESIGN.md section 3.8) or everything again (mode -1); a thread started afterwards
    inherits the mask; a one-node host is left alone (n_cpus = 0)."""
    import threading
    import ma_amd
    before = os.sched_getaffinity(0)
    try:
        n = ma_amd.bind_host_thread(0, 0)
        local = os.sched_getaffinity(0)
        if n == 0:
            assert local == before  # no topology information or a single node: nothing changed
            return
        assert n == len(local) and local <= before and len(local) < len(before)
        seen = []
        t = threading.Thread(target=lambda: seen.append(os.sched_getaffinity(0)))
        t.start()
        t.join()
        assert seen[0] == local
        m = ma_amd.bind_host_thread(0, 1)
        other = os.sched_getaffinity(0)
        assert m == len(other) and not (other & local) and (other | local) == before
        assert ma_amd.bind_host_thread(0, -1) == len(before) and os.sched_getaffinity(0) == before
        with pytest.raises(RuntimeError, match="mode must be"):
            ma_amd.bind_host_thread(0, 7)
        dev = C.c_int(-1)
        idx_lens = np.array([5000], dtype=np.uint64)
        import torch
        g = torch.randint(0, 4, (5000,), dtype=torch.uint8, device="cuda")
        idx = ma_amd.Index.build_device(idx_lens, g.data_ptr())
        assert ma_amd.lib().ma_index_device(idx.h, C.byref(dev)) == 0 and dev.value == 0
        idx.close()
    finally:
        os.sched_setaffinity(0, before)
