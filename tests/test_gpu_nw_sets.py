"""The DP stage from GIVEN harmonized sets (Batch.set_hsets -> dp()) against the oracle's NeedlemanWunsch + MappingQuality on the same
sets (OrIndex.nw_sets, pinned to the compiled reference by tests/golden/nw_sets.*.pipe.gz): the hand-made sets of
tests/nw_sets.py -- overlapping and zero-length seeds, pure INS / DEL gaps, every clamp of nw_window, the off-by-one of the
bridging test, empty sets, score ties in finish_read, and long sets whose seeds and jobs straddle the 64-entry LDS windows of
k_stitch_wave -- every one certified, run through the product's walk on the CPU and through the sanitizers by
test_nw_sets_host.py before it gets here.  Everything is integer or the same double operations: no tolerances."""
import time

import numpy as np
import pytest

import nw_sets as ns
from ma_testlib import OrIndex, or_params, rand_genome, sample_reads

pytestmark = pytest.mark.gpu

ENVS = [{}, {"MA_LANES_PER_WAVE": "64"}, {"MA_STITCH_WAVE": "0"}, {"MA_DP_1X1": "0"}]
ENV_IDS = ["-".join("%s=%s" % kv for kv in e.items()) or "default" for e in ENVS]
FIELDS = ("begin_ref", "end_ref", "begin_q", "end_q", "score", "soc_index", "n_ops", "secondary", "supplementary")


@pytest.fixture(scope="module")
def ctx(gpu_device):
    import ma_amd
    g = list(ns.genome())
    idx = ma_amd.Index.build(g)
    oidx = OrIndex.from_parts(idx.download())  # the index downloaded from the device
    ns.check()
    names, reads, hset_off, hseed_off, hset_soc, seeds = ns.case_batch()
    want = {}
    for sc in ns.SCORINGS:  # the oracle's result, once per scoring
        want[sc] = oidx.nw_sets(reads, hset_off, hseed_off, hset_soc, seeds, ns.or_scoring(or_params("default", 1), sc))
    yield dict(idx=idx, oidx=oidx, names=names, reads=reads, sets=(hset_off, hseed_off, hset_soc, seeds), want=want)
    idx.close()


def params(scoring):
    import ma_amd
    P = ns.or_scoring(ma_amd.Params.preset("default"), scoring)
    P.srand_seed = 1
    return P


def new_batch(ctx, reads, scoring):
    import ma_amd
    b = ma_amd.Batch(ctx["idx"], params(scoring), len(reads), sum(len(r) for r in reads) + 64)
    b.set_reads(reads)
    return b


def downloads(b):
    """(alignments(), mapq_alignments(), aligned reads) with every record's ops gathered in record order."""
    out = []
    for off, alns, ops in (b.alignments(), b.mapq_alignments()):
        flat = np.concatenate([np.zeros(0, dtype=np.uint64)] + [ops[2 * int(x["ops_off"]):2 * (int(x["ops_off"]) + int(x["n_ops"]))] for x in alns])
        out.append((off.copy(), alns.copy(), flat))
    return out[0], out[1], b.counts()["aligned_reads"]


def dp_given_sets(ctx, reads, sets, scoring):
    b = new_batch(ctx, reads, scoring)
    b.set_hsets(*sets)
    b.dp()
    b.sync()
    out = downloads(b)
    b.close()
    return out


def same_mapq(a, b):
    """bit for bit, NaN equal to NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def assert_same_as_oracle(got, want, names, what):
    (aoff, alns, aops), (moff, mq, mops), aligned = got
    for key_off, key_rec, key_ops, off, rec, ops in (("aln_off", "alns", "ops", aoff, alns, aops), ("mq_off", "mq", "mq_ops", moff, mq, mops)):
        assert np.array_equal(off, want[key_off]), (what, key_off, [names[r] for r in np.nonzero(np.diff(off.astype(np.int64)) != np.diff(want[key_off].astype(np.int64)))[0]][:5])
        read_of = np.repeat(np.arange(len(names)), np.diff(off.astype(np.int64)))
        for f in FIELDS:  # order within each read, positions, score, flags
            bad = np.nonzero(rec[f] != want[key_rec][f])[0]
            assert len(bad) == 0, (what, key_rec, f, names[read_of[bad[0]]], rec[bad[0]], want[key_rec][bad[0]])
        assert same_mapq(rec["mapq"], want[key_rec]["mapq"]), (what, key_rec, "mapq")
        wops = np.concatenate([np.zeros(0, dtype=np.uint64)] + [want[key_ops][2 * int(x["ops_off"]):2 * (int(x["ops_off"]) + int(x["n_ops"]))] for x in want[key_rec]])
        assert np.array_equal(ops, wops), (what, key_ops)
    assert aligned == want["n_aligned"], what


@pytest.mark.parametrize("k", range(len(ENVS)), ids=ENV_IDS)
@pytest.mark.parametrize("scoring", list(ns.SCORINGS))
def test_given_sets_vs_oracle(ctx, monkeypatch, scoring, k):
    """The whole list as one batch: alignments(), mapq_alignments() and the aligned-read count are the oracle's -- offsets, every
    record field, the ops, the order within each read, the flags, mapq bit for bit -- for both scorings, with one set per
    wavefront and 64, with and without k_stitch_wave, with the 1 x 1 gap fills answered by the enumeration and by the kernels.
    MI355X: 0.01 - 0.03 s per combination (147 reads, 185 sets, 1 506 kswcpp calls; printed below); building the index and the
    oracle's results, once per module: 1.6 - 1.9 s."""
    for kk, v in ENVS[k].items():
        monkeypatch.setenv(kk, v)
    t0 = time.time()
    got = dp_given_sets(ctx, ctx["reads"], ctx["sets"], scoring)
    print("nw_sets %s %s: %d reads, %d sets, %.2f s" % (scoring, ENVS[k], len(ctx["reads"]), len(ctx["sets"][2]), time.time() - t0))
    assert_same_as_oracle(got, ctx["want"][scoring], ctx["names"], (scoring, ENVS[k]))


def test_long_cases_take_the_wave_kernel_and_give_the_lane_kernels_bytes(ctx, monkeypatch):
    """Routing of the long cases: from the case data, the set spanning 1023 query bases does not meet stitch_is_big's condition
    and every other long set does (the batch's longest read has >= 1024 bases, so the split is on); and what k_stitch_wave
    writes for them is byte for byte what k_stitch writes with MA_STITCH_WAVE=0.  MI355X: 0.01 s."""
    cases = ns.all_cases()
    big = {c["name"]: ns.set_span(c["sets"][0][1]) >= ns.WAVE_SPAN for c in cases if c["name"].startswith("long_")}
    assert max(len(r) for r in ctx["reads"]) >= 1024
    assert [nm for nm, b in big.items() if not b] == ["long_64_seeds_span_1023"] and sum(big.values()) >= 20
    assert ns.set_span([c for c in cases if c["name"] == "long_64_seeds_span_1024"][0]["sets"][0][1]) == ns.WAVE_SPAN
    wave = dp_given_sets(ctx, ctx["reads"], ctx["sets"], "default")
    monkeypatch.setenv("MA_STITCH_WAVE", "0")
    lane = dp_given_sets(ctx, ctx["reads"], ctx["sets"], "default")
    for which, ((woff, wrec, wops), (loff, lrec, lops)) in enumerate(zip(wave[:2], lane[:2])):
        assert woff.tobytes() == loff.tobytes() and wops.tobytes() == lops.tobytes()
        kept = 0
        for r, c in enumerate(cases):
            if c["name"] in big:
                a, e = int(woff[r]), int(woff[r + 1])
                assert (e > a or which == 1) and wrec[a:e].tobytes() == lrec[a:e].tobytes(), c["name"]
                kept += e > a
        assert kept >= 12  # (the sets with a dual gap at every fourth seed score below min_alignment_score: no MappingQuality record)


def test_hsets_round_trip_through_set_hsets_and_a_second_dp(ctx):
    """hsets() of a normally chained batch (150 bp and a few 3 kb sampled reads) -> set_hsets on a fresh batch -> dp(): the
    alignments of the fused path; and a second dp() on the same batch gives the same downloads.  Mirrors
    test_gpu_chain_seeds.test_seeds_round_trip_through_set_seeds.  MI355X: 0.07 s."""
    import ma_amd
    g = rand_genome(73, [300000, 200000], repeat_unit=300, repeat_copies=80, repeat_div=0.06)
    idx = ma_amd.Index.build(g)
    try:
        reads = sample_reads(g, 300, 150, 3, sub=0.02) + sample_reads(g, 5, 3000, 4, sub=0.02, ins=0.01, dele=0.01)
        c2 = dict(ctx, idx=idx)
        b = new_batch(c2, reads, "default")
        b.align()
        b.sync()
        want = downloads(b)
        sets = b.hsets()
        b.close()
        assert len(sets[2]) > 300 and int(np.diff(sets[1].astype(np.int64)).max()) >= 16
        b = new_batch(c2, reads, "default")
        b.set_hsets(*sets)
        for turn in ("first dp()", "second dp()"):
            b.dp()
            b.sync()
            got = downloads(b)
            for x, y in zip(got[:2], want[:2]):
                for u, v in zip(x, y):
                    assert u.tobytes() == v.tobytes(), turn
            assert got[2] == want[2], turn
        b.close()
    finally:
        idx.close()


def test_refusals_leave_the_batch_usable(ctx):
    """Every violation of the contract of ma_batch_set_hsets (include/ma_amd.h) is refused on the host, before anything is
    uploaded, with a message that names the read and the set; counts() then shows no sets, dp() is refused too, and the next good
    set_hsets + dp() gives the oracle's result.  MI355X: under 0.01 s."""
    import ma_amd
    cases = [c for c in ns.all_cases() if c["name"] in ("gap_2x1_fwd", "read_without_sets", "three_places_equal_scores_210", "gap_21x5_rev")]
    names, reads, hset_off, hseed_off, hset_soc, seeds = ns.case_batch(cases)
    want = ctx["oidx"].nw_sets(reads, hset_off, hseed_off, hset_soc, seeds, or_params("default", 1))
    b = new_batch(ctx, reads, "default")

    def broken(field, at, value, off=None):
        s, ho, so = seeds.copy(), hset_off.copy(), hseed_off.copy()
        if field == "hset_off":
            ho[at] = value
        elif field == "hseed_off":
            so[at] = value
        else:
            s[field][at] = value
        return ho, so, hset_soc, s

    # read 2 has three sets of one seed each: S is its set 1, K that set's seed
    assert [len(c["sets"]) for c in cases] == [1, 1, 3, 0]
    S = int(hset_off[2]) + 1
    K = int(hseed_off[S])
    assert int(hseed_off[S + 1]) == K + 1
    qlen2, s3 = len(reads[2]), seeds[K]
    bad = [
        (broken("hset_off", 1, 3), "hset_off decreases at read 1"),
        (broken("hseed_off", S + 1, K - 1), "hseed_off decreases (read 2, set 1)"),
        (broken("q_start", K, -1), "negative field (read 2, set 1, seed 0)"),
        (broken("len", K, -5), "negative field (read 2, set 1, seed 0)"),
        (broken("r_start", K, -7), "negative field (read 2, set 1, seed 0)"),
        (broken("delta", K, -1), "negative field (read 2, set 1, seed 0)"),
        (broken("len", K, qlen2 - int(s3["q_start"]) + 1), "seed ends beyond its read of %d bases (read 2, set 1, seed 0)" % qlen2),
        (broken("q_start", K, qlen2 + 1), "seed ends beyond its read of %d bases (read 2, set 1, seed 0)" % qlen2),
        (broken("r_start", K, ns.N - int(s3["len"]) + 1), "seed ends beyond the doubled text of %d bases (read 2, set 1, seed 0)" % ns.N),
        (broken("r_start", 0, ns.N + 5), "seed ends beyond the doubled text of %d bases (read 0, set 0, seed 0)" % ns.N),
    ]
    for turn, (sets, message) in enumerate(bad):
        if turn % 3 == 0:  # refusals follow a good call as well as each other
            b.set_hsets(hset_off, hseed_off, hset_soc, seeds)
            assert b.counts()["hsets"] == len(hset_soc)
        with pytest.raises(ma_amd.MaError) as e:
            b.set_hsets(*sets)
        assert str(e.value) == "ma_batch_set_hsets: " + message
        c = b.counts()
        assert c["hsets"] == 0 and c["hseeds"] == 0, message
        with pytest.raises(ma_amd.MaError):
            b.dp()
    # seeds at the very limits are taken: the whole read, the last base of the text
    b.set_hsets(hset_off, hseed_off, hset_soc, seeds)
    b.dp()
    b.sync()
    assert_same_as_oracle(downloads(b), want, names, "after the refusals")
    b.close()
