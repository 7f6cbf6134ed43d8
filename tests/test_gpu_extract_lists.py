"""Seed extraction from GIVEN segments (Batch.set_segments -> extract() -> seeds(), counts(), counters()) against the plain
reference of tests/extract_lists.py -- a brute-force suffix array of the doubled text, pinned to the oracle and to the compiled
reference's ExtractSeeds by test_extract_lists_host.py --: the hand-made list (every filter edge, the rows of chosen text
positions, rows around the multiples of both sampling intervals, reads without segments or without seeds), batches of exactly
the seed totals at which k_lf_walk's refill protocol changes its path, and a generated batch of one seed more than the launch has
lanes.  Every seed field and the LF-step counter are compared exactly, under the dense SA sample and under MA_SA_DENSE=0:
everything is integer, there are no tolerances.  ma_batch_set_segments refuses what breaks its contract (include/ma_amd.h)."""
import os
import time

import numpy as np
import pytest

import extract_lists as ex
from ma_testlib import rand_genome, sample_reads

pytestmark = pytest.mark.gpu

SEED_FIELDS = ("q_start", "len", "r_start", "delta", "ambiguity", "on_forward")


@pytest.fixture(scope="module")
def indices(gpu_device):
    """{"dense": the index with the default dense SA sample (every 8th row), "sparse": built under MA_SA_DENSE=0 (every 32nd)}"""
    import ma_amd
    ex.check()
    g = list(ex.genome())
    old = os.environ.pop("MA_SA_DENSE", None)
    out = {}
    try:
        out["dense"] = ma_amd.Index.build(g)
        os.environ["MA_SA_DENSE"] = "0"
        out["sparse"] = ma_amd.Index.build(g)
    finally:
        os.environ.pop("MA_SA_DENSE", None)
        if old is not None:
            os.environ["MA_SA_DENSE"] = old
    # the index the device built is the one the plain reference describes
    sa = ex.suffix_array()[0]
    for idx in out.values():
        d = idx.download()
        assert int(d["primary"]) == ex.primary() and int(d["ref_len"]) == ex.N and np.array_equal(d["sa"], sa[::32])
    yield out
    for idx in out.values():
        idx.close()


def new_batch(idx, batch, min_seed_len, max_ambiguity):
    import ma_amd
    names, reads, seg_off, segs = batch
    P = ma_amd.Params.preset("default")
    P.min_seed_len, P.max_ambiguity = min_seed_len, max_ambiguity
    b = ma_amd.Batch(idx, P, len(reads), sum(len(r) for r in reads) + 64)
    b.set_reads(reads)
    return b


def results(b):
    b.sync()
    off, seeds = b.seeds()
    return off.copy(), seeds.copy(), b.counts(), int(b.counters()[2])


def extract_given(idx, batch, min_seed_len, max_ambiguity):
    b = new_batch(idx, batch, min_seed_len, max_ambiguity)
    b.set_segments(batch[2], batch[3])
    b.extract()
    out = results(b)
    b.close()
    return out


def assert_is_the_plain_references(got, batch, min_seed_len, max_ambiguity, shift, what):
    names = batch[0]
    off, seeds, counts, lf = got
    want_off, want = ex.expected_seeds(batch, min_seed_len, max_ambiguity)
    assert counts["segments"] == len(batch[3]) and counts["seeds"] == len(want) == len(seeds), (what, counts, len(want))
    assert np.array_equal(off, want_off), (what, "seed_off", [names[r] for r in np.nonzero(off != want_off)[0]][:5])
    read_of = np.repeat(np.arange(len(names)), np.diff(want_off.astype(np.int64)))
    for f in SEED_FIELDS:
        bad = np.nonzero(seeds[f] != want[f])[0]
        assert len(bad) == 0, (what, f, len(bad), names[read_of[bad[0]]], int(bad[0] - want_off[read_of[bad[0]]]), seeds[bad[0]], want[bad[0]])
    assert seeds.tobytes() == want.tobytes(), what
    steps = ex.expected_lf_steps(batch, min_seed_len, max_ambiguity, shift)
    assert lf == steps, (what, "LF steps", lf, steps)


@pytest.mark.parametrize("sample", list(ex.SHIFTS))
@pytest.mark.parametrize("params", ex.PARAMS, ids=["min%d-amb%d" % p for p in ex.PARAMS])
def test_whole_list_vs_plain_reference(indices, params, sample):
    """The whole list as one batch: seed_off, every field of every seed, the seed count and the LF-step counter are the plain
    reference's, with max_ambiguity 0, 1 and 100 (and without the length filter), under both SA sampling intervals.
    MI355X: 0.001 - 0.008 s per combination (48 reads, 218 segments, 188 - 851 seeds; printed below); the two indices and the
    first use of the device, once per module: 1.6 s."""
    t0 = time.time()
    batch = ex.case_batch()
    got = extract_given(indices[sample], batch, *params)
    print("extract_lists %s %s: %d reads, %d segments, %d seeds, %d LF steps, %.3f s" % (params, sample, len(batch[1]), len(batch[3]), len(got[1]), got[3],
                                                                                      time.time() - t0))
    assert_is_the_plain_references(got, batch, params[0], params[1], ex.SHIFTS[sample], (params, sample))


@pytest.mark.parametrize("total", list(ex.TOTALS) + ["no_seeds", "no_segments"])
def test_sharp_seed_totals(indices, total):
    """Each total at which k_lf_walk takes another path -- fewer seeds than the 8 needy lanes a refill waits for, one wavefront's
    64, the slice of 256, the block -- alone in its batch; a batch whose segments yield no seed; a batch without segments.
    MI355X: under 0.005 s each."""
    batch = ex.no_seed_batch() if total == "no_seeds" else ex.no_segment_batch() if total == "no_segments" else ex.total_batch(total)
    for sample, shift in ex.SHIFTS.items():
        got = extract_given(indices[sample], batch, ex.MIN_SEED_LEN, 0)
        assert len(got[1]) == (total if isinstance(total, int) else 0)
        assert_is_the_plain_references(got, batch, ex.MIN_SEED_LEN, 0, shift, (total, sample))


def test_one_seed_more_than_the_launch_has_lanes(indices):
    """The generated batch of 256 * 2048 + 1 seeds (21 MB): every lane of the capped launch takes a seed and one is left for a
    refill; half the reads finish at once, the others walk longest.  The same comparison as for the list; and a second extract()
    on the same batch gives the same bytes and the same counter -- the queue starts at 0 again, the steps do not double.
    MI355X: 0.05 - 0.06 s per sampling interval for set_segments, both extract() calls, the downloads and the comparison
    (5 877 segments, 3.5 M / 19.8 M LF steps; printed below), 0.25 s for the test with the plain reference's seeds."""
    batch = ex.cap_batch()
    for sample, shift in ex.SHIFTS.items():
        t0 = time.time()
        b = new_batch(indices[sample], batch, ex.MIN_SEED_LEN, 100)
        b.set_segments(batch[2], batch[3])
        b.extract()
        first = results(b)
        assert len(first[1]) == ex.LANE_CAP + 1
        assert_is_the_plain_references(first, batch, ex.MIN_SEED_LEN, 100, shift, ("cap + 1", sample))
        b.extract()
        second = results(b)
        b.close()
        print("extract_lists cap + 1 %s: %d segments, %d seeds, %d LF steps, %.2f s" % (sample, len(batch[3]), len(first[1]), first[3], time.time() - t0))
        assert second[0].tobytes() == first[0].tobytes() and second[1].tobytes() == first[1].tobytes(), ("second extract()", sample)
        assert second[3] == first[3] and second[2] == first[2], ("second extract()", sample, first[3], second[3])


def test_segments_round_trip_through_set_segments():
    """segments() of a normally seeded batch -> set_segments on a fresh batch -> extract(): byte for byte the seeds of the
    fused path.  Twice: 150 bp sampled reads, which the seeding's text mode takes (reads of up to 240 bases), so that its pool
    holds segments that carry their position -- extraction does not walk for them, and the fused path took fewer LF steps than
    the round trip, whose segments all carry rows --; and the same reads with a few of 3 kb, seeded as tasks.  Mirrors
    test_gpu_chain_seeds.test_seeds_round_trip_through_set_seeds.  MI355X: 0.06 s with the index (862 / 1 196 seeds; 411 LF
    steps fused against 5 894 from the given segments of the short reads; printed below)."""
    import ma_amd
    g = rand_genome(73, [300000, 200000], repeat_unit=300, repeat_copies=80, repeat_div=0.06)
    idx = ma_amd.Index.build(g)
    try:
        short = sample_reads(g, 300, 150, 3, sub=0.02)
        P = ma_amd.Params.preset("default")
        assert P.min_ambiguity == 0 and P.seeding_technique == 0  # (what the text mode needs)
        for kind, reads in (("short", short), ("mixed", short + sample_reads(g, 5, 3000, 4, sub=0.02, ins=0.01, dele=0.01))):
            b = ma_amd.Batch(idx, P, len(reads), sum(len(r) for r in reads) + 64)
            b.set_reads(reads)
            b.seed()
            b.extract()
            want = results(b)
            seg_off, segs = b.segments()
            b.close()
            assert len(segs) > 1000 and len(want[1]) > 500 and np.all(segs["sa_start"] >= 1) and int(segs["sa_size"].max()) > 1, kind
            b = ma_amd.Batch(idx, P, len(reads), sum(len(r) for r in reads) + 64)
            b.set_reads(reads)
            b.set_segments(seg_off, segs)
            b.extract()
            got = results(b)
            b.close()
            print("extract_lists round trip %s: %d segments, %d seeds, LF steps %d fused, %d from given segments" % (kind, len(segs), len(got[1]), want[3], got[3]))
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), kind
            assert got[2]["segments"] == want[2]["segments"] and got[2]["seeds"] == want[2]["seeds"], kind
            if kind == "short":
                assert want[3] < got[3], ("the fused path walked for position-carrying segments too", want[3], got[3])
            else:
                assert want[3] == got[3], (kind, want[3], got[3])
    finally:
        idx.close()


def test_refusals_leave_the_batch_usable(indices):
    """Every violation of the contract of ma_batch_set_segments (include/ma_amd.h) is refused on the host, before anything is
    uploaded, with a message that names the read and the segment; counts() then shows no segments, extract() is refused too, and
    the next good set_segments + extract() gives the plain reference's seeds.  Segments at the very limits -- the last row, a
    seed that covers its whole read -- are in that good batch.  MI355X: under 0.005 s."""
    import ma_amd
    pick = ("interval_of_3_rows", "no_segments_middle", "overlapping_segments", "first_and_last_row", "seed_covers_whole_read")
    by_name = {c["name"]: c for c in ex.all_cases()}
    batch = ex.make_batch([by_name[nm] for nm in pick])
    names, reads, seg_off, segs = batch
    b = new_batch(indices["dense"], batch, ex.MIN_SEED_LEN, 0)

    def broken(field, at, value):
        s, o = segs.copy(), seg_off.copy()
        if field == "seg_off":
            o[at] = value
        else:
            s[field][at] = value
        return o, s

    # read 2 has four segments: K is its segment 1
    assert [len(by_name[nm]["segs"]) for nm in pick] == [1, 0, 4, 4, 1]
    K = int(seg_off[2]) + 1
    qlen2, s2 = len(reads[2]), segs[K]
    assert int(segs["sa_start"].max()) == ex.N and int(segs[-1]["q_size"]) + 1 == len(reads[-1])
    rows = "interval outside rows 1 .. %d (read 2, segment 1)" % ex.N
    beyond = "segment ends beyond its read of %d bases (read 2, segment 1)" % qlen2
    bad = [
        (broken("seg_off", 0, 1), "seg_off does not start at 0"),
        (broken("seg_off", 2, 0), "seg_off decreases at read 1"),
        (broken("seg_off", 4, 3), "seg_off decreases at read 3"),
        (broken("q_start", K, -1), "negative field (read 2, segment 1)"),
        (broken("q_size", K, -1), "negative field (read 2, segment 1)"),
        (broken("sa_start", K, -1 - 77), "negative field (read 2, segment 1)"),  # the pool's own position-carrying form
        (broken("sa_size", K, -3), "negative field (read 2, segment 1)"),
        (broken("sa_size", K, 0), "empty interval (read 2, segment 1)"),
        (broken("sa_start", K, 0), rows),
        (broken("sa_start", K, ex.N + 1), rows),
        (broken("sa_start", K, ex.N + 2 - int(s2["sa_size"])), rows),
        (broken("sa_size", K, ex.N + 2 - int(s2["sa_start"])), rows),
        (broken("q_start", K, qlen2 + 1), beyond),
        (broken("q_start", K, qlen2 - int(s2["q_size"])), beyond),
        (broken("q_size", K, qlen2 - int(s2["q_start"])), beyond),
        (broken("q_size", 0, len(reads[0])), "segment ends beyond its read of %d bases (read 0, segment 0)" % len(reads[0])),
    ]
    for turn, ((o, s), message) in enumerate(bad):
        if turn % 3 == 0:  # refusals follow a good call as well as each other
            b.set_segments(seg_off, segs)
            assert b.counts()["segments"] == len(segs)
        with pytest.raises(ma_amd.MaError) as e:
            b.set_segments(o, s)
        assert str(e.value) == "ma_batch_set_segments: " + message
        c = b.counts()
        assert c["segments"] == 0 and c["seeds"] == 0, message
        with pytest.raises(ma_amd.MaError):
            b.extract()
    b.set_segments(seg_off, segs)
    b.extract()
    assert_is_the_plain_references(results(b), batch, ex.MIN_SEED_LEN, 0, ex.SHIFTS["dense"], "after the refusals")
    b.close()
