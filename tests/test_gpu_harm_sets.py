"""The chain stage on hand-made seeds (tests/harm_sets.py; certified on the CPU by test_harm_sets_host.py) on the device: every
parameter set's batch through set_seeds -> chain() under every route launch_chain.h has --

  default               k_chain_split + k_chain_list (the longest read has at most 254 bases)
  MA_CHAIN_SPLIT=0      k_chain on the thirteen arrays
  with one long filler read added, so that the batch takes the route of long reads:
  MA_WSORT_MIN=20       k_sort_seeds_wave + k_soc_windows_wave take the reads of 20 seeds and more
  .. MA_SOC_WAVE=0 / 2  the sweep of those reads by their lane / by the wave kernel's fallback to the lane form
  MA_CHAIN_WAVE_SORT=0  everything in k_chain
  set_soc_heap          the oracle's queue and re-sorted seeds handed in: k_chain on a given queue

-- and for each the harmonized sets are the oracle's byte for byte (offsets, strip indices, every seed field, seeds of length 0
included) and, as text, the compiled reference's (tests/golden/harm_sets.*.pipe.gz); the strips in both layouts are the oracle's;
a second run gives the same bytes; libm_probe 1 to 5 gives the bytes of mode 0; ma_batch_sync reports no overflow on the case
that fills set_cap exactly.  No tolerance anywhere: the stage's doubles decide, they are not output.
MI355X: 1 to 6 ms per route and batch, set_seeds to the last download (the largest batch: 29 reads, 183 seeds; printed below);
the whole file with the index build and the oracle's results, computed once per module, takes under 3 s."""
import gzip
import time

import numpy as np
import pytest

import harm_sets as hs
from ma_testlib import OrIndex, or_params

pytestmark = pytest.mark.gpu

WAVE_ROUTES = [{"MA_WSORT_MIN": "20"}, {"MA_WSORT_MIN": "20", "MA_SOC_WAVE": "0"}, {"MA_WSORT_MIN": "20", "MA_SOC_WAVE": "2"},
               {"MA_CHAIN_WAVE_SORT": "0"}]


@pytest.fixture(scope="module")
def ctx(gpu_device):
    import ma_amd
    hs.check()
    idx = ma_amd.Index.build(list(hs.genome()))
    oidx = OrIndex.from_parts(idx.download())
    batches = {}
    for pset in hs.PARAM_SETS:
        for filler in (False, True):
            names, reads, lens, off, seeds = hs.case_batch(pset, filler)
            want = oidx.chain_seeds(lens, off, seeds, hs.apply_params(or_params(hs.PARAM_SETS[pset][0], hs.SRAND_SEED), pset))
            batches[pset, filler] = dict(names=names, reads=reads, lens=lens, off=off, seeds=seeds, want=want)
    yield dict(idx=idx, batches=batches)
    idx.close()


def params(pset, libm_probe=0):
    import ma_amd
    P = hs.apply_params(ma_amd.Params.preset(hs.PARAM_SETS[pset][0]), pset)
    P.srand_seed = hs.SRAND_SEED
    P.libm_probe = libm_probe
    return P


def run(ctx, pset, filler=False, libm_probe=0, via_soc_heap=False, with_socs=True):
    """set_seeds (or set_soc_heap with the oracle's queue) -> chain() -> sync(): (hsets, socs(heap=True), socs(heap=False))"""
    import ma_amd
    B = ctx["batches"][pset, filler]
    b = ma_amd.Batch(ctx["idx"], params(pset, libm_probe), len(B["reads"]), sum(len(r) for r in B["reads"]) + 64)
    b.set_reads(B["reads"])
    if via_soc_heap:
        w = B["want"]
        b.set_soc_heap(w["soc_off"], w["soc_heap"].astype(ma_amd.api.SOC_DT), w["seed_off"], w["sorted_seeds"].astype(ma_amd.api.SEED_DT))
    else:
        b.set_seeds(B["off"], B["seeds"].astype(ma_amd.api.SEED_DT))
    b.chain()
    b.sync()  # raises on a scratch or seed overflow
    out = b.hsets(), (b.socs(heap=True) if with_socs else None), (b.socs(heap=False) if with_socs else None)
    b.close()
    return out


def raw(hsets):
    return [x.tobytes() for x in hsets]


def assert_is_oracles(ctx, pset, filler, got, what, socs=True):
    B = ctx["batches"][pset, filler]
    want, names = B["want"], B["names"]
    (hoff, hsoff, hsoc, hseeds), heap, pops = got
    bad = [names[r] for r in range(len(names)) if hoff[r + 1] - hoff[r] != want["hset_off"][r + 1] - want["hset_off"][r]]
    assert not bad, (pset, what, "number of sets", bad)
    assert np.array_equal(hoff, want["hset_off"]) and np.array_equal(hsoff, want["hseed_off"]), (pset, what)
    for r, nm in enumerate(names):
        a, e = int(hoff[r]), int(hoff[r + 1])
        assert np.array_equal(hsoc[a:e], want["hset_soc"][a:e]), (pset, what, nm, "strip indices")
        a, e = int(hsoff[a]), int(hsoff[e])
        assert hseeds[a:e].tobytes() == want["hseeds"][a:e].tobytes(), (pset, what, nm, "seeds")
    assert hseeds.tobytes() == want["hseeds"].tobytes() and hsoc.tobytes() == want["hset_soc"].tobytes(), (pset, what)
    if socs:
        for k, (soc_off, sc, seed_off, sorted_seeds) in (("soc_heap", heap), ("soc_pops", pops)):
            assert np.array_equal(soc_off, want["soc_off"]) and np.array_equal(seed_off, want["seed_off"]), (pset, what, k)
            assert sorted_seeds.tobytes() == want["sorted_seeds"].tobytes(), (pset, what, k)
            assert sc.tobytes() == want[k].tobytes(), (pset, what, k)
    if pset not in hs.ORACLE_ONLY:  # the reference's dump holds the cases only, not the filler read
        n = len(hs.cases_of(pset))
        text = hs.hsets_text(B["lens"][:n], hoff[:n + 1], hsoff, hsoc, hseeds)
        ref = gzip.open(hs.golden_path(pset), "rt").read()
        assert text == ref, (pset, what, "differs from the compiled reference's dump")


@pytest.mark.parametrize("pset", list(hs.PARAM_SETS))
def test_every_route_vs_oracle_and_reference(ctx, monkeypatch, pset):
    times = {}

    def timed(name, **kw):
        t0 = time.time()
        got = run(ctx, pset, **kw)
        times[name] = time.time() - t0
        return got

    got = timed("default")
    assert_is_oracles(ctx, pset, False, got, "default")
    again = run(ctx, pset)
    assert raw(again[0]) == raw(got[0]), (pset, "two runs differ")
    monkeypatch.setenv("MA_CHAIN_SPLIT", "0")
    assert_is_oracles(ctx, pset, False, timed("MA_CHAIN_SPLIT=0"), "MA_CHAIN_SPLIT=0")
    monkeypatch.delenv("MA_CHAIN_SPLIT")
    # (this route does not sweep: the strips are the oracle's own, so only the sets are compared)
    assert_is_oracles(ctx, pset, False, timed("set_soc_heap", via_soc_heap=True, with_socs=False), "set_soc_heap", socs=False)
    B = ctx["batches"][pset, True]
    assert max(len(r) for r in B["reads"]) > 254 and len(B["seeds"]) >= 64
    for env in WAVE_ROUTES:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        name = " ".join("%s=%s" % kv for kv in env.items())
        assert_is_oracles(ctx, pset, True, timed(name, filler=True), name)
        for k in env:
            monkeypatch.delenv(k)
    print("harm_sets %s: %d reads, %d seeds; %s" % (pset, len(ctx["batches"][pset, False]["reads"]), len(ctx["batches"][pset, False]["seeds"]),
                                                      ", ".join("%s %.3f s" % kv for kv in times.items())))


@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5])
def test_no_case_depends_on_the_last_bit_of_the_devices_libm(ctx, mode):
    """libm_probe moves every result of tan, sin, atan and log by an ulp: the sets of every case stay, on both routes of the sweep."""
    for pset in hs.PARAM_SETS:
        for filler in (False, True):
            got = run(ctx, pset, filler=filler, libm_probe=mode, with_socs=False)
            assert_is_oracles(ctx, pset, filler, got, "libm_probe %d" % mode, socs=False)


def test_the_case_that_fills_set_cap_exactly(ctx):
    """2 * max_num_soc sets of one read: every slot of its table written, none beyond; sync() reported nothing (run())."""
    names = ctx["batches"]["fewsoc", False]["names"]
    r = names.index("both_strands_twice_fill_set_cap_fewsoc")
    hoff, hsoff, hsoc, hseeds = run(ctx, "fewsoc", with_socs=False)[0]
    assert int(hoff[r + 1] - hoff[r]) == 2 * hs.PARAM_SETS["fewsoc"][1]["max_num_soc"]
    assert [int(x) for x in hsoc[int(hoff[r]):int(hoff[r + 1])]] == [0, 0, 1, 0]
