"""The chain stage from GIVEN seeds (Batch.set_seeds -> chain()) against the oracle's sweep and harmonization on the same seeds
with the real std::sort (OrIndex.chain_seeds): the lists of tests/chain_lists.py -- tie-heavy patterns and McIlroy's adversary,
certified on the CPU by test_chain_seeds_host.py -- as the seeds of one read each, so that the heap-sort branches of
ws::wave_std_sort (wave_sort.h) and ss::finish_range / ss::sort (stdsort.h) run on a device, in the LDS form, the global-memory
form and the lane-serial form of the sorts.

What each comparison sees: socs() sweeps with the lane-serial ss::sort whatever the environment (k_soc_dump); the wave kernels
of ma_chain_batch show in hsets(), which depend on the order both sorts leave among equal keys (RANSAC draws its samples by
position in the strip, the line sweeps break ties by position)."""
import time

import numpy as np
import pytest

import chain_lists as cl
from ma_testlib import OrIndex, or_params, rand_genome, sample_reads

pytestmark = pytest.mark.gpu

WSORT_MIN, WSORT_SMALL, WSORT_HUGE = 768, 1024, 65535  # MA_WSORT_* of stage_chain.h

ENVS = [
    {},
    {"MA_WSORT_MIN": "20", "MA_WSORT_SMALL": "200"},
    {"MA_WSORT_MIN": "20", "MA_WSORT_SMALL": "1024"},
    {"MA_CHAIN_WAVE_SORT": "0"},
    {"MA_WSORT_MIN": "20", "MA_SOC_WAVE": "0"},
    {"MA_WSORT_MIN": "20", "MA_SOC_WAVE": "2"},
]
# list lengths (chain_lists.LENGTHS) each environment is meant to send to the LDS form / the global-memory form of
# k_sort_seeds_wave; the others are sorted by their lane
MEANT = [
    ((1023, 1024), (1025, 2000, 4096)),
    ((20, 21, 64, 65, 127, 128, 129, 130, 160, 199, 200), (257, 1023, 1024, 1025, 2000, 4096)),
    ((20, 21, 64, 65, 127, 128, 129, 130, 160, 199, 200, 257, 1023, 1024), (1025, 2000, 4096)),
    ((), ()),
    ((20, 21, 64, 65, 127, 128, 129, 130, 160, 199, 200, 257, 1023, 1024), (1025, 2000, 4096)),
    ((20, 21, 64, 65, 127, 128, 129, 130, 160, 199, 200, 257, 1023, 1024), (1025, 2000, 4096)),
]


def sort_form(n, env):
    """Which form of the sort ma_chain_batch (launch_chain.h) gives a read of n seeds under the thresholds in force."""
    if env.get("MA_CHAIN_WAVE_SORT") == "0":
        return "lane"
    ws_min = max(17, int(env["MA_WSORT_MIN"])) if "MA_WSORT_MIN" in env else WSORT_MIN
    ws_small = min(max(17, int(env["MA_WSORT_SMALL"])), WSORT_SMALL) if "MA_WSORT_SMALL" in env else WSORT_SMALL
    if ws_min <= n <= ws_small:
        return "lds"
    if max(ws_small + 1, ws_min) <= n <= WSORT_HUGE:
        return "global"
    return "lane"


@pytest.fixture(scope="module")
def ctx(gpu_device):
    import ma_amd
    g = rand_genome(cl.GENOME_SEED, cl.CONTIG_LENS)
    idx = ma_amd.Index.build(g)
    oidx = OrIndex.from_parts(idx.download())
    P = ma_amd.Params.preset("default")
    P.srand_seed = 1
    yield dict(g=g, idx=idx, oidx=oidx, P=P, op=or_params("default", 1))
    idx.close()


@pytest.fixture(scope="module")
def list_reads(ctx):
    """Both flavours of the whole list set as one batch, and the oracle's result on it (computed once)."""
    names, reads, lens, off, seeds = cl.reads_of_lists(cl.list_set(), ("delta", "refpos"), ctx["oidx"].contig_starts)
    return dict(names=names, reads=reads, lens=lens, off=off, seeds=seeds, want=ctx["oidx"].chain_seeds(lens, off, seeds, ctx["op"]))


def chain_given_seeds(ctx, reads, off, seeds):
    """set_seeds -> chain() on a fresh batch: (hsets, socs(heap=True), socs(heap=False), seeds per read)."""
    import ma_amd
    b = ma_amd.Batch(ctx["idx"], ctx["P"], len(reads), sum(len(r) for r in reads) + 64)
    b.set_reads(reads)
    b.set_seeds(off, seeds.astype(ma_amd.api.SEED_DT))
    n_seeds = np.diff(b.seeds()[0].astype(np.int64))
    b.chain()
    b.sync()
    out = b.hsets(), b.socs(heap=True), b.socs(heap=False), n_seeds
    b.close()
    return out


def assert_same_as_oracle(got, want, what):
    hsets, heap, pops, _ = got
    for k, (soc_off, socs, seed_off, sorted_seeds) in (("soc_heap", heap), ("soc_pops", pops)):
        assert np.array_equal(soc_off, want["soc_off"]), (what, k)
        assert np.array_equal(seed_off, want["seed_off"]), (what, k)
        assert sorted_seeds.tobytes() == want["sorted_seeds"].tobytes(), (what, k, "seeds re-sorted by reference position")
        assert socs.tobytes() == want[k].tobytes(), (what, k)
    hoff, hsoff, hsoc, hseeds = hsets
    assert np.array_equal(hoff, want["hset_off"]), what
    assert np.array_equal(hsoff, want["hseed_off"]), what
    assert np.array_equal(hsoc, want["hset_soc"]), what
    assert hseeds.tobytes() == want["hseeds"].tobytes(), what


def test_seeds_round_trip_through_set_seeds(ctx, monkeypatch):
    """seeds() of a normally seeded batch -> set_seeds on a fresh batch -> chain(): the harmonized sets of the fused path, with
    the thresholds at their defaults (every read sorted by its lane) and moved down so that the long reads take the wave kernels."""
    import ma_amd
    g, idx, P = ctx["g"], ctx["idx"], ctx["P"]
    reads = sample_reads(g, 300, 150, 3, sub=0.02) + sample_reads(g, 6, 6000, 4, sub=0.02, ins=0.01, dele=0.01)
    for env in ({}, {"MA_WSORT_MIN": "20"}):
        for kk, v in env.items():
            monkeypatch.setenv(kk, v)
        b = ma_amd.Batch(idx, P, len(reads), sum(len(r) for r in reads) + 64)
        b.set_reads(reads)
        b.seed(), b.extract(), b.chain()
        b.sync()
        want = b.hsets()
        off, seeds = b.seeds()
        b.close()
        assert len(want[3]) > 300 and int(np.diff(off.astype(np.int64)).max()) >= 64
        got = chain_given_seeds(ctx, reads, off, seeds)[0]
        for x, y in zip(got, want):
            assert x.tobytes() == y.tobytes(), env


@pytest.mark.parametrize("k", range(len(ENVS)), ids=["-".join("%s=%s" % kv for kv in e.items()) or "default" for e in ENVS])
def test_adversarial_and_tied_seed_orders(ctx, list_reads, monkeypatch, k):
    """Both flavours of every list as one batch, per environment: the strip array with the re-sorted seeds, the strips in pop
    order and the harmonized sets are the oracle's, byte for byte; and the lists meant for the LDS form, the global-memory form
    and the lane form of the sorts fall there under the thresholds in force.
    MI355X: 1.6 s per environment (396 reads, 235 070 seeds; printed below); the oracle's result is computed once per module (0.4 s)."""
    env = ENVS[k]
    for kk, v in env.items():
        monkeypatch.setenv(kk, v)
    t0 = time.time()
    got = chain_given_seeds(ctx, list_reads["reads"], list_reads["off"], list_reads["seeds"])
    dt = time.time() - t0
    n_seeds = got[3]
    forms = {}
    for (name, fl), n in zip(list_reads["names"], n_seeds):
        forms.setdefault(sort_form(int(n), env), set()).add(int(n))
    count = {f: sum(1 for n in n_seeds if sort_form(int(n), env) == f) for f in ("lds", "global", "lane")}
    print("chain_seeds env %s: %d reads, lists by sort form %s, %.2f s" % (env, len(n_seeds), count, dt))
    lds, glob = MEANT[k]
    assert forms.get("lds", set()) == set(lds), forms
    assert forms.get("global", set()) == set(glob), forms
    assert forms.get("lane", set()) == set(cl.LENGTHS) - set(lds) - set(glob), forms
    assert_same_as_oracle(got, list_reads["want"], env)


@pytest.mark.parametrize("pattern", ["equal"])
def test_sixteen_bit_limit_of_the_wave_sort(ctx, pattern):
    """One read of 65535 seeds -- the last size k_sort_seeds_wave takes: positions packed as first | last << 16, uint16_t
    stopper lists -- and one of 65536, the first size its lane sorts, in both flavours (4 reads): the same comparison as above.
    One lane harmonizes all seeds of a read, so the pattern decides the time.  Measured on an MI355X (set_seeds to the last
    download, 4 reads): all keys equal 5.9 s; n / 16 distinct random keys 123 s (oracle: 0.5 s) -- that pattern passed the same
    comparison when measured and is left out for its time (its lists stay in the CPU census, test_chain_seeds_host.py)."""
    lists = [("%s_%d" % (pattern, n), pattern, n, cl.pattern_keys(pattern, n)) for n in (65535, 65536)]
    names, reads, lens, off, seeds = cl.reads_of_lists(lists, ("delta", "refpos"), ctx["oidx"].contig_starts)
    t0 = time.time()
    want = ctx["oidx"].chain_seeds(lens, off, seeds, ctx["op"])
    t1 = time.time()
    got = chain_given_seeds(ctx, reads, off, seeds)
    t2 = time.time()
    print("chain_seeds 16-bit limit %s: oracle %.2f s, device %.2f s" % (pattern, t1 - t0, t2 - t1))
    assert sorted(sort_form(int(n), {}) for n in got[3]) == ["global", "global", "lane", "lane"]
    assert_same_as_oracle(got, want, pattern)
