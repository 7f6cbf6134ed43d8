"""The short-read chain stage with reads of at most one seed answered outside k_chain (k_chain_split, k_chain_list on scratch
packed per read; ma_amd/csrc/stage_chain.h, launch_chain.h): the harmonized sets and the MappingQuality records of every batch
shape are the oracle's, those of MA_CHAIN_SPLIT=0 (every read a lane of k_chain on the thirteen scratch arrays) byte for byte,
and those of a second run of the same batch byte for byte -- the list's order comes out of atomics and must not matter."""
import numpy as np
import pytest

from ma_testlib import OrIndex, or_params, revcomp, sample_reads
import seed_text_cases

pytestmark = pytest.mark.gpu

ALN_FIELDS = ("begin_ref", "end_ref", "begin_q", "end_q", "score", "n_ops", "secondary", "supplementary")
# the default parameter set, and one under which reads of one short seed are dropped: no strip is exempt from the score tests
# and a set must cover 40 % of its read
PARAM_SETS = {"default": {}, "strict": {"min_num_soc": 0, "harm_score_min_rel": 0.4}}


def _mutated(r, k, rng):
    r = r.copy()
    for j in rng.choice(len(r), size=k, replace=False):
        r[j] = (r[j] + 1 + rng.integers(0, 3)) % 4
    return r


def _pool(g):
    """About 3 000 reads: random ones (no seed), exact ones on both strands (one seed), one to three substitutions (two to four
    seeds), one short exact stretch in a random read, reads out of the exact and the diverged repeats (many seeds, several strips), both sides of the contig border and of
    the strand junction, reads of 12 and 240 bases."""
    rng = np.random.default_rng(311)
    out = sample_reads(g, 400, 150, 301, random_frac=1.0)
    exact = sample_reads(g, 1800, 150, 302, sub=0.0)
    for i, r in enumerate(exact):
        r = _mutated(r, (0, 0, 0, 1, 2, 3)[i % 6], rng)
        out.append(revcomp(r) if i % 2 else r)
    out += sample_reads(g, 500, 150, 303, sub=0.02)
    # one short seed: 50 exact bases in a random read (the strict parameter set drops it)
    for i, r in enumerate(sample_reads(g, 200, 50, 304, sub=0.0)):
        r = np.concatenate([rng.integers(0, 4, size=100 - 10 * (i % 5), dtype=np.uint8), r, rng.integers(0, 4, size=10 * (i % 5), dtype=np.uint8)])
        out.append(revcomp(r) if i % 2 else r)
    for k in range(120):
        c, p = seed_text_cases.REPEAT_AT[k % len(seed_text_cases.REPEAT_AT)]
        o = int(rng.integers(0, seed_text_cases.REPEAT_UNIT - 150))
        r = _mutated(g[c][p + o:p + o + 150], k % 3, rng)
        out.append(revcomp(r) if k % 2 else r)
    T = np.concatenate(g)
    border = seed_text_cases.CONTIGS[0]
    for r in (T[border - 75:border + 75], T[border - 149:border + 1], T[border - 1:border + 149], T[:150], T[-150:]):
        out += [r.copy(), revcomp(r)]
    for k in range(40):
        p = 123456 + 1000 * k
        out += [g[0][p:p + 12].copy(), revcomp(g[1][p:p + 12]), _mutated(g[0][p:p + 240], k % 4, rng), revcomp(g[1][p:p + 240])]
    return out


def _per_read(hsets, mq):
    """One bytes object per read: its sets (strip index and seeds of each) and its MappingQuality records (every field but the
    two that index the caller's arrays; the ops themselves are in the raw comparisons)."""
    hoff, soff, soc, seeds = hsets
    moff, alns = mq[0], mq[1]
    out = []
    for r in range(len(hoff) - 1):
        parts = []
        for k in range(int(hoff[r]), int(hoff[r + 1])):
            parts += [b"S", soc[k:k + 1].tobytes(), seeds[int(soff[k]):int(soff[k + 1])].tobytes()]
        for a in alns[int(moff[r]):int(moff[r + 1])]:
            parts += [b"A"] + [a[f].tobytes() for f in ALN_FIELDS] + [np.float64(a["mapq"]).tobytes()]
        out.append(b"".join(parts))
    return out


def _raw(hsets, mq):
    return [x.tobytes() for x in hsets] + [x.tobytes() for x in mq]


@pytest.fixture(scope="module")
def ctx(gpu_device):
    import ma_amd
    g = seed_text_cases.genome()
    reads = _pool(g)
    idx = ma_amd.Index.build(g)
    oidx = OrIndex.from_parts(idx.download())
    want, seeds_of = {}, None
    for name, over in PARAM_SETS.items():
        op = or_params("default", 1)
        for k, v in over.items():
            setattr(op, k, v)
        res = oidx.align(reads, op, threads=8)
        want[name] = _per_read((res["hset_off"], res["hseed_off"], res["hset_soc"], res["hseeds"]), (res["mq_off"], res["mq"]))
        seeds_of = np.diff(res["seed_off"].astype(np.int64))
        if name == "strict":  # reads of one seed that lose their only set
            nset = np.diff(res["hset_off"].astype(np.int64))
            assert int(((seeds_of == 1) & (nset == 0)).sum()) > 50
    yield {"reads": reads, "idx": idx, "want": want, "seeds_of": seeds_of}
    idx.close()


def _params(name):
    import ma_amd
    P = ma_amd.Params.preset("default")
    P.srand_seed = 1
    for k, v in PARAM_SETS[name].items():
        setattr(P, k, v)
    return P


def _run(ctx, which, name, via_soc_heap=False):
    import ma_amd
    reads = [ctx["reads"][i] for i in which]
    b = ma_amd.Batch(ctx["idx"], _params(name), len(reads), sum(len(r) for r in reads) + 64)
    b.set_reads(reads)
    if via_soc_heap:
        b.seed()
        b.extract()
        b.set_soc_heap(*b.socs(heap=True))
        b.chain()
        b.dp()
    else:
        b.align()
    b.sync()
    out = b.hsets(), b.mapq_alignments()
    b.close()
    return out


def _shapes(ctx):
    n = ctx["seeds_of"]
    few, many = np.nonzero(n <= 1)[0], np.nonzero(n >= 2)[0]
    mix = np.random.default_rng(5).permutation(len(n))
    return {"1": mix[:1], "63": mix[:63], "64": mix[100:164], "65": mix[200:265], "no_list": few[:700], "all_listed": many[:700],
            "one_listed": np.concatenate([few[:70], many[:1], few[70:100]]), "full": np.arange(len(n))}


def test_the_pool_has_every_kind_of_read(ctx):
    n = ctx["seeds_of"]
    assert 2500 <= len(n) <= 3500
    for lo, hi, least in ((0, 0, 300), (1, 1, 500), (2, 2, 100), (3, 3, 100), (4, 8, 100), (9, 10 ** 6, 50)):
        assert int(((n >= lo) & (n <= hi)).sum()) >= least, (lo, hi, np.bincount(np.minimum(n, 10)))


@pytest.mark.parametrize("name", list(PARAM_SETS))
def test_every_batch_shape_vs_oracle_vs_unsplit_vs_itself(ctx, monkeypatch, name):
    for shape, which in _shapes(ctx).items():
        got = _run(ctx, which, name)
        mine = _per_read(*got)
        bad = [int(which[i]) for i in range(len(which)) if mine[i] != ctx["want"][name][int(which[i])]]
        assert not bad, (name, shape, "differs from the oracle", bad[:5], [int(ctx["seeds_of"][i]) for i in bad[:5]])
        again = _run(ctx, which, name)
        assert _raw(*again) == _raw(*got), (name, shape, "two runs differ")
        monkeypatch.setenv("MA_CHAIN_SPLIT", "0")
        unsplit = _run(ctx, which, name)
        monkeypatch.delenv("MA_CHAIN_SPLIT")
        assert _raw(*unsplit) == _raw(*got), (name, shape, "differs from MA_CHAIN_SPLIT=0")


def test_strips_given_from_outside_keep_the_old_path(ctx, monkeypatch):
    """ma_batch_set_soc_heap -> ma_chain_batch only harmonizes, every read a lane of k_chain, with and without the switch."""
    which = _shapes(ctx)["full"][::3]
    want = _raw(*_run(ctx, which, "default"))
    assert _raw(*_run(ctx, which, "default", via_soc_heap=True)) == want
    monkeypatch.setenv("MA_CHAIN_SPLIT", "0")
    assert _raw(*_run(ctx, which, "default", via_soc_heap=True)) == want
