"""The chain stage's sorts on adversarial and tie-heavy seed lists, CPU part (tests/chain_lists.py has the lists): the census
that certifies what each list makes introsort do, the agreement of std::sort, ss::sort (stdsort.h) and the wave form's host
skeleton (the WS_SERIAL split of wave_sort.h with ss::finish_range) on every list, and the pin of the oracle entry the GPU
tests compare against (OrIndex.chain_seeds)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import chain_lists as cl
from ma_testlib import OrIndex, or_params, parse_pipe_dump, rand_genome, sample_reads, write_case
from test_host_logic import emul  # noqa: F401 (fixture: tests/emul/host_emul)


@pytest.fixture(scope="module")
def counted():
    lists = cl.all_lists()
    return lists, cl.census(lists)


def test_list_set_conditions(counted):
    """What the lists are there for, asserted before anything runs on a GPU: the d = 2 adversary of every length >= 160 gets a
    range of more than WS_SERIAL elements with equal keys in it heap-sorted (lane 0's branch of ws::wave_std_sort), the one of
    130 a range of 17..WS_SERIAL elements (ss::finish_range's branch), and on every list with ties std::sort's permutation is
    not a stable sort's."""
    lists, c = counted
    serial, shift = cl.ws_constants()
    assert (serial, shift) == (128, 20)  # the lengths of chain_lists.LENGTHS straddle this WS_SERIAL
    for n in cl.LENGTHS:
        ev = c["adversary_d2_%d" % n]["events"]
        if n >= 160:
            assert any(ln > serial and ties for ln, ties in ev), (n, ev)
        if n == 130:
            assert any(16 < ln <= serial and ties for ln, ties in ev), (n, ev)
    # the table of the census this set was designed around (range that is heap-sorted at depth 0)
    want = {130: 102, 160: 132, 200: 172, 1025: 985, 2000: 1960}
    for d in (1, 2):
        for n, ln in want.items():
            assert [e[0] for e in c["adversary_d%d_%d" % (d, n)]["events"]] == [ln], (d, n)
    stable = sorted((p, n) for name, p, n, _ in lists if p in cl.TIED and not c[name]["unstable"])
    assert stable == sorted(cl.DROPPED), stable
    for name, p, n, keys in lists:
        assert (len(np.unique(keys)) < n) == (p in cl.TIED), name


def test_three_sorts_leave_one_permutation(counted):
    """std::sort, ss::sort and the wave skeleton (introsort loop at WS_SERIAL, heap sort at depth 0, ss::finish_range on every
    range the loop leaves) on (key << 20 | index) under PackedKeyLess's order: one permutation, on every list."""
    lists, c = counted
    bad = [name for name, _, _, _ in lists if not c[name]["perms"]]
    assert not bad, bad
    # the set reaches both heap-sort branches, and finish_range with and without budget left
    ev = [e for name, _, _, _ in cl.list_set() for e in c[name]["events"]]
    assert any(ln > 128 for ln, _ in ev) and any(16 < ln <= 128 for ln, _ in ev)


def test_sixteen_bit_edge_lists_agree_too():
    """The lists of the GPU test at the last wave-sorted and the first lane-sorted size."""
    lists = [("%s_%d" % (p, n), p, n, cl.pattern_keys(p, n)) for n in (65535, 65536) for p in ("few_random", "equal")]
    c = cl.census(lists)
    assert all(c[name]["perms"] and c[name]["unstable"] for name, _, _, _ in lists), c


def test_chain_seeds_reproduces_the_oracles_own_chain_stage():
    """OrIndex.chain_seeds fed the seeds OrIndex.align extracted gives align's harmonized sets: the entry runs the same sweep and
    harmonization, only from given seeds."""
    g = rand_genome(73, [300000, 200000], repeat_unit=300, repeat_copies=80, repeat_div=0.06)
    oidx = OrIndex.build(g)
    reads = sample_reads(g, 300, 150, 1, sub=0.02) + sample_reads(g, 4, 5000, 2, sub=0.02, ins=0.01, dele=0.01)
    for preset in ("default", "illumina"):
        op = or_params(preset, 1)
        res = oidx.align(reads, op, threads=4)
        assert len(res["hseeds"]) > 300 and int(np.diff(res["seed_off"].astype(np.int64)).max()) > 64
        cs = oidx.chain_seeds([len(r) for r in reads], res["seed_off"], res["seeds"], op)
        for k in ("hset_off", "hseed_off", "hset_soc"):
            assert np.array_equal(cs[k], res[k]), (preset, k)
        assert cs["hseeds"].tobytes() == res["hseeds"].tobytes(), preset
        assert np.array_equal(cs["seed_off"], res["seed_off"])
        # the strips: the same ones in both layouts, the first pop is the heap's root, every range inside the read's seeds
        for r in range(len(reads)):
            a, e = int(cs["soc_off"][r]), int(cs["soc_off"][r + 1])
            n = int(cs["seed_off"][r + 1] - cs["seed_off"][r])
            assert sorted(map(tuple, cs["soc_heap"][a:e].tolist())) == sorted(map(tuple, cs["soc_pops"][a:e].tolist()))
            if e > a:
                assert tuple(cs["soc_heap"][a].tolist()) == tuple(cs["soc_pops"][a].tolist())
                assert int(cs["soc_heap"]["end"][a:e].max()) <= n
            s = cs["sorted_seeds"][int(cs["seed_off"][r]):int(cs["seed_off"][r + 1])]
            assert np.all(np.diff(s["r_start"]) >= 0)


def test_stage_logic_on_the_list_set_vs_oracle(emul, tmp_path):  # noqa: F811
    """The product's chain stage compiled for the CPU (chain.h: lane-serial ss::sort, sweep, harmonization) from the seeds of
    every list in both flavours: the strips in pop order with their seeds and the harmonized sets are OrIndex.chain_seeds'.
    What a GPU run of test_gpu_chain_seeds.py compares, minus the wave kernels."""
    g = rand_genome(cl.GENOME_SEED, cl.CONTIG_LENS)
    oidx = OrIndex.build(g)
    names, reads, lens, off, seeds = cl.reads_of_lists(cl.list_set(), ("delta", "refpos"), oidx.contig_starts)
    want = oidx.chain_seeds(lens, off, seeds, or_params("default", 1))
    case, given, out = str(tmp_path / "lists.case"), str(tmp_path / "lists.seeds"), str(tmp_path / "lists.pipe")
    write_case(case, g, reads)
    with open(given, "wb") as f:
        f.write(struct.pack("<Q", len(reads)))
        f.write(off.astype("<u8").tobytes())
        f.write(seeds.tobytes())
    subprocess.check_call([emul, case, "default", "1", out, "all"], env=dict(os.environ, MA_EMUL_SEEDS=given))
    got = parse_pipe_dump(out)
    assert len(got) == len(reads)

    def recs(a):  # dump order of a seed: q, len, r, ambiguity, forward, delta
        return [(int(s["q_start"]), int(s["len"]), int(s["r_start"]), int(s["ambiguity"]), int(s["on_forward"]), int(s["delta"]))
                for s in a]

    for r, rd in enumerate(got):
        so, sd = int(want["seed_off"][r]), want["sorted_seeds"]
        pops = want["soc_pops"][int(want["soc_off"][r]):int(want["soc_off"][r + 1])]
        assert len(rd["socs"]) == len(pops), names[r]
        for c, p in zip(rd["socs"], pops):
            assert (c["score"], c["amb"]) == (int(p["acc_len"]), int(p["ambiguity"])), names[r]
            assert c["seeds"] == recs(sd[so + int(p["begin"]):so + int(p["end"])]), names[r]
        a, e = int(want["hset_off"][r]), int(want["hset_off"][r + 1])
        assert len(rd["hsets"]) == e - a, names[r]
        for h, k in zip(rd["hsets"], range(a, e)):
            assert h["soc"] == int(want["hset_soc"][k]), names[r]
            assert h["seeds"] == recs(want["hseeds"][int(want["hseed_off"][k]):int(want["hseed_off"][k + 1])]), names[r]
