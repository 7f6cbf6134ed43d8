"""Seed extraction on hand-made segment lists, CPU part (tests/extract_lists.py has the cases and the plain reference).  In the
order a case has to pass before a device sees it: the contract of the list and what it covers, the certification of what each case
is for from the plain reference's own output, the brute-force suffix array against the oracle's bwt_sa, the plain reference
against the oracle's extraction on sampled reads, and against the compiled reference's ExtractSeeds on the list itself."""
import gzip

import numpy as np
import pytest

import extract_lists as ex
from ma_testlib import OrIndex, or_params, sample_reads

SEED_FIELDS = ("q_start", "len", "r_start", "delta", "ambiguity", "on_forward")


@pytest.fixture(scope="module")
def batch():
    ex.check()
    return ex.case_batch()


@pytest.fixture(scope="module")
def expected(batch):
    """{(min_seed_len, max_ambiguity): (seed_off, seeds)} of the whole list"""
    return {p: ex.expected_seeds(batch, *p) for p in ex.PARAMS}


def test_list_contract_and_coverage(batch):
    """check() holds, the genome is what the cases need, every kind of case the list is there for is in it, and the size stays small."""
    names, reads, seg_off, segs = batch
    cases = ex.all_cases()
    assert len(ex.CONTIG_LENS) >= 3 and all(ln % 4 for ln in ex.CONTIG_LENS) and min(ex.CONTIG_LENS) < 32 and 2500 <= ex.F <= 3500
    assert [len(g) for g in ex.genome()] == list(ex.CONTIG_LENS) and ex.N == 2 * ex.F == len(ex.text())
    for nm in ("seed_of_min_seed_len_minus_1_bases", "seed_of_exactly_min_seed_len_bases", "seed_of_min_seed_len_plus_1_bases",
               "interval_of_1_rows", "interval_of_2_rows", "interval_of_3_rows", "interval_of_99_rows", "interval_of_100_rows",
               "interval_of_101_rows", "made_up_interval", "row_primary", "row_of_text_position_0", "row_of_text_position_n_minus_1",
               "row_of_last_forward_base", "row_of_first_reverse_base", "first_and_last_row", "intervals_straddle_samples", "q_start_0",
               "seed_ends_at_read_end", "seed_covers_whole_read", "read_of_one_base", "no_segments_first", "no_segments_middle",
               "no_segments_last", "longest_walks", "only_sampled_rows", "all_segments_filtered", "filtered_between_kept",
               "identical_segments", "overlapping_segments"):
        assert nm in names, nm
    for c in range(len(ex.CONTIG_LENS)):
        for end in ("first", "last"):
            for strand in ("forward", "reverse"):
                assert "row_of_%s_base_of_contig_%d_%s" % (end, c, strand) in names
    assert {0, 1, 7, 31} <= {m % 32 for m in ex.ROW_MODS} and {0, 1, 7} <= {m % 8 for m in ex.ROW_MODS}
    for base in ex.ROW_BASES:
        assert base % 64 == 0 and "rows_around_samples_%d" % base in names
    assert names[0] == "no_segments_first" and names[-1] == "no_segments_last"
    i = names.index("no_segments_middle")
    assert not len(cases[0]["segs"]) and not len(cases[-1]["segs"]) and not len(cases[i]["segs"])
    assert names[i - 1] == "longest_walks" and names[i - 2] == "no_segments_before_long_walks" and len(cases[i + 1]["segs"])
    assert min(len(r) for r in reads) == 1 and max(len(r) for r in reads) > 3000
    assert len(cases) <= 400 and max(ex.n_seeds(batch, *p) for p in ex.PARAMS) <= 20000
    assert set(ex.PARAMS) >= {(16, 0), (16, 1), (16, 100)} and set(ex.SHIFTS.values()) == {3, 5}


def test_cases_are_what_they_are_for(batch, expected):
    """Certification from the plain reference's own output: every expectation a case carries (extract_lists.py) holds."""
    names, reads, seg_off, segs = batch
    sa, row, lf = ex.suffix_array()
    seen = set()
    for r, c in enumerate(ex.all_cases()):
        nm, e = c["name"], c["expect"]
        seen.update(e)
        for p in ex.PARAMS:  # the filters: how many seeds the case yields under every parameter set
            off, seeds = expected[p]
            assert int(off[r + 1]) - int(off[r]) == e["count"][p], (nm, p)
        off, seeds = expected[(16, 0)]
        mine = seeds[int(off[r]):int(off[r + 1])]
        if "seed" in e:  # the record follows from the text position alone
            assert len(mine) == 1 and {f: int(mine[0][f]) for f in SEED_FIELDS} == e["seed"], (nm, mine, e["seed"])
        if "rows" in e:
            assert [int(k) for k in c["segs"]["sa_start"]] == e["rows"] and all(1 <= k <= ex.N for k in e["rows"]), nm
            for shift in ex.SHIFTS.values():
                st = ex.walk_steps(shift)[e["rows"]]
                assert all((st[i] == 0) == (k % (1 << shift) == 0) for i, k in enumerate(e["rows"])), (nm, shift)
                assert (st > 0).sum() >= 6
        if "straddles" in e:
            for a, n, interval in e["straddles"]:
                assert a % interval and (a + n - 1) // interval > a // interval, (nm, a, n)
        if e.get("real"):
            a, n = int(c["segs"]["sa_start"][0]), int(c["segs"]["sa_size"][0])
            pos = np.sort(sa[a:a + n])
            pat = ex.text()[pos[0]:pos[0] + 8].tobytes()
            assert all(ex.text()[p:p + 8].tobytes() == pat for p in pos) and n in (2, 3, 100, 101), nm
            assert ex.REPEAT_AT in pos and np.all(np.diff(pos) == ex.REPEAT_UNIT), (nm, "the copies of the tandem repeat")
        if e.get("longest"):
            st = ex.walk_steps(5)
            assert int(st[c["segs"]["sa_start"]].min()) >= np.sort(st)[-65] and int(st[c["segs"]["sa_start"]].min()) > 60, nm
        if e.get("no_walk"):
            assert all(int(ex.walk_steps(s)[c["segs"]["sa_start"]].sum()) == 0 for s in ex.SHIFTS.values()), nm
    assert {"count", "seed", "rows", "straddles", "real", "longest", "no_walk"} <= seen
    i = names.index("seed_of_exactly_min_seed_len_bases")
    assert int(segs[int(seg_off[i])]["q_size"]) + 1 == ex.MIN_SEED_LEN and expected[(16, 0)][0][i] == expected[(16, 0)][0][i + 1]
    i = names.index("row_primary")
    s = expected[(16, 0)][1][int(expected[(16, 0)][0][i])]
    assert int(s["r_start"]) == 0 and int(s["on_forward"]) == 1 and int(segs[int(seg_off[i])]["sa_start"]) == ex.primary()
    assert ex.primary() % 32 != 0 and int(ex.walk_steps(3)[ex.primary()]) == 1 and int(lf[ex.primary()]) == 0
    # both strands and every contig occur, on_forward both ways
    allseeds = expected[(0, 0)][1]
    assert set(allseeds["on_forward"]) == {0, 1}
    qlen_of = np.repeat([len(x) for x in reads], np.diff(expected[(0, 0)][0].astype(np.int64)))
    contig = (allseeds["delta"] - allseeds["r_start"] - (qlen_of - allseeds["q_start"])) // (qlen_of + 1)
    assert set(int(x) for x in contig) == {0, 1, 2}


def test_sharp_totals_and_generated_batches():
    """The batches cut or padded to the totals where k_lf_walk's refill protocol changes its path hold exactly those totals;
    the generated batch has one seed more than the launch has lanes, a few thousand segments of at most 100 rows, half its reads on
    sampled rows only and the other half on the longest walks."""
    for t in ex.TOTALS:
        b = ex.total_batch(t)
        ex.check(b)
        assert int(ex.expected_seeds(b, 16, 0)[0][-1]) == t == len(ex.expected_seeds(b, 16, 0)[1])
    assert {1, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025} <= set(ex.TOTALS)
    b = ex.no_seed_batch()
    ex.check(b)
    assert len(b[3]) > 0 and len(ex.expected_seeds(b, 16, 0)[1]) == 0
    b = ex.no_segment_batch()
    assert len(b[1]) >= 3 and len(b[3]) == 0 and not ex.expected_seeds(b, 16, 0)[0].any()
    names, reads, seg_off, segs = b = ex.cap_batch()
    ex.check(b)
    off, seeds = ex.expected_seeds(b, 16, 100)
    assert len(seeds) == ex.LANE_CAP + 1 == 256 * 2048 + 1 == int(off[-1])
    assert 2000 <= len(segs) <= 9000 and int(segs["sa_size"].max()) == 100
    st3, st5 = ex.walk_steps(3), ex.walk_steps(5)
    mean5 = st5[1:].mean()
    win = np.convolve(st5[1:], np.ones(ex.CAP_WIDTH, dtype=np.int64), mode="valid")  # win[i]: the steps of rows 1 + i .. 100 + i
    for r, nm in enumerate(names):
        s = segs[int(seg_off[r]):int(seg_off[r + 1])]
        if r % 2 == 0:
            assert np.all(s["sa_size"] == 1) and np.all(s["sa_start"] % 32 == 0) and st3[s["sa_start"]].sum() == 0, nm
        else:
            rows = np.concatenate([np.arange(a, a + n) for a, n in zip(s["sa_start"], s["sa_size"])])
            # (100 neighbouring rows average over short and long walks: "longest" means the windows with the most steps, below)
            assert st5[rows].mean() > mean5 and st3[rows].mean() > st3[1:].mean(), (nm, st5[rows].mean(), mean5)
            full = s[s["sa_size"] == ex.CAP_WIDTH]
            assert len(full) >= len(s) - 1 and np.all(win[full["sa_start"] - 1] >= np.sort(win)[-ex.CAP_WINDOWS]), nm


def test_brute_force_sa_equals_the_oracles_bwt_sa():
    """Rows 1 .. n of the brute-force suffix array against OrIndex.bwt_sa (the FM index walk): the same positions, row by row;
    and the row of position 0 is the index's primary."""
    oidx = OrIndex.build(list(ex.genome()))
    sa = ex.suffix_array()[0]
    assert np.array_equal(oidx.bwt_sa(range(1, ex.N + 1)), sa[1:])
    a = oidx.arrays()
    assert int(a["primary"]) == ex.primary() and int(a["ref_len"]) == ex.N


def test_plain_reference_equals_the_oracles_extraction_on_sampled_reads():
    """OrIndex.align returns segments and seeds: its segments fed to expected_seeds() give its seeds, field by field."""
    g = list(ex.genome())
    oidx = OrIndex.build(g)
    reads = sample_reads(g, 80, 150, 5, sub=0.03, ins=0.005, dele=0.005) + sample_reads(g, 4, 1000, 6, sub=0.03, ins=0.01, dele=0.01)
    for preset, max_amb in (("default", None), ("default", 1), ("default", 0)):
        op = or_params(preset, 1)
        if max_amb is not None:
            op.max_ambiguity = max_amb
        res = oidx.align(reads, op)
        b = (["sampled_%d" % i for i in range(len(reads))], reads, res["seg_off"], res["segs"])
        ex.check(b)
        off, seeds = ex.expected_seeds(b, int(op.min_seed_len), int(op.max_ambiguity))
        assert len(seeds) > 100 and np.array_equal(off, res["seed_off"]), (preset, max_amb)
        for f in SEED_FIELDS:
            assert np.array_equal(seeds[f], res["seeds"][f]), (preset, max_amb, f)
    assert int(res["segs"]["sa_size"].max()) > 1  # (max_ambiguity 0: the repeat's intervals are kept)


def test_plain_reference_vs_reference_golden(batch):
    """The plain reference against the compiled reference's ExtractSeeds::execute on the hand-made list
    (tests/golden/make_extract_golden.py), every parameter set: every seed line."""
    want = gzip.open(ex.golden_path(), "rt").read().splitlines()
    got = "".join(ex.result_text(batch, *p) for p in ex.PARAMS).splitlines()
    r, p = -1, None
    for a, b in zip(got, want):
        if a.startswith("P "):
            p = a
        if a.startswith("R "):
            r = int(a.split()[1])
        assert a == b, (p, batch[0][r], a, b)
    assert len(got) == len(want) and sum(1 for x in want if x.startswith("P ")) == len(ex.PARAMS)
    assert sum(1 for x in want if x.startswith("d ")) > 2000
