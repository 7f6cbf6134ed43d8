"""Hand-made seed lists that put the chain stage (ma_chain_batch: the window sweep, the RANSAC line fit, the two line sweeps, the
gap-cost cut with the artifact filter and the strip loop of chain_read, ma_amd/csrc/chain.h) where seeds extracted from sampled
reads rarely or never put it; shared by the golden maker (tests/golden/make_harm_sets_golden.py), test_harm_sets_host.py and
test_gpu_harm_sets.py.

A case is one read: its length (the bases are random, the chain stage does not read them), its seeds in the order handed to
ma_batch_set_seeds, and the name of its parameter set; all cases of one parameter set are one batch (case_batch()).  Every case
has a name, and check() -- the contract ma_batch_set_seeds enforces -- names it in every assertion.  `expect` says what the case
is for: the branches of chain.h it has to run (counted by tests/emul/harm_census.cpp through the CH_HIT hooks) and what has to
come out; test_harm_sets_host.py certifies both before a device sees the case.

The genome: three contigs as in nw_sets.py.  Seeds are written as (q, len, position on the doubled text); a reverse-strand seed
at doubled-text position p >= F is handed in as ExtractSeeds leaves it (segment.h:99-105): mirrored to r = N - 1 - p with
on_forward = 0.  delta is ExtractSeeds' r + (qlen - q) + (qlen + 1) * contig (stripOfConsideration.h:41-53, 97-112; the default
rectangular strips), which StripOfConsiderationSeeds::execute reads as stored (stripOfConsideration.cpp:33, 81).

Parameter sets: every parameter but one reaches the reference through its ParameterSetManager.  sv_penalty does not:
Harmonization::applyFilters reads it from the reference library's own copy of the global parameters (see the note in
test_oracle_vs_ref.py), so the cases of ORACLE_ONLY sets are held to the oracle and the host form only and have no golden.

What the reference leaves undefined, and therefore no case may do (the census rejects it, harm_all_removed_undefined):
  - an outlier removal that leaves no seed of a strand's part of a strip: harmonizeOne then reads (*pSeedsIn)[0] of an empty
    vector (harmonization.cpp:352-356);
  - nothing else was found in harmonization.cpp:251-373 for seeds that keep the contract: linesweep's first shadow always opens
    an interval because r + len and q + len are >= 1.  (The cast of a NaN intercept to int64_t, harmonization.cpp:284/309/319, is
    formally undefined as well; the reference is an x86 program and gets cvttsd2si's 0x8000...0, which double_to_i64 restates, so
    the no-model cases stay.)
fMAD == 0 cannot be reached with len >= 1: a seed contributes the three different ordinates q, q + len / 2 and q + len, so no
value holds more than a third of the points and the median of the absolute deviations is at least 0.5 (seeds of length 1 on one
q: the case smallest_mad).  With it go the model of zero inliers and the 0 / 0 means.

One comparison of chain.h has no case, and cannot have one: `delta_distance > fMAD` of the outlier removal differs from `>=` only
where the distance EQUALS fMAD.  fMAD is a positive multiple of 0.25; the distance is a product of results of tan and sin, and
LibmProbe moves every such result unless it is 0, infinite or NaN -- so a distance that equals fMAD under one libm does not
under the probes, and test_harm_sets_host.py would have to drop the case as one that sits within an ulp of a libm-dependent
threshold.  (The ties of the line sweep, `fO <= fD`, are held by distances that are exactly 0: tie_at_zero_distance.)

Cases dropped because the compiled reference died on them (at most three may go this way): none."""
import functools
import os

import numpy as np

from ma_testlib import OR_SEED_DT, ROOT, rand_genome

GENOME_SEED, CONTIG_LENS = 97, (5003, 701, 3001)
F = sum(CONTIG_LENS)
N = 2 * F
CSTART = (0, CONTIG_LENS[0], CONTIG_LENS[0] + CONTIG_LENS[1])
SRAND_SEED = 1

# name -> (the reference's preset, overrides by the field names of Params / OrParams / ChainParams)
PARAM_SETS = {
    "default": ("default", {}),
    "strict": ("default", {"min_num_soc": 0, "harm_score_min_rel": 0.4}),  # as in test_gpu_chain_split.py
    "minlen": ("default", {"genome_size_disable": 0}),  # the fMinLen gate of the sweep is live on the small genome
    "long": ("pacbio", {"min_num_soc": 5}),  # the preset's own value; reads on both sides of switch_qlen = 800 and one at it
    "noheur": ("default", {"disable_heuristics": 1}),
    "fewsoc": ("default", {"max_num_soc": 2}),  # set_cap = 4 and the try limit with a handful of seeds
    "width": ("default", {"soc_width": 40}),
    "artifact": ("default", {"min_delta_dist": 4, "max_delta_dist": 0.5}),
    "longrel": ("pacbio", {"min_num_soc": 5, "harm_score_min_rel": 0.1}),  # exempt strips that the relative minimum still drops
    "svoff": ("default", {"sv_penalty": 0}),
}
ORACLE_ONLY = ("svoff",)  # no golden: the reference's Harmonization does not take sv_penalty from the parameter set
SWITCH_QLEN = 800

# behaviour -> the hook of chain.h that counts it (harm_census.cpp); every one needs a case whose expect["hits"] names it
BEHAVIOURS = {
    "draw table: a read's generator runs past MA_RNG_TAB draws": "rng_past_table",
    "run_ransac: no model, NaN angle and intercept": "ransac_no_model",
    "run_ransac: s1 == s0 retry": "ransac_same_point_retry",
    "run_ransac: the iteration limit ends the loop": "ransac_iteration_limit",
    "run_ransac: all points inliers, pNo clamped": "ransac_pno_clamped",
    "harmonize_one: outliers removed": "harm_outliers_removed",
    "harmonize_one: n3 <= 1 falls back to S[n / 2]": "harm_middle_seed",
    "harmonize_one: the fallback after outlier removal shrank n": "harm_middle_seed_after_removal",
    "harmonize_one: NaN model, nothing removed": "harm_nan_model",
    "linesweep: every fO <= fD false under a NaN model": "sweep_nan_distance",
    "linesweep: nested or duplicated seeds": "sweep_shadowed",
    "linesweep: shadows equal under ShadowOrder": "sweep_equal_shadows",
    "linesweep: fO == fD keeps the earlier end": "sweep_equal_distance",
    "linesweep: the earlier end is closer": "sweep_not_closer",
    "linesweep: a later shadow pops several earlier ends": "sweep_pops_several",
    "apply_filters: iScore == gap keeps the run": "filt_score_equals_gap",
    "apply_filters: iScore < gap restarts the run": "filt_score_below_gap",
    "apply_filters: gap capped at sv_penalty": "filt_gap_capped",
    "apply_filters: sv_penalty == 0 leaves a large gap uncapped": "filt_gap_uncapped",
    "apply_filters: the optimal range ends at the last seed": "filt_range_ends_at_last",
    "apply_filters: the optimal range ends one before the last seed": "filt_range_ends_one_before_last",
    "apply_filters: the optimal range starts behind the first seed": "filt_range_starts_later",
    "artifact filter: diff is 0 / 0": "art_diff_nan",
    "artifact filter: toPre == min_delta_dist does not trigger": "art_at_min_delta_dist",
    "artifact filter: a seed of length 0 is left in the set": "art_triggered",
    "artifact filter: a run of triggers keeps pre fixed": "art_run_keeps_pre",
    "chain_read: qlen == switch_qlen takes neither branch": "loop_qlen_at_switch",
    "chain_read: lastHarm > curSoC skips a strip of a long read": "loop_skip_soc_below_last_harm",
    "chain_read: lastHarm > curHarm skips a strip of a long read": "loop_skip_harm_below_last",
    "chain_read: soc_score_decrease_tol breaks the loop": "loop_break_soc_decrease",
    "chain_read: a strip is exempt while numTries <= min_num_soc": "loop_strip_exempt",
    "chain_read: harm_score_min skips a strip": "loop_skip_harm_score_min",
    "chain_read: harm_score_min_rel skips a strip": "loop_skip_harm_score_min_rel",
    "chain_read: the equal-score lookahead breaks the loop": "loop_break_lookahead",
    "chain_read: the tail pops repeat sets": "tail_pops_sets",
    "chain_read: the tail stops at min_num_soc": "tail_stops_at_min_num_soc",
    "chain_read: a strip holds seeds of both strands": "loop_both_strands_in_strip",
    "chain_read: the reverse set of a later strip is emitted with strip index 0": "loop_reverse_set_of_later_strip",
    "chain_read: the try limit max_num_soc ends the loop": "loop_try_limit",
    "chain_read: set_cap = 2 * max_num_soc is filled exactly": "loop_set_cap_filled",
    "chain_read: disable_heuristics": "loop_heuristics_off",
    "sweep: delta exactly at the strip's limit is inside (lim >= delta)": "win_delta_at_limit",
    "sweep: a window stops at a contig border": "win_contig_stop",
    "sweep: soc_width replaces the strip width": "win_soc_width",
    "sweep: fMinLen is live and rejects a window": "win_below_min_len",
    "sweep: push_back_no_overlap cuts the earlier strip": "push_overlap",
    "sweep: push_back_no_overlap cuts the new strip": "push_overlap_cur_cut",
    "sweep: push_back_no_overlap drops a strip cut below fMinLen": "push_overlap_back_dropped",
    "sweep: heap ties on accLen go by ambiguity": "soc_tie_by_ambiguity",
}
UNREACHABLE = ("ransac_mad_zero", "ransac_zero_inliers")  # see the module docstring
UNDEFINED = ("harm_all_removed_undefined",)


def golden_path(pset):
    return os.path.join(ROOT, "tests", "golden", "harm_sets.%s.pipe.gz" % pset)


@functools.lru_cache(maxsize=None)
def genome():
    return tuple(rand_genome(GENOME_SEED, CONTIG_LENS))


def contig_of(r):
    return sum(1 for c in CSTART[1:] if r >= c)


def seed_array(qlen, seeds):
    """seeds: (q, len, p[, ambiguity]) with p on the doubled text -> records as ExtractSeeds leaves them"""
    s = np.zeros(len(seeds), dtype=OR_SEED_DT)
    for i, sd in enumerate(seeds):
        q, ln, p = sd[:3]
        fwd = p < F
        r = p if fwd else N - 1 - p
        s[i]["q_start"], s[i]["len"], s[i]["r_start"] = q, ln, r
        s[i]["delta"] = r + (qlen - q) + (qlen + 1) * contig_of(r)
        s[i]["ambiguity"] = sd[3] if len(sd) > 3 else 1
        s[i]["on_forward"] = 1 if fwd else 0
    return s


def case(name, pset, qlen, seeds, hits=(), **expect):
    assert pset in PARAM_SETS, pset
    expect["hits"] = tuple(hits)
    return dict(name=name, pset=pset, qlen=int(qlen), seeds=seed_array(qlen, seeds), expect=expect)


def diag(base, qs, ln, shift=0):
    """seeds of length ln at the query positions qs on the diagonal p = base + q (+ shift)"""
    return [(q, ln, base + q + shift) for q in qs]


A0, A1, A2 = 100, CSTART[1] + 100, CSTART[2] + 500  # places far from every contig end, one per contig
R0 = N - CSTART[0] - 3000  # the reverse strand of contig 0: doubled-text positions N - 5003 .. N


def scattered(base, n, salt, width=240, qspan=3, ln=8):
    """n seeds of one strip that fit no line: q in a narrow range, positions scattered over `width`"""
    rng = np.random.default_rng(4000 + salt)
    return [(int(rng.integers(0, qspan)), ln, base + int(rng.integers(0, width))) for _ in range(n)]


def default_cases():
    out = []

    def add(name, qlen, seeds, hits=(), pset="default", **expect):
        out.append(case(name, pset, qlen, seeds, hits, **expect))

    # ---- the line fit
    add("perfect_diagonal", 150, diag(A0, (0, 40, 80, 120), 30), ("ransac_pno_clamped", "art_diff_nan", "filt_range_ends_at_last"),
        set_lens=[[30, 30, 30, 30]])
    # same q, positions 40 apart, 12 long: no pair of points of two seeds lies between 20 and 70 degrees; the loop ends at the
    # first s1 == s0 retry if no pair of points of ONE seed was drawn before it (k stays 1)
    add("no_model", 250, [(10, 12, A0 + 500 + 40 * i) for i in range(5)],
        ("ransac_no_model", "ransac_same_point_retry", "harm_nan_model", "sweep_nan_distance", "harm_middle_seed", "sweep_shadowed"), set_lens=[[12]])
    add("smallest_mad", 100, [(10, 1, A0 + 700), (10, 1, A0 + 703), (10, 1, A0 + 706)],
        ("harm_middle_seed", "harm_middle_seed_after_removal", "harm_outliers_removed"), set_lens=[[1]])
    # the nested seed B (same q and r as A, shorter) has the distance of A: with rStart == r and q == 0 both are exactly 0,
    # whatever the last bit of tan and sin -- the sums are chosen so that the means, the slope (1) and the intercept are exact
    add("tie_at_zero_distance", 150, [(0, 30, A0 + 1500), (0, 20, A0 + 1500), (40, 30, A0 + 1540), (80, 16, A0 + 1580)],
        ("sweep_equal_distance", "sweep_not_closer", "sweep_shadowed"), set_lens=[[30, 30, 16]])
    add("duplicate_seeds", 150, [(0, 30, A0 + 1700, 1), (0, 30, A0 + 1700, 2), (40, 30, A0 + 1740), (80, 18, A0 + 1780)],
        ("sweep_equal_shadows", "sweep_shadowed"), set_lens=[[30, 30, 18]])
    # O1 and O2 lie 15 beside the diagonal and end behind D3, which is on it: D3 pops both
    add("later_shadow_pops_two", 150, [(0, 15, A0 + 2000), (20, 30, A0 + 2035), (30, 30, A0 + 2045), (40, 20, A0 + 2040), (70, 30, A0 + 2070),
                                      (110, 30, A0 + 2110)], ("sweep_pops_several",), set_lens=[[15, 20, 30, 30]])
    # two strips of seeds that fit no line: each runs RANSAC into its iteration limit, the second one past the table
    add("past_the_draw_table", 250, scattered(A0 + 2400, 16, 1) + scattered(A2, 16, 2), ("rng_past_table", "ransac_iteration_limit",
                                                                                        "harm_outliers_removed"))
    # behind the first strip's draws the second one's outcome (which of its seeds is left) depends on the draws it gets
    add("draws_behind_the_table_decide", 250, scattered(A0 + 2400, 16, 1) + [(10, 12, A2 + 40 * i) for i in range(5)], ("rng_past_table",))
    add("past_the_draw_table_three_strips", 250, scattered(A0 + 2400, 10, 3) + scattered(A1, 10, 4) + scattered(A2, 10, 5), ("rng_past_table",))
    # ---- the gap-cost cut
    add("score_equals_gap", 200, [(0, 1, A0 + 3000), (1, 1, A0 + 3002), (2, 30, A0 + 3003), (60, 40, A0 + 3061), (120, 40, A0 + 3121)],
        ("filt_score_equals_gap",), set_lens=[[1, 1, 30, 40, 40]])
    add("score_below_gap", 230, [(0, 5, A0 + 3300), (6, 5, A0 + 3336), (100, 40, A0 + 3430), (180, 40, A0 + 3510)],
        ("filt_score_below_gap", "filt_range_starts_later"), set_lens=[[5, 40, 40]])
    add("range_ends_before_last", 250, [(0, 30, A0 + 3700), (40, 30, A0 + 3740), (80, 30, A0 + 3780), (120, 30, A0 + 3820), (160, 10, A0 + 3860),
                                        (170, 5, A0 + 3925)], ("filt_range_ends_one_before_last", "filt_gap_capped"), set_lens=[[30, 30, 30, 30, 10]])
    # ---- the artifact filter (default: max_delta_dist 0.1, min_delta_dist 16)
    add("artifact_triggers", 200, [(0, 30, A0 + 4000), (40, 20, A0 + 4060), (80, 30, A0 + 4080), (130, 30, A0 + 4130)], ("art_triggered",),
        set_lens=[[30, 0, 30, 30]])
    add("artifact_at_min_delta_dist", 200, [(0, 30, A0 + 4200), (40, 20, A0 + 4256), (80, 30, A0 + 4280), (130, 30, A0 + 4330)],
        ("art_at_min_delta_dist",), set_lens=[[30, 20, 30, 30]])
    add("artifact_run_keeps_pre", 250, [(0, 30, A0 + 4400), (40, 15, A0 + 4460), (60, 15, A0 + 4500), (110, 30, A0 + 4510), (150, 30, A0 + 4550),
                                        (200, 30, A0 + 4600)], ("art_triggered", "art_run_keeps_pre"), set_lens=[[30, 0, 0, 30, 30, 30]])
    # ---- both strands in one strip: a small inversion.  Reverse seeds lie on the doubled text's second half; mirrored, their
    # deltas fall by 2 per query base
    inv = diag(A2, (0, 30, 130, 160), 25) + diag(N - 1 - (A2 + 100), (70, 85), 12, shift=-70 - 11)
    add("inversion_in_one_strip", 200, inv, ("loop_both_strands_in_strip",), socs=[0, 0])
    # ---- the strip loop below switch_qlen: equal scores
    one = [(10, 30, A0 + 200 + 300 * i) for i in range(6)]
    add("lookahead_breaks_and_tail_pops", 100, one, ("loop_break_lookahead", "tail_pops_sets"), nsets=1)
    add("tail_pops_without_break", 100, one[:3], ("tail_pops_sets",), nsets=1)
    add("score_decrease_breaks", 150, diag(A0, (0, 40, 80, 110), 30) + [(10, 20, A2), (60, 8, A1)], ("loop_break_soc_decrease",), nsets=2)
    add("harm_score_min_skips", 150, diag(A0, (0, 40), 30) + [(10, 17, A2)], ("loop_skip_harm_score_min",), nsets=1)
    # reverse seeds of the second strip: their set is emitted with strip index 0
    add("reverse_set_of_second_strip", 150, diag(A0, (0, 40, 80), 30) + diag(N - 1 - (A2 + 100), (20, 45), 24, shift=-20 - 23),
        ("loop_reverse_set_of_later_strip",), socs=[0, 0])
    # ---- the window sweep
    # two seeds on contig 0 whose deltas differ by exactly the strip width qlen - 2 = 98, a third one a base further
    add("delta_at_strip_limit", 100, [(0, 20, A0 + 4500), (0, 20, A0 + 4598), (50, 20, A0 + 4500 + 50 + 99 + 98)], ("win_delta_at_limit",))
    # the last bases of contig 0 and the first of contig 1: the second seed's delta is inside the first one's strip (15 reference
    # bases for 60 query bases take back most of the qlen + 1 between the contigs), its contig is another
    add("window_stops_at_contig_border", 100, [(0, 8, CSTART[1] - 10), (60, 20, CSTART[1] + 5)], ("win_contig_stop",), nsets=1)
    add("seed_across_contig_border", 100, [(0, 40, CSTART[1] - 20), (50, 30, CSTART[1] + 30)], ())
    add("overlapping_windows", 100, [(0, 20, A0 + 100), (10, 30, A0 + 170), (20, 25, A0 + 250), (30, 20, A0 + 330)], ("push_overlap", "push_overlap_cur_cut"))
    add("heap_tie_by_ambiguity", 100, [(10, 30, A0 + 200, 3), (10, 30, A0 + 900, 1), (10, 30, A0 + 1600, 2)], ("soc_tie_by_ambiguity",))
    add("no_seeds", 80, [], ())
    add("one_seed", 80, [(5, 40, A1 + 20)], (), set_lens=[[40]])
    add("one_reverse_seed", 80, [(5, 40, R0)], (), set_lens=[[40]])
    return out


def other_cases():
    out = []

    def add(pset, name, qlen, seeds, hits=(), **expect):
        out.append(case(name + "_" + pset, pset, qlen, seeds, hits, **expect))

    one = [(10, 30, A0 + 200 + 300 * i) for i in range(6)]
    # strict: no strip is exempt, a set must cover 40 % of its read
    add("strict", "short_seed_dropped", 100, [(10, 39, A0 + 100)], ("loop_skip_harm_score_min_rel",), nsets=0)
    add("strict", "seed_of_40_percent_kept", 100, [(10, 40, A0 + 100)], (), nsets=1)
    add("strict", "second_strip_dropped", 100, diag(A0, (0, 50), 30) + [(10, 39, A2)], ("loop_skip_harm_score_min_rel",), nsets=1)
    add("strict", "equal_scores", 100, [(10, 45, A0 + 200 + 300 * i) for i in range(5)], ("loop_break_lookahead", "tail_pops_sets"))
    # minlen: fMinLen = max(0.002 qlen, 18) = 18
    add("minlen", "window_below_min_len", 100, [(10, 17, A0 + 100), (10, 18, A0 + 900)], ("win_below_min_len",), nsets=1)
    # the window of seed 0 holds seeds 0 and 1, that of seed 1 seeds 1 and 2 and is better: the first is cut to seed 0, 10 < 18
    add("minlen", "cut_strip_dropped", 100, [(10, 10, A0 + 100), (10, 30, A0 + 150), (10, 30, A0 + 210)], ("push_overlap", "push_overlap_back_dropped"))
    add("minlen", "diagonal", 150, diag(A0, (0, 40, 80, 120), 30), (), set_lens=[[30, 30, 30, 30]])
    # long / longrel: min_num_soc = 5.  A long read's strip is qlen - 2 wide, so nine places 900 apart are nine strips; the strips pop by
    # score, equal scores by ambiguity
    places = [100, 1000, 1900, 2800, 3700, CSTART[1] + 100, CSTART[2] + 100, CSTART[2] + 1000, CSTART[2] + 1900]
    singles = [(10, ln, places[i], 1 + i) for i, ln in enumerate((100, 95, 90, 85, 80, 60, 60, 60, 60))]
    add("long", "nine_strips_qlen_799", SWITCH_QLEN - 1, singles, ("loop_strip_exempt", "loop_break_lookahead", "tail_pops_sets"), nsets=6)
    add("long", "nine_strips_qlen_800", SWITCH_QLEN, singles, ("loop_strip_exempt", "loop_qlen_at_switch"), nsets=9)
    add("long", "nine_strips_qlen_801", SWITCH_QLEN + 1, singles, ("loop_strip_exempt", "loop_skip_soc_below_last_harm"), nsets=5)
    # strip 5 holds two seeds of 30 that exclude each other: its score is strip 4's harmonized 60, it harmonizes to 30
    pair = lambda at, ln, amb: [(10, ln, at, amb), (10, ln, at + 50, amb)]  # noqa: E731
    add("long", "harm_below_last_qlen_801", SWITCH_QLEN + 1, [(10, ln, places[i], 1) for i, ln in enumerate((100, 95, 90, 85, 60))] + pair(places[5], 30, 1)
        + [(10, 60, places[6], 3)], ("loop_strip_exempt", "loop_skip_harm_below_last"), nsets=6)
    add("long", "diagonal_with_noise", 1500, diag(A0 + 200, range(0, 1400, 35), 20) + scattered(A0 + 600, 12, 7, width=700, qspan=1400, ln=16), ())
    # longrel: a set must cover 10 % of 700 bases; strips 2 and 3 are exempt and dropped all the same, so the tail stops at
    # min_num_soc before it has popped `repeat` sets
    add("longrel", "tail_stops_early", 700, [(10, 120, places[0]), (10, 110, places[1])] + pair(places[2], 50, 1) + pair(places[3], 48, 1)
        + [(10, 80, places[4 + i], 1 + i) for i in range(4)],
        ("loop_strip_exempt", "loop_skip_harm_score_min_rel", "loop_break_lookahead", "tail_pops_sets", "tail_stops_at_min_num_soc"), nsets=5)
    add("longrel", "diagonal", 900, diag(A0 + 200, range(0, 800, 90), 60), ())
    # noheur: what the heuristics would have dropped stays
    add("noheur", "short_seeds_stay", 150, diag(A0, (0, 40, 80, 110), 30) + [(10, 20, A2), (60, 8, A1)], ("loop_heuristics_off",), nsets=3)
    add("noheur", "equal_scores_stay", 100, one, ("loop_heuristics_off",), nsets=6)
    # fewsoc: max_num_soc = 2, set_cap = 4
    both = lambda base, rbase: diag(base, (0, 30), 25) + diag(rbase, (62, 80), 12, shift=-62 - 11)  # noqa: E731
    add("fewsoc", "both_strands_twice_fill_set_cap", 120, both(A0, N - 1 - (A0 + 70)) + [(q, ln - 1, p) for q, ln, p in both(A2, N - 1 - (A2 + 70))] + [(5, 20, A1)],
        ("loop_set_cap_filled", "loop_try_limit", "loop_both_strands_in_strip", "loop_reverse_set_of_later_strip"), nsets=4, socs=[0, 0, 1, 0])
    add("fewsoc", "third_strip_not_tried", 100, one[:4], ("loop_try_limit",))
    # width: soc_width = 40 instead of qlen - 2
    add("width", "delta_at_fixed_width", 150, [(0, 20, A0 + 100), (0, 20, A0 + 140), (0, 20, A0 + 181)], ("win_soc_width", "win_delta_at_limit"))
    add("width", "diagonal_in_narrow_strip", 150, diag(A0, (0, 40, 80, 120), 30), ("win_soc_width",), set_lens=[[30, 30, 30, 30]])
    # artifact: min_delta_dist = 4, max_delta_dist = 0.5
    add("artifact", "small_offset_triggers", 200, [(0, 30, A0 + 4000), (40, 20, A0 + 4045), (80, 30, A0 + 4080), (130, 30, A0 + 4130)],
        ("art_triggered",), set_lens=[[30, 0, 30, 30]])
    add("artifact", "offset_at_min_delta_dist", 200, [(0, 30, A0 + 4200), (40, 20, A0 + 4244), (80, 30, A0 + 4280), (130, 30, A0 + 4330)],
        ("art_at_min_delta_dist",), set_lens=[[30, 20, 30, 30]])
    # toPre 10, toPost 6: diff = 2 * 4 / 16 is max_delta_dist exactly and does not trigger; toPost 7 does
    add("artifact", "diff_at_max_delta_dist", 200, [(0, 30, A0 + 4400), (40, 20, A0 + 4450), (80, 30, A0 + 4484), (130, 30, A0 + 4534)], (),
        set_lens=[[30, 20, 30, 30]])
    add("artifact", "unequal_offsets_trigger", 200, [(0, 30, A0 + 4400), (40, 20, A0 + 4450), (80, 30, A0 + 4483), (130, 30, A0 + 4533)],
        ("art_triggered",), set_lens=[[30, 0, 30, 30]])
    # svoff (oracle only): a gap of more than sv_penalty's default is charged in full
    add("svoff", "large_gap_uncapped", 250, [(0, 30, A0 + 3700), (40, 30, A0 + 3740), (80, 30, A0 + 3780), (120, 30, A0 + 3820), (160, 10, A0 + 3860),
                                              (170, 30, A0 + 3930)], ("filt_gap_uncapped",))
    add("svoff", "diagonal", 150, diag(A0, (0, 40, 80, 120), 30), (), set_lens=[[30, 30, 30, 30]])
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = default_cases() + other_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return tuple(cases)


def cases_of(pset):
    return tuple(c for c in all_cases() if c["pset"] == pset)


def case_batch(pset, filler=False):
    """(names, reads, read_lens, seed_off, seeds) of a parameter set's cases as one batch.  filler: one more read, longer than 254
    bases with 70 seeds on a diagonal, so that a batch of short reads takes the route of long reads (launch_chain.h)."""
    cases = list(cases_of(pset))
    if filler:
        cases.append(case("filler_long_read", pset, 2200, diag(A2, range(0, 2100, 30), 22)))
    rng = np.random.default_rng(11)
    reads = [rng.integers(0, 4, c["qlen"], dtype=np.uint8) for c in cases]
    off = np.zeros(len(cases) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(c["seeds"]) for c in cases])
    seeds = np.concatenate([c["seeds"] for c in cases] + [np.zeros(0, dtype=OR_SEED_DT)])
    return [c["name"] for c in cases], reads, np.array([c["qlen"] for c in cases], dtype=np.uint64), off, seeds


def check_seeds(name, qlen, sd):
    """The contract of ma_batch_set_seeds (include/ma_amd.h) for the seeds of one read."""
    for f in ("q_start", "len", "r_start", "delta"):
        assert np.all(sd[f] >= 0), (name, f, "negative field")
    assert np.all(sd["len"] >= 1), (name, "empty seed")
    assert np.all(sd["q_start"] + sd["len"] <= qlen), (name, "seed beyond its read")
    assert np.all(sd["on_forward"] <= 1), (name, "on_forward")
    assert np.all(sd["r_start"] < F), (name, "r_start outside the forward text")
    fw = sd["on_forward"] == 1
    assert np.all(sd["r_start"][fw] + sd["len"][fw] <= N), (name, "forward seed beyond the doubled text")
    assert np.all(sd["len"][~fw] <= sd["r_start"][~fw] + 1), (name, "reverse seed beyond the doubled text")
    for x in sd:
        want = int(x["r_start"]) + (qlen - int(x["q_start"])) + (qlen + 1) * contig_of(int(x["r_start"]))
        assert int(x["delta"]) == want, (name, "delta is not ExtractSeeds'", int(x["delta"]), want)


def check(cases=None):
    cases = all_cases() if cases is None else cases
    for c in cases:
        assert 1 <= c["qlen"], c["name"]
        check_seeds(c["name"], c["qlen"], c["seeds"])
        assert set(c["expect"]["hits"]) <= set(BEHAVIOURS.values()), (c["name"], "unknown branch")
    for pset in PARAM_SETS:
        assert cases_of(pset), pset
        assert sum(len(c["seeds"]) for c in cases_of(pset)) <= 600, pset


def write_seeds_file(path, seed_off, seeds):
    """The seeds file of ref_dump chainseeds and harm_census (oracle/dump_format.h, CHSEED01)."""
    with open(path, "wb") as f:
        f.write(b"CHSEED01")
        f.write(np.array([len(seed_off) - 1, len(seeds)], dtype="<u8").tobytes())
        f.write(np.asarray(seed_off, dtype="<u8").tobytes())
        f.write(np.asarray(seeds, dtype=OR_SEED_DT).tobytes())


def param_args(pset, **more):
    """name=value arguments of ref_dump chainseeds and harm_census"""
    over = dict(PARAM_SETS[pset][1], **more)
    return ["%s=%s" % (k, v) for k, v in over.items()]


def apply_params(p, pset):
    """An OrParams / Params of the set's preset with its overrides"""
    for k, v in PARAM_SETS[pset][1].items():
        setattr(p, k, v)
    return p


def hsets_text(read_lens, hset_off, hseed_off, hset_soc, hseeds):
    """Harmonized sets (the layout of Batch.hsets() / OrIndex.chain_seeds) as the R / HARM / h / g lines of the pipe dump."""
    lines = []
    for r in range(len(read_lens)):
        a, e = int(hset_off[r]), int(hset_off[r + 1])
        lines.append("R %d %d" % (r, read_lens[r]))
        lines.append("HARM %d" % (e - a))
        for s in range(a, e):
            sd = hseeds[int(hseed_off[s]):int(hseed_off[s + 1])]
            lines.append("h %d %d" % (hset_soc[s], len(sd)))
            for x in sd:
                lines.append("g %d %d %d %d %d %d" % (x["q_start"], x["len"], x["r_start"], x["ambiguity"], x["on_forward"], x["delta"]))
    return "\n".join(lines) + "\n"
