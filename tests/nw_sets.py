"""Hand-made harmonized seed sets that put the DP stage (ma_dp_batch: nw_window, NwWalk::run, the stitch kernels, finish_read)
where sets made by seeding and harmonization from sampled reads rarely or never put it; shared by the golden maker
(tests/golden/make_nw_sets_golden.py), test_nw_sets_host.py and test_gpu_nw_sets.py.

A case is one read with its sets in the hsets() layout; all cases together are one batch (case_batch()).  Every case has a name,
and check() -- the contract ma_batch_set_hsets enforces plus the seed order Harmonization guarantees -- names it in every
assertion.  `expect` says what the case is for; test_nw_sets_host.py certifies it from the oracle's result and job list before a
device sees the case.

The genome: three contigs whose lengths are no multiples of 4, the first longer than 2 * padding, the second shorter than
padding.  Positions are on the doubled text T = forward . reverse complement (n = 2 F): a read "cut at p" is T[p : p + L], so the
reverse-strand cases simply lie at p >= F and their seeds carry on_forward = 0.

Cases dropped because the compiled reference died on them (at most three may go this way): none."""
import functools
import os

import numpy as np

from ma_testlib import OR_SEED_DT, ROOT, rand_genome

GENOME_SEED, CONTIG_LENS = 97, (5003, 701, 3001)
PADDING, MAX_GAP_AREA, MAX_OVERLAP_SUPPLEMENTARY, MAX_SUPPLEMENTARY, MIN_ALIGNMENT_SCORE = 1000, 20, 0.1, 1, 75  # "default" preset
# (match, mismatch, gap, extend, gap2, extend2); None: the preset's.  The second has gap2 + extend2 < gap + extend: kswcpp swaps the
# two gap models
SCORINGS = {"default": None, "swapped": (2, 4, 12, 1, 6, 3)}


def golden_path(scoring):
    return os.path.join(ROOT, "tests", "golden", "nw_sets.%s.pipe.gz" % scoring)


def or_scoring(op, scoring):
    """An OrParams (or the product's Params: the same field names) with the scoring of SCORINGS[scoring]."""
    if SCORINGS[scoring] is not None:
        op.match, op.mismatch, op.gap, op.extend, op.gap2, op.extend2 = SCORINGS[scoring]
    return op
F = sum(CONTIG_LENS)
N = 2 * F
CSTART = (0, CONTIG_LENS[0], CONTIG_LENS[0] + CONTIG_LENS[1])
J_GAP, J_END, J_BEGIN = 0, 0x40, 0x40 | 0x02 | 0x80  # flags of the kswcpp calls: gap fill, end extension / left half of a dual
#                                                      extension, begin extension / right half


@functools.lru_cache(maxsize=None)
def genome():
    return tuple(rand_genome(GENOME_SEED, CONTIG_LENS))


@functools.lru_cache(maxsize=None)
def text():
    """The doubled text: T[p] for p < F is the forward strand, T[p] = 3 - T[N - 1 - p] behind it."""
    fwd = np.concatenate(genome())
    return np.concatenate([fwd, 3 - fwd[::-1]]).astype(np.uint8)


def span_of(contig, reverse):
    """[begin, end) of a contig on the doubled text."""
    b, e = CSTART[contig], CSTART[contig] + CONTIG_LENS[contig]
    return (N - e, N - b) if reverse else (b, e)


# ---- building a read and its seeds from a description of the alignment ---------------------------------------------------
# segments: ("S", n) a seed of n matching bases; ("M", n) n matching bases without a seed; ("X", n) n mismatching bases;
# ("N", n) n N bases of the read opposite n reference bases; ("G", q, r) a gap of q read bases (random) opposite r reference
# bases; ("GN", q, r) the same with every third read base an N; ("Z",) a seed of length 0
def build(r0, segs, salt):
    T = text()
    rng = np.random.default_rng(7000 + salt)
    read, seeds = [], []
    q, r = 0, int(r0)
    for sg in segs:
        k = sg[0]
        if k in ("S", "M"):
            read.append(T[r:r + sg[1]].copy())
            if k == "S":
                seeds.append((q, sg[1], r))
            q, r = q + sg[1], r + sg[1]
        elif k == "X":
            read.append((T[r:r + sg[1]] + 1 + rng.integers(0, 3, sg[1]).astype(np.uint8)) % 4)
            q, r = q + sg[1], r + sg[1]
        elif k == "N":
            read.append(np.full(sg[1], 4, dtype=np.uint8))
            q, r = q + sg[1], r + sg[1]
        elif k in ("G", "GN"):
            g = rng.integers(0, 4, sg[1]).astype(np.uint8)
            if k == "GN":
                g[::3] = 4
            read.append(g)
            q, r = q + sg[1], r + sg[2]
        elif k == "Z":
            seeds.append((q, 0, r))
        else:
            raise ValueError(k)
    assert 0 <= r0 and r <= N, (r0, r)
    return np.concatenate(read).astype(np.uint8) if read else np.zeros(0, dtype=np.uint8), seeds


def seed_array(seeds, qlen):
    s = np.zeros(len(seeds), dtype=OR_SEED_DT)
    for i, (q, ln, r) in enumerate(seeds):
        s[i]["q_start"], s[i]["len"], s[i]["r_start"] = q, ln, r
        s[i]["delta"] = r + (qlen - q)
        s[i]["ambiguity"] = 1
        s[i]["on_forward"] = 1 if r < F else 0
    return s


def case(name, read, sets, **expect):
    """sets: [(soc index, [(q, len, r)])]"""
    read = np.asarray(read, dtype=np.uint8)
    return dict(name=name, read=read, sets=[(int(soc), seed_array(sd, len(read))) for soc, sd in sets], expect=expect)


def one(name, r0, segs, salt, **expect):
    read, seeds = build(r0, segs, salt)
    return case(name, read, [(0, seeds)], **expect)


def force_mismatch(read, q, r, n=8, step=1):
    """read[q], read[q + step], ... (n bases, as far as the read goes) mismatch T[r], T[r + step], ...: an extension that starts
    there ends at once, whatever the bases were (the walk never compares the bases under a seed)."""
    T = text()
    for j in range(n):
        if 0 <= q + step * j < len(read) and 0 <= r + step * j < N:
            read[q + step * j] = (int(T[r + step * j]) + 1) % 4


# ---- short reads -----------------------------------------------------------------------------------------------------
def generic_short(tag, base, salt):
    """The cases that are not tied to a place, at reference position `base` (far from every contig end)."""
    out = []
    s = salt

    def add(name, segs, **expect):
        nonlocal s
        s += 1
        out.append(one("%s_%s" % (name, tag), base, segs, s, **expect))

    add("whole_read_one_seed", [("S", 120)], flags=[[]])
    add("one_seed_middle", [("M", 30), ("S", 40), ("M", 30)], flags=[[J_BEGIN, J_END]])
    add("one_base_seed_last_base", [("M", 50), ("S", 1)], flags=[[J_BEGIN]])
    add("one_base_seed_first_base", [("S", 1), ("M", 50)], flags=[[J_END]])
    add("read_of_one_base", [("S", 1)], flags=[[]])
    add("gap_1x1_mismatch", [("S", 30), ("X", 1), ("S", 30)], flags=[[J_GAP]])
    add("gap_1x1_n", [("S", 30), ("N", 1), ("S", 30)], flags=[[J_GAP]])
    add("gap_2x1", [("S", 30), ("G", 2, 1), ("S", 30)], flags=[[J_GAP]])
    add("gap_1x2", [("S", 30), ("G", 1, 2), ("S", 30)], flags=[[J_GAP]])
    add("gap_pure_ins", [("S", 30), ("G", 5, 0), ("S", 30)], flags=[[]])
    add("gap_pure_del", [("S", 30), ("G", 0, 5), ("S", 30)], flags=[[]])
    add("gap_pure_ins_21", [("S", 30), ("G", 21, 0), ("S", 30)], flags=[[]])
    add("gap_20x20", [("S", 30), ("X", 20), ("S", 30)], flags=[[J_GAP]])
    add("gap_20x5", [("S", 30), ("G", 20, 5), ("S", 30)], flags=[[J_GAP]])
    add("gap_5x20", [("S", 30), ("G", 5, 20), ("S", 30)], flags=[[J_GAP]])
    add("gap_21x5", [("S", 30), ("G", 21, 5), ("S", 30)], flags=[[J_END, J_BEGIN]])
    add("gap_5x21", [("S", 30), ("G", 5, 21), ("S", 30)], flags=[[J_END, J_BEGIN]])
    add("gap_21x21", [("S", 30), ("X", 21), ("S", 30)], flags=[[J_END, J_BEGIN]])
    add("gap_40_mismatches_dual", [("S", 40), ("X", 40), ("S", 40)], flags=[[J_END, J_BEGIN]])
    add("gap_dual_with_indel", [("M", 10), ("S", 40), ("M", 12), ("G", 3, 0), ("M", 15), ("S", 40), ("M", 10)],
        flags=[[J_BEGIN, J_END, J_BEGIN, J_END]])
    add("ns_inside_gap", [("S", 30), ("GN", 7, 6), ("S", 30)], flags=[[J_GAP]])
    add("ns_inside_dual_gap", [("S", 30), ("M", 10), ("N", 3), ("M", 12), ("S", 30)], flags=[[J_END, J_BEGIN]])
    add("ns_in_unseeded_ends", [("M", 8), ("N", 2), ("M", 10), ("S", 40), ("M", 9), ("N", 1), ("M", 10), ("N", 1)],
        flags=[[J_BEGIN, J_END]])
    add("two_hundred_sixty_bases", [("M", 20), ("S", 100), ("X", 1), ("S", 119), ("M", 20)], flags=[[J_BEGIN, J_GAP, J_END]])
    add("zero_length_seed_middle", [("S", 30), ("X", 1), ("Z",), ("M", 2), ("S", 30)], flags=[[J_GAP]])
    add("zero_length_seed_first", [("M", 10), ("Z",), ("S", 30), ("M", 10)], flags=[[J_BEGIN, J_END]])
    add("zero_length_seed_first_then_gap", [("M", 10), ("Z",), ("X", 2), ("S", 30)], flags=[[J_BEGIN, J_GAP]])
    add("zero_length_seed_last", [("S", 30), ("M", 10), ("Z",), ("M", 5)], flags=[[J_END]])

    # the second seed overlaps the first: read = T[base : base + 100], first seed (10, 30, base + 10)
    def overlap(name, second, **expect):
        nonlocal s
        s += 1
        read, _ = build(base, [("M", 100)], s)
        q2, l2, d2 = second
        out.append(case("%s_%s" % (name, tag), read, [(0, [(10, 30, base + 10), (q2, l2, base + d2)])], **expect))

    overlap("overlap_query_only", (35, 30, 40), flags=[[J_BEGIN, J_END]], ops_have=[(4, 5), (0, 25)])  # ovQ 5 > ovR 0: DEL 5
    overlap("overlap_reference_only", (40, 30, 35), flags=[[J_BEGIN, J_END]], ops_have=[(3, 5), (0, 25)])  # ovR 5 > ovQ 0: INS 5
    overlap("overlap_both_query_more", (37, 30, 38), flags=[[J_BEGIN, J_END]], ops_have=[(4, 1), (0, 27)])  # ovQ 3, ovR 2
    overlap("overlap_both_reference_more", (39, 30, 36), flags=[[J_BEGIN, J_END]], ops_have=[(3, 3), (0, 26)])  # ovQ 1, ovR 4
    overlap("overlap_both_equal", (36, 30, 36), flags=[[J_BEGIN, J_END]], ops_have=[(0, 56)])  # ovQ = ovR = 4: the seeds merge
    overlap("overlap_query_with_reference_gap", (35, 30, 50), flags=[[J_BEGIN, J_END]], ops_have=[(4, 15), (0, 25)])
    overlap("overlap_swallowed", (15, 10, 15), flags=[[J_BEGIN, J_END]], ops_have=[(0, 30)])  # overlap 25 >= len 10
    overlap("overlap_swallowed_exactly_len", (30, 10, 30), flags=[[J_BEGIN, J_END]], ops_have=[(0, 30)])  # overlap 10 == len
    overlap("overlap_all_but_one_base", (30, 11, 30), flags=[[J_BEGIN, J_END]], ops_have=[(0, 31)])  # overlap 10 == len - 1
    return out


def placed_short():
    """The cases tied to a place on the reference."""
    out = []
    T = text()
    rng = np.random.default_rng(31)
    c0, c1, c2 = span_of(0, False), span_of(1, False), span_of(2, False)
    r2, r1, r0 = span_of(2, True), span_of(1, True), span_of(0, True)
    assert r2[0] == F and r0[1] == N and c2[1] == F

    # unseeded query bases in front of a set at the very first base of the text / a contig / the reverse strand: the begin
    # extension has an empty reference
    for nm, p in (("text_position_0", 0), ("first_base_of_contig_1", c1[0]), ("first_base_of_reverse_strand", F)):
        read = np.concatenate([rng.integers(0, 4, 5).astype(np.uint8), T[p:p + 60]])
        out.append(case("front_bases_at_%s" % nm, read, [(0, [(5, 60, p)])], flags=[[]], begin_ref=p, begin_q=5))
    # the padded window is clamped at a contig's start / end, at n - 1, at both ends of the contig shorter than the padding
    out.append(one("window_clamped_at_contig_start", c2[0] + 100, [("M", 20), ("S", 50), ("M", 20)], 41, flags=[[J_BEGIN, J_END]],
                   window=(c2[0], c2[0] + 120 + 50 + 1000)))
    out.append(one("window_clamped_at_text_start", 300, [("M", 20), ("S", 50), ("M", 20)], 42, flags=[[J_BEGIN, J_END]],
                   window=(0, 320 + 50 + 1000)))
    out.append(one("window_clamped_at_contig_end", c0[1] - 200, [("M", 20), ("S", 50), ("M", 20)], 43, flags=[[J_BEGIN, J_END]],
                   window=(c0[1] - 180 - 1000, c0[1] - 1)))
    # (on the reverse strand the reference's uiEndOfSequenceWithIdOrReverse is the contig's last base but one, pack.h:1040-1045,
    # and the clamp takes one more off: the window ends three bases before the contig's end)
    out.append(one("window_clamped_at_reverse_contig_start", r1[0] + 50, [("M", 20), ("S", 50), ("M", 20)], 44,
                   flags=[[J_BEGIN, J_END]], window=(r1[0], r1[1] - 3)))
    out.append(one("window_clamped_at_n_minus_1", N - 300, [("M", 20), ("S", 50), ("M", 20)], 45, flags=[[J_BEGIN, J_END]],
                   window=(N - 280 - 1000, N - 1)))
    out.append(one("window_clamped_at_both_ends_of_short_contig", c1[0] + 300, [("M", 20), ("S", 50), ("M", 20)], 46,
                   flags=[[J_BEGIN, J_END]], window=(c1[0], c1[1] - 1)))
    # a set that ends exactly on the last base of a contig is bridging (the test takes endRef - beginRef + 1 bases); one that
    # ends a base earlier is not, and its window ends at the clamp
    for nm, e in (("contig_0", c0[1]), ("last_forward_contig", F), ("doubled_text", N), ("reverse_contig_2", r2[1])):
        out.append(one("ends_on_last_base_of_%s" % nm, e - 80, [("M", 10), ("S", 30), ("X", 1), ("S", 39)], 50, empty=True, flags=[[]]))
        out.append(one("ends_a_base_before_last_of_%s" % nm, e - 81, [("M", 10), ("S", 30), ("X", 1), ("S", 39), ("M", 1)], 51,
                       flags=[[J_BEGIN, J_GAP]], end_ref=e - 1))
    # bridging sets: two contigs, the strand border
    for nm, e in (("two_contigs", c0[1]), ("strand_border", F), ("two_reverse_contigs", r2[1])):
        read = np.concatenate([T[e - 40:e], T[e:e + 40]])
        out.append(case("bridging_%s" % nm, read, [(0, [(0, 40, e - 40), (40, 40, e)])], empty=True, flags=[[]]))
        out.append(case("bridging_%s_one_seed" % nm, read, [(0, [(0, 80, e - 40)])], empty=True, flags=[[]]))
    return out


# ---- several sets per read: finish_read ----------------------------------------------------------------------------
def list_cases():
    out = []
    T = text()
    A, B, Cc, D = 1200, 2600, 3900, CSTART[2] + 1200  # four places far from each other and from every contig end
    rng = np.random.default_rng(57)

    def isolated(read, seeds):
        """forced mismatches at both sides of every seed: no extension moves an end"""
        for q, ln, r in seeds:
            force_mismatch(read, q - 1, r - 1, step=-1)
            force_mismatch(read, q + ln, r + ln)

    real = [(10, 60, A + 10)]
    rd = T[A:A + 80].copy()
    out.append(case("empty_set_alone", rd, [(0, [])], empty=True, flags=[[]], mq_len=0))
    out.append(case("empty_set_then_real", rd, [(0, []), (1, real)], mq_flags=[(0, 0)]))
    out.append(case("real_then_empty_set", rd, [(0, real), (1, [])], mq_flags=[(0, 0)]))
    out.append(case("two_identical_sets_soc_0_1", rd, [(0, real), (1, real)], tie=True, mq_socs=[0, 1]))
    out.append(case("two_identical_sets_soc_1_0", rd, [(1, real), (0, real)], tie=True, mq_socs=[0, 1]))
    out.append(case("two_identical_sets_soc_7_3", rd, [(7, real), (3, real)], tie=True, mq_socs=[3, 7]))
    for perm in ((0, 1, 2), (2, 0, 1), (1, 2, 0), (2, 1, 0)):
        out.append(case("three_equal_scores_%d%d%d" % perm, rd, [(k, real) for k in perm], tie=True))
    out.append(case("five_equal_scores", rd, [(k, real) for k in (4, 2, 0, 3, 1)], tie=True))
    # three different places, equal scores
    rd3 = np.concatenate([T[A:A + 50], T[B:B + 50], T[Cc:Cc + 50]])
    s3 = [[(0, 50, A)], [(50, 50, B)], [(100, 50, Cc)]]
    for sd in s3:
        isolated(rd3, sd)
    for perm in ((0, 1, 2), (2, 1, 0), (1, 0, 2)):
        out.append(case("three_places_equal_scores_%d%d%d" % perm, rd3, [(k, s3[k]) for k in perm], tie=True))
    out.append(case("more_candidates_than_max_supplementary", rd3, [(0, s3[0]), (1, s3[1]), (2, s3[2])], tie=True,
                    mq_kinds={"supplementary": MAX_SUPPLEMENTARY, "secondary": 1}))
    # the second set's query overlap with the first: sz = 100 bases, overlap k / 100 against 0.1
    for k, side in ((9, "under"), (10, "at"), (11, "over")):
        rdo = rng.integers(0, 4, 215).astype(np.uint8)
        rdo[0:110] = T[A:A + 110]
        rdo[110:210 - k] = T[B + k:B + 100]
        first, second = [(0, 110, A)], [(110 - k, 100, B)]
        isolated(rdo, first)
        isolated(rdo, second)
        out.append(case("second_overlaps_first_just_%s_threshold" % side, rdo, [(0, first), (1, second)], overlap=(k, 100),
                        mq_flags=[(0, 0), (0, 1)] if k < 10 else [(0, 0), (1, 0)]))
    # below min_alignment_score; one seed only; one seed only with n >= 3 and a score of >= 0.8 of the maximum
    rdl = T[D:D + 50].copy()
    low = [(10, 30, D + 10)]
    isolated(rdl, low)
    out.append(case("best_score_below_min_alignment_score", rdl, [(0, low)], mq_len=0, best_score=60))
    out.append(case("two_sets_below_min_alignment_score", rdl, [(0, low), (1, low)], mq_len=0, best_score=60, tie=True))
    out.append(one("first_alignment_one_seed_only", D, [("S", 100)], 61, mq_len=1, one_seed=True))
    rdw = T[D:D + 100].copy()
    whole, part1, part2 = [(0, 100, D)], [(0, 40, B)], [(60, 40, Cc)]
    out.append(case("one_seed_only_three_sets_high_score", rdw, [(0, whole), (1, part1), (2, part2)], one_seed=True, high=True))
    out.append(case("one_seed_only_three_sets_high_score_other_order", rdw, [(2, part2), (1, part1), (0, whole)], one_seed=True,
                    high=True))
    two_seeds = [(0, 45, D), (55, 45, D + 55)]
    out.append(case("two_seeds_three_sets_high_score", rdw, [(0, two_seeds), (1, part1), (2, part2)], high=True))
    # all alignments empty
    e = CSTART[1]
    rdb = np.concatenate([T[e - 40:e], T[e:e + 40]])
    out.append(case("all_alignments_empty", rdb, [(0, [(0, 40, e - 40), (40, 40, e)]), (1, [(0, 80, e - 40)]), (2, [])], empty=True,
                    mq_len=0))
    out.append(case("empty_alignments_and_a_real_one", rdb, [(0, [(0, 40, e - 40), (40, 40, e)]), (1, [(0, 39, e - 40)]), (2, [])], mq_len=1,
                    mq_flags=[(0, 0)]))
    # a read without sets between reads with sets
    out.append(case("read_with_sets_before", rd, [(0, real)]))
    out.append(case("read_without_sets", rd, []))
    out.append(case("read_with_sets_after", rd, [(0, real)]))
    return out


# ---- long reads: k_stitch_wave ---------------------------------------------------------------------------------------
WAVE_SPAN = 1024  # stitch_is_big: the set's last seed ends >= 1024 query bases behind the first seed's start
LONG_SEED_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 200)
STRADDLES = ((62, 63), (63, 64), (64, 65), (127, 128))
END_LENGTHS = ((63, 63), (64, 64), (65, 65), (128, 128), (200, 64), (64, 200))  # (front, back)
DUAL = ("X", 24)


def gap_of_kind(i, dual_every):
    if i % dual_every == dual_every - 1:
        return [DUAL]
    return ([], [("X", 1)], [("G", 2, 3)])[i % 3]  # touching seeds (no job), a 1 x 1 gap, a small gap


def long_segments(n_seeds, span, front=40, back=40, shorten=0):
    """front unseeded bases, n_seeds seeds with the gap kinds cycling between them over exactly `span` query bases, back unseeded
    bases; shorten: bases taken off the last seed (and off the span)."""
    dual_every = 4 if n_seeds <= 65 else 16
    gaps = [gap_of_kind(i, dual_every) for i in range(n_seeds - 1)]
    gq = sum(sg[1] for g in gaps for sg in g)
    room = span - gq
    assert room >= n_seeds, (n_seeds, span, gq)
    ln = [room // n_seeds] * n_seeds
    ln[-1] += room - sum(ln) - shorten
    segs = [("M", front)] if front else []
    for i in range(n_seeds):
        segs.append(("S", ln[i]))
        if i < n_seeds - 1:
            segs += gaps[i]
    if back:
        segs.append(("M", back))
    return segs


def set_span(seeds):
    return int(seeds[-1]["q_start"] + seeds[-1]["len"] - seeds[0]["q_start"]) if len(seeds) else 0


def long_cases():
    out = []
    fwd, rev = 1100, span_of(0, True)[0] + 1700  # inside contig 0 / its reverse complement, > padding from both ends
    for i, n in enumerate(LONG_SEED_COUNTS):
        span = 1100 + 20 * i
        out.append(one("long_%d_seeds" % n, rev if i % 2 else fwd, long_segments(n, span), 100 + i, wave=True, n_seeds=n))
    # the same set spanning 1024 and 1023 query bases: the last size k_stitch_wave takes and the first k_stitch keeps
    out.append(one("long_64_seeds_span_1024", fwd + 50, long_segments(64, WAVE_SPAN), 120, wave=True, n_seeds=64))
    out.append(one("long_64_seeds_span_1023", fwd + 50, long_segments(64, WAVE_SPAN, shorten=1), 120, wave=False, n_seeds=64))
    # a dual extension's two jobs on both sides of a reload of the 64-entry job window: job 0 is the begin extension, then
    # 1 x 1 gaps (one job slot each) up to the dual gap
    for a, b in STRADDLES:
        segs = [("M", 30), ("S", 6)]
        for _ in range(a - 1):
            segs += [("X", 1), ("S", 6)]
        segs += [DUAL, ("S", 6)]
        q = 30 + 6 + 7 * (a - 1) + DUAL[1] + 6
        k = 0
        while q - 30 < WAVE_SPAN + 40:
            segs += gap_of_kind(k, 4) + [("S", 9)]
            q += sum(sg[1] for sg in gap_of_kind(k, 4)) + 9
            k += 1
        segs.append(("M", 30))
        out.append(one("long_dual_jobs_%d_%d" % (a, b), rev + 100 if a % 2 else fwd + 100, segs, 130 + a, wave=True, dual_at=(a, b)))
    # unseeded ends with mismatches where the 64-base trips of match_run begin and end
    def end_run(e):
        marks = sorted(set(m for m in (0, 63, 64, 127, e - 1) if m < e))
        segs, at = [], 0
        for m in marks:
            if m > at:
                segs.append(("M", m - at))
            segs.append(("X", 1))
            at = m + 1
        if e > at:
            segs.append(("M", e - at))
        return segs

    for i, (ef, eb) in enumerate(END_LENGTHS):
        segs = end_run(ef) + long_segments(8 + i, 1060, front=0, back=0) + end_run(eb)
        out.append(one("long_unseeded_ends_%d_%d" % (ef, eb), fwd + 200 if i % 2 else rev + 200, segs, 150 + i, wave=True, ends=(ef, eb)))
    return out


# ---- the whole list -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_cases():
    fwd_base = 2000  # contig 0, > padding from both ends
    rev_base = span_of(0, True)[0] + 1500
    cases = generic_short("fwd", fwd_base, 0) + generic_short("rev", rev_base, 500) + placed_short() + list_cases() + long_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    assert len(cases) <= 400 and sum(len(c["sets"]) for c in cases) <= 2000
    return tuple(cases)


def case_batch(cases=None):
    """(names, reads, hset_off, hseed_off, hset_soc, seeds) of the cases as one batch, in the hsets() layout."""
    cases = all_cases() if cases is None else cases
    hset_off, hseed_off, soc, seeds = [0], [0], [], [np.zeros(0, dtype=OR_SEED_DT)]
    for c in cases:
        for k, sd in c["sets"]:
            soc.append(k)
            seeds.append(sd)
            hseed_off.append(hseed_off[-1] + len(sd))
        hset_off.append(len(soc))
    return ([c["name"] for c in cases], [c["read"] for c in cases], np.array(hset_off, dtype=np.uint64),
            np.array(hseed_off, dtype=np.uint64), np.array(soc, dtype=np.uint32), np.concatenate(seeds))


def check(cases=None):
    """The contract the product may rely on, for every set of every case."""
    cases = all_cases() if cases is None else cases
    names, reads, hset_off, hseed_off, soc, seeds = case_batch(cases)
    assert np.all(np.diff(hset_off.astype(np.int64)) >= 0) and hset_off[0] == 0, "hset_off is not monotone"
    assert np.all(np.diff(hseed_off.astype(np.int64)) >= 0) and hseed_off[0] == 0, "hseed_off is not monotone"
    assert int(hset_off[-1]) == len(soc) == len(hseed_off) - 1 and int(hseed_off[-1]) == len(seeds)
    for r, c in enumerate(cases):
        nm, qlen = c["name"], len(c["read"])
        assert 1 <= qlen and c["read"].max() <= 4, nm
        for s in range(int(hset_off[r]), int(hset_off[r + 1])):
            sd = seeds[int(hseed_off[s]):int(hseed_off[s + 1])]
            for f in ("q_start", "len", "r_start", "delta"):
                assert np.all(sd[f] >= 0), (nm, s, f, "negative field")
            assert np.all(np.diff(sd["q_start"]) >= 0), (nm, s, "seeds not ordered by q_start")
            assert np.all(sd["q_start"] + sd["len"] <= qlen), (nm, s, "seed beyond its read")
            assert np.all(sd["r_start"] + sd["len"] <= N), (nm, s, "seed beyond the doubled text")
            assert np.all((sd["r_start"] < F) == (sd["on_forward"] == 1)), (nm, s, "on_forward")


def write_sets_file(path, reads, hset_off, hseed_off, hset_soc, seeds):
    """The sets file of ref_dump nwsets and host_emul's MA_EMUL_HSETS (oracle/dump_format.h, NWSETS01)."""
    with open(path, "wb") as f:
        f.write(b"NWSETS01")
        f.write(np.array([len(reads), len(hset_soc), len(seeds)], dtype="<u8").tobytes())
        f.write(np.asarray(hset_off, dtype="<u8").tobytes())
        f.write(np.asarray(hseed_off, dtype="<u8").tobytes())
        f.write(np.asarray(hset_soc, dtype="<u4").tobytes())
        f.write(np.asarray(seeds, dtype=OR_SEED_DT).tobytes())


def result_text(reads, res):
    """An OrIndex.nw_sets result as the ALN / MQ lines of the pipe dump (ref_dump's cmdPipe, %.17g for mapq)."""
    lines = []
    for r in range(len(reads)):
        lines.append("R %d %d" % (r, len(reads[r])))
        a, e = int(res["aln_off"][r]), int(res["aln_off"][r + 1])
        lines.append("ALN %d" % (e - a))
        for x in res["alns"][a:e]:
            o = res["ops"][2 * int(x["ops_off"]):2 * (int(x["ops_off"]) + int(x["n_ops"]))]
            lines.append("a %d %d %d %d %d %d %d" % (x["begin_ref"], x["end_ref"], x["begin_q"], x["end_q"], x["score"], x["soc_index"],
                                                     x["n_ops"]) + "".join(" %d:%d" % (o[2 * i], o[2 * i + 1]) for i in range(int(x["n_ops"]))))
        a, e = int(res["mq_off"][r]), int(res["mq_off"][r + 1])
        lines.append("MQ %d" % (e - a))
        for x in res["mq"][a:e]:
            lines.append("m %d %d %d %d %d %d %d %s" % (x["begin_ref"], x["end_ref"], x["begin_q"], x["end_q"], x["score"], x["secondary"],
                                                        x["supplementary"], "%.17g" % float(x["mapq"])))
    return "\n".join(lines) + "\n"
