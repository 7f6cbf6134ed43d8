"""Hand-made segment lists that put seed extraction (ma_batch_set_segments -> ma_extract_seeds_batch: k_seg_seed_counts,
k_read_seed_ranges, k_seed_rows, k_lf_walk, k_seed_final) where segments made by seeding sampled reads rarely or never put it,
and a PLAIN reference of the stage; shared by the golden maker (tests/golden/make_extract_golden.py),
test_extract_lists_host.py and test_gpu_extract_lists.py.

The reference is a brute-force suffix array: the suffixes of the doubled text T = forward . reverse complement (n = 2 F) sorted
as byte strings (a shorter prefix sorts first).  Row 0 is the sentinel's (SA = -1), row k >= 1 the k-th suffix.  It touches
neither the FM index nor the oracle nor a device; expected_seeds() restates Segment::forEachSeed (segment.h:89-113),
SegmentVector::forEachSeed with bSkip (segment.h:316-369) and setDeltaOfSeed in rectangular mode (stripOfConsideration.h:97-112)
on it in numpy, expected_lf_steps() the number of LF steps bwt_sa (fMIndex.h:788-814) takes: the LF map sends the row of
position p to the row of position p - 1 and the row of position 0 to row 0; a walk ends on the first row that is a multiple
of the sampling interval.

A case is one read (only its length matters to the stage) with a list of segments (q_start, q_size, sa_start, sa_size); q_size
is the seed's length minus 1.  All cases together are one batch (case_batch()); every case has a name, and check() -- the
contract ma_batch_set_segments enforces -- names it in every assertion.  `expect` says what the case is for;
test_extract_lists_host.py certifies it from the plain reference's own output before a device sees the case.

The genome: three contigs whose lengths are no multiples of 4, the second shorter than 32 bases, and in the first a tandem
repeat of 102 copies of a 7-mer: a prefix of the repeat occurs once per copy it still fits into, which gives REAL intervals of
2, 3, 100 and 101 rows (real_interval()).  Any row range inside 1 .. n is legal input, so the other
intervals are made up.

Cases dropped from the golden because the compiled reference died on them: none."""
import functools
import os

import numpy as np

from ma_testlib import OR_SEED_DT, OR_SEGMENT_DT, ROOT, rand_genome

GENOME_SEED, CONTIG_LENS = 211, (1801, 23, 1201)
REPEAT_UNIT, REPEAT_COPIES, REPEAT_AT = 7, 102, 500  # in contig 0
F = sum(CONTIG_LENS)
N = 2 * F
CSTART = (0, CONTIG_LENS[0], CONTIG_LENS[0] + CONTIG_LENS[1])
MIN_SEED_LEN = 16  # of every preset
# (min_seed_len, max_ambiguity) of the runs: the preset's length filter with the ambiguity filter off, at 1 and at the default's 100;
# and no length filter at all (the read of one base yields its seed)
PARAMS = ((16, 0), (16, 1), (16, 100), (0, 0))
SHIFTS = {"dense": 3, "sparse": 5}  # log2 of the SA sampling interval: the default dense sample, MA_SA_DENSE=0
TOTALS = (1, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)  # where the refill protocol of k_lf_walk changes its path
LANE_CAP = 256 * 2048  # lanes of the k_lf_walk launch
QLEN = 40


def golden_path():
    return os.path.join(ROOT, "tests", "golden", "extract_lists.seeds.gz")


@functools.lru_cache(maxsize=None)
def genome():
    g = rand_genome(GENOME_SEED, CONTIG_LENS)
    unit = np.random.default_rng(GENOME_SEED + 1).integers(0, 4, REPEAT_UNIT).astype(np.uint8)
    g[0][REPEAT_AT:REPEAT_AT + REPEAT_UNIT * REPEAT_COPIES] = np.tile(unit, REPEAT_COPIES)
    return tuple(g)


@functools.lru_cache(maxsize=None)
def text():
    """The doubled text: T[p] for p < F is the forward strand, T[p] = 3 - T[N - 1 - p] behind it."""
    fwd = np.concatenate(genome())
    return np.concatenate([fwd, 3 - fwd[::-1]]).astype(np.uint8)


# ---- the plain reference ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def suffix_array():
    """(SA, ROW, LF): SA[k] = text position of row k (SA[0] = -1), ROW[p] = row of position p, LF[k] = ROW[SA[k] - 1], 0 for the
    row of position 0 (and for row 0, which no walk leaves)."""
    tb = text().tobytes()
    sa = np.array([-1] + sorted(range(N), key=lambda i: tb[i:]), dtype=np.int64)
    row = np.zeros(N, dtype=np.int64)
    row[sa[1:]] = np.arange(1, N + 1)
    lf = np.zeros(N + 1, dtype=np.int64)
    inner = sa > 0
    lf[inner] = row[sa[inner] - 1]
    return sa, row, lf


def primary():
    return int(suffix_array()[1][0])


@functools.lru_cache(maxsize=None)
def walk_steps(shift):
    """LF steps from every row to the first row that is a multiple of 1 << shift."""
    sa, _, lf = suffix_array()
    mask = (1 << shift) - 1
    k = np.arange(N + 1, dtype=np.int64)
    steps = np.zeros(N + 1, dtype=np.int64)
    live = (k & mask) != 0
    while live.any():
        k[live] = lf[k[live]]
        steps[live] += 1
        live = (k & mask) != 0
    assert np.array_equal(sa[k] + steps, sa)  # the walk is bwt_sa: sample + steps is the position (row 0: -1 + steps)
    return steps


def interval_of(pattern):
    """(first row, rows) of the suffixes that begin with `pattern` (codes): a real SA interval."""
    sa = suffix_array()[0]
    tb, pb = text().tobytes(), np.asarray(pattern, dtype=np.uint8).tobytes()
    hit = np.array([tb.startswith(pb, int(p)) for p in sa[1:]])
    rows = np.nonzero(hit)[0] + 1
    assert len(rows) and rows[-1] - rows[0] + 1 == len(rows), "occurrences of a pattern are one row range"
    return int(rows[0]), len(rows)


def repeat_prefix(n_bases):
    return text()[REPEAT_AT:REPEAT_AT + n_bases]


def real_interval(size):
    """The interval of the shortest prefix of the tandem repeat that occurs exactly `size` times (the count falls with the
    prefix's length: bisection)."""
    lo, hi = 1, REPEAT_UNIT * REPEAT_COPIES  # count(lo - 1) > size >= count(hi)
    while lo < hi:
        mid = (lo + hi) // 2
        if interval_of(repeat_prefix(mid))[1] > size:
            lo = mid + 1
        else:
            hi = mid
    got = interval_of(repeat_prefix(lo))
    assert got[1] == size, (size, lo, got)
    return got


def contig_of(r):
    """contig of a forward position, by scanning"""
    for c in range(len(CONTIG_LENS)):
        if CSTART[c] <= r < CSTART[c] + CONTIG_LENS[c]:
            return c
    raise ValueError(r)


def seed_of_position(p, q_start, q_size, qlen, ambiguity):
    """The seed record of text position p, from the geometry alone (no suffix array): what certifies the placed cases."""
    fwd = p < F
    r = p if fwd else N - 1 - p
    return dict(q_start=q_start, len=q_size + 1, r_start=r, delta=r + (qlen - q_start) + (qlen + 1) * contig_of(r),
                ambiguity=ambiguity, on_forward=1 if fwd else 0)


def kept(segs, min_seed_len, max_ambiguity):
    """The two filters of SegmentVector::forEachSeed with bSkip."""
    k = segs["q_size"] >= min_seed_len
    if max_ambiguity != 0:
        k &= segs["sa_size"] <= max_ambiguity
    return k


def seed_rows(batch, min_seed_len, max_ambiguity):
    """(index of the segment, SA row) of every seed the batch yields, in order."""
    segs = batch[3]
    cnt = np.where(kept(segs, min_seed_len, max_ambiguity), segs["sa_size"], 0).astype(np.int64)
    seg = np.repeat(np.arange(len(segs)), cnt)
    first = np.cumsum(cnt) - cnt
    return seg, segs["sa_start"][seg] + (np.arange(int(cnt.sum())) - first[seg]), cnt


def expected_seeds(batch, min_seed_len, max_ambiguity):
    """(seed_off, seeds) of the batch in the layout of Batch.seeds(), from the brute-force suffix array."""
    names, reads, seg_off, segs = batch
    sa = suffix_array()[0]
    seg, rows, cnt = seed_rows(batch, min_seed_len, max_ambiguity)
    read_of_seg = np.repeat(np.arange(len(reads)), np.diff(seg_off.astype(np.int64)))
    qlen = np.array([len(r) for r in reads], dtype=np.int64)[read_of_seg[seg]] if len(seg) else np.zeros(0, dtype=np.int64)
    pos = sa[rows]
    fwd = pos < N // 2
    r = np.where(fwd, pos, N - pos - 1)  # the mirror (segment.h:100-105)
    contig = np.searchsorted(np.array(CSTART), r, side="right") - 1
    out = np.zeros(len(seg), dtype=OR_SEED_DT)
    out["q_start"] = segs["q_start"][seg]
    out["len"] = segs["q_size"][seg] + 1
    out["r_start"] = r
    out["delta"] = r + (qlen - segs["q_start"][seg]) + (qlen + 1) * contig
    out["ambiguity"] = segs["sa_size"][seg]
    out["on_forward"] = fwd
    per_read = np.zeros(len(reads), dtype=np.int64)
    np.add.at(per_read, read_of_seg, cnt)
    seed_off = np.zeros(len(reads) + 1, dtype=np.uint64)
    seed_off[1:] = np.cumsum(per_read)
    return seed_off, out


def expected_lf_steps(batch, min_seed_len, max_ambiguity, shift):
    """The exact number of LF steps of all kept seeds under the sampling interval 1 << shift."""
    return int(walk_steps(shift)[seed_rows(batch, min_seed_len, max_ambiguity)[1]].sum())


# ---- the cases ---------------------------------------------------------------------------------------------------------
def case(name, qlen, segments, **expect):
    """segments: [(q_start, q_size, sa_start, sa_size)]"""
    s = np.zeros(len(segments), dtype=OR_SEGMENT_DT)
    for i, (q, z, a, c) in enumerate(segments):
        s[i]["q_start"], s[i]["q_size"], s[i]["sa_start"], s[i]["sa_size"] = q, z, a, c
    read = np.random.default_rng(9000 + len(name) * 131 + qlen).integers(0, 4, qlen).astype(np.uint8)
    return dict(name=name, read=read, segs=s, expect=expect)


def counts(*per_params):
    """the seeds a case is to yield under each of PARAMS, stated by hand"""
    assert len(per_params) == len(PARAMS)
    return dict(zip(PARAMS, per_params))


def amb_counts(size):
    """... for ONE segment of `size` rows with a seed of more than 16 bases"""
    return counts(size, size if size <= 1 else 0, size if size <= 100 else 0, size)


PLACES = (("text_position_0", 0), ("last_forward_base", F - 1), ("first_reverse_base", F), ("text_position_n_minus_1", N - 1)) + tuple(
    ("%s_base_of_contig_%d_%s" % (end, c, strand), p if strand == "forward" else N - 1 - p)
    for c in range(len(CONTIG_LENS)) for end, p in (("first", CSTART[c]), ("last", CSTART[c] + CONTIG_LENS[c] - 1))
    for strand in ("forward", "reverse"))
ROW_MODS = (0, 1, 7, 8, 9, 15, 31, 32, 33, 39, 63)  # offsets from a multiple of 64: k mod 8 and k mod 32 in {0, 1, 7, 31}
ROW_BASES = (64, 2048, 5952)


@functools.lru_cache(maxsize=None)
def all_cases():
    sa, row, lf = suffix_array()
    M, Q = MIN_SEED_LEN, QLEN
    out = [case("no_segments_first", Q, [], count=amb_counts(0))]
    # the length filter: q_size < min_seed_len drops the segment, so a seed of exactly min_seed_len bases is absent
    for q_size, nm in ((M - 2, "seed_of_min_seed_len_minus_1_bases"), (M - 1, "seed_of_exactly_min_seed_len_bases"),
                       (M, "seed_of_min_seed_len_plus_1_bases"), (M + 1, "seed_of_min_seed_len_plus_2_bases")):
        out.append(case(nm, Q, [(3, q_size, 777, 1)], count={p: 1 if q_size >= p[0] else 0 for p in PARAMS}))
    # the ambiguity filter at 1 and at 100, each at -1, 0, +1; the sizes 2, 3, 100 and 101 are real intervals of the tandem repeat
    real = {size: real_interval(size) for size in (2, 3, 100, 101)}
    for size in (1, 2, 3, 99, 100, 101):
        a = real[size][0] if size in real else 1500
        assert size not in real or real[size][1] == size, (size, real[size])
        out.append(case("interval_of_%d_rows" % size, Q, [(0, 20, a, size)], count=amb_counts(size), real=size in real))
    out.append(case("made_up_interval", Q, [(5, 25, 1234, 37)], count=amb_counts(37)))
    # rows of chosen text positions: the record follows from the geometry alone
    out.append(case("row_primary", Q, [(2, 30, primary(), 1)], count=amb_counts(1), seed=seed_of_position(0, 2, 30, Q, 1)))
    for nm, p in PLACES:
        out.append(case("row_of_" + nm, Q + 1, [(1, 17, int(row[p]), 1)], count=amb_counts(1), seed=seed_of_position(p, 1, 17, Q + 1, 1)))
    # rows one before, on and one after the multiples of both sampling intervals; row 1 and row n
    for base in ROW_BASES:
        out.append(case("rows_around_samples_%d" % base, Q, [(0, 16 + i, base + m, 1) for i, m in enumerate(ROW_MODS)],
                        count=counts(*[len(ROW_MODS)] * 4), rows=[base + m for m in ROW_MODS]))
    out.append(case("first_and_last_row", Q, [(0, 20, 1, 1), (0, 20, N, 1), (0, 20, N - 4, 5), (0, 20, 1, 5)], count=counts(12, 2, 12, 12)))
    # intervals that straddle a multiple of 8, of 32, of both
    out.append(case("intervals_straddle_samples", Q, [(0, 20, 8 * 101 + 5, 6), (4, 20, 32 * 40 - 3, 7), (8, 20, 32 * 41 - 1, 2), (9, 20, 32 * 50 + 31, 34)],
                    count=counts(49, 0, 49, 49), straddles=[(8 * 101 + 5, 6, 8), (32 * 40 - 3, 7, 32), (32 * 41 - 1, 2, 32), (32 * 50 + 31, 34, 32)]))
    # the read's ends
    out.append(case("q_start_0", Q, [(0, 18, 901, 2)], count=amb_counts(2)))
    out.append(case("seed_ends_at_read_end", Q, [(Q - 20, 19, 902, 2)], count=amb_counts(2)))
    out.append(case("seed_covers_whole_read", Q, [(0, Q - 1, 903, 1)], count=amb_counts(1)))
    out.append(case("read_of_one_base", 1, [(0, 0, 904, 3)], count=counts(0, 0, 0, 3)))
    out.append(case("long_read", 3001, [(2950, 50, 905, 1), (0, 3000, 906, 1), (1500, 16, 907, 2)], count=counts(4, 2, 4, 4)))
    # a read with the longest walks of the index next to reads without any
    far = np.argsort(-walk_steps(5)[1:], kind="stable")[:64] + 1
    out.append(case("no_segments_before_long_walks", Q, [], count=amb_counts(0)))
    out.append(case("longest_walks", Q, [(0, 20, int(k), 1) for k in far], count=counts(64, 64, 64, 64), longest=True))
    out.append(case("no_segments_middle", Q, [], count=amb_counts(0)))
    out.append(case("only_sampled_rows", Q, [(0, 20, 32 * k, 1) for k in range(1, 65)], count=counts(64, 64, 64, 64), no_walk=True))
    # segments that are all filtered out (by the length filter, whatever max_ambiguity is)
    out.append(case("all_segments_filtered", Q, [(0, M - 1, 300, 2), (5, 3, 400, 101), (7, 0, 500, 1)],
                    count=counts(0, 0, 0, 2 + 101 + 1)))
    out.append(case("filtered_between_kept", Q, [(0, 20, 310, 2), (0, M - 1, 320, 2), (0, 20, 330, 101), (0, 20, 340, 1)],
                    count=counts(2 + 101 + 1, 1, 2 + 1, 2 + 2 + 101 + 1)))
    # overlapping and identical segments
    out.append(case("identical_segments", Q, [(3, 20, 2000, 4)] * 3, count=counts(12, 0, 12, 12)))
    out.append(case("overlapping_segments", Q, [(0, 20, 2100, 10), (1, 20, 2105, 10), (2, 19, 2100, 10), (0, 30, 2109, 1)], count=counts(31, 1, 31, 31)))
    out.append(case("no_segments_last", Q, [], count=amb_counts(0)))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return tuple(out)


def make_batch(cases):
    seg_off = np.zeros(len(cases) + 1, dtype=np.uint64)
    seg_off[1:] = np.cumsum([len(c["segs"]) for c in cases])
    segs = np.concatenate([np.zeros(0, dtype=OR_SEGMENT_DT)] + [c["segs"] for c in cases])
    return [c["name"] for c in cases], [c["read"] for c in cases], seg_off, segs


def case_batch(cases=None):
    """(names, reads, seg_off, segs) of the cases as one batch, in the layout of Batch.segments()."""
    return make_batch(all_cases() if cases is None else cases)


def n_seeds(batch, min_seed_len=MIN_SEED_LEN, max_ambiguity=0):
    return int(seed_rows(batch, min_seed_len, max_ambiguity)[2].sum())


def pad_case(name, count, salt):
    """`count` seeds (under min_seed_len 16, any max_ambiguity >= 64 or 0) from made-up intervals of at most 64 rows"""
    rng = np.random.default_rng(4000 + salt)
    segments = []
    while count:
        c = min(count, int(rng.integers(1, 65)))
        segments.append((int(rng.integers(0, 10)), int(rng.integers(16, 30)), int(rng.integers(1, N + 2 - c)), c))
        count -= c
    return case(name, QLEN, segments)


def total_batch(total):
    """The list cut after the last case that fits and padded to exactly `total` seeds under (16, 0)."""
    cases, have = [], 0
    for c in all_cases():
        k = n_seeds(make_batch([c]))
        if have + k > total:
            break
        cases.append(c)
        have += k
    if have < total:
        cases.append(pad_case("pad_to_%d" % total, total - have, total))
    b = make_batch(cases)
    assert n_seeds(b) == total
    return b


def no_seed_batch():
    """Reads with segments, none of which yields a seed under (16, 0)."""
    b = make_batch([c for c in all_cases() if len(c["segs"]) and c["expect"]["count"][(16, 0)] == 0] * 3)
    assert len(b[3]) >= 9 and n_seeds(b) == 0
    return b


def no_segment_batch():
    return make_batch([c for c in all_cases() if len(c["segs"]) == 0])


CAP_READS, CAP_WIDTH, CAP_WINDOWS = 64, 100, 32


@functools.lru_cache(maxsize=None)
def cap_batch():
    """Generated, not stored: LANE_CAP + 1 seeds under (16, 100) from a few thousand segments of at most 100 rows.  The even reads
    have sampled rows only (multiples of 32: no walk under either interval), the odd reads the 32 windows of 100 rows with the most LF
    steps under the sparse sample, so that lanes which finish at once share their wave's refills with lanes that walk longest."""
    total = LANE_CAP + 1
    half = CAP_READS // 2
    sampled = [[(0, 20, 32 * (1 + (r * 20 + i) % (N // 32 - 1)), 1) for i in range(20)] for r in range(half)]
    rest = total - half * 20
    win = np.convolve(walk_steps(5)[1:], np.ones(CAP_WIDTH, dtype=np.int64), mode="valid")  # win[i]: rows 1 + i .. 100 + i
    best = np.argsort(-win, kind="stable")[:CAP_WINDOWS] + 1
    n_full, tail = divmod(rest, CAP_WIDTH)
    walkers = [(i % 7, 16 + i % 17, int(best[i % len(best)]), CAP_WIDTH) for i in range(n_full)] + ([(0, 20, int(best[0]), tail)] if tail else [])
    per = -(-len(walkers) // half)
    cases = []
    for r in range(half):
        cases.append(case("cap_sampled_%d" % r, QLEN, sampled[r]))
        cases.append(case("cap_walkers_%d" % r, QLEN, walkers[r * per:(r + 1) * per]))
    b = make_batch(cases)
    assert n_seeds(b, 16, 100) == total
    return b


def check(batch=None):
    """The contract of ma_batch_set_segments (include/ma_amd.h), for every segment of every case."""
    names, reads, seg_off, segs = case_batch() if batch is None else batch
    assert seg_off[0] == 0 and np.all(np.diff(seg_off.astype(np.int64)) >= 0), "seg_off is not monotone"
    assert int(seg_off[-1]) == len(segs) and len(seg_off) == len(reads) + 1
    for r, nm in enumerate(names):
        qlen = len(reads[r])
        assert 1 <= qlen and reads[r].max() <= 4, nm
        s = segs[int(seg_off[r]):int(seg_off[r + 1])]
        for f in ("q_start", "q_size", "sa_start", "sa_size"):
            assert np.all(s[f] >= 0), (nm, f, "negative field")
        assert np.all(s["sa_size"] >= 1), (nm, "empty interval")
        assert np.all(s["sa_start"] >= 1) and np.all(s["sa_start"] + s["sa_size"] <= N + 1), (nm, "interval outside rows 1 .. n")
        assert np.all(s["q_start"] + s["q_size"] + 1 <= qlen), (nm, "segment beyond its read")


def write_segs_file(path, batch):
    """The segments file of ref_dump_extract (oracle/dump_format.h, EXSEGS01)."""
    names, reads, seg_off, segs = batch
    with open(path, "wb") as f:
        f.write(b"EXSEGS01")
        f.write(np.array([len(reads), len(segs)], dtype="<u8").tobytes())
        f.write(np.asarray(seg_off, dtype="<u8").tobytes())
        f.write(np.asarray(segs, dtype=OR_SEGMENT_DT).tobytes())


def result_text(batch, min_seed_len, max_ambiguity):
    """expected_seeds() as the lines ref_dump_extract prints."""
    names, reads, seg_off, segs = batch
    off, seeds = expected_seeds(batch, min_seed_len, max_ambiguity)
    lines = ["P %d %d" % (min_seed_len, max_ambiguity)]
    for r in range(len(reads)):
        a, e = int(off[r]), int(off[r + 1])
        lines += ["R %d %d" % (r, len(reads[r])), "SEED %d" % (e - a)]
        lines += ["d %d %d %d %d %d %d" % (x["q_start"], x["len"], x["r_start"], x["ambiguity"], x["on_forward"], x["delta"]) for x in seeds[a:e]]
    return "\n".join(lines) + "\n"
