"""Seed lists that put the chain stage's sorts where sampled reads never put them (shared by test_chain_seeds_host.py and
test_gpu_chain_seeds.py): tie-heavy key patterns and McIlroy's adversary against libstdc++'s std::sort, whose lists run
introsort out of its depth budget so that the heap-sort branches of stdsort.h / wave_sort.h execute.

A list is a sequence of keys in the order the sort is to see them.  It becomes the seeds of one read in two flavours:
  "delta"   the keys are the deltas (the first sort of the sweep, stripOfConsideration.cpp:33), in input order;
  "refpos"  the keys are the reference positions (the second sort, soc.h:213): the deltas rise strictly, so the first sort
            leaves the input order alone and hands it to the second one.
tests/emul/sort_census.cpp (built here with g++) supplies the adversary's keys and certifies each list: which ranges get
heap-sorted, whether ss::sort and the wave form's host skeleton leave std::sort's permutation, whether that permutation
differs from a stable sort's."""
import functools
import os
import re
import subprocess
import tempfile

import numpy as np

from ma_testlib import OR_SEED_DT, ROOT

CSRC = os.path.join(ROOT, "ma_amd", "csrc")
CENSUS = os.path.join(ROOT, "tests", "emul", "sort_census")

LENGTHS = (17, 20, 21, 64, 65, 127, 128, 129, 130, 160, 199, 200, 257, 1023, 1024, 1025, 2000, 4096)
PATTERNS = ("equal", "two_alternating", "two_blocked", "few_random", "ascending_runs", "descending", "organ_pipe", "sawtooth",
            "random_distinct", "adversary_d1", "adversary_d2")
# patterns whose lists hold equal keys (descending, random_distinct and the d = 1 adversary are permutations of 0..n-1)
TIED = ("equal", "two_alternating", "two_blocked", "few_random", "ascending_runs", "organ_pipe", "sawtooth", "adversary_d2")
# A list with ties on which std::sort happens to leave std::stable_sort's permutation could not tell the algorithms apart and
# would have to be dropped here; the census finds none (test_chain_seeds_host.test_list_set_conditions asserts it).
DROPPED = ()


@functools.lru_cache(maxsize=None)
def ws_constants():
    """(WS_SERIAL, shift of PackedKeyLess) as the product's headers define them."""
    with open(os.path.join(CSRC, "wave_sort.h")) as f:
        serial = re.findall(r"^#define WS_SERIAL (\d+)\s*$", f.read(), re.M)
    with open(os.path.join(CSRC, "stage_chain.h")) as f:
        body = re.search(r"struct PackedKeyLess\s*\{.*?\};", f.read(), re.S).group(0)
    shifts = re.findall(r">> (\d+)", body)
    assert len(serial) == 1 and len(shifts) == 2 and shifts[0] == shifts[1], (serial, shifts)
    return int(serial[0]), int(shifts[0])


@functools.lru_cache(maxsize=None)
def census_tool():
    src = [os.path.join(ROOT, "tests", "emul", f) for f in ("sort_census.cpp", "sort_adversary.h")]
    deps = src + [os.path.join(CSRC, f) for f in ("stdsort.h", "ma_common.h", "wave_sort.h", "stage_chain.h")]
    if not os.path.exists(CENSUS) or any(os.path.getmtime(d) > os.path.getmtime(CENSUS) for d in deps):
        serial, shift = ws_constants()
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-w", "-I" + os.path.join(ROOT, "include"), "-DWS_SERIAL=%d" % serial,
                               "-DWS_KEY_SHIFT=%d" % shift, src[0], "-o", CENSUS])
    return CENSUS


def adversary_keys(lengths, d):
    """{n: keys} of McIlroy's adversary against std::sort, every key divided by d."""
    out = subprocess.check_output([census_tool(), "adversary", str(d)] + [str(n) for n in lengths]).decode()
    res = {}
    for line in out.splitlines():
        v = np.array(line.split(), dtype=np.int64)
        res[int(v[0])] = v[1:]
        assert len(v) == v[0] + 1
    return res


def pattern_keys(pattern, n, adversary=None):
    """Keys in [0, n) of one pattern; the adversary's come from adversary_keys."""
    i = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(1000 + n)
    if pattern == "equal":
        return np.zeros(n, dtype=np.int64)
    if pattern == "two_alternating":
        return i % 2
    if pattern == "two_blocked":
        return (i >= n // 2).astype(np.int64)
    if pattern == "few_random":  # n / 16 distinct values
        return rng.integers(0, max(2, n // 16), n).astype(np.int64)
    if pattern == "ascending_runs":
        return i // 3
    if pattern == "descending":
        return n - 1 - i
    if pattern == "organ_pipe":
        return np.minimum(i, n - 1 - i)
    if pattern == "sawtooth":
        return i % 13
    if pattern == "random_distinct":
        return rng.permutation(n).astype(np.int64)
    if pattern in ("adversary_d1", "adversary_d2"):
        return np.asarray(adversary[n], dtype=np.int64)
    raise ValueError(pattern)


@functools.lru_cache(maxsize=None)
def all_lists():
    """Every (pattern, length) before any is dropped: [(name, pattern, n, keys)]."""
    adv = {"adversary_d1": adversary_keys(LENGTHS, 1), "adversary_d2": adversary_keys(LENGTHS, 2)}
    out = []
    for p in PATTERNS:
        for n in LENGTHS:
            keys = pattern_keys(p, n, adv.get(p))
            assert len(keys) == n and keys.min() >= 0 and keys.max() < n
            out.append(("%s_%d" % (p, n), p, n, keys))
    return tuple(out)


def list_set():
    """The set the CPU and the GPU tests run: all_lists() without DROPPED."""
    return tuple(l for l in all_lists() if (l[1], l[2]) not in DROPPED)


def census(lists):
    """{name: dict(events=[(range length, has equal keys)], perms=bool, unstable=bool)} from sort_census (see its header)."""
    with tempfile.NamedTemporaryFile("w", suffix=".lists", delete=False) as f:
        for name, _, n, keys in lists:
            f.write("%s %d %s\n" % (name, n, " ".join(str(int(k)) for k in keys)))
        path = f.name
    try:
        out = subprocess.check_output([census_tool(), "census", path]).decode()
    finally:
        os.unlink(path)
    res = {}
    for line in out.splitlines():
        name, n, ev, perms, unstable = line.split()
        ev = ev.split("=")[1]
        res[name] = dict(n=int(n), events=[tuple(int(x) for x in e.split(":")) for e in ev.split(",")] if ev else [],
                         perms=perms == "perms=1", unstable=unstable == "unstable=1")
    assert len(res) == len(lists)
    return res


# ---- lists -> reads with given seeds ----------------------------------------------------------------------------------
GENOME_SEED, CONTIG_LENS = 71, (90000, 150000)
SEED_LEN = 16
MIN_QLEN = 300  # reads of up to 254 bases never reach the wave kernels (ma_chain_batch)


def seeds_of_list(keys, flavour, contig_starts, salt):
    """(qlen, OR_SEED_DT seeds in input order) of one list: all seeds forward on the second contig, away from its ends, SEED_LEN
    long, delta = r + qlen - q + (qlen + 1) * contig as ExtractSeeds sets it (stripOfConsideration.h:41-53)."""
    keys = np.asarray(keys, dtype=np.int64)
    n = len(keys)
    contig = 1
    base = int(contig_starts[contig]) + 20000
    rng = np.random.default_rng(5000 + 7 * n + salt)
    s = np.zeros(n, dtype=OR_SEED_DT)
    if flavour == "delta":
        qlen = 1000
        q = rng.integers(0, qlen - SEED_LEN + 1, n).astype(np.int64)  # varied, so that the reference positions mostly differ
        delta = base + (qlen + 1) * contig + qlen + keys
        r = delta - qlen + q - (qlen + 1) * contig
    elif flavour == "refpos":
        qlen = max(MIN_QLEN, 2 * n + 16)
        i = np.arange(n, dtype=np.int64)
        r = base + keys
        q = keys - i + (n - 1)
        delta = r + qlen - q + (qlen + 1) * contig
        assert np.all(np.diff(delta) == 1)
    else:
        raise ValueError(flavour)
    assert q.min() >= 0 and q.max() + SEED_LEN <= qlen and r.min() >= base and r.max() + SEED_LEN <= int(contig_starts[contig]) + CONTIG_LENS[contig] - 1000
    s["q_start"], s["len"], s["r_start"], s["delta"] = q, SEED_LEN, r, delta
    s["ambiguity"] = rng.integers(1, 4, n)
    s["on_forward"] = 1
    return qlen, s


def reads_of_lists(lists, flavours, contig_starts):
    """One read per (list, flavour): (names, reads of random bases, read_lens, seed_off, seeds)."""
    names, reads, seeds = [], [], []
    rng = np.random.default_rng(9)
    for fi, fl in enumerate(flavours):
        for name, _, n, keys in lists:
            qlen, s = seeds_of_list(keys, fl, contig_starts, fi)
            names.append((name, fl))
            reads.append(rng.integers(0, 4, qlen, dtype=np.uint8))
            seeds.append(s)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seeds])
    return names, reads, np.array([len(r) for r in reads], dtype=np.uint64), off, np.concatenate(seeds)
