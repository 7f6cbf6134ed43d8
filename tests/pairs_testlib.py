"""Helpers of the pairing tests (test_gpu_pairs.py): the oracle's f4 dump of mate pairs, parsed; what its lists say about the
input (ties, improper winners, empty mates: the things a pairing test has to contain to prove anything)."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ma_testlib import orlib


def _rec(t):
    """one 'f' / 'p' line of an f4 dump (oracle/ma_oracle_api.inc dumpF4Line) after its tag"""
    n = int(t[11])
    return dict(first=int(t[0]), other=int(t[1]), begin_ref=int(t[2]), end_ref=int(t[3]), begin_q=int(t[4]), end_q=int(t[5]),
                score=int(t[6]), soc_index=int(t[7]), secondary=int(t[8]), supplementary=int(t[9]), mapq=t[10], n_ops=n,
                ops=[tuple(int(x) for x in o.split(":")) for o in t[12:12 + n]], text=" ".join(t))


def parse_f4_pairs(path):
    """[{l1, l2, fin: ([records of mate 1], [of mate 2]), pair: [records]}] of a paired f4 dump"""
    pairs = []
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t:
                continue
            if t[0] == "P":
                pairs.append(dict(l1=int(t[2]), l2=int(t[3]), fin=([], []), pair=[]))
                cur = None
            elif t[0] == "FIN":
                cur = pairs[-1]["fin"][int(t[1])]
            elif t[0] == "f":
                cur.append(_rec(t[1:]))
            elif t[0] == "p":
                pairs[-1]["pair"].append(_rec(t[1:]))
    return pairs


def oracle_pairs(oidx, reads, params, prefix, threads=16):
    """ma_or_dump_f4 (single-threaded per call) over `threads` slices of whole pairs at once, parsed"""
    L = orlib()
    n_pairs = len(reads) // 2
    cuts = [2 * (n_pairs * i // threads) for i in range(threads + 1)]

    def run(i):
        part = reads[cuts[i]:cuts[i + 1]]
        if not part:
            return []
        off = np.zeros(len(part) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in part])
        cat = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.uint8) for r in part] + [np.zeros(1, dtype=np.uint8)]))
        path = "%s.%d.f4" % (prefix, i)
        rc = L.ma_or_dump_f4(oidx.h, C.byref(params), cat.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                             C.c_uint64(len(part)), path.encode())
        assert rc == 0
        out = parse_f4_pairs(path)
        os.remove(path)
        return out

    with ThreadPoolExecutor(max_workers=threads) as ex:
        parts = list(ex.map(run, range(threads)))
    return [p for part in parts for p in part]


def pair_stats(pairs, params, ref_len, tie_cap=32):
    """What the oracle's lists hold, counted with the definition of pairedReads.cpp:14-110 (integer / double arithmetic of
    Python is that of C here: the products stay far below 2^53)."""
    st = dict(pairs=len(pairs), tied=0, improper_winner=0, one_empty=0, both_empty=0, over_cap=0, max_cand=0, mapq_set=0)
    mean, std, bonus = int(params.mean_paired_dist), params.std_paired_dist, params.paired_bonus
    F = ref_len // 2
    for p in pairs:
        a, b = p["fin"]
        if not a and not b:
            st["both_empty"] += 1
            continue
        if not a or not b:
            st["one_empty"] += 1
            continue
        cands = []
        for x in a:
            if sum(o[1] for o in x["ops"]) == 0:
                continue
            for y in b:
                if sum(o[1] for o in y["ops"]) == 0:
                    continue
                key, proper = x["score"] + y["score"], False
                if (x["begin_ref"] >= F) != (y["begin_ref"] >= F):
                    d = abs(x["begin_ref"] - (ref_len - (y["begin_ref"] + 1)))
                    if float(mean) - std * 3 <= float(d) <= float(mean) + std * 3:
                        key, proper = int(key * bonus), True
                cands.append((key, proper))
        best = max(cands, key=lambda c: (c[0], c[1]))
        tied = sum(c == best for c in cands)
        st["max_cand"] = max(st["max_cand"], len(cands))
        if tied > 1:
            st["tied"] += 1
            if len(cands) > tie_cap:
                st["over_cap"] += 1
        if not best[1]:
            st["improper_winner"] += 1
        elif len(cands) > 1:
            st["mapq_set"] += 1
    return st
