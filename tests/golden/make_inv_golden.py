#!/usr/bin/env python3
"""Generates the inv.* goldens: the compiled reference's SmallInversions (smallInversions.h:22-221) + PairedReads + file
writers on reads with small inversions, several of them with TWO inverted stretches and most of the inversion records
followed by another record of their list (f4.case has at most one inversion per list, 5 of them in 9 records).

Needs oracle/_ref/ref_dump (make -C oracle ref, where the reference's sources exist).  The outputs are data only: the
synthetic case and the reference's dumps and SAM text on it.  Run:  python tests/golden/make_inv_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from ma_testlib import _mutate, have_ref, rand_genome, revcomp, run_ref, sample_inversion_reads, sample_pairs, write_case  # noqa
from make_golden import gz  # noqa

# (preset, paired, Z Drop Inversions, SAM options); "Detect Small Inversions" is on in all of them
INV_CONFIGS = [("default", 0, 40, 3), ("default", 1, 40, 1), ("default", 0, 100, 0)]


def inv_name(preset, paired, zd, opt):
    return "inv.%s.pair%d.zd%d.opt%d" % (preset, paired, zd, opt)


def two_inversion_reads(contigs, n, length, seed, inv_min, inv_max, sub=0.01):
    """reads with two in-place reverse-complemented stretches, one in each half; every second read reverse-complemented"""
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(n):
        c = contigs[int(rng.integers(0, len(contigs)))]
        p = int(rng.integers(0, len(c) - length + 1))
        rd = _mutate(c[p:p + length], rng, sub)
        for half in (0, 1):
            w = int(rng.integers(inv_min, inv_max + 1))
            lo = half * (length // 2) + length // 10
            a = int(rng.integers(lo, (half + 1) * (length // 2) - length // 10 - w))
            rd[a:a + w] = revcomp(rd[a:a + w])
        if i % 2 == 1:
            rd = revcomp(rd)
        reads.append(rd)
    return reads


def inv_case():
    g = rand_genome(11, [60000, 45000, 30000])
    reads = (sample_pairs(g, 24, 150, 5) + sample_inversion_reads(g, 8, 1200, 7) + two_inversion_reads(g, 8, 2400, 21, 100, 300)
             + sample_inversion_reads(g, 8, 400, 13, inv_min=60, inv_max=120) + two_inversion_reads(g, 8, 1000, 22, 60, 140))
    return g, reads


def fin_lists(path):
    """the FIN lists of an f4 dump: per list the text of its 'f' lines"""
    lists = []
    for line in open(path):
        if line.startswith("FIN"):
            lists.append([])
        elif line.startswith("f "):
            lists[-1].append(line.strip())
    return lists


def inversion_stats(with_inv, without):
    """(inversion records, parents with two of them, inversion records that are not the last of their list): an inversion
    record is a supplementary record with mapq 0 of the list with the module that the list without it does not hold"""
    records = two = not_last = 0
    for a, b in zip(fin_lists(with_inv), fin_lists(without)):
        assert len(a) >= len(b)
        j = run = 0
        for i, line in enumerate(a):
            if j < len(b) and line == b[j]:
                j, run = j + 1, 0
                continue
            records += 1
            run += 1
            two += run == 2
            not_last += i + 1 < len(a)
        assert j == len(b), "the list without the module is not a subsequence of the one with it"
    return records, two, not_last


def main():
    if not have_ref():
        sys.exit("oracle/_ref/ref_dump missing: run `make -C oracle ref` where the reference's sources exist")
    os.chdir(HERE)
    g, reads = inv_case()
    assert len(reads) == 80 and sum(len(r) for r in reads) == 47200
    write_case("inv.case", g, reads)
    for preset, paired, zd, opt in INV_CONFIGS:
        nm = inv_name(preset, paired, zd, opt)
        run_ref("f4", "inv.case", preset, 1, nm + ".f4", 1, paired, zd, nm + ".sam", opt)
        run_ref("f4", "inv.case", preset, 1, "inv.off.f4", 0, paired, zd, "inv.off.sam", opt)
        st = inversion_stats(nm + ".f4", "inv.off.f4")
        print(nm, "inversion records %d, parents with two %d, not last in their list %d" % st)
        if zd == 40:
            assert st[0] >= 20 and st[1] >= 3 and st[2] >= 10, st
        os.remove("inv.off.f4")
        os.remove("inv.off.sam")
        gz(nm + ".f4")
        gz(nm + ".sam")
    gz("inv.case")


if __name__ == "__main__":
    main()
