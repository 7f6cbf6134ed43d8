"""Genome and reads of the tests of the seeding kernel's text mode (ma_amd/csrc/seeding.h): test_seed_text_host.py runs them
through the CPU build of the state machine, test_gpu_seed_text.py through the kernels."""
import numpy as np

from ma_testlib import rand_genome, revcomp, sample_reads

CONTIGS = [600000, 300000]
REPEAT_UNIT = 400
REPEAT_AT = [(0, 50000), (0, 222222), (0, 431000), (1, 10000), (1, 155555), (1, 280000)]


def genome():
    """Two contigs with diverged repeats (as the round-3 tests plant them) and six exact copies of one 400-base unit, two of them
    reverse-complemented: a read out of a copy never becomes unique."""
    g = rand_genome(97, CONTIGS, repeat_unit=180, repeat_copies=150, repeat_div=0.03)
    unit = np.random.default_rng(98).integers(0, 4, size=REPEAT_UNIT, dtype=np.uint8)
    for k, (c, p) in enumerate(REPEAT_AT):
        g[c][p:p + REPEAT_UNIT] = revcomp(unit) if k % 3 == 2 else unit
    return g


def reads(g):
    T = np.concatenate(g)
    F = len(T)
    T2 = np.concatenate([T, revcomp(T)])
    out = (sample_reads(g, 1500, 150, 101, sub=0.02) + sample_reads(g, 300, 150, 102, sub=0.03, n_rate=0.02)
           + sample_reads(g, 200, 150, 103, random_frac=1.0))
    # out of the exact repeat copies, both strands, some with a substitution
    rng = np.random.default_rng(104)
    for k in range(40):
        c, p = REPEAT_AT[k % len(REPEAT_AT)]
        o = int(rng.integers(0, REPEAT_UNIT - 150))
        r = g[c][p + o:p + o + 150].copy()
        if k % 4 == 3:
            j = int(rng.integers(0, 150))
            r[j] = (r[j] + 1) % 4
        out.append(revcomp(r) if k % 2 else r)
    # the ends of the doubled text, the junction of the strands, a contig border (both strands)
    border = CONTIGS[0]
    for r in (T2[:150], T2[-150:], T2[F - 150:F], T2[F:F + 150], T2[F - 75:F + 75], T2[F - 20:F + 130], T2[border - 75:border + 75],
              T2[border - 149:border + 1]):
        out += [r.copy(), revcomp(r)]
    # a reverse-complement palindrome that is not in the text as a whole
    half = g[0][300000:300075]
    out.append(np.concatenate([half, revcomp(half)]))
    # lengths around the K-mer table's K = 12, one base, and the longest read the kernel keeps in LDS
    for k, ln in enumerate((1, 11, 12, 13, 240)):
        p = 123456 + 1000 * k
        out += [g[0][p:p + ln].copy(), revcomp(g[1][p:p + ln])]
    return out
