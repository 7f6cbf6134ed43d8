"""Differential tests of the oracle against the real reference: every output file of the oracle must equal the reference's
on the same inputs, byte for byte.  tests/golden/oracle_vs_ref.sha256.json holds SHA-256 of the reference's files; where the
reference is compiled into oracle/_ref its fresh output is compared as well (MA_UPDATE_GOLDEN=1 records its hashes instead)."""
import filecmp
import hashlib
import json
import os

import pytest

from ma_testlib import (ROOT, sample_inversion_reads, sample_pairs, have_ref, rand_genome, sample_reads, write_case, write_ksw_cases, rand_ksw_cases,
                        run_ref, run_oracle, first_diff)

HASHES = os.path.join(ROOT, "tests", "golden", "oracle_vs_ref.sha256.json")


def _sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def same_as_reference(key, ref_path, or_path, *ref_args):
    """The oracle's file `or_path` against the reference's output `key` (written to `ref_path` by `ref_dump *ref_args`)."""
    with open(HASHES) as f:
        want = json.load(f)
    if have_ref():
        run_ref(*ref_args)
        assert filecmp.cmp(ref_path, or_path, shallow=False), key if key.startswith("index_") else first_diff(ref_path, or_path)
        if os.environ.get("MA_UPDATE_GOLDEN") == "1":
            want[key] = _sha256(ref_path)
            with open(HASHES, "w") as f:
                json.dump(want, f, indent=1, sort_keys=True)
                f.write("\n")
    assert _sha256(or_path) == want[key], key


def test_ksw_random_cases(tmp_path):
    cases = rand_ksw_cases(4000, 991, max_len=150) + rand_ksw_cases(40, 992, long_frac=1.0)
    p = str(tmp_path / "k.case")
    write_ksw_cases(p, cases)
    run_oracle("ksw", p, str(tmp_path / "or.out"))
    same_as_reference("ksw_random", str(tmp_path / "ref.out"), str(tmp_path / "or.out"), "ksw", p, str(tmp_path / "ref.out"))


# match, mismatch, gap, extend, gap2, extend2 -- the third has q2 + e2 < q + e, which makes
# kswcpp swap the two models internally (kswcpp_core.h:367-377) while still seeding H[0] from the un-swapped one
OTHER_SCORINGS = [(3, 5, 6, 3, 30, 2), (1, 3, 5, 2, 24, 1), (2, 4, 24, 1, 4, 2), (5, 4, 2, 1, 40, 1)]


@pytest.mark.parametrize("sc", OTHER_SCORINGS)
def test_ksw_other_scoring_schemes(tmp_path, sc):
    cases = rand_ksw_cases(1500, 993 + sc[0], max_len=150) + rand_ksw_cases(12, 994, long_frac=1.0)
    p = str(tmp_path / "k.case")
    write_ksw_cases(p, cases)
    run_oracle("ksw", p, str(tmp_path / "or.out"), "clean", *sc)
    same_as_reference("ksw_scoring_%s" % "_".join(map(str, sc)), str(tmp_path / "ref.out"), str(tmp_path / "or.out"),
                      "ksw", p, str(tmp_path / "ref.out"), "clean", *sc)


# No whole-pipeline test under other scoring schemes: `pGlobalParams` is a namespace-scope const shared_ptr defined in a
# header (parameter.h:1064), i.e. every translation unit of the reference holds its OWN copy; a value set by the caller
# reaches the code inlined into the caller's unit (NeedlemanWunsch's kswcpp parameters) but not alignment.cpp or
# harmonization.cpp, so the reference's pipeline under non-default scoring is not a single well-defined function.
# kswcpp itself takes its parameters explicitly and is pinned above.


@pytest.mark.parametrize("preset", ["default", "illumina", "default+mems", "illumina+mems"])
def test_pipeline_with_heuristics_and_repeats(tmp_path, preset):
    # doubled length > 10 Mnt so that the genome-size gated heuristics are active
    g = rand_genome(5, [2600000, 1500000, 1000000], repeat_unit=300, repeat_copies=200, repeat_div=0.08)
    reads = (sample_reads(g, 250, 150, 31, sub=0.01) + sample_reads(g, 60, 150, 32, sub=0.06, n_rate=0.01)
             + sample_reads(g, 8, 6000, 33, sub=0.005, ins=0.003, dele=0.003)
             + sample_reads(g, 2, 30000, 34, sub=0.03, ins=0.03, dele=0.04) + sample_reads(g, 10, 150, 35, random_frac=1.0))
    p = str(tmp_path / "c.case")
    write_case(p, g, reads)
    run_oracle("pipe", p, preset, 3, str(tmp_path / "or.pipe"))
    same_as_reference("pipe_%s" % preset, str(tmp_path / "ref.pipe"), str(tmp_path / "or.pipe"), "pipe", p, preset, 3, str(tmp_path / "ref.pipe"))


@pytest.mark.parametrize("preset,inv,paired,zdrop_inv", [("default", 1, 0, 100), ("default", 1, 0, 30), ("default", 0, 1, 100),
                                                         ("illumina", 1, 1, 100), ("default", 1, 1, 60)])
def test_f4_small_inversions_and_paired_reads(tmp_path, preset, inv, paired, zdrop_inv):
    """SmallInversions (smallInversions.h) and PairedReads (pairedReads.cpp) after MappingQuality."""
    g = rand_genome(21, [60000, 35000, 12000], repeat_unit=250, repeat_copies=30, repeat_div=0.05)
    reads = (sample_pairs(g, 250, 150, 71) + sample_pairs(g, 30, 250, 72, sub=0.05, insert_mean=600, insert_std=200)
             + sample_inversion_reads(g, 24, 1400, 73) + sample_inversion_reads(g, 6, 4000, 74, inv_min=300, inv_max=900, sub=0.03))
    p = str(tmp_path / "c.case")
    write_case(p, g, reads)
    run_oracle("f4", p, preset, 5, str(tmp_path / "or.f4"), inv, paired, zdrop_inv)
    same_as_reference("f4_%s_inv%d_pair%d_zd%d" % (preset, inv, paired, zdrop_inv), str(tmp_path / "ref.f4"), str(tmp_path / "or.f4"),
                      "f4", p, preset, 5, str(tmp_path / "ref.f4"), inv, paired, zdrop_inv)
    if inv:  # the case must actually contain inversions that are found (the oracle's file is the reference's, checked above)
        with open(str(tmp_path / "or.f4")) as f:
            assert sum(1 for l in f if l.startswith("f ") and " 0:" not in l) >= 10


def test_index_and_traces(tmp_path):
    g = rand_genome(8, [70000, 1, 129, 40000])
    reads = sample_reads(g[:1], 80, 120, 41, sub=0.02)
    p = str(tmp_path / "c.case")
    write_case(p, g, reads)
    run_oracle("index", p, str(tmp_path / "or"))
    for ext in ("bwt", "sa", "pac"):
        same_as_reference("index_" + ext, str(tmp_path / ("ref." + ext)), str(tmp_path / ("or." + ext)), "index", p, str(tmp_path / "ref"))
    run_oracle("ext", p, str(tmp_path / "or.ext"))
    same_as_reference("ext", str(tmp_path / "ref.ext"), str(tmp_path / "or.ext"), "ext", p, str(tmp_path / "ref.ext"))
