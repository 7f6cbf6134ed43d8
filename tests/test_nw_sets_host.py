"""The DP stage on hand-made harmonized sets, CPU part (tests/nw_sets.py has the cases).  In the order a case has to pass before a
device sees it: the contract of the list, the certification of what each case is for (from the oracle's result and job list),
the oracle against the compiled reference's goldens, the product's walk compiled for the CPU (tests/emul/host_emul.cpp with
MA_EMUL_HSETS) against the oracle, and the same program under the address and undefined-behaviour sanitizers."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import nw_sets as ns
from ma_testlib import ROOT, OrIndex, build_oracle, or_params, parse_pipe_dump, write_case
from test_host_logic import emul  # noqa: F401 (fixture: tests/emul/host_emul)

MT_SEED, MT_MATCH, MT_MISS, MT_INS, MT_DEL = range(5)


@pytest.fixture(scope="module")
def oidx():
    return OrIndex.build(list(ns.genome()))


@pytest.fixture(scope="module")
def batch():
    ns.check()
    return ns.case_batch()


@pytest.fixture(scope="module")
def results(oidx, batch):
    """{scoring: OrIndex.nw_sets on the whole list}"""
    names, reads, hset_off, hseed_off, hset_soc, seeds = batch
    return {sc: oidx.nw_sets(reads, hset_off, hseed_off, hset_soc, seeds, ns.or_scoring(or_params("default", 1), sc)) for sc in ns.SCORINGS}


def ops_of(res, x, key="ops"):
    o = res[key][2 * int(x["ops_off"]):2 * (int(x["ops_off"]) + int(x["n_ops"]))]
    return [(int(o[2 * i]), int(o[2 * i + 1])) for i in range(int(x["n_ops"]))]


def test_list_contract_and_coverage():
    """check() holds, the genome is what the clamps need, every kind of case the list is there for is in it, and the size stays small."""
    ns.check()
    cases = ns.all_cases()
    assert all(ln % 4 for ln in ns.CONTIG_LENS) and ns.CONTIG_LENS[0] > 2 * ns.PADDING and ns.CONTIG_LENS[1] < ns.PADDING
    names = [c["name"] for c in cases]
    for part in ("whole_read_one_seed", "one_seed_middle", "one_base_seed_last_base", "one_base_seed_first_base", "read_of_one_base",
                 "gap_1x1_mismatch", "gap_1x1_n", "gap_2x1", "gap_pure_ins", "gap_pure_del", "gap_20x20", "gap_21x5", "gap_5x21", "gap_20x5",
                 "gap_5x20", "gap_40_mismatches_dual", "overlap_query_only", "overlap_reference_only", "overlap_both_query_more",
                 "overlap_swallowed", "overlap_swallowed_exactly_len", "zero_length_seed_middle", "zero_length_seed_first",
                 "zero_length_seed_last", "ns_inside_gap", "ns_in_unseeded_ends"):
        assert part + "_fwd" in names and part + "_rev" in names, part
    for nm in ("front_bases_at_text_position_0", "front_bases_at_first_base_of_contig_1", "front_bases_at_first_base_of_reverse_strand",
               "window_clamped_at_contig_start", "window_clamped_at_contig_end", "window_clamped_at_n_minus_1",
               "window_clamped_at_both_ends_of_short_contig", "bridging_two_contigs", "bridging_strand_border", "empty_set_alone",
               "empty_set_then_real", "two_identical_sets_soc_0_1", "two_identical_sets_soc_1_0", "five_equal_scores",
               "more_candidates_than_max_supplementary", "best_score_below_min_alignment_score", "first_alignment_one_seed_only",
               "one_seed_only_three_sets_high_score", "all_alignments_empty", "read_without_sets", "long_64_seeds_span_1023"):
        assert nm in names, nm
    for e in ("contig_0", "last_forward_contig", "doubled_text"):
        assert "ends_on_last_base_of_" + e in names and "ends_a_base_before_last_of_" + e in names
    assert [c["expect"]["n_seeds"] for c in cases if c["name"].startswith("long_") and c["name"].endswith("_seeds")] == list(ns.LONG_SEED_COUNTS)
    assert [c["expect"]["dual_at"] for c in cases if "dual_at" in c["expect"]] == list(ns.STRADDLES)
    lens = [len(c["read"]) for c in cases]
    assert min(lens) == 1 and all(ln <= 260 or 1100 <= ln <= 1400 for ln in lens)
    i = names.index("read_without_sets")
    assert not cases[i]["sets"] and cases[i - 1]["sets"] and cases[i + 1]["sets"]
    assert len(cases) <= 400 and sum(len(c["sets"]) for c in cases) <= 2000


@pytest.mark.parametrize("scoring", list(ns.SCORINGS))
def test_cases_are_what_they_are_for(batch, results, scoring):
    """Certification from the oracle's alignments and its kswcpp calls: every expectation a case carries (nw_sets.py) holds."""
    names, reads, hset_off, hseed_off, hset_soc, seeds = batch
    res = results[scoring]
    cases = ns.all_cases()
    P = ns.or_scoring(or_params("default", 1), scoring)
    assert (P.padding, P.max_gap_area, P.max_overlap_supplementary, P.max_supplementary, P.min_alignment_score) == (
        ns.PADDING, ns.MAX_GAP_AREA, ns.MAX_OVERLAP_SUPPLEMENTARY, ns.MAX_SUPPLEMENTARY, ns.MIN_ALIGNMENT_SCORE)
    seen = set()
    for r, c in enumerate(cases):
        nm, e = c["name"], c["expect"]
        seen.update(e)
        s0, s1 = int(hset_off[r]), int(hset_off[r + 1])
        jobs = [res["jobs"][int(res["job_off"][s]):int(res["job_off"][s + 1])] for s in range(s0, s1)]
        alns = res["alns"][int(res["aln_off"][r]):int(res["aln_off"][r + 1])]
        mq = res["mq"][int(res["mq_off"][r]):int(res["mq_off"][r + 1])]
        assert len(alns) == s1 - s0, nm
        if "flags" in e:  # the kswcpp calls of every set, in call order, by their flags
            assert [[int(j["flag"]) for j in js] for js in jobs] == e["flags"], nm
            for js in jobs:
                for j in js:
                    big = max(int(j["qlen"]), int(j["tlen"])) > ns.MAX_GAP_AREA
                    assert int(j["flag"]) != ns.J_GAP or not big, (nm, "a gap beyond max_gap_area takes the dual extension")
        if e.get("empty"):  # bridging, ending exactly on a contig's last base, or no seeds: the empty alignment
            for x in alns:
                assert (int(x["n_ops"]), int(x["score"]), int(x["begin_ref"]), int(x["end_ref"]), int(x["begin_q"]), int(x["end_q"])) == (0,) * 6, nm
            assert all(len(js) == 0 for js in jobs), nm
        if "end_ref" in e:  # one base earlier: not bridging, and the alignment ends at the clamp
            assert int(alns[0]["n_ops"]) > 0 and int(alns[0]["end_ref"]) == e["end_ref"], (nm, alns[0])
        if "begin_ref" in e:
            assert (int(alns[0]["begin_ref"]), int(alns[0]["begin_q"])) == (e["begin_ref"], e["begin_q"]), (nm, alns[0])
        if "window" in e:  # the extensions' reference stretches show where the window begins and ends
            lo, hi = e["window"]
            sd = c["sets"][0][1]
            assert int(jobs[0][0]["tlen"]) == int(sd["r_start"][0]) - lo, (nm, "window begin")
            assert int(jobs[0][-1]["tlen"]) == hi - 1 - int(sd["r_start"][-1] + sd["len"][-1]), (nm, "window end")
        if "ops_have" in e:
            have = ops_of(res, alns[0])
            for op in e["ops_have"]:
                assert op in have, (nm, op, have)
        if "dual_at" in e:  # the two halves of the dual extension sit on the stated job indices, everything before is 1 x 1 but job 0
            a, b = e["dual_at"]
            fl = [int(j["flag"]) for j in jobs[0]]
            assert (fl[a], fl[b]) == (ns.J_END, ns.J_BEGIN) and fl[0] == ns.J_BEGIN and fl[1:a] == [ns.J_GAP] * (a - 1), nm
            assert all((int(j["qlen"]), int(j["tlen"])) == (1, 1) for j in jobs[0][1:a]), nm
        if "wave" in e:  # stitch_is_big's condition, from the case data
            sd = c["sets"][0][1]
            assert (ns.set_span(sd) >= ns.WAVE_SPAN) == e["wave"], nm
            assert int(alns[0]["n_ops"]) > 0, nm
            if not e["wave"]:
                assert ns.set_span(sd) == ns.WAVE_SPAN - 1
        if "n_seeds" in e:
            assert len(c["sets"][0][1]) == e["n_seeds"], nm
            if e["n_seeds"] >= 63:  # all four gap kinds occur: touching seeds, 1 x 1, a small gap, a dual gap
                sd = c["sets"][0][1]
                gq = sd["q_start"][1:] - (sd["q_start"][:-1] + sd["len"][:-1])
                assert {0, 1, 2, ns.DUAL[1]} <= set(int(g) for g in gq), nm
                assert sum(1 for j in jobs[0] if int(j["flag"]) == ns.J_BEGIN) >= 3, nm
        if "ends" in e:
            sd = c["sets"][0][1]
            assert (int(sd["q_start"][0]), len(c["read"]) - int(sd["q_start"][-1] + sd["len"][-1])) == e["ends"], nm
            assert int(jobs[0][0]["qlen"]) == e["ends"][0] and int(jobs[0][-1]["qlen"]) == e["ends"][1] - 1, nm
            have = ops_of(res, alns[0])
            assert sum(1 for t, ln in have if t == MT_MISS) >= 4, (nm, "the planted mismatches are inside the alignment")
        if e.get("tie"):
            assert len(set(int(x["score"]) for x in alns)) == 1 and len(alns) >= 2, nm
            assert [int(x["soc_index"]) for x in alns] == sorted(int(x["soc_index"]) for x in alns), (nm, "ties go by soc_index")
        if "mq_len" in e:
            assert len(mq) == e["mq_len"], nm
        if "mq_flags" in e:
            assert [(int(x["secondary"]), int(x["supplementary"])) for x in mq] == e["mq_flags"], nm
        if "mq_socs" in e:
            assert [int(x["soc_index"]) for x in mq] == e["mq_socs"], nm
        if "mq_kinds" in e:
            assert sum(int(x["supplementary"]) for x in mq) == e["mq_kinds"]["supplementary"], nm
            assert sum(int(x["secondary"]) for x in mq) == e["mq_kinds"]["secondary"], nm
        if "overlap" in e:  # the second alignment's query interval overlaps the first's by k of its sz bases: k / sz against the threshold
            k, sz = e["overlap"]
            a, b = alns[0], alns[1]
            assert int(b["end_q"]) - int(b["begin_q"]) == sz <= int(a["end_q"]) - int(a["begin_q"]), nm
            assert min(int(a["end_q"]), int(b["end_q"])) - max(int(a["begin_q"]), int(b["begin_q"])) == k, nm
            assert (k / sz < ns.MAX_OVERLAP_SUPPLEMENTARY) == (e["mq_flags"][1] == (0, 1)), nm
        if "best_score" in e:
            assert int(alns[0]["score"]) == e["best_score"] * int(P.match) // 2 < ns.MIN_ALIGNMENT_SCORE, nm
        if e.get("one_seed"):
            assert sum(1 for t, _ in ops_of(res, mq[0], "mq_ops") if t == MT_SEED) == 1, nm
        if e.get("high"):
            assert len(alns) >= 3 and int(mq[0]["score"]) >= 0.8 * int(P.match) * len(c["read"]), nm
    assert {"flags", "empty", "end_ref", "window", "dual_at", "wave", "tie", "overlap", "one_seed", "high", "ends"} <= seen
    # every walk branch the list is there for, counted over the whole list
    allops = [op for x in res["alns"] for op in ops_of(res, x)]
    assert any(t == MT_INS for t, _ in allops) and any(t == MT_DEL for t, _ in allops)
    assert res["n_aligned"] == sum(1 for r in range(len(cases)) if res["mq_off"][r + 1] > res["mq_off"][r])
    assert 0 < res["n_aligned"] < len(cases)


@pytest.mark.parametrize("scoring", list(ns.SCORINGS))
def test_oracle_vs_reference_golden(batch, results, scoring):
    """OrIndex.nw_sets against the compiled reference's NeedlemanWunsch::execute + MappingQuality::execute on the same sets
    (tests/golden/make_nw_sets_golden.py): every ALN and MQ field, mapq as %.17g text."""
    want = gzip.open(ns.golden_path(scoring), "rt").read().splitlines()
    got = ns.result_text(batch[1], results[scoring]).splitlines()
    r = -1
    for a, b in zip(got, want):
        if a.startswith("R "):
            r = int(a.split()[1])
        assert a == b, (batch[0][r], a, b)
    assert len(got) == len(want)


def write_inputs(tmp_path, batch):
    names, reads, hset_off, hseed_off, hset_soc, seeds = batch
    case, sets = str(tmp_path / "nw_sets.case"), str(tmp_path / "nw_sets.sets")
    write_case(case, list(ns.genome()), reads)
    ns.write_sets_file(sets, reads, hset_off, hseed_off, hset_soc, seeds)
    return case, sets


def emul_env(sets, scoring):
    env = dict(os.environ, MA_EMUL_HSETS=sets)
    if ns.SCORINGS[scoring] is not None:
        env["MA_EMUL_SCORING"] = ",".join(str(v) for v in ns.SCORINGS[scoring])
    return env


def assert_dump_is_oracles(path, batch, res):
    """host_emul's dump of the given-sets mode against OrIndex.nw_sets: the jobs of every set, the ALN and the MQ lines."""
    names, reads = batch[0], batch[1]
    hset_off = batch[2]
    jobs = {}
    with open(path) as f:
        for line in f:
            if line.startswith("j "):
                t = [int(v) for v in line.split()[1:]]
                jobs.setdefault((cur, t[0]), []).append(tuple(t[1:]))
            elif line.startswith("R "):
                cur = int(line.split()[1])
    for r in range(len(reads)):
        for k, s in enumerate(range(int(hset_off[r]), int(hset_off[r + 1]))):
            want = [tuple(int(j[f]) for f in ("qlen", "tlen", "w", "zdrop", "flag")) for j in
                    res["jobs"][int(res["job_off"][s]):int(res["job_off"][s + 1])]]
            assert jobs.get((r, k), []) == want, (names[r], k)
    with open(path) as f:
        got = [ln for ln in f.read().splitlines() if ln[0] not in "jhH"]
    want = ns.result_text(reads, res).splitlines()
    r = -1
    for a, b in zip(got, want):
        if a.startswith("R "):
            r = int(a.split()[1])
        assert a == b, (names[r], a, b)
    assert len(got) == len(want)
    assert len(parse_pipe_dump(path)) == len(reads)


@pytest.mark.parametrize("scoring", list(ns.SCORINGS))
def test_stage_logic_on_the_sets_vs_oracle(emul, tmp_path, batch, results, scoring):  # noqa: F811
    """The product's nw.h compiled for the CPU -- nw_window, the enumeration walk, the stitch walk with the ops capacity of
    k_ops_caps, finish_read -- on the given sets: the jobs of every set are the oracle's kswcpp calls, the alignments and the
    MappingQuality output the oracle's.  What a GPU run of test_gpu_nw_sets.py compares, minus the kernels."""
    case, sets = write_inputs(tmp_path, batch)
    out = str(tmp_path / "emul.pipe")
    subprocess.check_call([emul, case, "default", "1", out, "all"], env=emul_env(sets, scoring))
    assert_dump_is_oracles(out, batch, results[scoring])


def test_stage_logic_on_the_sets_is_clean_under_address_and_ub_sanitizers(tmp_path, batch, results):
    """The same stand-alone program built with clang's -fsanitize=address,undefined (as
    test_host_logic.test_stage_logic_is_clean_under_address_and_ub_sanitizers builds it) on the whole list, both scorings: the same
    output and no report.  Every set's ops live in a heap block of exactly the capacity the product gives it, so a walk that
    wrote or read behind it would be reported: the evidence that no case makes the walk leave its arrays."""
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("no clang")
    build_oracle()
    exe = str(tmp_path / "host_emul_san")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-w",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emul", "host_emul.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "oracle"), "-lma_oracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    case, sets = write_inputs(tmp_path, batch)
    for scoring in ns.SCORINGS:
        out = str(tmp_path / ("san.%s.pipe" % scoring))
        p = subprocess.run([exe, case, "default", "1", out, "all"], env=dict(emul_env(sets, scoring), ASAN_OPTIONS="detect_leaks=0"),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-2000:]
        assert_dump_is_oracles(out, batch, results[scoring])


def test_nw_sets_reproduces_the_oracles_own_dp_stage(oidx):
    """OrIndex.nw_sets fed the harmonized sets OrIndex.align made gives align's alignments and MappingQuality output: the entry
    runs the same NeedlemanWunsch and MappingQuality, only from given sets."""
    from ma_testlib import sample_reads
    g = list(ns.genome())
    reads = sample_reads(g, 60, 150, 1, sub=0.03, ins=0.005, dele=0.005) + sample_reads(g, 3, 1500, 2, sub=0.03, ins=0.01, dele=0.01)
    for scoring in ns.SCORINGS:
        op = ns.or_scoring(or_params("default", 1), scoring)
        res = oidx.align(reads, op)
        assert len(res["hseeds"]) > 60
        got = oidx.nw_sets(reads, res["hset_off"], res["hseed_off"], res["hset_soc"], res["hseeds"], op)
        assert np.array_equal(got["aln_off"], res["aln_off"]) and np.array_equal(got["mq_off"], res["mq_off"])
        assert got["alns"].tobytes() == res["alns"].tobytes() and np.array_equal(got["ops"], res["ops"])
        for f in ("begin_ref", "end_ref", "begin_q", "end_q", "score", "soc_index", "n_ops", "secondary", "supplementary"):
            assert np.array_equal(got["mq"][f], res["mq"][f]), f
        assert np.array_equal(got["mq"]["mapq"].view(np.uint64), res["mq"]["mapq"].view(np.uint64))
        assert got["n_aligned"] == res["n_aligned"]
