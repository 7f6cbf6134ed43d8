"""The chain stage on hand-made seeds, CPU part (tests/harm_sets.py has the cases).  In the order a case has to pass before a device
sees it: the contract of the list; the certification of what each case is for, from the branch census of the product's chain.h
compiled for the CPU (tests/emul/harm_census.cpp; the table of behaviours against covering cases is printed, no row may be
empty); the oracle against the compiled reference's goldens, byte for byte; the host form of chain_read -- sweeping for itself,
on strips swept beforehand over prefix sums, and on a given queue -- against the oracle; the same bytes under every mode of the
libm probe (a case within an ulp of a libm-dependent threshold is no test of the kernel: the device's libm and glibc differ
there); and the census under the address and undefined-behaviour sanitizers (a stand-alone program, nothing is preloaded)."""
import gzip
import os
import subprocess

import pytest

import harm_sets as hs
from ma_testlib import REF_DUMP, ROOT, OrIndex, have_ref, or_params, write_case

SRC = os.path.join(ROOT, "tests", "emul", "harm_census.cpp")
CSRC = os.path.join(ROOT, "ma_amd", "csrc")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def build_census(kind, exe=None, include=None):
    """tests/emul/harm_census(_san), rebuilt when a source is newer; include: a directory that holds another chain.h"""
    exe = exe or os.path.join(ROOT, "tests", "emul", "harm_census" + ("" if kind == "plain" else "_san"))
    deps = [SRC, os.path.join(ROOT, "oracle", "dump_format.h")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror"] + BUILDS[kind] +
                              ["-I" + os.path.join(ROOT, "include"), SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def census_exe():
    return build_census("plain")


@pytest.fixture(scope="module")
def oidx():
    return OrIndex.build(list(hs.genome()))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """{set: (case file, seeds file)}"""
    hs.check()
    tmp = tmp_path_factory.mktemp("harm_sets")
    out = {}
    for pset in hs.PARAM_SETS:
        names, reads, read_lens, seed_off, seeds = hs.case_batch(pset)
        case, sf = str(tmp / (pset + ".case")), str(tmp / (pset + ".seeds"))
        write_case(case, list(hs.genome()), reads)
        hs.write_seeds_file(sf, seed_off, seeds)
        out[pset] = (case, sf)
    return out


def run_census(exe, inputs, pset, out, **more):
    """(the dump without its census lines, [{branch: count}] per read)"""
    p = subprocess.run([exe] + list(inputs[pset]) + [out] + hs.param_args(pset, srand_seed=hs.SRAND_SEED, **more), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert p.returncode == 0, (pset, more, p.stderr[-2000:])
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-2000:]
    lines = open(out).read().splitlines()
    hits = [{k: int(v) for k, v in (kv.split("=") for kv in ln.split()[1:])} for ln in lines if ln.startswith("B ")]
    return "\n".join(ln for ln in lines if not ln.startswith("B ")) + "\n", hits


@pytest.fixture(scope="module")
def census(census_exe, inputs, tmp_path_factory):
    """{set: run_census of the product's parameters}"""
    tmp = tmp_path_factory.mktemp("census")
    return {pset: run_census(census_exe, inputs, pset, str(tmp / (pset + ".pipe"))) for pset in hs.PARAM_SETS}


@pytest.fixture(scope="module")
def oracle_text(oidx):
    out = {}
    for pset in hs.PARAM_SETS:
        names, reads, read_lens, seed_off, seeds = hs.case_batch(pset)
        res = oidx.chain_seeds(read_lens, seed_off, seeds, hs.apply_params(or_params(hs.PARAM_SETS[pset][0], hs.SRAND_SEED), pset))
        out[pset] = hs.hsets_text(read_lens, res["hset_off"], res["hseed_off"], res["hset_soc"], res["hseeds"])
    return out


def per_read(text):
    """[[(strip index, [seed lines])]] per read of a dump"""
    reads = []
    for ln in text.splitlines():
        t = ln.split()
        if t[0] == "R":
            reads.append([])
        elif t[0] == "h":
            reads[-1].append((int(t[1]), []))
        elif t[0] == "g":
            reads[-1][-1][1].append(tuple(int(v) for v in t[1:]))
    return reads


def assert_same_text(got, want, names, what):
    r = -1
    for a, b in zip(got.splitlines(), want.splitlines()):
        if a.startswith("R "):
            r = int(a.split()[1])
        assert a == b, (what, names[r], a, b)
    assert got == want, (what, "lengths differ")


def test_list_contract_and_size():
    """check() holds; the sets the issue names are there; the dropped-case list is short; the goldens are a few kilobytes."""
    hs.check()
    assert {"default", "strict", "minlen", "long", "noheur", "fewsoc", "width", "artifact", "svoff"} <= set(hs.PARAM_SETS)
    assert hs.PARAM_SETS["strict"][1] == {"min_num_soc": 0, "harm_score_min_rel": 0.4} and hs.PARAM_SETS["long"][1]["min_num_soc"] == 5
    assert hs.PARAM_SETS["minlen"][1]["genome_size_disable"] == 0 and hs.PARAM_SETS["fewsoc"][1]["max_num_soc"] in (2, 3)
    qlens = [c["qlen"] for c in hs.cases_of("long")]
    assert hs.SWITCH_QLEN in qlens and min(qlens) < hs.SWITCH_QLEN < max(qlens)
    assert all(c["qlen"] <= 254 for p in hs.PARAM_SETS if p not in ("long", "longrel") for c in hs.cases_of(p))
    assert all(len(c["seeds"]) <= 60 for c in hs.all_cases())
    for pset in hs.PARAM_SETS:
        assert (pset in hs.ORACLE_ONLY) != os.path.exists(hs.golden_path(pset)), pset
        if pset not in hs.ORACLE_ONLY:
            assert os.path.getsize(hs.golden_path(pset)) < 8192, pset
    assert "Cases dropped because the compiled reference died on them (at most three may go this way): none." in hs.__doc__


def test_cases_are_what_they_are_for(census):
    """Every behaviour of the list is reached by a case that names it, every case's `expect` holds in the host form's output, no
    case does what the reference leaves undefined, and what cannot be reached is not reached."""
    covering = {hook: [] for hook in hs.BEHAVIOURS.values()}
    for pset in hs.PARAM_SETS:
        text, hits = census[pset]
        cases, sets = hs.cases_of(pset), per_read(text)
        assert len(hits) == len(sets) == len(cases), pset
        for c, h, st in zip(cases, hits, sets):
            nm, e = c["name"], c["expect"]
            assert h["err"] == 0, (nm, "overflow flags")
            for hook in hs.UNDEFINED:
                assert hook not in h, (nm, "undefined in the reference", hook)
            for hook in hs.UNREACHABLE:
                assert hook not in h, (nm, "thought unreachable", hook)
            for hook in e["hits"]:
                assert h.get(hook, 0) > 0, (nm, "does not reach", hook, h)
                covering[hook].append(nm)
            if "nsets" in e:
                assert len(st) == e["nsets"], (nm, len(st))
            if "socs" in e:
                assert [s[0] for s in st] == e["socs"], (nm, [s[0] for s in st])
            if "set_lens" in e:
                assert [[x[1] for x in s[1]] for s in st] == e["set_lens"], (nm, st)
    print()
    for what, hook in hs.BEHAVIOURS.items():
        print("%-78s %-34s %s" % (what, hook, " ".join(covering[hook])))
    empty = [what for what, hook in hs.BEHAVIOURS.items() if not covering[hook]]
    assert not empty, empty
    # seeds of length 0 inside a set, and the set that fills set_cap exactly, are in the output
    assert any(x[1] == 0 for st in per_read(census["default"][0]) for s in st for x in s[1])
    full = [c["name"] for c in hs.cases_of("fewsoc")].index("both_strands_twice_fill_set_cap_fewsoc")
    assert len(per_read(census["fewsoc"][0])[full]) == 2 * hs.PARAM_SETS["fewsoc"][1]["max_num_soc"]


@pytest.mark.parametrize("pset", [p for p in hs.PARAM_SETS if p not in hs.ORACLE_ONLY])
def test_oracle_vs_reference_golden(oracle_text, pset):
    """OrIndex.chain_seeds against the compiled reference's StripOfConsiderationSeeds::execute + Harmonization::execute on the same
    seeds (tests/golden/make_harm_sets_golden.py): the strip index and every seed field of every set, byte for byte."""
    want = gzip.open(hs.golden_path(pset), "rt").read()
    assert_same_text(oracle_text[pset], want, hs.case_batch(pset)[0], "oracle vs golden")


@pytest.mark.parametrize("pset", [p for p in hs.PARAM_SETS if p not in hs.ORACLE_ONLY])
def test_fresh_reference_dump_is_the_golden(inputs, tmp_path, pset):
    if not have_ref():
        pytest.skip("oracle/_ref not built")
    # a _ref that was not built from this tree's oracle/ref_dump.cpp (Makefile.ref rebuilds it where the reference's sources exist;
    # without them a prebuilt one stays) has no chainseeds mode: its usage line says so
    usage = subprocess.run([REF_DUMP], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    if "chainseeds" not in usage:
        pytest.skip("oracle/_ref/ref_dump was built from an earlier oracle/ref_dump.cpp: no chainseeds mode")
    out = str(tmp_path / "ref.pipe")
    subprocess.check_call([REF_DUMP, "chainseeds", inputs[pset][0], hs.PARAM_SETS[pset][0], str(hs.SRAND_SEED), inputs[pset][1], out] + hs.param_args(pset))
    assert open(out).read() == gzip.open(hs.golden_path(pset), "rt").read(), pset


@pytest.mark.parametrize("pset", list(hs.PARAM_SETS))
def test_host_form_of_chain_read_vs_oracle(census, oracle_text, pset):
    """chain.h compiled for the CPU: chain_read sweeping for itself; the census ends with a failure status if the run on strips
    swept over prefix sums (the route of long reads) or the run on a given queue (ma_batch_set_soc_heap) differs from it."""
    assert_same_text(census[pset][0], oracle_text[pset], hs.case_batch(pset)[0], "host form vs oracle")


@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5])
def test_no_case_depends_on_the_last_bit_of_libm(census_exe, inputs, census, tmp_path, mode):
    """libm_probe moves every result of tan, sin, atan and log by an ulp (chain.h: LibmProbe): the sets of every case stay."""
    for pset in hs.PARAM_SETS:
        text, _ = run_census(census_exe, inputs, pset, str(tmp_path / (pset + ".pipe")), libm_probe=mode)
        assert_same_text(text, census[pset][0], hs.case_batch(pset)[0], "libm_probe %d" % mode)


def test_draws_past_a_short_table_are_the_rings(census_exe, inputs, census, tmp_path):
    """The same sets with a table of 7 draws and with none: the generator behind the table continues the ring."""
    for n in (7, 0):
        for pset in ("default", "long"):
            text, _ = run_census(census_exe, inputs, pset, str(tmp_path / ("%s.%d.pipe" % (pset, n))), rng_tab_n=n)
            assert_same_text(text, census[pset][0], hs.case_batch(pset)[0], "rng_tab_n %d" % n)


def test_census_is_clean_under_address_and_ub_sanitizers(inputs, census, tmp_path):
    """The stand-alone program built with -fsanitize=address,undefined on every set: the same output and no report.  Every array of
    a read has exactly the size the product carves for it, so a read that left them would be reported."""
    exe = build_census("sanitized")
    for pset in hs.PARAM_SETS:
        text, hits = run_census(exe, inputs, pset, str(tmp_path / (pset + ".pipe")))
        assert text == census[pset][0] and hits == census[pset][1], pset
