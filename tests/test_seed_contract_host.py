"""The contract of ma_batch_set_seeds and ma_batch_set_soc_heap (include/ma_amd.h; ma_amd/host/ma_seed_contract.h has the checks) on
the CPU: tests/emul/seed_contract_test.cpp includes that header alone and goes through the contract clause by clause -- every
violation with the message the library gives, and the seeds of the reference's own extraction that must not be refused.  Once as
an optimised build, once under AddressSanitizer + UBSan (a stand-alone program, nothing is preloaded anywhere).  The hand-made
seeds of harm_sets.py and chain_lists.py keep the contract as the header states it."""
import os
import subprocess

import numpy as np
import pytest

from ma_testlib import ROOT

SRC = os.path.join(ROOT, "tests", "emul", "seed_contract_test.cpp")
HEADER = os.path.join(ROOT, "ma_amd", "host", "ma_seed_contract.h")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(BUILDS))
def exe(request):
    exe = os.path.join(ROOT, "tests", "emul", "seed_contract_test" + ("" if request.param == "plain" else "_san"))
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in (SRC, HEADER)):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + BUILDS[request.param] +
                              ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ma_amd", "host"), SRC, "-o", exe])
    return exe


def test_every_clause_of_the_contract(exe):
    """offsets, negative fields, len >= 1, the read's length, on_forward, r_start inside the forward text, the doubled text's end
    for both strands, delta; the strips' ranges and counts; and what the contract takes: seeds across a contig border and across
    the strand junction, mirrored seeds at both ends, duplicates, empty strips"""
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    assert out.splitlines()[-1] == "seed_contract ok: 25 refusals, 12 accepted", out[-4000:]


def test_the_header_needs_a_host_compiler_only():
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-include", HEADER,
                           "-x", "c++", os.devnull])
    assert not [ln for ln in open(HEADER) if ln.startswith("#include") and "hip" in ln]


def test_the_sort_lists_keep_the_contract():
    """chain_lists.py hands its seeds to ma_batch_set_seeds as well: forward seeds on the second contig with ExtractSeeds' delta."""
    import chain_lists as cl
    import harm_sets as hs
    starts = np.concatenate([[0], np.cumsum(cl.CONTIG_LENS)[:-1]])
    F = int(sum(cl.CONTIG_LENS))
    for fl in ("delta", "refpos"):
        for n in (17, 129):
            qlen, s = cl.seeds_of_list(cl.pattern_keys("sawtooth", n), fl, starts, 0)
            assert np.all(s["len"] >= 1) and np.all(s["q_start"] + s["len"] <= qlen) and np.all(s["r_start"] + s["len"] <= F)
            contig = np.searchsorted(starts, s["r_start"], side="right") - 1
            assert np.array_equal(s["delta"], s["r_start"] + (qlen - s["q_start"]) + (qlen + 1) * contig), fl
    hs.check()
