"""The short-read chain stage's host-checkable parts (ma_amd/csrc/chain.h) on the CPU: tests/emul/chain_split_test.cpp includes
chain.h alone and checks
  - chain_read_one, the answer k_chain_split gives a read of at most one seed, against chain_read itself -- nsets, the HSet
    records and the seed bytes, also those chain_read writes and then takes back -- for every combination of strand, seed
    length 1 / 11 / 150, harm_score_min 0 / 18, harm_score_min_rel 0 / 0.5, genome size below / above genome_size_disable,
    min_num_soc 0 / 1, max_num_soc 0 / 1 / 10, heuristics on / off (and switch_qlen, score_diff_tol, the read's length and a
    sink with and without the read's private region on top of those);
  - chain_scratch_carve, the one scratch block per read, for reads of 0, 1, 2, 3, 17 and 1000 seeds: every array aligned for its
    type, inside its read's block, no two arrays and no two reads overlapping, every array written in full;
  - GlibcRand as a counter into a table of K draws, K = 4 (and 1 and 256), against the ring-only generator and libc's rand( ) for
    10 000 draws per srand seed.
Once as an optimised build, once under AddressSanitizer + UBSan (a stand-alone program, nothing is preloaded anywhere)."""
import os
import subprocess

import pytest

from ma_testlib import ROOT

SRC = os.path.join(ROOT, "tests", "emul", "chain_split_test.cpp")
CSRC = os.path.join(ROOT, "ma_amd", "csrc")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(BUILDS))
def exe(request):
    exe = os.path.join(ROOT, "tests", "emul", "chain_split_test" + ("" if request.param == "plain" else "_san"))
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror"] + BUILDS[request.param] +
                              ["-I" + os.path.join(ROOT, "include"), SRC, "-o", exe])
    return exe


def test_one_seed_answers_carving_and_draw_table(exe):
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    last = out.splitlines()[-1]
    assert last.startswith("chain_split ok: "), out[-4000:]
    cases, arrays, draws = (int(w) for w in last.split() if w.isdigit())
    # 2 seed counts x 2 strands x (3 seed lengths in the 150-base read + 2 in the 12-base read) x 2^5 x 3 max_num_soc x
    # 3 switch_qlen x 2 tolerances x 2 sinks; 9 reads x 13 arrays; 4 srand seeds x 3 table sizes x 10 000 draws
    assert cases == 2 * 2 * (3 + 2) * 32 * 3 * 3 * 2 * 2 and arrays == 9 * 13 and draws == 120000
