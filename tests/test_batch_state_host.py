"""What of a batch is valid, and what a call takes away (ma_amd/host/ma_batch_state.h) on the CPU: tests/emul/batch_state_test.cpp
includes that header alone, drives a state through a full pass and applies every row of the header's call table to it; the
complete sets of valid products after "enter", after "enter + finish" and after an early return are literals in the program.
Once as an optimised build, once under AddressSanitizer + UBSan (a stand-alone program, nothing is preloaded anywhere)."""
import os
import subprocess

import pytest

from ma_testlib import ROOT

SRC = os.path.join(ROOT, "tests", "emul", "batch_state_test.cpp")
HEADER = os.path.join(ROOT, "ma_amd", "host", "ma_batch_state.h")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=list(BUILDS))
def exe(request):
    exe = os.path.join(ROOT, "tests", "emul", "batch_state_test" + ("" if request.param == "plain" else "_san"))
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in (SRC, HEADER)):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + BUILDS[request.param] +
                              ["-I" + os.path.join(ROOT, "ma_amd", "host"), SRC, "-o", exe])
    return exe


def test_every_row_of_the_call_table(exe):
    """sixteen rows -- every form of new reads, the names, the four stages and their hand-in calls, a refused set_hsets, the
    inversions (which keep ALIGNED), the pairs (which keep the single-end text), both texts and their members --, the counts
    that go with each product, and the stage jump of the hand-in calls"""
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    assert out.splitlines()[-1] == "batch_state ok: 16 rows", out[-4000:]


def test_the_header_needs_a_host_compiler_only():
    """no HIP include, no library header: the file compiles on its own as C++17"""
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-include", HEADER, "-x", "c++", os.devnull])
    assert not [l for l in open(HEADER) if l.startswith("#include") and ("hip" in l or '"' in l)]
