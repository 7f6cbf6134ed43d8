"""The text mode of the maxSpan runs (ma_amd/csrc/seeding.h, template flag TXT) on the CPU: tests/emul/seed_text_test.cpp runs
seed_read_serial with the mode off and on -- the compare base by base and word-wise, as the kernel does it -- on the genome and
reads of seed_text_cases.py."""
import os
import re
import subprocess

import pytest

from ma_testlib import ROOT, build_oracle, write_case
import seed_text_cases

PROG = os.path.join(ROOT, "tests", "emul", "seed_text_test")


@pytest.fixture(scope="module")
def prog():
    build_oracle()
    src = PROG + ".cpp"
    deps = [src] + [os.path.join(ROOT, "ma_amd", "csrc", f) for f in ("seeding.h", "fm_device.h", "ma_common.h")]
    if not os.path.exists(PROG) or any(os.path.getmtime(d) > os.path.getmtime(PROG) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-w", "-I" + os.path.join(ROOT, "include"), src, "-o", PROG,
                               "-L" + os.path.join(ROOT, "oracle"), "-lma_oracle", "-Wl,-rpath," + os.path.join(ROOT, "oracle")])
    return PROG


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    g = seed_text_cases.genome()
    path = str(tmp_path_factory.mktemp("seed_text") / "case.bin")
    write_case(path, g, seed_text_cases.reads(g))
    return path


@pytest.mark.parametrize("min_amb", [0, 2])
def test_text_mode_gives_the_same_segments_with_fewer_fm_steps(prog, case, min_amb):
    """Order, extents, sa_start, sa_start_rc and sa_size of every segment are the same once the segments that carry a position
    have their rows back, and the position they carried is the row's.  uiMinAmbiguity == 0: strictly fewer extend_backward
    calls; 2: a run stops on an interval of size 1, the mode is never entered, the counts are equal."""
    out = subprocess.check_output([prog, case, str(min_amb)]).decode()
    print(out)
    m = re.search(r"steps off (\d+) on (\d+) blocks off (\d+) on (\d+) marked (\d+) segments (\d+)", out)
    off, on, _, _, marked, nseg = (int(x) for x in m.groups())
    assert nseg > 2000
    if min_amb == 0:
        assert on < off
        assert marked > 1000
    else:
        assert on == off and marked == 0


def test_extend_backward_of_one_row_is_a_text_comparison(prog, case):
    """10^5 random rows plus `primary`, row 0 and the rows of the suffixes at 0, F - 1, F and n - 1: extend_backward of the
    size-1 interval by each base has size 1 iff the base stands in front of the suffix in the doubled text."""
    out = subprocess.check_output([prog, case, "prop"]).decode()
    print(out)
    assert "prop ok" in out
