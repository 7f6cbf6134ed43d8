#!/usr/bin/env python3
"""Writes tests/golden/dp_plan.txt.gz: the launches of the DP stage (scratch regions, lanes, LDS limits, band event, and every
launch in issue order) that ksw_plan_stage plans for 132 job populations under lists / side streams / scratch budget / waves per
CU.  tests/emul/dp_plan_test.cpp makes the inputs and writes the records; tests/test_dp_plan.py holds the planning to them.  The
committed file was NOT made by this script: it was recorded from the ksw_run_all that issued its launches by hand, behind logging
stand-ins for the HIP calls (profiles/dp_launch_table.md), and this program's dump equalled it byte for byte.  Run this again only
when a change of the launch planning is intended.
Run:  python tests/golden/make_dp_plan_golden.py"""
import gzip
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_dp_plan import build_dp_plan_test  # noqa

if __name__ == "__main__":
    exe = build_dp_plan_test()
    txt = os.path.join(HERE, "dp_plan.txt")
    route = os.path.join(HERE, "dp_route.txt")
    with gzip.open(route + ".gz", "rb") as g, open(route, "wb") as f:
        f.write(g.read())
    subprocess.check_call([exe, "dump", txt, route])
    with open(txt, "rb") as f, gzip.GzipFile(txt + ".gz", "wb", compresslevel=9, mtime=0) as g:
        g.write(f.read())
    os.remove(txt)
    os.remove(route)
