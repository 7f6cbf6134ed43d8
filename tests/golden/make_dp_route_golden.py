#!/usr/bin/env python3
"""Records tests/golden/dp_route.txt.gz: the kernel class and the launch sizes that the host routing of ma_ksw_ext_batch gives a
fixed population of 4 000 DP jobs (lengths 1..9000, bands 64 / 512 / 1024, z-drop on and off, global / left / right, matching /
few-mismatch / random pairs) under MA_KSW_GRP = 1 / 1033 x MA_KSW_BANDL = 0 / 1.  tests/emul/dp_route_test.cpp generates the jobs
and writes the records; tests/test_dp_route.py holds the router to them.  The committed file was recorded from the two hand-written
copies of the routing, before ksw_route_job replaced them; run this again only when a change of the routing is intended.
Run:  python tests/golden/make_dp_route_golden.py"""
import gzip
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_dp_route import build_dp_route_test  # noqa

if __name__ == "__main__":
    exe = build_dp_route_test()
    txt = os.path.join(HERE, "dp_route.txt")
    subprocess.check_call([exe, "dump", txt])
    with open(txt, "rb") as f, gzip.GzipFile(txt + ".gz", "wb", compresslevel=9, mtime=0) as g:
        g.write(f.read())
    os.remove(txt)
