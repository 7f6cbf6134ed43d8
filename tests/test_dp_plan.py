"""The launch planning of the DP stage (ma_amd/csrc/ksw_launch.h: ksw_plan_stage) on the CPU: tests/emul/dp_plan_test.cpp, the
planning function compiled for the host, against the launches recorded in tests/golden/dp_plan.txt.gz."""
import os
import subprocess

from ma_testlib import ROOT, gunzip_to

EXE = os.path.join(ROOT, "tests", "emul", "dp_plan_test")
HIPCC = "/opt/rocm/bin/hipcc"


def build_dp_plan_test():
    src = EXE + ".cpp"
    csrc = os.path.join(ROOT, "ma_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        # host side only: the kernels of the headers are parsed, not compiled, and nothing of the program touches a GPU
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-ffp-contract=off", "-w", src, "-o", EXE])
    return EXE


def test_planned_launches_match_the_recorded_launches(tmp_path):
    """132 job populations (the 64 KswSizing blocks of dp_route.txt.gz, the same with 2000 times the jobs, three hand-made long-read
    ones, one that only ksw_size_job has seen) x lists / side streams / scratch budget / waves per CU: the table ksw_plan_stage
    writes -- scratch regions, lanes used, LDS limits, the band event, and every field of every launch in issue order -- equals the
    fixture line by line.  The fixture holds the launches ksw_run_all issued before there was a table, recorded behind logging
    stand-ins for the HIP calls (profiles/dp_launch_table.md); it must reach every kernel family, both tiers, all four lanes, the band
    event on and off, the whole-budget rule firing and not firing in both layouts, an LDS limit above 48 KB, k_ksw in LDS and in
    HBM, and a launch whose waves the budget cut."""
    exe = build_dp_plan_test()
    fixture = gunzip_to(os.path.join(ROOT, "tests", "golden", "dp_plan.txt.gz"), str(tmp_path / "dp_plan.txt"))
    route = gunzip_to(os.path.join(ROOT, "tests", "golden", "dp_route.txt.gz"), str(tmp_path / "dp_route.txt"))
    r = subprocess.run([exe, "check", fixture, route], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "dp_plan_test ok" in r.stdout and "132 inputs" in r.stdout
