"""The routing of DP jobs to kernel classes (ma_amd/csrc/ksw_launch.h: ksw_route_job, ksw_size_route) on the CPU:
tests/emul/dp_route_test.cpp, the router compiled for the host, against the routing recorded in tests/golden/dp_route.txt.gz."""
import os
import subprocess

from ma_testlib import ROOT, gunzip_to

EXE = os.path.join(ROOT, "tests", "emul", "dp_route_test")
HIPCC = "/opt/rocm/bin/hipcc"


def build_dp_route_test():
    src = EXE + ".cpp"
    csrc = os.path.join(ROOT, "ma_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        # host side only: the kernels of the headers are parsed, not compiled, and nothing of the program touches a GPU
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-ffp-contract=off", "-w", src, "-o", EXE])
    return EXE


def test_routing_matches_the_recorded_routing_and_the_device_path(tmp_path):
    """4 000 jobs x (grp 1 / 1033) x (band_long 0 / 1): class per job and KswSizing per block of 250 jobs equal the fixture, which
    was recorded from the host routing before there was one router; all 15 classes occur in the fixture; and the router reached
    the way k_dp_enum reaches it (ksw_route_slot over DpJob, reads and the packed reference) gives the same route as the byte path
    of ma_ksw_ext_batch for every job."""
    exe = build_dp_route_test()
    fixture = gunzip_to(os.path.join(ROOT, "tests", "golden", "dp_route.txt.gz"), str(tmp_path / "dp_route.txt"))
    r = subprocess.run([exe, "check", fixture], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "dp_route_test ok" in r.stdout and "16000 routes compared" in r.stdout
