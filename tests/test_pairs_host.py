"""The flat pairing (ma_amd/host/ma_pair_flat.h: the pick the device stage of ma_pair_batch runs per pair, and what the library
finishes on the host) without a GPU: against the goldens the compiled reference wrote (tests/golden/f4.*pair1*) and against
PairedReads::execute of ma_amd/host/ma_modules.h on lists full of tied candidates."""
import gzip
import os
import subprocess

import pytest

from ma_testlib import ROOT, gunzip_to

G = os.path.join(ROOT, "tests", "golden")
# (preset, search inversions, paired, Z Drop Inversions, SAM options): the paired ones of make_golden.py F4_CONFIGS
PAIRED_CONFIGS = [("default", 1, 1, 100, 0), ("illumina", 0, 1, 100, 3), ("default", 1, 1, 40, 1)]


def build(name):
    exe = os.path.join(ROOT, "tests", "emul", name)
    src = exe + ".cpp"
    deps = [src, os.path.join(ROOT, "include", "ma_amd.h"), os.path.join(ROOT, "ma_amd", "csrc", "stdsort.h"),
            os.path.join(ROOT, "ma_amd", "libma_amd.so")] + [os.path.join(ROOT, "ma_amd", "host", h)
                                                             for h in ("ma_sam.h", "ma_modules.h", "ms_graph.h", "ma_pair_flat.h", "ma_flat_sam.h",
                                                                       "ma_sam_dev.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "ma_amd", "host"), src, "-o", exe, "-L" + os.path.join(ROOT, "ma_amd"),
                               "-lma_amd", "-Wl,-rpath," + os.path.join(ROOT, "ma_amd"), "-lpthread"])
    return exe


@pytest.mark.parametrize("cfg", PAIRED_CONFIGS)
def test_flat_pick_matches_reference_goldens(tmp_path, cfg):
    """The reference's own per-mate lists (FIN / f records, inversion records included) through pickFlat: the PAIR / p
    records -- which records, in which order, flags, mapq to the last digit, mate and partner columns -- are the reference's."""
    nm = "f4.%s.inv%d.pair%d.zd%d.opt%d" % cfg
    exe = build("pair_flat_test")
    case = gunzip_to(os.path.join(G, "f4.case.gz"), str(tmp_path / "f4.case"))
    dump = gunzip_to(os.path.join(G, nm + ".f4.gz"), str(tmp_path / "ref.f4"))
    subprocess.check_call([exe, "golden", case, dump, cfg[0], str(tmp_path / "o.f4"), str(cfg[4]), str(tmp_path / "o.sam")])
    got = open(str(tmp_path / "o.f4")).read().split("\n")
    want = gzip.open(os.path.join(G, nm + ".f4.gz"), "rt").read().split("\n")
    assert sum(l.startswith("p ") for l in want) > 100
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "%s line %d differs" % (nm, i)
    assert len(got) == len(want)


@pytest.mark.parametrize("cfg", PAIRED_CONFIGS)
def test_flat_paired_sam_matches_reference_goldens(tmp_path, cfg):
    """The same picks through the flat pair formatter (ma_flat_sam.h formatPair) under the SAM options of the golden (0,
    1: soft clipping, 3: soft clipping and =/X cigars): the bytes of the reference's PairedFileWriter, all three record
    shapes (aligned mate, pair without any alignment, one mate unaligned)."""
    nm = "f4.%s.inv%d.pair%d.zd%d.opt%d" % cfg
    exe = build("pair_flat_test")
    case = gunzip_to(os.path.join(G, "f4.case.gz"), str(tmp_path / "f4.case"))
    dump = gunzip_to(os.path.join(G, nm + ".f4.gz"), str(tmp_path / "ref.f4"))
    subprocess.check_call([exe, "golden", case, dump, cfg[0], str(tmp_path / "o.f4"), str(cfg[4]), str(tmp_path / "o.sam")])
    got = open(str(tmp_path / "o.sam"), "rb").read()
    want = gzip.open(os.path.join(G, nm + ".sam.gz"), "rb").read()
    flags = [int(l.split(b"\t")[1]) for l in want.split(b"\n") if l and not l.startswith(b"@")]
    assert any(f & 4 and f & 8 for f in flags) and any(f & 4 and not f & 8 for f in flags) and any(f & 0x20 for f in flags)
    assert got == want, [(i, a, b) for i, (a, b) in enumerate(zip(got.split(b"\n"), want.split(b"\n"))) if a != b][:2]


def test_tied_candidates_match_the_container_path():
    """2, 5, 16, 17, 33, 40 and 100 candidates of one key (16 / 17 straddle the insertion-sort threshold of libstdc++'s
    std::sort), all improper, all proper, mixed, with a runner-up; 3000 random lists of few distinct scores: pickFlat and
    PairedReads::execute pick the same records with the same mapq bits, and the kernel's sort of up to 32 candidates
    (ss::sort_upto32) leaves the permutation of std::sort."""
    exe = build("pair_flat_test")
    r = subprocess.run([exe, "ties"], stdout=subprocess.PIPE, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
