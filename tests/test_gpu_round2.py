"""Round-2 GPU parity tests (VERDICT r1 "Next round" items 1b, 8, 10 and ADVICE r1): the 50 kb / 10 % error shape of
BASELINE config 5 against the compiled reference, the index builder at the scale where the reference switches to
BWA's bwtLarge construction, the device libm against glibc over the arguments the chaining stage can reach, the C ABI
called from fresh host threads, pool re-growth and argument validation."""
import ctypes as C
import hashlib
import json
import math
import os
import subprocess
import threading

import numpy as np
import pytest

from ma_testlib import ROOT, gunzip_to, high_error_50kb_case, parse_pipe_dump, rand_genome, read_case, sample_reads, write_case
from test_gpu_parity import compare_reads, gpu_pipeline

pytestmark = pytest.mark.gpu
G = os.path.join(ROOT, "tests", "golden")


def test_50kb_high_error_reads_vs_compiled_reference(gpu_device):
    """BASELINE config 5's shape (50 kb reads, 3 / 3 / 4 % substitutions / insertions / deletions): every stage record
    of the GPU path equals the reference's own modules (oracle/Makefile.ref; their output on these reads is
    tests/golden/gpu_c50k.default.pipe.gz, make_golden.py), Default preset."""
    import ma_amd
    g, reads = high_error_50kb_case()
    want = parse_pipe_dump(os.path.join(G, "gpu_c50k.default.pipe.gz"))
    assert len(want) == len(reads) and all(w["len"] == len(r) for w, r in zip(want, reads))
    idx = ma_amd.Index.build(g)
    got, counters, counts = gpu_pipeline(idx, "default", 3, reads)
    compare_reads(got, want)
    assert counts["aligned_reads"] == sum(1 for w in want if w["mq"])
    idx.close()


def test_index_build_at_bwtlarge_scale_matches_reference_hashes(gpu_device, tmp_path):
    """30 Mnt forward = 60 Mnt doubled text: above the 50 Mnt switch of FMIndex::build_FMIndex (fMIndex.cpp:316-338) the
    reference builds its BWT with BWA's bwtLarge code.  tests/golden/large_index.sha256.json holds SHA-256 of the files
    the reference wrote for this genome (make_large_index_hashes.py); the GPU builder must produce the same bytes."""
    import torch
    import ma_amd
    want = json.load(open(os.path.join(G, "large_index.sha256.json")))
    L = ma_amd.lib()
    lens = np.array(want["contigs"], dtype=np.uint64)
    F = int(lens.sum())
    g = torch.empty(F, dtype=torch.uint8, device="cuda")
    assert L.ma_synth_genome_device(C.c_uint64(want["seed"]), C.c_uint64(F), C.c_int32(want["with_repeats"]),
                                    C.c_void_p(g.data_ptr())) == 0
    # the numpy restatement of the generator that fed the reference produced the same genome
    assert hashlib.sha256(g.cpu().numpy().tobytes()).hexdigest() == want["genome_sha256"]
    idx = ma_amd.Index.build_device(lens, g.data_ptr())
    prefix = str(tmp_path / "large")
    idx.store(prefix)
    for ext in ("bwt", "sa", "pac"):
        data = open(prefix + "." + ext, "rb").read()
        assert len(data) == want[ext]["bytes"], ext
        assert hashlib.sha256(data).hexdigest() == want[ext]["sha256"], ext
    idx.close()


def _glibc(op, x):
    return (math.tan, math.sin, math.atan, math.log)[op](x)


def _device_libm(op, x):
    import ma_amd
    L = ma_amd.lib()
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    assert L.ma_debug_libm(C.c_int(op), x.ctypes.data_as(C.c_void_p), C.c_uint64(len(x)),
                           out.ctypes.data_as(C.c_void_p)) == 0, L.ma_last_error()
    return out


def test_device_libm_is_within_one_ulp_of_glibc(gpu_device):
    """The chaining stage decides with tan / sin / atan / log (harmonization.h:82-89, ransac.cpp:112,131-135): the
    reference evaluates them with glibc, the device with ocml.  They are NOT bit-identical (about 1 in 8 atan results
    differs in the last bit), which is why the decisions are pinned separately below; here the distance is bounded:
    over the arguments the call sites can see no device result is further than one ulp from glibc's (CPython's math
    module is the glibc of this image)."""
    rng = np.random.default_rng(77)
    PI_TRUNC = 3.14159265

    def check(op, x, what):
        got = _device_libm(op, x)
        want = np.array([_glibc(op, float(v)) for v in x], dtype=np.float64)
        d = np.abs(got.view(np.int64) - want.view(np.int64))
        assert d.max() <= 1, "%s: device is %d ulp from glibc at %r" % (what, d.max(), x[int(d.argmax())])
        return float((d != 0).mean())

    rates = {}
    dv = rng.integers(1, 400000, 100000) * 0.5
    dh = rng.integers(1, 400000, 100000) * 0.5
    rates["atan(dV/dH)"] = check(2, dv / dh, "atan(dV/dH)")
    slope = np.tan(np.deg2rad(rng.uniform(15.0, 75.0, 100000)))
    rates["atan(slope)"] = check(2, slope, "atan(slope)")
    ang = np.array([math.atan(float(s)) for s in slope])
    rates["sin(a)"] = check(1, ang, "sin(fAngle)")
    rates["sin(pi/2-a)"] = check(1, PI_TRUNC / 2 - ang, "sin(pi/2 - fAngle)")
    rates["tan(pi/2-a)"] = check(0, PI_TRUNC / 2 - ang, "tan(pi/2 - fAngle)")
    w = rng.integers(1, 3000, 50000) / 3000.0
    p = np.clip(1 - w * w, 2.220446049250313e-16, 1 - 2.220446049250313e-16)
    rates["log(pNo)"] = check(3, p, "log(pNo)")
    print("fraction of arguments whose device result differs from glibc in the last bit:", rates)


def test_ransac_decisions_do_not_depend_on_the_last_bits_of_libm(gpu_device):
    """Two of the libm call sites feed DISCRETE decisions whose worst cases can be enumerated (ransac.cpp:112,131-135):
    (a) a sampled model is accepted iff 20 <= atan(dV / dH) * 180 / pi <= 70, dV and dH differences of half-integer
        coordinates: the rationals closest to tan(20 deg) and tan(70 deg) with numerator / denominator up to 2^20 half-units
        (reads of 500 kb) -- the convergents and semiconvergents of the two thresholds' continued fractions -- are decided
        by the device exactly like exact arithmetic decides them, and their margin is > 10^2 ulp;
    (b) the adaptive iteration count k = log(1 - 0.99) / log(1 - (nIn / nPts)^2) is only compared with integers
        (`while iterations < k`, at most 100): over all 1 <= nIn <= nPts <= 3 x 6000 points, k < 101 is never closer
        than 10^-12 (relative) to an integer (the closest case is 5 x 10^-11), thousands of times the libm's error."""
    from fractions import Fraction
    from decimal import Decimal, getcontext
    getcontext().prec = 60

    def tan_deg(d):  # tan of d degrees to 60 digits (Taylor series of sin and cos)
        x = Decimal(d) * Decimal("3.14159265358979323846264338327950288419716939937510582097494") / 180
        s, c, t = Decimal(0), Decimal(0), Decimal(1)
        for n in range(60):
            if n % 2 == 0:
                c += t if n % 4 == 0 else -t
            else:
                s += t if n % 4 == 1 else -t
            t = t * x / (n + 1)
        return s / c

    cases = []
    LIM = 1 << 20
    for deg in (20, 70):
        T = tan_deg(deg)
        # continued fraction of T; convergents and semiconvergents with denominator / numerator <= LIM
        h0, h1, k0, k1 = 0, 1, 1, 0
        x = T
        for _ in range(40):
            a = int(x)
            for m in range(1, a + 1):  # semiconvergents ... the convergent itself at m == a
                p, q = h0 + m * h1, k0 + m * k1
                if 0 < q <= LIM and 0 < p <= LIM:
                    cases.append((deg, p, q, Decimal(p) / Decimal(q) >= T))
            h0, h1, k0, k1 = h1, h0 + a * h1, k1, k0 + a * k1
            if k1 > LIM or h1 > LIM:
                break
            fr = x - a
            if fr == 0:
                break
            x = 1 / fr
    assert len(cases) > 40
    q = np.array([(p * 0.5) / (d * 0.5) for _, p, d, _ in cases])
    ang = _device_libm(2, q) * 180 / 3.141592653589793
    for (deg, p, d, above), a in zip(cases, ang):
        got = (a >= 20) if deg == 20 else (a > 70)  # "inside at the lower bound" / "outside at the upper bound"
        assert got == above, "atan(%d/%d) is decided differently from exact arithmetic at %d degrees" % (p, d, deg)
        assert abs(a - deg) > 100 * np.spacing(float(deg)), "margin at %d/%d" % (p, d)
    # (b) in double arithmetic with numpy (error ~1e-15 relative), chunked over nPts
    worst = 1.0
    for npts in range(2, 18001):
        nin = np.arange(1, npts + 1, dtype=np.float64)
        w = nin / npts
        p = np.clip(1 - w * w, 2.220446049250313e-16, 1 - 2.220446049250313e-16)
        k = math.log(1 - 0.99) / np.log(p)
        k = k[(k < 101.5) & (k > 0.5)]
        if len(k):
            worst = min(worst, float(np.min(np.abs(k - np.rint(k)) / k)))
    assert worst > 1e-12, worst


@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5])
def test_pipeline_is_insensitive_to_one_ulp_of_libm(gpu_device, tmp_path, mode):
    """The continuous libm call sites (the guide line's angle and delta distances, harmonization.h:82-89) cannot be
    enumerated.  ma_params.libm_probe nudges EVERY tan / sin / atan / log result of the chaining stage by one ulp (the
    measured distance between ocml and glibc): up, down, or up / same / down by call (three different patterns).  Over a
    corpus with repeats, nested SMEM seeds, N bases and long high-error reads the results must stay bit-identical."""
    import ma_amd
    g = rand_genome(29, [2800000, 1500000, 900000], repeat_unit=300, repeat_copies=400, repeat_div=0.06)
    reads = (sample_reads(g, 6000, 150, 151, sub=0.01) + sample_reads(g, 1500, 150, 152, sub=0.05, ins=0.01, dele=0.01)
             + sample_reads(g, 1500, 250, 153, sub=0.02, ins=0.005, dele=0.005) + sample_reads(g, 40, 8000, 154, sub=0.01, ins=0.01, dele=0.01)
             + sample_reads(g, 6, 40000, 155, sub=0.03, ins=0.03, dele=0.04))
    idx = ma_amd.Index.build(g)
    for preset in ("default", "illumina"):
        out = []
        for m in (0, mode):
            P = ma_amd.Params.preset(preset)
            P.srand_seed = 3
            P.libm_probe = m
            b = ma_amd.Batch(idx, P, len(reads), sum(len(r) for r in reads) + 64)
            b.set_reads(reads)
            b.align()
            b.sync()
            hs = b.hsets()
            al = b.mapq_alignments()
            out.append([np.asarray(x).tobytes() for x in hs] + [np.asarray(x).tobytes() for x in al])
            b.close()
        assert out[0] == out[1], "preset %s: results change when libm results move by one ulp (mode %d)" % (preset, mode)
    idx.close()


def test_c_abi_from_fresh_host_threads(gpu_device, tmp_path):
    """HIP's current device is per host thread: every entry point binds the calling thread to the device its index / batch
    lives on.  Batches created, run and read back from freshly spawned threads give the golden result."""
    import ma_amd
    case = gunzip_to(os.path.join(G, "small.case.gz"), str(tmp_path / "small.case"))
    contigs, reads, _ = read_case(case)
    idx = ma_amd.Index.build(contigs)
    want = parse_pipe_dump(os.path.join(G, "small_ref.default.pipe.gz"))
    results, errors = {}, []

    def worker(k):
        try:
            results[k] = gpu_pipeline(idx, "default", 1, reads)[0]
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(k,)) for k in range(3)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for k in range(3):
        compare_reads(results[k], want)
    out = {}

    def closer():
        out["sizes"] = idx.sizes()
        idx.close()

    t = threading.Thread(target=closer)
    t.start()
    t.join()
    assert out["sizes"][2] == 2 * sum(len(c) for c in contigs)


@pytest.mark.parametrize("env", [{"MA_SEG_POOL_CAP": "64"}, {"MA_CIG_POOL_CAP": "16"},
                                 {"MA_SEG_POOL_CAP": "1", "MA_CIG_POOL_CAP": "1", "MA_SEED_STAGE_CAP": "3"}])
def test_pool_overflow_is_regrown_and_rerun(gpu_device, tmp_path, monkeypatch, env):
    """Segment and cigar pool sizes are heuristics: a batch that needs more re-runs the stage with the counted need
    instead of failing.  The test hooks force a far too small first attempt."""
    import ma_amd
    case = gunzip_to(os.path.join(G, "small.case.gz"), str(tmp_path / "small.case"))
    contigs, reads, _ = read_case(case)
    idx = ma_amd.Index.build(contigs)
    want = parse_pipe_dump(os.path.join(G, "small_ref.default.pipe.gz"))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, _, _ = gpu_pipeline(idx, "default", 1, reads)
    compare_reads(got, want)
    idx.close()


def test_unknown_seeding_technique_is_rejected(gpu_device, tmp_path):
    import ma_amd
    case = gunzip_to(os.path.join(G, "small.case.gz"), str(tmp_path / "small.case"))
    contigs, reads, _ = read_case(case)
    idx = ma_amd.Index.build(contigs)
    P = ma_amd.Params.preset("default")
    P.seeding_technique = 7
    with pytest.raises(ma_amd.MaError, match="unknown seeding technique 7"):
        ma_amd.Batch(idx, P, 4, 1000)
    idx.close()


def _bench(args, nproc=1, env=None, self_launch=False):
    """Runs bench.py --full and returns its line with the per-workload blocks of the detail file put back under config.workloads.
    nproc > 1: under an outer torchrun as the driver starts it -- or, self_launch, by bench.py's own --gpus N."""
    import sys
    import tempfile
    e = dict(os.environ, **(env or {}))
    base = [sys.executable]
    if nproc > 1 and not self_launch:
        base += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
                 "--master-port", "29617"]
        e.pop("WORLD_SIZE", None)
    with tempfile.TemporaryDirectory() as td:
        detail = os.path.join(td, "detail.json")
        out = subprocess.check_output(base + [os.path.join(ROOT, "bench.py"), "--full"] + args + ["--detail-file", detail], env=e,
                                      stderr=subprocess.DEVNULL).decode()
        line = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
        with open(detail) as f:
            d = json.load(f)
    line["config"]["workloads"] = d["workloads"]
    line["config"]["boundary"] = d["boundary"]
    line["c1_anchor_detail"] = d["c1_anchor"]
    return line


def test_bench_two_ranks_partition_one_read_set(gpu_device):
    """The multi-rank flow of bench.py with the real engine (both ranks on GPU 0 over gloo: MA_BENCH_ONE_DEVICE, the
    driver's runs use one GPU per rank over RCCL): weak scaling = every rank its own reads; strong scaling = ONE read set
    cut into contiguous blocks, so two ranks must align exactly the reads (and find exactly the alignments) of one."""
    common = ["--workload", "150bp", "--genome-scale", "0.01", "--steps", "2", "--warmup", "1", "--reads-per-step", "30000",
              "--cpu-sample", "0", "--boundary-reads", "0"]
    one = _bench(common + ["--gpus", "1"])
    weak = _bench(common + ["--gpus", "2"], nproc=2, env={"MA_BENCH_ONE_DEVICE": "1"})
    strong = _bench(common + ["--gpus", "2", "--scaling", "strong"], nproc=2, env={"MA_BENCH_ONE_DEVICE": "1"})
    w1, ww, ws = one["config"]["workloads"][0], weak["config"]["workloads"][0], strong["config"]["workloads"][0]
    assert weak["n_gpus"] == 2 and strong["n_gpus"] == 2 and weak["scaling"] == "weak" and strong["scaling"] == "strong"
    assert w1["aligned_reads"] > 0.95 * 60000
    # strong: the same 60 000 reads as the single process, so the same number of aligned reads
    assert ws["aligned_reads"] == w1["aligned_reads"]
    # weak: rank 0 repeats the single process' reads, rank 1 adds as many others
    assert 1.9 * w1["aligned_reads"] < ww["aligned_reads"] < 2.1 * w1["aligned_reads"]
    # every leg of the line: one batch at a time, batches in flight, host to host (reads from / results into page-locked host
    # memory) -- the same reads, so the same number of aligned reads per step
    for key in ("overlapped", "host_to_host"):
        assert abs(w1[key]["aligned_reads"] / w1[key]["steps"] - w1["aligned_reads"] / w1["steps"]) < 0.01 * 30000, key
        assert ww[key]["value"] > 0
    assert w1["host_to_host"]["aligned_reads"] == w1["overlapped"]["aligned_reads"]  # the same reads through both I/O paths
    assert one["value"] == w1["host_to_host"]["value"] and "host to host" in one["config"]["value_is"]
    assert one["value_150bp_device_resident"] == w1["overlapped"]["value"] and one["value_150bp_single_stream"] == w1["value"]


def test_bench_plain_run_is_the_headline_leg_of_a_full_run(gpu_device, tmp_path):
    """Without --full the bench times the leg `value` comes from and nothing else: the same reads aligned as that leg of a --full
    run; --dump-outputs writes the files of the --full run, every leg's, byte for byte."""
    import sys
    common = ["--workload", "150bp", "--genome-scale", "0.01", "--steps", "3", "--warmup", "1", "--reads-per-step", "30000",
              "--cpu-sample", "0", "--boundary-reads", "0", "--gpus", "1"]
    full = _bench(common + ["--dump-outputs", str(tmp_path / "full")])
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py")] + common + ["--dump-outputs", str(tmp_path / "plain")],
                                  stderr=subprocess.DEVNULL).decode()
    plain = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    h2h = full["config"]["workloads"][0]["host_to_host"]
    assert plain["steps"] == full["steps"] == 3 and plain["warmup"] == full["warmup"] == 1 and plain["n_gpus"] == 1
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert plain[k] == full[k], k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["config"]["value_is"].startswith("workload '150bp' (configs[1] (C2)), 3 batch(es) in flight per GPU, host to host")
    assert abs(plain["value"] * plain["ms_per_step"] * plain["steps"] / 1e3 - h2h["aligned_reads"]) < 2e-3 * h2h["aligned_reads"]
    assert "roofline" not in plain and "cpu_baseline" not in plain and "parity_150bp_h2h" not in plain
    names = sorted(os.listdir(tmp_path / "plain"))
    assert len(names) == 3 * 13 and names == sorted(os.listdir(tmp_path / "full"))
    for f in names:
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "full" / f).read_bytes(), f


def test_bench_gpus_flag_starts_the_ranks_itself(gpu_device):
    """`bench.py --gpus 2` WITHOUT an outer torchrun starts its two ranks itself (here both on GPU 0 over
    gloo) and reports n_gpus = 2; with a torchrun environment of another size it refuses instead of printing a 1-rank number."""
    common = ["--workload", "150bp", "--genome-scale", "0.01", "--steps", "2", "--warmup", "1", "--reads-per-step", "20000",
              "--cpu-sample", "0", "--boundary-reads", "0", "--overlap", "0"]
    two = _bench(common + ["--gpus", "2"], nproc=2, env={"MA_BENCH_ONE_DEVICE": "1"}, self_launch=True)
    assert two["n_gpus"] == 2
    assert two["config"]["workloads"][0]["aligned_reads"] > 0.95 * 2 * 40000
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common + ["--gpus", "4"],
                       env=dict(os.environ, WORLD_SIZE="1", RANK="0"), capture_output=True, text=True)
    assert r.returncode != 0 and "refusing" in r.stderr


def band_cut_extension_cases(n, seed):
    """Extension jobs whose band cuts the DP rectangle (qlen > w + 1), shaped like the end extensions of long reads: the
    query is a noisy copy of the (shorter) target followed by sequence that is not in the target, so the maximum sits at
    the last target column and the rest of the band can only be left by the early stop or by running out of band."""
    from ma_testlib import KSW_EXTZ, KSW_REV, KSW_RIGHT
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(n):
        w = int(rng.choice([64, 128, 300, 512]))
        tl = int(rng.integers(40, 1300))
        ql = int(rng.integers(w + 2, w + 2 + 2500))
        t = rng.integers(0, 4, size=tl, dtype=np.uint8)
        kind = rng.random()
        if kind < 0.15:  # tandem repeat target: late maxima are plausible
            unit = rng.integers(0, 4, size=int(rng.integers(1, 7)), dtype=np.uint8)
            t = np.tile(unit, tl // len(unit) + 1)[:tl].copy()
        if kind < 0.8:
            body = t.copy()
            er = rng.choice([0.0, 0.01, 0.05, 0.15])
            mut = rng.random(len(body)) < er
            body[mut] = (body[mut] + rng.integers(1, 4, size=int(mut.sum()), dtype=np.uint8)) % 4
            for _ in range(int(rng.integers(0, 4))):  # a few indels
                if len(body) > 20:
                    p = int(rng.integers(5, len(body) - 5))
                    if rng.random() < 0.5:
                        body = np.concatenate([body[:p], body[p + int(rng.integers(1, 30)):]])
                    else:
                        body = np.concatenate([body[:p], rng.integers(0, 4, size=int(rng.integers(1, 30)), dtype=np.uint8), body[p:]])
            q = np.concatenate([body, rng.integers(0, 4, size=max(0, ql - len(body)), dtype=np.uint8)])[:ql]
            if len(q) < ql:
                q = np.concatenate([q, rng.integers(0, 4, size=ql - len(q), dtype=np.uint8)])
        else:  # unrelated
            q = rng.integers(0, 4, size=ql, dtype=np.uint8)
        if rng.random() < 0.1:
            q[int(rng.integers(0, ql))] = 4
        flag = KSW_EXTZ if k % 2 == 0 else (KSW_EXTZ | KSW_RIGHT | KSW_REV)
        cases.append((np.ascontiguousarray(q, dtype=np.uint8), t, w, int(rng.choice([200, 200, 50, -1])), flag))
    return cases


@pytest.mark.parametrize("scoring", [None, (3, 5, 6, 3, 30, 2), (1, 3, 5, 2, 24, 1), (2, 4, 24, 1, 4, 2)])
def test_band_cut_extensions_stop_early_with_the_same_result(gpu_device, scoring):
    """The early stop of ksw_pk for bands that cut the rectangle (ksw_reg.h, second part of the proof): pipeline semantics
    against the exact kernel (which computes every diagonal) on max / max_q / max_t and the cigar, and against the
    oracle's kswcpp for a sample."""
    import ma_amd
    from ma_testlib import or_ksw, or_params
    P = ma_amd.Params.preset("default")
    op = or_params()
    if scoring is not None:
        for prm in (P, op):
            prm.match, prm.mismatch, prm.gap, prm.extend, prm.gap2, prm.extend2 = scoring
    cases = band_cut_extension_cases(240, 7 if scoring is None else 70 + scoring[0])
    ez, cigs = ma_amd.ksw_batch(P, cases)
    ez2, cigs2 = ma_amd.ksw_batch(P, cases, pipeline_semantics=True)
    for i, (q, t, w, zd, fl) in enumerate(cases):
        for f in ("max", "max_q", "max_t"):
            assert int(ez2[f][i]) == int(ez[f][i]), "case %d field %s: %d vs %d (qlen %d tlen %d w %d zdrop %d flag %d)" % (
                i, f, int(ez2[f][i]), int(ez[f][i]), len(q), len(t), w, zd, fl)
        assert np.array_equal(cigs2[i], cigs[i]), "case %d cigar (qlen %d tlen %d w %d zdrop %d flag %d)" % (i, len(q), len(t), w, zd, fl)
    for i in range(0, len(cases), 8):
        q, t, w, zd, fl = cases[i]
        oez, ocig = or_ksw(op, q, t, w, zd, fl)
        for f in oez.dtype.names:
            assert int(ez[f][i]) == int(oez[f]), "exact kernel vs oracle: case %d field %s" % (i, f)
        assert np.array_equal(cigs[i], ocig)


@pytest.mark.parametrize("scoring,pacbio", [((3, 5, 6, 3, 30, 2), False), ((1, 3, 5, 2, 24, 1), True), (None, True)])
def test_long_reads_other_scoring_and_pacbio_settings_vs_oracle(gpu_device, scoring, pacbio):
    """Long reads (end extensions whose band cuts the rectangle -> sparse early stop; dual extensions between seeds;
    thin-wave chaining) under non-default scoring and under the PacBio / Nanopore preset's settings (SMEM seeding, at least
    5 strips, up to 100 supplementary alignments, parameter.h:1096-1104), on a 3.4 Mnt genome with repeats: every
    NeedlemanWunsch alignment and every MappingQuality record against the oracle (which computes every diagonal)."""
    import ma_amd
    from ma_testlib import OrIndex, or_params
    g = rand_genome(19, [1700000, 1100000, 600000], repeat_unit=300, repeat_copies=150, repeat_div=0.08)
    reads = (sample_reads(g, 150, 150, 41, sub=0.01) + sample_reads(g, 10, 6000, 42, sub=0.005, ins=0.003, dele=0.003)
             + sample_reads(g, 3, 25000, 43, sub=0.03, ins=0.03, dele=0.04) + sample_reads(g, 2, 12000, 44, sub=0.01, ins=0.01, dele=0.01))
    gidx = ma_amd.Index.build(g)
    oidx = OrIndex.from_parts(gidx.download())
    P = ma_amd.Params.preset("default")
    op = or_params("default", 1)
    for prm in (P, op):
        if scoring is not None:
            prm.match, prm.mismatch, prm.gap, prm.extend, prm.gap2, prm.extend2 = scoring
        if pacbio:
            prm.max_supplementary, prm.min_num_soc, prm.seeding_technique = 100, 5, 1
        prm.srand_seed = 1
    b = ma_amd.Batch(gidx, P, len(reads), sum(len(r) for r in reads) + 64)
    b.set_reads(reads)
    b.align()
    b.sync()
    res = oidx.align(reads, op, threads=8)
    aoff, alns, ops = b.alignments()
    assert np.array_equal(aoff, res["aln_off"])
    for f in ("begin_ref", "end_ref", "begin_q", "end_q", "score", "soc_index", "n_ops"):
        assert np.array_equal(alns[f], res["alns"][f]), f
    for ga, oa in zip(alns, res["alns"]):
        assert np.array_equal(ops[2 * int(ga["ops_off"]):2 * int(ga["ops_off"] + ga["n_ops"])],
                              res["ops"][2 * int(oa["ops_off"]):2 * int(oa["ops_off"] + oa["n_ops"])])
    moff, malns, _ = b.mapq_alignments()
    assert np.array_equal(moff, res["mq_off"])
    for f in ("begin_ref", "end_ref", "score", "secondary", "supplementary"):
        assert np.array_equal(malns[f], res["mq"][f]), f
    assert np.array_equal(malns["mapq"].view(np.uint64), res["mq"]["mapq"].view(np.uint64))
    assert len(alns) >= len(reads) - 5
    gidx.close()


@pytest.mark.parametrize("shift", [0, 5, 11])
def test_reads_in_a_caller_owned_device_array_without_padding(gpu_device, shift):
    """ma_batch_set_reads_device with long reads in an unaligned, unpadded device array: the seeding kernels read such
    reads through a 16-byte register window that must stay inside [codes, codes + n_bases) at both ends of the array."""
    import torch
    import ma_amd
    g = rand_genome(23, [900000, 400000], repeat_unit=300, repeat_copies=60, repeat_div=0.08)
    reads = sample_reads(g, 5, 3000, 51, sub=0.01, ins=0.003, dele=0.003) + sample_reads(g, 3, 700, 52, sub=0.01) + \
        sample_reads(g, 1, 17, 53) + sample_reads(g, 2, 5000, 54, sub=0.02)
    gidx = ma_amd.Index.build(g)
    P = ma_amd.Params.preset("default")
    nb = sum(len(r) for r in reads)
    ref = ma_amd.Batch(gidx, P, len(reads), nb + 64)
    ref.set_reads(reads)
    ref.align()
    ref.sync()
    want = ref.alignments()
    want_segs = ref.segments()
    # poison around the array: bytes outside [shift, shift + nb) must never influence the result
    host = np.full(nb + shift + 40, 3, dtype=np.uint8)
    host[shift:shift + nb] = np.concatenate(reads)
    dev = torch.from_numpy(host).cuda()
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)).cuda()
    for technique in (0, 1):
        P.seeding_technique = technique
        b0 = ma_amd.Batch(gidx, P, len(reads), nb + 64)
        b0.set_reads(reads)
        b0.align()
        b0.sync()
        b = ma_amd.Batch(gidx, P, len(reads), nb + 64)
        b.set_reads_device(dev.data_ptr() + shift, offs.data_ptr(), len(reads), nb)
        b.align()
        b.sync()
        for x, y in zip(b.segments(), b0.segments()):
            assert np.array_equal(x, y)
        for x, y in zip(b.alignments(), b0.alignments()):
            assert np.array_equal(x, y)
        if technique == 0:
            for x, y in zip(b.alignments(), want):
                assert np.array_equal(x, y)
            for x, y in zip(b.segments(), want_segs):
                assert np.array_equal(x, y)
        b.close()
        b0.close()
    ref.close()
    gidx.close()


def test_dp_scratch_budget_paths(gpu_device):
    """The launch planning of the DP stage (ksw_launch.h): with a small scratch budget a modest batch takes the paths of a
    large long-read batch -- fewer waves per launch, classes split into two launches by job size, the huge jobs on the side
    stream with their own scratch region.  Same alignments as with the default budget."""
    import sys
    probe = os.path.join(ROOT, "tests", "gpu_probe_dp_budget.py")

    def run(mb):
        env = dict(os.environ)
        env.pop("MA_KSW_SCRATCH_MB", None)
        if mb:
            env["MA_KSW_SCRATCH_MB"] = str(mb)
        out = subprocess.run([sys.executable, probe], env=env, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        line = [l for l in out.stdout.splitlines() if l.startswith("DIGEST")][-1].split()
        return line[1], int(line[2])

    want, n = run(0)
    assert n >= 300
    for mb in (256, 40):
        got, m = run(mb)
        assert (got, m) == (want, n), "scratch budget %d MB" % mb


@pytest.mark.parametrize("env", [{"MA_SEED_TASKS": "0"}, {"MA_SEED_TASKS": "0", "MA_SEED_WINDOW": "0"}, {"MA_SEED_TASKS": "1"},
                                 {"MA_LANES_PER_WAVE": "64"}, {"MA_LANES_PER_WAVE": "1"}, {"MA_LANES_PER_WAVE": "7"},
                                 {"MA_SMEM_COMPACT": "0", "technique": "1"}, {"technique": "1"}])
def test_kernel_variants_give_identical_results(gpu_device, monkeypatch, env):
    """The variants a batch's shape selects between -- read-per-lane vs area-per-lane maxSpan seeding, the register window
    on the read, full vs thin waves in the one-item-per-lane kernels, 16- vs 40-byte SMEM list entries -- forced through
    their environment hooks on one mixed read set: every stage record equals the default choice's."""
    import ma_amd
    g = rand_genome(31, [1200000, 500000], repeat_unit=300, repeat_copies=60, repeat_div=0.08)
    reads = (sample_reads(g, 400, 150, 71, sub=0.01) + sample_reads(g, 8, 5000, 72, sub=0.005, ins=0.003, dele=0.003)
             + sample_reads(g, 2, 16000, 73, sub=0.03, ins=0.02, dele=0.02) + sample_reads(g, 30, 1000, 74, sub=0.02))
    env = dict(env)
    technique = int(env.pop("technique", "0"))
    if env.get("MA_SMEM_COMPACT") == "0" or technique == 1:
        reads = [r for r in reads if len(r) < 2000]  # the packed entries are for reads < 2048 bases
    idx = ma_amd.Index.build(g)

    def run():
        P = ma_amd.Params.preset("default")
        P.seeding_technique = technique
        b = ma_amd.Batch(idx, P, len(reads), sum(len(r) for r in reads) + 64)
        b.set_reads(reads)
        b.align()
        b.sync()
        out = [b.segments(), b.seeds(), b.hsets(), b.alignments(), b.mapq_alignments()]
        b.close()
        return out

    want = run()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = run()
    for gs, ws in zip(got, want):
        for x, y in zip(gs, ws):
            assert np.array_equal(x, y)
    idx.close()


@pytest.mark.parametrize("env", [{"MA_SA_DENSE": "0"}, {"MA_SA_DENSE": "1"}, {"MA_KMER_K": "0"}, {"MA_KMER_K": "5"}, {"MA_KMER_K": "14"},
                                 {"MA_SA_DENSE": "0", "MA_KMER_K": "0"}])
def test_index_acceleration_structures_do_not_change_results(gpu_device, monkeypatch, env):
    """The dense SA sample and the K-mer table are private accelerators of the index: with other intervals / K, or without
    them, every stage record is the same; and an index created from the reference's arrays (dense sample derived by LF
    walks) equals one built on the device (dense sample taken from the full suffix array)."""
    import ma_amd
    g = rand_genome(37, [900000, 300000], repeat_unit=300, repeat_copies=60, repeat_div=0.08)
    reads = (sample_reads(g, 300, 150, 81, sub=0.01) + sample_reads(g, 6, 4000, 82, sub=0.01, ins=0.005, dele=0.005)
             + sample_reads(g, 20, 150, 83, sub=0.05, n_rate=0.02) + sample_reads(g, 2, 14, 84))

    def run(idx):
        out = []
        for technique in (0, 1):
            P = ma_amd.Params.preset("default")
            P.seeding_technique = technique
            b = ma_amd.Batch(idx, P, len(reads), sum(len(r) for r in reads) + 64)
            b.set_reads(reads)
            b.align()
            b.sync()
            out += [b.segments(), b.seeds(), b.hsets(), b.alignments(), b.mapq_alignments()]
            b.close()
        return out

    idx = ma_amd.Index.build(g)
    want = run(idx)
    parts = idx.download()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    idx2 = ma_amd.Index.build(g)
    idx3 = ma_amd.Index.from_arrays(**parts) if isinstance(parts, dict) else None
    for other in (idx2, idx3):
        if other is None:
            continue
        got = run(other)
        for gs, ws in zip(got, want):
            for x, y in zip(gs, ws):
                assert np.array_equal(x, y)
        other.close()
    idx.close()
