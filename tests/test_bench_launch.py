"""bench.py's launch contract on the CPU (no GPU is touched: MA_BENCH_DRY_RUN=1 stops after the rendezvous)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, **env):
    e = dict(os.environ, MA_BENCH_DRY_RUN="1", **env)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        if k not in env:
            e.pop(k, None)
    return subprocess.run([sys.executable, BENCH] + args, env=e, capture_output=True, text=True, timeout=300)


def test_gpus_flag_starts_that_many_ranks_without_an_outer_torchrun():
    """`python bench.py --gpus 2` (no torchrun environment): the process starts two ranks itself before anything touches a GPU,
    they rendezvous over 127.0.0.1 (gloo here) and rank 0 reports n_gpus = 2 (the flag was parsed and ignored)."""
    r = _run(["--gpus", "2"])
    assert r.returncode == 0, r.stderr[-500:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["ranks_seen"] == [0, 1] and line["gpus_flag"] == 2


def test_single_rank_needs_no_launcher():
    r = _run(["--gpus", "1"])
    assert r.returncode == 0
    assert json.loads(r.stdout.splitlines()[-1])["n_gpus"] == 1


def test_world_size_must_equal_the_gpus_flag():
    """inside a torchrun environment of another size the bench refuses: a 1-rank number is never printed as an N-GPU one"""
    r = _run(["--gpus", "8"], WORLD_SIZE="1", RANK="0")
    assert r.returncode != 0 and "refusing" in r.stderr
    r = _run(["--gpus", "1"], WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 0


def test_dump_outputs_writes_a_fixed_float_sample_within_its_budget(tmp_path):
    """--dump-outputs: the same records give the same files, every array is float64, the files fit the budget, and the sampled
    reads' alignments and ops are the records of those reads."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from ma_amd.api import ALIGNMENT_DT
    rng = np.random.default_rng(5)
    B = 5000
    na = rng.integers(0, 4, B)
    off = np.zeros(B + 1, dtype=np.uint64)
    off[1:] = np.cumsum(na)
    al = np.zeros(int(off[B]), dtype=ALIGNMENT_DT)
    al["begin_ref"] = rng.integers(0, 6 * 10 ** 9, al.size)
    al["score"] = rng.integers(-50, 300, al.size)
    al["n_ops"] = rng.integers(1, 40, al.size)
    al["mapq"] = rng.random(al.size)
    al["ops_off"] = np.concatenate([[0], np.cumsum(al["n_ops"][:-1])])
    ops = rng.integers(0, 200, 2 * int(al["n_ops"].sum()) + 2).astype(np.uint64)
    budget = 200000
    n = bench.dump_outputs(str(tmp_path / "a"), "w.leg", off, al, ops, B, budget)
    assert 0 < n <= budget
    assert bench.dump_outputs(str(tmp_path / "b"), "w.leg", off, al, ops, B, budget) == n
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) == 3 + len(bench.DUMP_FIELDS)
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b)
    d = {f[len("w.leg."):-4]: np.load(tmp_path / "a" / f) for f in names}
    sel = d["read"].astype(np.int64)
    assert 0 < sel.size < B and np.all(np.diff(sel) > 0)
    assert np.array_equal(d["n_alignments"], na[sel])
    rows = np.concatenate([np.arange(off[r], off[r + 1]) for r in sel]).astype(np.int64)
    for f in bench.DUMP_FIELDS:
        assert np.array_equal(d[f], al[f][rows].astype(np.float64)), f
    want = np.concatenate([ops[2 * int(o):2 * int(o + k)] for o, k in zip(al["ops_off"][rows], al["n_ops"][rows])])
    assert np.array_equal(d["ops"].ravel(), want.astype(np.float64))


def test_detail_file_goes_with_full():
    """The per-workload blocks are a --full run's: a plain run refuses --detail-file instead of leaving the file unwritten."""
    r = _run(["--gpus", "1", "--detail-file", "d.json"])
    assert r.returncode == 2 and "--full" in r.stderr
    assert _run(["--gpus", "1", "--full", "--detail-file", "d.json"]).returncode == 0


def test_plain_run_runs_only_the_leg_value_comes_from(monkeypatch):
    """Without --full one leg of the workload runs: the one `value` comes from under --full (the last of leg_plan), with the
    batches in flight and I/O --full gives it; if it fails to set up, the leg before it runs instead.  --dump-outputs names the
    legs of a --full run (dumped_legs) as run_legs runs them."""
    import types
    sys.path.insert(0, ROOT)
    import bench
    calls = []

    def fake_run_workload(E, name, wl, args, leg=None):
        calls.append((leg, args.inflight, args.host_io))
        if leg in E.failing:
            raise RuntimeError("no HBM for %s" % leg)
        return {"name": name, "leg": leg, "roofline": {"kernel_ms_per_step": {}}, "batches_in_flight": args.inflight, "io": "",
                "value": 1.0, "unit": "", "steps": 1, "ms_per_step": 1.0, "step_ms_min": 1.0, "step_ms_max": 1.0, "gbases_per_s": 0,
                "aligned_reads": 1}

    monkeypatch.setattr(bench, "run_workload", fake_run_workload)
    streams = []
    torch = types.SimpleNamespace(cuda=types.SimpleNamespace(empty_cache=lambda: None, Stream=lambda: streams.append(1)))
    E = types.SimpleNamespace(live=[], live_host=[], torch=torch, failing=())
    # (workload, the leg `value` comes from, streams the legs before it take from torch's pool under --full)
    for name, want, n_streams in (("150bp", ("host_to_host", 3, 1), 3), ("10kb", ("host_to_host", 1, 1), 2),
                                  ("50kb", ("host_to_host", 2, 1), 2), ("10kb_pacbio", ("single_stream", 1, 0), 0)):
        args = bench.build_parser().parse_args(["--workload", name])
        wl = dict(bench.WORKLOADS[name], steps=10, warmup=1)
        calls.clear()
        bench.run_legs(E, name, wl, args)
        assert calls[-1] == want, name  # the leg `value` comes from under --full
        assert [c[0] for c in calls] == [leg for leg, _, _ in bench.dumped_legs(wl, args)], name
        calls.clear()
        streams.clear()
        assert bench.run_headline_leg(E, name, wl, args)[0] == want[0]
        assert calls == [want] and len(streams) == n_streams, name
    wl = dict(bench.WORKLOADS["150bp"], steps=2, warmup=1)  # fewer steps than batches: fewer batches in flight
    calls.clear()
    streams.clear()
    bench.run_headline_leg(E, "150bp", wl, bench.build_parser().parse_args([]))
    assert calls == [("host_to_host", 3, 1)] and len(streams) == 2
    calls.clear()
    bench.run_headline_leg(E, "150bp", wl, bench.build_parser().parse_args(["--overlap", "0"]))
    assert calls == [("single_stream", 1, 0)]
    E.failing = ("host_to_host",)
    calls.clear()
    assert bench.run_headline_leg(E, "150bp", wl, bench.build_parser().parse_args([]))[0] == "overlapped"
    assert calls == [("host_to_host", 3, 1), ("overlapped", 3, 0)]
