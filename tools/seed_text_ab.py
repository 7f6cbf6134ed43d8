#!/usr/bin/env python3
"""The text mode of k_seed against the plain kernel in ONE process, on the benchmark's genome and its 150 bp reads: the switch
MA_SEED_TEXT is read per call, so the two alternate on one batch object and one index.  Per mode, over the timed steps: stage
times (HIP events), extend_backward steps, 64-byte gathers of the seeding kernel and LF steps of the extraction per read, and
whether the alignment records of the two modes are the same bytes.
usage: python tools/seed_text_ab.py [--steps 6] [--genome-scale 1.0]   (one JSON line)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    ap = bench.build_parser()
    args = ap.parse_args()
    E = bench.Env(args)
    wl = dict(bench.WORKLOADS["150bp"])
    wl["steps"], wl["warmup"] = 1, 0
    codes, offs, offs_h, B, _ = bench.make_reads(E, wl, args)
    P = E.ma.Params.preset("default")
    nbases = int(offs_h[B] - offs_h[0])
    bt = E.ma.Batch(E.idx, P, B, nbases + 64)
    bt.enable_timing(True)
    res = {"0": dict(kms=[], ctr=None, sig=None), "1": dict(kms=[], ctr=None, sig=None)}
    for it in range(2 + 2 * args.steps):  # one warm-up of each mode, then alternating
        mode = str(it & 1)
        os.environ["MA_SEED_TEXT"] = mode
        bt.set_reads_device(codes.data_ptr(), offs.data_ptr(), B, nbases)
        bt.align()
        bt.sync()
        if it < 2:
            off, alns, ops = bt.mapq_alignments()
            res[mode]["sig"] = (off.tobytes(), alns.tobytes(), ops.tobytes())
            res[mode]["ctr"] = bt.counters().astype(np.float64)
            continue
        res[mode]["kms"].append(bt.kernel_ms().astype(np.float64)[:6])
    out = {"reads": B, "genome_nt": E.F, "steps_per_mode": args.steps, "records_equal": res["0"]["sig"] == res["1"]["sig"]}
    for mode, name in (("0", "plain"), ("1", "text")):
        k = np.array(res[mode]["kms"])
        c = res[mode]["ctr"]
        out[name] = {"stage_ms_median": {bench.STAGES[i]: round(float(np.median(k[:, i])), 3) for i in range(6)},
                     "seed_ms_min_max": [round(float(k[:, 0].min()), 3), round(float(k[:, 0].max()), 3)],
                     "extract_ms_min_max": [round(float(k[:, 1].min()), 3), round(float(k[:, 1].max()), 3)],
                     "extend_steps_per_read": round(c[0] / B, 2), "seed_gathers_per_read": round(c[1] / B, 2),
                     "extract_lf_steps_per_read": round(c[2] / B, 2)}
    print(json.dumps(out))
    bt.close()
    E.close()


if __name__ == "__main__":
    main()
