"""The text mode of k_seed (ma_amd/csrc/seeding.h, stage_seed.h): maxSpan runs whose interval is down to one row go on by
comparing the read with the packed text.  Every record of the pipeline equals that of the plain kernel (MA_SEED_TEXT=0) and the
oracle's, on the genome and reads of seed_text_cases.py; the extension counter shows where the mode is entered."""
import numpy as np
import pytest

from ma_testlib import OrIndex, or_params
import seed_text_cases

pytestmark = pytest.mark.gpu


def _all_records(b):
    return [b.segments(), b.seeds(), b.hsets(), b.alignments(), b.mapq_alignments()]


def _same(got, want):
    for gs, ws in zip(got, want):
        assert len(gs) == len(ws)
        for x, y in zip(gs, ws):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.fixture(scope="module")
def case(gpu_device):
    import ma_amd
    g = seed_text_cases.genome()
    reads = seed_text_cases.reads(g)
    idx = ma_amd.Index.build(g)
    yield reads, idx
    idx.close()


def _run(idx, reads, min_amb):
    import ma_amd
    P = ma_amd.Params.preset("default")
    P.min_ambiguity = min_amb
    P.srand_seed = 1
    b = ma_amd.Batch(idx, P, len(reads), sum(len(r) for r in reads) + 64)
    b.set_reads(reads)
    b.align()
    b.sync()
    out = _all_records(b)
    ctr = b.counters()
    b.close()
    return out, int(ctr[0]), int(ctr[1]), int(ctr[2])


@pytest.mark.parametrize("min_amb", [0, 2])
def test_text_mode_records_equal_the_plain_kernels_and_the_oracles(case, monkeypatch, min_amb):
    reads, idx = case
    monkeypatch.setenv("MA_SEED_TEXT", "0")
    want, steps_fm, blocks_fm, lf_fm = _run(idx, reads, min_amb)
    monkeypatch.delenv("MA_SEED_TEXT")
    got, steps, blocks, lf = _run(idx, reads, min_amb)
    print("min_amb %d: extend_backward steps %d -> %d, 64-byte gathers of k_seed %d -> %d, LF steps of extraction %d -> %d"
          % (min_amb, steps_fm, steps, blocks_fm, blocks, lf_fm, lf))
    _same(got, want)
    assert len(want[0][1]) > 2000 and len(want[1][1]) > 2000
    if min_amb == 0:
        assert steps < steps_fm
        assert lf < lf_fm  # the seeds of segments that carry their position need no walk
    else:
        assert steps == steps_fm and blocks == blocks_fm and lf == lf_fm
    # the oracle on the same index bytes
    op = or_params("default", 1)
    op.min_ambiguity = min_amb
    res = OrIndex.from_parts(idx.download()).align(reads, op, threads=8)
    (seg_off, segs), (seed_off, seeds) = got[0], got[1]
    assert np.array_equal(seg_off, res["seg_off"]) and np.array_equal(seed_off, res["seed_off"])
    for f in ("q_start", "q_size", "sa_start", "sa_start_rc", "sa_size"):
        assert np.array_equal(segs[f], res["segs"][f]), f
    for f in ("q_start", "len", "r_start", "delta", "ambiguity", "on_forward"):
        assert np.array_equal(seeds[f], res["seeds"][f]), f
    for (off, alns, _), o, a in ((got[3], "aln_off", "alns"), (got[4], "mq_off", "mq")):
        assert np.array_equal(off, res[o])
        for f in ("begin_ref", "end_ref", "begin_q", "end_q", "score", "n_ops"):
            assert np.array_equal(alns[f], res[a][f]), (a, f)
    if min_amb == 0:
        # 256 resident lanes for more than 2000 reads: lanes take their next read from the queue in the middle of a wavefront's walk
        monkeypatch.setenv("MA_SEED_LANES", "256")
        got2, steps2, _, _ = _run(idx, reads, min_amb)
        _same(got2, want)
        assert steps2 == steps
