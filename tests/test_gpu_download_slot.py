"""The one download slot of a batch object: ma_batch_start_mapq_download, ma_batch_start_pair_download,
ma_batch_start_sam_download and ma_batch_start_pair_sam_download share ONE I/O stream and ONE pending download, whichever kind
it is.  While one is pending every start_* is refused with its own message, every synchronous get of another kind waits for it
first (the packed arrays and the texts may be overwritten only then), and ma_sam_batch / ma_pair_sam_batch wait for it before
they touch a text.  The expected values are what the four synchronous gets return on the same batch."""
import numpy as np
import pytest

from ma_testlib import sample_pairs
from test_gpu_sam import Ctx, make_quals, mixed, params  # noqa: F401  (mixed: the fixture of the small random genome)

pytestmark = pytest.mark.gpu
KINDS = ("mapq", "pair", "sam", "pair_sam")
# the synchronous get that runs while a download of the kind is pending: the two record kinds share their packed arrays on
# the device, the two texts nothing
OTHER = dict(mapq="pair", pair="mapq", sam="pair_sam", pair_sam="sam")
SYNC = dict(mapq="mapq_alignments", pair="pairs", sam="sam_text", pair_sam="pair_sam_text")


def canon(kind, parts):
    """what a get of the kind returned, or what its host arrays hold, cut to the sizes its offsets give"""
    parts = [np.frombuffer(p, dtype=np.uint8) if isinstance(p, bytes) else np.asarray(p) for p in parts]
    off, n = parts[0], int(parts[0][-1])
    if kind in ("sam", "pair_sam"):
        return off, parts[1][:n]
    alns = parts[1][:n]
    return (off, alns, parts[2][:2 * int(alns["n_ops"].sum())]) + tuple(p[:n] for p in parts[3:])


def same(x, y):
    return len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))


class Slot:
    """a batch, the host arrays of the four downloads and the expected value of each"""

    def __init__(self, b):
        import ma_amd
        self.b = b
        c, pc, u64 = b.counts(), b.pair_counts(), np.uint64
        self.arr = dict(
            mapq=[ma_amd.HostArray(b.n + 1, u64), ma_amd.HostArray(c["alignments"] + 1, ma_amd.ALIGNMENT_DT),
                  ma_amd.HostArray(2 * c["ops_cap"] + 2, u64)],
            pair=[ma_amd.HostArray(pc["pairs"] + 1, u64), ma_amd.HostArray(pc["records"], ma_amd.ALIGNMENT_DT),
                  ma_amd.HostArray(2 * pc["ops"], u64), ma_amd.HostArray(pc["records"], np.int32),
                  ma_amd.HostArray(pc["records"], np.int32)],
            sam=[ma_amd.HostArray(b.n + 1, u64), ma_amd.HostArray(b.sam_bytes(), np.uint8)],
            pair_sam=[ma_amd.HostArray(b.n // 2 + 1, u64), ma_amd.HostArray(b.pair_sam_bytes(), np.uint8)])
        self.want = {k: canon(k, self.get(k)) for k in KINDS}

    def get(self, kind):
        return getattr(self.b, SYNC[kind])()

    def start(self, kind, fill=True):
        for h in self.arr[kind] if fill else []:
            h.a.view(np.uint8)[:] = 0xA5
        assert getattr(self.b, "start_%s_download" % kind)(*self.arr[kind]) is not None

    def holds(self, kind):
        return same(canon(kind, [h.a for h in self.arr[kind]]), self.want[kind])

    def close(self):
        for hs in self.arr.values():
            for h in hs:
                h.close()
        self.b.close()


def run_all(b):
    b.align()
    b.pair()
    b.sam(0)
    b.pair_sam(0)


@pytest.fixture(scope="module")
def slot(mixed):  # noqa: F811
    ctx = mixed
    reads = sample_pairs(ctx.g, 8, 100, 120)
    b = ctx.batch(params("illuminapaired"), reads, ["m%d" % i for i in range(len(reads))], make_quals(reads, 121))
    run_all(b)
    s = Slot(b)
    # the four values are there and differ: a download that lands in the wrong place, or not at all, cannot pass for another
    assert len(s.want["mapq"][1]) > 0 and len(s.want["pair"][1]) > 0 and len(s.want["sam"][1]) > 0
    assert not same(s.want["sam"], s.want["pair_sam"]) and not same(s.want["mapq"][:3], s.want["pair"][:3])
    yield s
    s.close()


@pytest.mark.parametrize("kind", KINDS)
def test_one_slot_for_the_four_download_kinds(slot, kind):
    """with a download of `kind` pending: all four start_* are refused, each under its own name; a synchronous get of another
    kind returns its value, and behind it the pending download is complete and the slot free"""
    import ma_amd
    s = slot
    s.start(kind)
    for k in KINDS:
        with pytest.raises(ma_amd.MaError, match="ma_batch_start_%s_download: .*was not finished" % k):
            s.start(k, fill=False)  # (refused before anything is copied: the arrays of the pending download stay alone)
    assert same(canon(OTHER[kind], s.get(OTHER[kind])), s.want[OTHER[kind]])
    assert s.holds(kind)
    s.b.finish_download()  # nothing is pending any more
    s.start(OTHER[kind])
    s.b.finish_download()
    assert s.holds(OTHER[kind]) and s.holds(kind)


@pytest.mark.parametrize("again", ["sam", "pair_sam"])
@pytest.mark.parametrize("kind", ["sam", "pair_sam"])
def test_formatting_again_waits_for_a_pending_text_download(slot, kind, again):
    """ma_sam_batch / ma_pair_sam_batch while a text is on its way down: the downloaded bytes are the expected ones, the slot
    is free, and the text formatted again is the same"""
    s = slot
    s.start(kind)
    assert getattr(s.b, again)(0) == len(s.want[again][1])
    assert s.holds(kind)
    s.start(again)
    s.b.finish_download()
    assert s.holds(again) and s.holds(kind)


def test_empty_batch_leaves_no_download_pending(mixed):  # noqa: F811
    """0 reads: every start_* returns at once and leaves nothing pending, so a second start_* is not refused"""
    import ma_amd
    b = ma_amd.Batch(mixed.idx, params("illuminapaired"), 8, 1024)
    b.set_reads([])
    b.set_read_text([], None)
    run_all(b)
    s = Slot(b)
    for _ in range(2):
        for k in KINDS:
            s.start(k)
            assert int(s.arr[k][0].a[0]) == 0
    b.finish_download()
    s.close()
