"""What a batch forgets, and when (ma_amd/host/ma_batch_state.h, kept by ma_amd/csrc/pipeline.hip).  Every form of "this
batch has new reads" -- the host arrays, the staged upload, caller-owned device arrays, a text, a refused text, mate texts, BGZF
members -- puts a batch that has been through every stage back to the start: no stage output, no SAM text, no pairs, no names
unless the form brings them, and the next pass computes what a fresh batch computes.  Every call that changes the alignment
lists (ma_dp_batch, ma_batch_set_alignments, ma_inversions_batch) drops both SAM texts and the pairs; ma_pair_batch drops only
the pairs' text.  An earlier stage run again, or its input handed in, drops every product of the later stages; a refused
ma_batch_set_reads_device leaves the batch as it was."""
import numpy as np
import pytest

from ma_testlib import rand_genome, revcomp, sample_reads
from test_gpu_bgzf import END, member

pytestmark = pytest.mark.gpu
NO_READS = dict(reads=0, bases=0, name_bytes=0, has_qual=0)


def params():
    import ma_amd
    P = ma_amd.Params.preset("default")
    P.srand_seed = 1
    return P


def names_of(reads):
    return ["r%d" % i for i in range(len(reads))]


def fastq(reads, names=None):
    names = names or names_of(reads)
    return b"".join(("@%s\n%s\n+\n%s\n" % (nm, "".join("ACGT"[int(x)] for x in r), "I" * len(r))).encode() for nm, r in zip(names, reads))


def full_pass(b, reads, text_is_set):
    """every stage and both texts; returns the MappingQuality records (after the inversions) as bytes"""
    b.align()
    if not text_is_set:
        b.set_read_text(names_of(reads))
    b.inversions()
    b.pair()
    assert b.sam() >= 0 and b.pair_sam() >= 0
    b.sam_bytes(), b.pair_sam_bytes(), b.pair_counts()  # all there
    return tuple(x.tobytes() for x in b.mapq_alignments())


@pytest.fixture(scope="module")
def world(gpu_device):
    import ma_amd
    g = rand_genome(41, [20000])
    reads = sample_reads(g, 8, 100, 42, sub=0.01)  # the reads of the pass before each form, as 4 pairs
    fresh = sample_reads(g, 8, 100, 43, sub=0.01)  # the reads each form brings
    idx = ma_amd.Index.build(g)
    idx.set_contig_names(["chr1"])
    b = ma_amd.Batch(idx, params(), 64, 8192)
    want = {}
    for key, rs in (("fresh", fresh), ("none", [])):  # what a fresh batch computes for them
        f = ma_amd.Batch(idx, params(), 64, 8192)
        f.set_reads(rs)
        want[key] = full_pass(f, rs, False)
        f.close()
    yield b, reads, fresh, want
    b.close()
    idx.close()


def flat(reads):
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.ascontiguousarray(np.concatenate(reads + [np.zeros(1, dtype=np.uint8)])), off


def by_set_reads(b, reads):
    b.set_reads(reads)


def by_staged_reads(b, reads):
    import ma_amd
    cat, off = flat(reads)
    codes, offs = ma_amd.HostArray(len(cat), np.uint8), ma_amd.HostArray(len(off), np.uint64)
    codes.a[:], offs.a[:] = cat, off
    b.stage_reads_flat(codes.ptr, offs.ptr, len(reads))
    b.use_staged_reads()  # (waits for the upload: the host arrays are free again)
    codes.close()
    offs.close()


def by_set_reads_device(b, reads):
    import torch
    cat, off = flat(reads)
    b.keep = (torch.from_numpy(cat).cuda(), torch.from_numpy(off.astype(np.int64)).cuda())  # the caller owns them while they are set
    b.set_reads_device(b.keep[0].data_ptr(), b.keep[1].data_ptr(), len(reads), int(off[-1]))


def by_text(b, reads):
    assert b.set_reads_text(fastq(reads)) == len(reads)


def by_refused_text(b, reads):
    import ma_amd
    with pytest.raises(ma_amd.MaError, match="ma_batch_set_reads_text: line 1"):
        b.set_reads_text(b"x")


def by_mates_text(b, reads):
    nm = names_of(reads)
    n, _ = b.set_mates_text(fastq(reads[0::2], nm[0::2]), fastq([revcomp(r) for r in reads[1::2]], nm[1::2]))
    assert 2 * n == len(reads)


def by_bgzf(b, reads):
    text = fastq(reads)
    assert b.set_reads_bgzf(member(text[:700]) + member(text[700:]) + END) == len(reads)


FORMS = [("set_reads", by_set_reads, "array"), ("stage_reads_flat + use_staged_reads", by_staged_reads, "array"),
         ("set_reads_device", by_set_reads_device, "array"), ("set_reads_text", by_text, "text"),
         ("set_reads_text, refused", by_refused_text, "refused"), ("set_mates_text", by_mates_text, "text"),
         ("set_reads_bgzf", by_bgzf, "text")]


@pytest.mark.parametrize("name,form,kind", FORMS, ids=[f[0] for f in FORMS])
def test_new_reads_put_the_batch_back_to_the_start(world, name, form, kind):
    """after a complete pass (align, names, inversions, pairs, both texts) each form of new reads leaves: dp() without chains, no
    SAM text, no pairs' text, no pairs; read_counts() of the new reads with names only where the form brings them; and a pass
    that computes the MappingQuality records of a fresh batch with the same reads, byte for byte"""
    import ma_amd
    b, reads, fresh, want = world
    b.set_reads(reads)
    full_pass(b, reads, False)
    form(b, fresh)
    for call, message in ((b.dp, "ma_dp_batch: run ma_chain_batch first"), (b.sam_bytes, "ma_batch_sam_counts: run ma_sam_batch first"),
                          (b.pair_sam_bytes, "ma_batch_pair_sam_counts: run ma_pair_sam_batch first"),
                          (b.pair_counts, "ma_batch_pair_counts: run ma_pair_batch first")):
        with pytest.raises(ma_amd.MaError) as e:
            call()
        assert str(e.value) == message, name
    n_bases = sum(len(r) for r in fresh)
    if kind == "array":
        assert b.read_counts() == dict(reads=len(fresh), bases=n_bases, name_bytes=0, has_qual=0)
    elif kind == "text":
        assert b.read_counts() == dict(reads=len(fresh), bases=n_bases, name_bytes=sum(len(x) for x in names_of(fresh)), has_qual=1)
        assert b.read_text()[0] == [x.encode() for x in names_of(fresh)]
    else:
        assert b.read_counts() == NO_READS
    after = [] if kind == "refused" else fresh
    assert full_pass(b, after, kind == "text") == want["none" if kind == "refused" else "fresh"]
    b.keep = None


def gone(call, message):
    import ma_amd
    with pytest.raises(ma_amd.MaError) as e:
        call()
    assert str(e.value) == message


def test_changed_lists_drop_the_texts_and_the_pairs(world):
    """a second dp(), set_alignments with the records just downloaded, and inversions() each drop both SAM texts and the pairs
    of the lists before; pair() again drops only the pairs' text -- the single-end text does not read the picks and stays"""
    b, reads, fresh, want = world
    changes = [("dp", lambda: b.dp()), ("set_alignments", lambda: b.set_alignments(*b.alignments())), ("inversions", lambda: b.inversions())]
    for name, change in changes:
        b.set_reads(reads)
        full_pass(b, reads, False)
        change()
        gone(b.sam_bytes, "ma_batch_sam_counts: run ma_sam_batch first")
        gone(b.pair_sam_bytes, "ma_batch_pair_sam_counts: run ma_pair_sam_batch first")
        gone(b.pair_counts, "ma_batch_pair_counts: run ma_pair_batch first")
    b.set_reads(reads)
    full_pass(b, reads, False)
    single = b.sam_bytes()
    b.pair()  # the one asymmetry
    gone(b.pair_sam_bytes, "ma_batch_pair_sam_counts: run ma_pair_sam_batch first")
    assert b.sam_bytes() == single > 0
    assert b.pair_counts()["pairs"] == len(reads) // 2


def test_empty_input(world):
    """an empty text and no BGZF members at all: a batch of zero reads, which align() takes"""
    b, reads, fresh, want = world
    for empty in (lambda: b.set_reads_text(b""), lambda: b.set_reads_bgzf(b"")):
        b.set_reads(reads)
        full_pass(b, reads, False)
        assert empty() == 0
        assert b.read_counts() == NO_READS
        b.align()
        b.sync()


# ---- an earlier stage run again, or its input handed in: the products of the later stages go -------------------------------

def refused_hsets(b):
    import ma_amd
    hset_off, hseed_off, soc, seeds = b.hsets()
    bad = seeds.copy()
    bad["q_start"][0] = 1000  # beyond its read of 100 bases
    with pytest.raises(ma_amd.MaError, match="ma_batch_set_hsets: seed ends beyond its read of 100 bases"):
        b.set_hsets(hset_off, hseed_off, soc, bad)


def refused_seeds(b):
    import ma_amd
    off, seeds = b.seeds()
    bad = seeds.copy()
    bad["delta"][0] += 1
    with pytest.raises(ma_amd.MaError, match="ma_batch_set_seeds: delta is [0-9]+, ExtractSeeds computes [0-9]+ \\(read 0, seed 0\\)"):
        b.set_seeds(off, bad)
    gone(b.chain, "ma_chain_batch: run ma_extract_seeds_batch first")


def refused_soc_heap(b):
    import ma_amd
    soc_off, socs, seed_off, seeds = b.socs(heap=True)
    assert len(socs)
    bad = socs.copy()
    bad["end"][0] = 10 ** 6
    with pytest.raises(ma_amd.MaError, match="ma_batch_set_soc_heap: strip outside the read's [0-9]+ seeds \\(read 0, strip 0\\)"):
        b.set_soc_heap(soc_off, bad, seed_off, seeds)
    gone(b.chain, "ma_chain_batch: run ma_extract_seeds_batch first")


# (name, the call, the stage calls that are left before full_pass's tail)
EARLIER = [("seed", lambda b: b.seed(), ("extract", "chain", "dp")),
           ("extract", lambda b: b.extract(), ("chain", "dp")),
           ("chain", lambda b: b.chain(), ("dp",)),
           ("set_segments", lambda b: b.set_segments(*b.segments()), ("extract", "chain", "dp")),
           ("set_seeds", lambda b: b.set_seeds(*b.seeds()), ("chain", "dp")),
           ("set_soc_heap", lambda b: b.set_soc_heap(*b.socs(heap=True)), ("chain", "dp")),
           ("set_hsets", lambda b: b.set_hsets(*b.hsets()), ("dp",)),
           ("set_hsets, refused", refused_hsets, ("chain", "dp")),
           ("set_seeds, refused", refused_seeds, ("extract", "chain", "dp")),
           ("set_soc_heap, refused", refused_soc_heap, ("extract", "chain", "dp"))]
LATER_GONE = [(lambda b: b.sam_bytes(), "ma_batch_sam_counts: run ma_sam_batch first"),
              (lambda b: b.pair_sam_bytes(), "ma_batch_pair_sam_counts: run ma_pair_sam_batch first"),
              (lambda b: b.pair_counts(), "ma_batch_pair_counts: run ma_pair_batch first"),
              (lambda b: b.sam_bgzf_counts(False), "ma_batch_sam_bgzf_counts: no SAM text to deflate (run ma_sam_batch first)"),
              (lambda b: b.sam_bgzf_counts(True), "ma_batch_sam_bgzf_counts: no SAM text to deflate (run ma_pair_sam_batch first)"),
              (lambda b: b.inversion_counts(), "ma_batch_inversion_counts: run ma_inversions_batch first")]


@pytest.mark.parametrize("name,call,rest", EARLIER, ids=[e[0] for e in EARLIER])
def test_an_earlier_stage_drops_the_later_products(world, name, call, rest):
    """after a complete pass with the BGZF members of both texts, a stage run again or a stage input handed in leaves no SAM
    text, no pairs, no members and no inversion counts: each getter raises the message it has for "never made".  The stages that
    are left and the tail of the pass then compute the MappingQuality records of a fresh batch with the same reads, byte for
    byte."""
    b, reads, fresh, want = world
    b.set_reads(fresh)
    assert full_pass(b, fresh, False) == want["fresh"]
    assert b.sam_bgzf(False) and b.sam_bgzf(True)
    call(b)
    for getter, message in LATER_GONE:
        gone(lambda: getter(b), message)
    for stage in rest:
        getattr(b, stage)()
    b.inversions()
    b.pair()
    assert b.sam() >= 0 and b.pair_sam() >= 0
    assert tuple(x.tobytes() for x in b.mapq_alignments()) == want["fresh"]


def test_a_refused_set_reads_device_keeps_the_reads(world):
    """ma_batch_set_reads_device installs the caller's arrays last: a call it refuses (no offsets for n > 0 reads) leaves the reads,
    the texts and the pairs of the batch as they were"""
    import ma_amd
    b, reads, fresh, want = world
    b.set_reads(reads)
    full_pass(b, reads, False)
    before = b.read_counts(), b.sam_bytes(), b.pair_counts()
    with pytest.raises(ma_amd.MaError) as e:
        b.set_reads_device(0, 0, len(fresh), sum(len(r) for r in fresh))
    assert str(e.value) == "ma_batch_set_reads_device: null argument"
    assert (b.read_counts(), b.sam_bytes(), b.pair_counts()) == before
    assert before[0]["reads"] == len(reads) and before[1] > 0


def test_refused_seeds_and_strips_name_the_read_and_the_record(world):
    """Every clause of the contract of ma_batch_set_seeds / ma_batch_set_soc_heap (include/ma_amd.h; the clauses one by one on the
    host: test_seed_contract_host.py) through the library: the call fails with the message, the batch holds no seeds and no
    strips afterwards, and the same batch then takes the seeds as they were and chains them to the sets of the fused path."""
    import ma_amd
    b, reads, fresh, want = world
    b.set_reads(fresh)
    b.seed(), b.extract(), b.chain()
    b.sync()
    sets = tuple(x.tobytes() for x in b.hsets())
    off, seeds = b.seeds()
    soc_off, socs, seed_off, sorted_seeds = b.socs(heap=True)
    r = int(np.nonzero(np.diff(off.astype(np.int64)) >= 2)[0][0])  # a read of two seeds at least
    k = int(off[r])
    qlen = len(fresh[r])

    def seeds_with(field, value, at=k):
        bad = seeds.copy()
        bad[field][at] = value
        return off, bad

    assert off[-2] > 0
    bad_off = off.copy()
    bad_off[-1] = off[-2] - 1
    cases = [(lambda: (bad_off, seeds), "seed_off decreases at read %d" % (len(off) - 2)),
             (lambda: seeds_with("q_start", -1), "negative field (read %d, seed 0)" % r),
             (lambda: seeds_with("len", 0, k + 1), "empty seed (read %d, seed 1)" % r),
             (lambda: seeds_with("len", qlen + 1), "seed ends beyond its read of %d bases (read %d, seed 0)" % (qlen, r)),
             (lambda: seeds_with("on_forward", 2), "on_forward is neither 0 nor 1 (read %d, seed 0)" % r),
             (lambda: seeds_with("r_start", 20000), "r_start outside the forward text of 20000 bases (read %d, seed 0)" % r)]
    for make, message in cases:
        with pytest.raises(ma_amd.MaError) as e:
            b.set_seeds(*make())
        assert str(e.value) == "ma_batch_set_seeds: " + message
        gone(b.chain, "ma_chain_batch: run ma_extract_seeds_batch first")
        gone(lambda: b.socs(), "ma_batch_get_socs: run ma_extract_seeds_batch first")
    bad = socs.copy()
    bad["n_seeds"][0] += 1
    with pytest.raises(ma_amd.MaError) as e:
        b.set_soc_heap(soc_off, bad, seed_off, sorted_seeds)
    assert str(e.value) == "ma_batch_set_soc_heap: n_seeds is not end - begin (read 0, strip 0)"
    gone(b.chain, "ma_chain_batch: run ma_extract_seeds_batch first")
    with pytest.raises(ma_amd.MaError) as e:  # the seeds of a strip call are held to the seeds' contract, under the call's name
        b.set_soc_heap(soc_off, socs, *seeds_with("delta", 0))
    assert str(e.value).startswith("ma_batch_set_soc_heap: delta is 0, ExtractSeeds computes ")
    # recovery on the same batch, both ways in
    b.set_seeds(off, seeds)
    b.chain()
    b.sync()
    assert tuple(x.tobytes() for x in b.hsets()) == sets
    b.set_soc_heap(soc_off, socs, seed_off, sorted_seeds)
    b.chain()
    b.sync()
    assert tuple(x.tobytes() for x in b.hsets()) == sets
