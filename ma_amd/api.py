"""ctypes binding of include/ma_amd.h (the drop-in C ABI)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    # MA_AMD_LIB: an alternative build of the same library (e.g. the -DMA_KSW_PROF diagnostics build)
    return os.environ.get("MA_AMD_LIB") or os.path.join(_HERE, "libma_amd.so")


class MaError(RuntimeError):
    pass


class Params(C.Structure):
    _fields_ = [
        ("seeding_technique", C.c_int32), ("min_seed_len", C.c_int32), ("min_ambiguity", C.c_int32),
        ("max_ambiguity", C.c_int32), ("min_seed_size_drop", C.c_int32), ("max_num_soc", C.c_int32),
        ("min_num_soc", C.c_int32), ("harm_score_min", C.c_int32), ("max_score_lookahead", C.c_int32),
        ("switch_qlen", C.c_int32), ("min_delta_dist", C.c_int32), ("max_gap_area", C.c_int32),
        ("padding", C.c_int32), ("bandwidth_ext", C.c_int32), ("min_bandwidth_gap", C.c_int32),
        ("zdrop", C.c_int32), ("sv_penalty", C.c_int32), ("match", C.c_int32), ("mismatch", C.c_int32),
        ("gap", C.c_int32), ("extend", C.c_int32), ("gap2", C.c_int32), ("extend2", C.c_int32),
        ("disable_heuristics", C.c_int32), ("soc_width", C.c_int32), ("srand_seed", C.c_uint32),
        ("genome_size_disable", C.c_uint64), ("rel_min_seed_size_amount", C.c_double),
        ("harm_score_min_rel", C.c_double), ("soc_score_decrease_tol", C.c_double),
        ("score_diff_tol", C.c_double), ("max_delta_dist", C.c_double), ("min_alignment_score", C.c_int32),
        ("report_n_best", C.c_int32), ("max_supplementary", C.c_int32), ("max_overlap_supplementary", C.c_double),
        ("search_inversions", C.c_int32), ("zdrop_inversion", C.c_int32), ("use_paired_reads", C.c_int32), ("libm_probe", C.c_int32),
        ("mean_paired_dist", C.c_double), ("std_paired_dist", C.c_double), ("paired_bonus", C.c_double),
    ]

    @staticmethod
    def preset(name="default"):
        """ParameterSetManager::setSelected (parameter.h:1163-1170): default, illumina, illuminapaired, pacbio, nanopore."""
        p = Params()
        _chk(lib().ma_params_preset(name.encode(), C.byref(p)))
        return p


class BgzfText(C.Structure):
    """ma_bgzf_text: one side of ma_batch_set_mates_bgzf"""
    _fields_ = [("head", C.c_void_p), ("n_head", C.c_uint64), ("members", C.c_void_p), ("n_bytes", C.c_uint64), ("n_drop", C.c_uint64)]


SEGMENT_DT = np.dtype([("q_start", "<i8"), ("q_size", "<i8"), ("sa_start", "<i8"), ("sa_start_rc", "<i8"),
                       ("sa_size", "<i8")])
SEED_DT = np.dtype([("q_start", "<i8"), ("len", "<i8"), ("r_start", "<i8"), ("delta", "<i8"), ("ambiguity", "<u4"),
                    ("on_forward", "<u4")])
EZ_DT = np.dtype([(k, "<i4") for k in ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "score",
                                       "reach_end", "n_cigar")])
ALIGNMENT_DT = np.dtype([("begin_ref", "<i8"), ("end_ref", "<i8"), ("begin_q", "<i8"), ("end_q", "<i8"),
                         ("score", "<i8"), ("soc_index", "<u4"), ("n_ops", "<u4"), ("ops_off", "<u8"),
                         ("secondary", "<u4"), ("supplementary", "<u4"), ("mapq", "<f8")])
SOC_DT = np.dtype([("acc_len", "<u8"), ("ambiguity", "<u4"), ("n_seeds", "<u4"), ("begin", "<u4"), ("end", "<u4")])
KSW_JOB_DT = np.dtype([("qlen", "<i4"), ("tlen", "<i4"), ("w", "<i4"), ("zdrop", "<i4"), ("flag", "<i4"),
                       ("reserved", "<u4"), ("q_off", "<u8"), ("t_off", "<u8")])

_lib = None


def lib():
    """Loads libma_amd.so; fails loudly when the HIP extension was not built."""
    global _lib
    if _lib is None:
        try:
            # PyTorch-ROCm bundles its own HIP runtime; load it first so that libma_amd.so binds to the same
            # one (two runtimes in one process cannot both own the device)
            import torch  # noqa: F401
        except ImportError:
            pass
        p = lib_path()
        if not os.path.exists(p):
            raise MaError("libma_amd.so is missing (%s): run __graft_entry__.build(); there is no CPU fallback" % p)
        _lib = C.CDLL(p)
        _lib.ma_last_error.restype = C.c_char_p
    return _lib


def _chk(rc):
    if rc != 0:
        raise MaError(lib().ma_last_error().decode(errors="replace"))


def _ptr(a, t=C.c_void_p):
    if a is None:
        return None
    return a.ctypes.data_as(t)


SAM_SOFT_CLIP, SAM_EQX_CIGAR, SAM_NO_SECONDARY, SAM_NO_SUPPLEMENTARY, SAM_NO_CG_TAG = 1, 2, 4, 8, 16  # MA_SAM_*
SAM_NGMLR_TAGS = 32  # (Batch.sam only)


def _csr_text(strings):
    """strings (str or bytes) back to back + their offsets (n + 1 u64)"""
    bs = [x.encode() if isinstance(x, str) else bytes(x) for x in strings]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        off[1:] = np.cumsum([len(x) for x in bs])
    return np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8).copy(), off


def debug_ngmlr_floats(kind, num, den):
    """diagnostics (ma_debug_ngmlr_floats): the texts of the XI:f (kind 0: num / den) or CV:f (kind 1: 100 * num / den) tags as
    the device computes and prints them, a list of bytes"""
    num = np.ascontiguousarray(num, dtype=np.uint64)
    den = np.ascontiguousarray(den, dtype=np.uint64)
    if len(num) != len(den):
        raise MaError("debug_ngmlr_floats: %d numerators for %d denominators" % (len(num), len(den)))
    out = np.zeros((len(num), 16), dtype=np.uint8)
    _chk(lib().ma_debug_ngmlr_floats(C.c_int(kind), _ptr(num), _ptr(den), C.c_uint64(len(num)), _ptr(out)))
    return out.view("S16").ravel()


def device_count():
    n = C.c_int(0)
    _chk(lib().ma_device_count(C.byref(n)))
    return n.value


def set_device(d):
    _chk(lib().ma_set_device(C.c_int(d)))


def bind_host_thread(device, mode=0):
    """Pins the calling thread (and the threads it starts later) to the CPUs next to GPU `device` (ma_host_bind_thread); mode 1:
    to the other CPUs, -1: to all again.  Returns the CPUs of the new mask, 0 when it was left alone."""
    n = C.c_int(0)
    _chk(lib().ma_host_bind_thread(C.c_int(device), C.c_int(mode), C.byref(n)))
    return n.value


class HostArray:
    """Page-locked host memory (ma_host_alloc) as a numpy array: uploads from it and downloads into it are DMA transfers
    that run asynchronously on the batch's stream, so the copies of one batch hide behind the kernels of another."""

    def __init__(self, n, dtype):
        self.dtype = np.dtype(dtype)
        self.n = int(n)
        self.p = C.c_void_p()
        nbytes = max(self.n * self.dtype.itemsize, 64)
        _chk(lib().ma_host_alloc(C.c_uint64(nbytes), C.byref(self.p)))
        buf = (C.c_char * nbytes).from_address(self.p.value)
        self.a = np.frombuffer(buf, dtype=self.dtype, count=self.n)

    @property
    def ptr(self):
        return self.p.value

    def close(self):
        if self.p:
            self.a = None
            lib().ma_host_free(self.p)
            self.p = None


class Index:
    """Device-resident FMD-index + pack (ma_index*)."""

    def __init__(self, handle):
        self.h = handle

    @staticmethod
    def from_arrays(bwt, sa, L2, primary, ref_len, pac, contig_starts, contig_lens):
        bwt = np.ascontiguousarray(bwt, dtype=np.uint32)
        sa = np.ascontiguousarray(sa, dtype=np.int64)
        L2 = np.ascontiguousarray(L2, dtype=np.uint64)
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        cs = np.ascontiguousarray(contig_starts, dtype=np.uint64)
        cl = np.ascontiguousarray(contig_lens, dtype=np.uint64)
        h = C.c_void_p()
        _chk(lib().ma_index_create(_ptr(bwt), C.c_uint64(len(bwt)), _ptr(sa), C.c_uint64(len(sa)), _ptr(L2),
                                   C.c_int64(int(primary)), C.c_uint64(int(ref_len)), _ptr(pac), C.c_int32(len(cs)),
                                   _ptr(cs), _ptr(cl), C.byref(h)))
        return Index(h)

    @staticmethod
    def build(contigs):
        """GPU index construction from N-free contigs (list of uint8 code arrays); a FASTA text with N: build_text."""
        lens = np.array([len(c) for c in contigs], dtype=np.uint64)
        cat = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.uint8) for c in contigs]))
        h = C.c_void_p()
        _chk(lib().ma_index_build(C.c_int32(len(lens)), _ptr(lens), _ptr(cat), C.byref(h)))
        return Index(h)

    @staticmethod
    def build_device(contig_lens, d_codes_ptr):
        lens = np.ascontiguousarray(contig_lens, dtype=np.uint64)
        h = C.c_void_p()
        _chk(lib().ma_index_build_device(C.c_int32(len(lens)), _ptr(lens), C.c_void_p(int(d_codes_ptr)), C.byref(h)))
        return Index(h)

    @staticmethod
    def build_text(data, seed=1):
        """GPU index construction from a whole FASTA text held as bytes, holes (N and the other IUPAC letters) included: Genome
        reads the text on the device, build_index fills the hole bases with the draws of srand(seed) and sets the index's contig
        names and holes."""
        data = bytes(data)
        g = Genome(max(len(data), 1))
        try:
            g.append_text(data, end_of_file=True)
            return g.build_index(seed)
        finally:
            g.close()

    def sizes(self):
        nw, ns, rl, nc = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int32()
        _chk(lib().ma_index_sizes(self.h, C.byref(nw), C.byref(ns), C.byref(rl), C.byref(nc)))
        return nw.value, ns.value, rl.value, nc.value

    def download(self):
        nw, ns, rl, nc = self.sizes()
        bwt = np.empty(nw, dtype=np.uint32)
        sa = np.empty(ns, dtype=np.int64)
        L2 = np.zeros(5, dtype=np.uint64)
        primary = C.c_int64()
        pac = np.empty((rl // 2 + 3) // 4, dtype=np.uint8)
        cs = np.empty(nc, dtype=np.uint64)
        cl = np.empty(nc, dtype=np.uint64)
        _chk(lib().ma_index_download(self.h, _ptr(bwt), _ptr(sa), _ptr(L2), C.byref(primary), _ptr(pac), _ptr(cs),
                                     _ptr(cl)))
        return dict(bwt=bwt, sa=sa, L2=L2, primary=primary.value, ref_len=rl, pac=pac, contig_starts=cs,
                    contig_lens=cl)

    def store(self, prefix, names=None, title=None):
        """Write the index as the reference's <prefix>.bwt/.sa/.pac/.ann/.amb files (FMIndex::vStoreFMIndex
        fMIndex.h:515-549, Pack::vStoreCollection pack.h:230-269,725-770; same layout as storeIndex of the C++ host
        layer): maCMD / FMIndex(prefix) load an index that was built on the GPU."""
        if title:  # the genome file `maCMD -x` takes (execution-context.h:60-136)
            import json as _json
            import os as _os
            with open(_os.path.join(_os.path.dirname(prefix), title + ".json"), "w") as f:
                f.write(_json.dumps({"name": title, "prefix": _os.path.basename(prefix), "type": "MA Genome",
                                     "version": {"major": 1, "minor": 0}}, indent=4, sort_keys=True) + "\n")
        d = self.download()
        n = int(d["ref_len"])
        F = n // 2
        with open(prefix + ".bwt", "wb") as f:
            f.write(np.int64(d["primary"]).tobytes())
            f.write(np.ascontiguousarray(d["L2"][1:5], dtype=np.uint64).tobytes())
            d["bwt"].tofile(f)
        with open(prefix + ".sa", "wb") as f:
            f.write(np.int64(d["primary"]).tobytes())
            f.write(np.ascontiguousarray(d["L2"][1:5], dtype=np.uint64).tobytes())
            f.write(np.int32(32).tobytes())
            f.write(np.uint64(n).tobytes())
            d["sa"][1:].tofile(f)
        with open(prefix + ".pac", "wb") as f:
            d["pac"][:(F + 3) // 4].tofile(f)
            if F % 4 == 0:
                f.write(b"\0")
            f.write(bytes([F % 4]))
        nc = len(d["contig_starts"])
        with open(prefix + ".ann", "w") as f:
            f.write("%d %d 0\n" % (F, nc))
            for i in range(nc):
                f.write("0 %s none\n%d %d 0\n" % (names[i] if names else "chr%d" % (i + 1), int(d["contig_starts"][i]),
                                                  int(d["contig_lens"][i])))
        with open(prefix + ".amb", "w") as f:
            f.write("%d %d 0\n" % (F, nc))

    def extract(self, begin, end):
        """Pack::vExtract for ranges [begin[i], end[i]) of the doubled text: list of uint8 code arrays."""
        b = np.ascontiguousarray(begin, dtype=np.uint64)
        e = np.ascontiguousarray(end, dtype=np.uint64)
        n = np.where(e > b, e - b, 0)
        out = np.empty(int(n.sum()) + 1, dtype=np.uint8)
        _chk(lib().ma_pack_extract(self.h, _ptr(b), _ptr(e), C.c_uint64(len(b)), _ptr(out)))
        cuts = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        return [out[cuts[i]:cuts[i + 1]] for i in range(len(b))]

    def extend_backward(self, ik, c):
        ik = np.ascontiguousarray(ik, dtype=np.int64).reshape(-1, 3)
        c = np.ascontiguousarray(c, dtype=np.uint8)
        ok = np.empty_like(ik)
        _chk(lib().ma_extend_backward_batch(self.h, _ptr(ik), _ptr(c), C.c_uint64(len(c)), _ptr(ok)))
        return ok

    def bwt_sa(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        pos = np.empty_like(rows)
        _chk(lib().ma_bwt_sa_batch(self.h, _ptr(rows), C.c_uint64(len(rows)), _ptr(pos)))
        return pos

    def set_contig_names(self, names):
        """The RNAME strings of the SAM text (ma_index_set_contig_names): one str / bytes per contig."""
        cat, off = _csr_text(names)
        _chk(lib().ma_index_set_contig_names(self.h, _ptr(cat), _ptr(off)))

    def set_holes(self, starts, lens):
        """The runs of N of the forward strand that random bases replaced (ma_index_set_holes), read by the NM and SV tags of
        Batch.sam(SAM_NGMLR_TAGS | ...): sorted, not overlapping; setting again replaces the list."""
        st = np.ascontiguousarray(starts, dtype=np.uint64)
        ln = np.ascontiguousarray(lens, dtype=np.uint64)
        if len(st) != len(ln):
            raise MaError("set_holes: %d starts for %d lengths" % (len(st), len(ln)))
        _chk(lib().ma_index_set_holes(self.h, _ptr(st), _ptr(ln), C.c_uint64(len(st))))

    def close(self):
        if self.h:
            lib().ma_index_destroy(self.h)
            self.h = None


class Genome:
    """A genome being read from FASTA text on the device (ma_genome*): codes of 1 byte per base on the device (hole bases -- N and
    every letter that is not A C G T -- as 4 until build_index fills them), the contig table and the holes."""

    def __init__(self, max_bases, device=None):
        self.h = C.c_void_p()
        _chk(lib().ma_genome_create(C.c_int(-1 if device is None else int(device)), C.c_uint64(int(max_bases)), C.byref(self.h)))

    def append_text(self, data, end_of_file=False):
        """Appends the whole lines of a chunk of the file (bytes); returns how many bytes were consumed -- up to and including the
        chunk's last line feed, or all of them with end_of_file.  The caller carries the rest into its next call.  A refusal
        (MaError) leaves the genome as it was."""
        data = bytes(data)
        buf = np.frombuffer(data + b"\0", dtype=np.uint8)
        consumed = C.c_uint64(0)
        _chk(lib().ma_genome_append_text(self.h, _ptr(buf), C.c_uint64(len(data)), C.c_int32(1 if end_of_file else 0), C.byref(consumed)))
        return consumed.value

    def counts(self):
        v = [C.c_uint64() for _ in range(5)]
        _chk(lib().ma_genome_counts(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("contigs", "bases", "name_bytes", "holes", "hole_bases"), (x.value for x in v)))

    def contigs(self):
        """dict: names (list of bytes), starts, lens, n_holes (uint64 arrays)"""
        c = self.counts()
        nc = c["contigs"]
        off = np.zeros(nc + 1, dtype=np.uint64)
        names = np.zeros(c["name_bytes"] + 1, dtype=np.uint8)
        starts, lens, nh = (np.zeros(nc, dtype=np.uint64) for _ in range(3))
        _chk(lib().ma_genome_get_contigs(self.h, _ptr(off), _ptr(names), _ptr(starts), _ptr(lens), _ptr(nh)))
        raw = names.tobytes()
        return dict(names=[raw[int(off[i]):int(off[i + 1])] for i in range(nc)], starts=starts, lens=lens, n_holes=nh)

    def holes(self):
        """(starts, lens): the runs of hole bases, each inside one contig, in text order"""
        n = self.counts()["holes"]
        st, ln = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        _chk(lib().ma_genome_get_holes(self.h, _ptr(st), _ptr(ln)))
        return st, ln

    def codes(self, start=0, n=None):
        """codes [start, start + n) of the genome (uint8; 4 = a hole base not filled yet)"""
        if n is None:
            n = self.counts()["bases"] - start
        out = np.zeros(max(int(n), 1), dtype=np.uint8)
        _chk(lib().ma_genome_get_codes(self.h, C.c_uint64(int(start)), C.c_uint64(int(n)), _ptr(out)))
        return out[:int(n)]

    def build_index(self, seed=1):
        """Fills the hole bases (the k-th becomes rand() & 3 of the k-th draw after srand(seed)) and builds the index, contig names
        and holes set.  Once per genome."""
        h = C.c_void_p()
        _chk(lib().ma_genome_build_index(self.h, C.c_uint32(int(seed) & 0xffffffff), C.byref(h)))
        return Index(h)

    def close(self):
        if self.h:
            lib().ma_genome_destroy(self.h)
            self.h = None


def ksw_batch(params, cases, cigar_cap=None, pipeline_semantics=False):
    """cases: list of (q, t, w, zdrop, flag) -> (ez structured array, list of cigar arrays).
    pipeline_semantics: ma_ksw_ext_batch (only max, max_q, max_t, cigar defined)."""
    n = len(cases)
    jobs = np.zeros(n, dtype=KSW_JOB_DT)
    qs, ts = [], []
    qo = to = 0
    for i, (q, t, w, zd, fl) in enumerate(cases):
        jobs[i] = (len(q), len(t), w, zd, fl, 0, qo, to)
        qs.append(np.asarray(q, dtype=np.uint8))
        ts.append(np.asarray(t, dtype=np.uint8))
        qo += len(q)
        to += len(t)
    qb = np.ascontiguousarray(np.concatenate(qs + [np.zeros(1, dtype=np.uint8)]))
    tb = np.ascontiguousarray(np.concatenate(ts + [np.zeros(1, dtype=np.uint8)]))
    if cigar_cap is None:
        cigar_cap = qo + to + 2 * n + 16
    ez = np.zeros(n, dtype=EZ_DT)
    off = np.zeros(n + 1, dtype=np.uint64)
    cig = np.zeros(cigar_cap, dtype=np.uint32)
    fn = lib().ma_ksw_ext_batch if pipeline_semantics else lib().ma_ksw_batch
    _chk(fn(C.byref(params), _ptr(jobs), C.c_uint64(n), _ptr(qb), C.c_uint64(len(qb)), _ptr(tb),
            C.c_uint64(len(tb)), _ptr(ez), _ptr(off), _ptr(cig), C.c_uint64(cigar_cap)))
    cigs = [cig[int(off[i]):int(off[i]) + int(ez["n_cigar"][i])].copy() for i in range(n)]
    return ez, cigs


def bgzf_deflate(index, data):
    """(member_off, bytes): data (any bytes) deflated on index's device into BGZF members of 65 280 bytes of text each
    (ma_bgzf_deflate: the kernels of Batch.sam_bgzf); member k is bytes[member_off[k]:member_off[k + 1]].  The bytes followed by
    the 28-byte end-of-file marker are a file gzip reads."""
    buf = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
    nm, nb = C.c_uint64(), C.c_uint64()
    _chk(lib().ma_bgzf_deflate(index.h, _ptr(buf), C.c_uint64(len(buf) - 1), C.byref(nm), C.byref(nb), None, None, C.c_uint64(0)))
    off = np.zeros(nm.value + 1, dtype=np.uint64)
    out = np.zeros(nb.value + 1, dtype=np.uint8)
    _chk(lib().ma_bgzf_deflate(index.h, _ptr(buf), C.c_uint64(len(buf) - 1), C.byref(nm), C.byref(nb), _ptr(off), _ptr(out),
                               C.c_uint64(nb.value)))
    return off, out[:-1].tobytes()


class Batch:
    """Device-resident batch of reads and stage outputs (ma_batch*)."""

    def __init__(self, index, params, max_reads, max_bases):
        self.index = index
        self.params = params
        self.h = C.c_void_p()
        _chk(lib().ma_batch_create(index.h, C.byref(params), C.c_uint64(max_reads), C.c_uint64(max_bases),
                                   C.byref(self.h)))
        self.n = 0
        self.read_off, self.n_bases = np.zeros(1, dtype=np.uint64), 0  # CSR offsets of the reads that are set (set_read_text)

    def set_stream(self, stream_ptr):
        _chk(lib().ma_batch_set_stream(self.h, C.c_void_p(int(stream_ptr))))

    def set_blocking_sync(self, on=True):
        """waits of this batch sleep on an interrupt-driven event instead of spinning (hosts with more waiting threads than cores)"""
        _chk(lib().ma_batch_set_blocking_sync(self.h, C.c_int(1 if on else 0)))

    def enable_timing(self, on=True):
        _chk(lib().ma_batch_enable_timing(self.h, C.c_int(1 if on else 0)))

    def set_reads(self, reads):
        """reads: list of uint8 code arrays"""
        off = np.zeros(len(reads) + 1, dtype=np.uint64)
        if len(reads):
            off[1:] = np.cumsum([len(r) for r in reads])
            cat = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads]
                                                      + [np.zeros(1, dtype=np.uint8)]))
        else:
            cat = np.zeros(1, dtype=np.uint8)
        _chk(lib().ma_batch_set_reads(self.h, _ptr(cat), _ptr(off), C.c_uint64(len(reads))))
        self.n = len(reads)
        self.read_off, self.n_bases = off, int(off[-1])

    def set_reads_flat(self, codes_ptr, offsets_ptr, n_reads):
        """reads that already are one host array of codes + CSR offsets (n + 1 u64, starting at 0), e.g. in page-locked memory"""
        _chk(lib().ma_batch_set_reads(self.h, C.c_void_p(int(codes_ptr)), C.c_void_p(int(offsets_ptr)), C.c_uint64(n_reads)))
        self.n = n_reads
        self.read_off = np.ctypeslib.as_array((C.c_uint64 * (n_reads + 1)).from_address(int(offsets_ptr))).copy()
        self.n_bases = int(self.read_off[-1])

    def set_reads_device(self, d_codes_ptr, d_offsets_ptr, n_reads, n_bases):
        _chk(lib().ma_batch_set_reads_device(self.h, C.c_void_p(int(d_codes_ptr)), C.c_void_p(int(d_offsets_ptr)),
                                             C.c_uint64(n_reads), C.c_uint64(n_bases)))
        self.n = n_reads
        self.read_off, self.n_bases = None, int(n_bases)  # (the offsets live on the device)

    # ---- read text in (ma_batch_set_reads_text): a FASTQ / FASTA text parsed on the device
    def set_reads_text(self, text):
        """text: bytes of a FASTQ or FASTA text in the strict form (include/ma_amd.h).  Uploads and parses it on the device; the
        batch then is as after set_reads() + set_read_text().  Returns the number of reads.  A refused text raises MaError with
        "line <L> (byte <X>): <reason>" and leaves the batch without reads."""
        buf = np.frombuffer(bytes(text) + b"\0", dtype=np.uint8)
        n = C.c_uint64()
        self.n, self.read_off, self.n_bases = 0, np.zeros(1, dtype=np.uint64), 0
        _chk(lib().ma_batch_set_reads_text(self.h, _ptr(buf), C.c_uint64(len(buf) - 1), C.byref(n)))
        self.n = int(n.value)
        self.read_off, _ = self.reads(codes=False)
        self.n_bases = int(self.read_off[-1])
        return self.n

    def set_reads_bgzf(self, members, head=b"", drop=0):
        """members: bytes of whole BGZF members (what bgzip writes; the strict form of include/ma_amd.h).  The text is head
        followed by what the members inflate to, minus its last drop bytes; the device inflates the members, one per lane, and
        parses the text as set_reads_text() does.  Returns the number of reads.  A refusal raises MaError -- "member <k> (byte
        <X>): <reason>" or "text: line <L> (byte <X>): <reason>" -- and leaves the batch without reads; after "batch capacity
        exceeded" the exception's n_reads is the number of reads the text holds."""
        data = np.frombuffer(bytes(members) + b"\0", dtype=np.uint8)
        front = np.frombuffer(bytes(head) + b"\0", dtype=np.uint8)
        n = C.c_uint64()
        self.n, self.read_off, self.n_bases = 0, np.zeros(1, dtype=np.uint64), 0
        try:
            _chk(lib().ma_batch_set_reads_bgzf(self.h, _ptr(front), C.c_uint64(len(front) - 1), _ptr(data), C.c_uint64(len(data) - 1),
                                               C.c_uint64(drop), C.byref(n)))
        except MaError as e:
            e.n_reads = int(n.value)
            raise
        self.n = int(n.value)
        self.read_off, _ = self.reads(codes=False)
        self.n_bases = int(self.read_off[-1])
        return self.n

    def set_mates_text(self, text1, text2, rev_comp=True):
        """text1, text2: bytes of the two read files of a paired-end run (or runs of whole records of them), both FASTQ or both
        FASTA in the strict form (ma_batch_set_mates_text).  Record k of text1 becomes read 2k, record k of text2 read 2k + 1,
        reversed and complemented with rev_comp; the shorter text ends the stream.  The batch then is as after set_reads() on the
        interleaved reads + set_read_text().  Returns (n_pairs, (consumed1, consumed2)): the offsets at which the next call goes
        on.  A refusal raises MaError and leaves the batch without reads; after "batch capacity exceeded" the exception's n_pairs
        is the number of pairs the texts hold."""
        bufs = [np.frombuffer(bytes(t) + b"\0", dtype=np.uint8) for t in (text1, text2)]
        n, consumed = C.c_uint64(), (C.c_uint64 * 2)()
        self.n, self.read_off, self.n_bases = 0, np.zeros(1, dtype=np.uint64), 0
        try:
            _chk(lib().ma_batch_set_mates_text(self.h, _ptr(bufs[0]), C.c_uint64(len(bufs[0]) - 1), _ptr(bufs[1]), C.c_uint64(len(bufs[1]) - 1),
                                               C.c_int32(1 if rev_comp else 0), C.byref(n), consumed))
        except MaError as e:
            e.n_pairs = int(n.value)
            raise
        self.n = 2 * int(n.value)
        self.read_off, _ = self.reads(codes=False)
        self.n_bases = int(self.read_off[-1])
        return int(n.value), (int(consumed[0]), int(consumed[1]))

    def set_mates_bgzf(self, members1, members2, heads=(b"", b""), drops=(0, 0), rev_comp=True):
        """members1, members2: bytes of whole BGZF members of the two read files of a paired-end run.  Text i is heads[i] followed
        by what its members inflate to, minus its last drops[i] bytes; both chains are inflated by one launch on the device and the
        texts paired as set_mates_text() pairs them (ma_batch_set_mates_bgzf).  Returns (n_pairs, (consumed1, consumed2),
        (text_bytes1, text_bytes2)); mates_rest() serves what of each text lies beyond the last pair.  A refusal raises MaError
        and leaves the batch without reads; after "batch capacity exceeded" the exception's n_pairs is the number of pairs the
        texts hold."""
        bufs = [np.frombuffer(bytes(x) + b"\0", dtype=np.uint8) for x in (heads[0], members1, heads[1], members2)]
        sides = (BgzfText * 2)()
        for i in range(2):
            sides[i].head, sides[i].n_head = bufs[2 * i].ctypes.data, len(bufs[2 * i]) - 1
            sides[i].members, sides[i].n_bytes = bufs[2 * i + 1].ctypes.data, len(bufs[2 * i + 1]) - 1
            sides[i].n_drop = int(drops[i])
        n, consumed, size = C.c_uint64(), (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
        self.n, self.read_off, self.n_bases = 0, np.zeros(1, dtype=np.uint64), 0
        try:
            _chk(lib().ma_batch_set_mates_bgzf(self.h, sides, C.c_int32(1 if rev_comp else 0), C.byref(n), size, consumed))
        except MaError as e:
            e.n_pairs = int(n.value)
            raise
        self.n = 2 * int(n.value)
        self.read_off, _ = self.reads(codes=False)
        self.n_bases = int(self.read_off[-1])
        return int(n.value), (int(consumed[0]), int(consumed[1])), (int(size[0]), int(size[1]))

    def mates_rest(self):
        """(rest1, rest2): the bytes of each text of the last set_mates_bgzf() behind its last paired record
        (ma_batch_get_mates_rest); raises MaError once the batch has other reads, or none"""
        out = []
        for which in range(2):
            n = C.c_uint64()
            _chk(lib().ma_batch_get_mates_rest(self.h, C.c_int32(which), C.byref(n), None))
            buf = np.zeros(n.value + 1, dtype=np.uint8)
            _chk(lib().ma_batch_get_mates_rest(self.h, C.c_int32(which), C.byref(n), _ptr(buf)))
            out.append(buf[:-1].tobytes())
        return tuple(out)

    def read_counts(self):
        v = [C.c_uint64() for _ in range(3)]
        q = C.c_int32()
        _chk(lib().ma_batch_read_counts(self.h, *[C.byref(x) for x in v], C.byref(q)))
        return dict(zip(("reads", "bases", "name_bytes", "has_qual"), [x.value for x in v] + [q.value]))

    def reads(self, codes=True):
        """(offsets, codes) of the batch's reads, however they were set: read r is codes[offsets[r]:offsets[r + 1]]."""
        c = self.read_counts()
        off = np.zeros(c["reads"] + 1, dtype=np.uint64)
        cod = np.zeros(c["bases"] + 1, dtype=np.uint8) if codes else None
        _chk(lib().ma_batch_get_reads(self.h, _ptr(off), _ptr(cod)))
        return off, (cod[:-1] if codes else None)

    def read_text(self):
        """(names, quals): one bytes object per read; quals None when the reads have no qualities.  Fails when no text was set."""
        c = self.read_counts()
        noff = np.zeros(c["reads"] + 1, dtype=np.uint64)
        names = np.zeros(c["name_bytes"] + 1, dtype=np.uint8)
        qual = np.zeros(c["bases"] + 1, dtype=np.uint8) if c["has_qual"] else None
        _chk(lib().ma_batch_get_read_text(self.h, _ptr(noff), _ptr(names), _ptr(qual)))
        nb = names.tobytes()
        out = [nb[int(noff[r]):int(noff[r + 1])] for r in range(c["reads"])]
        if qual is None:
            return out, None
        off, _ = self.reads(codes=False)
        qb = qual.tobytes()
        return out, [qb[int(off[r]):int(off[r + 1])] for r in range(c["reads"])]

    def seed(self):
        _chk(lib().ma_seed_batch(self.h))

    def extract(self):
        _chk(lib().ma_extract_seeds_batch(self.h))

    def chain(self):
        _chk(lib().ma_chain_batch(self.h))

    def dp(self):
        _chk(lib().ma_dp_batch(self.h))

    def align(self):
        _chk(lib().ma_align_batch(self.h))

    def sync(self):
        _chk(lib().ma_batch_sync(self.h))

    def counts(self):
        v = [C.c_uint64() for _ in range(7)]
        _chk(lib().ma_batch_counts(self.h, *[C.byref(x) for x in v]))
        keys = ("segments", "seeds", "hsets", "hseeds", "alignments", "ops_cap", "aligned_reads")
        return dict(zip(keys, [x.value for x in v]))

    def counters(self):
        out = np.zeros(8, dtype=np.uint64)
        _chk(lib().ma_batch_counters(self.h, _ptr(out)))
        return out

    def dp_jobs(self):
        """(n, 8) int32: qlen, tlen, w, zdrop, flag, zdropped, max_q, max_t of every kswcpp call of the last dp stage."""
        n = C.c_uint64()
        _chk(lib().ma_batch_get_dp_jobs(self.h, C.byref(n), None, C.c_uint64(0)))
        out = np.zeros((int(n.value), 8), dtype=np.int32)
        if n.value:
            _chk(lib().ma_batch_get_dp_jobs(self.h, C.byref(n), _ptr(out), C.c_uint64(n.value)))
        return out

    def kernel_ms(self):
        out = np.zeros(8, dtype=np.float32)
        _chk(lib().ma_batch_kernel_ms(self.h, _ptr(out)))
        return out

    def segments(self):
        c = self.counts()
        off = np.zeros(self.n + 1, dtype=np.uint64)
        segs = np.zeros(c["segments"], dtype=SEGMENT_DT)
        _chk(lib().ma_batch_get_segments(self.h, _ptr(off), _ptr(segs)))
        return off, segs

    def seeds(self):
        c = self.counts()
        off = np.zeros(self.n + 1, dtype=np.uint64)
        seeds = np.zeros(c["seeds"], dtype=SEED_DT)
        _chk(lib().ma_batch_get_seeds(self.h, _ptr(off), _ptr(seeds)))
        return off, seeds

    def hsets(self):
        c = self.counts()
        hoff = np.zeros(self.n + 1, dtype=np.uint64)
        soff = np.zeros(c["hsets"] + 1, dtype=np.uint64)
        soc = np.zeros(c["hsets"], dtype=np.uint32)
        seeds = np.zeros(c["hseeds"], dtype=SEED_DT)
        _chk(lib().ma_batch_get_hsets(self.h, _ptr(hoff), _ptr(soff), _ptr(soc), _ptr(seeds)))
        return hoff, soff, soc, seeds[: int(soff[-1])]

    def set_segments(self, off, segs):
        """Segments from elsewhere (CSR per read, the layout of segments()) -> extract().  ma_batch_set_segments checks them on
        the host and raises MaError("ma_batch_set_segments: ...") for a decreasing offset array, a negative field, an empty
        interval, rows outside 1 .. n or a segment beyond its read; the batch then holds no segments and stays usable."""
        off = np.ascontiguousarray(off, dtype=np.uint64)
        segs = np.ascontiguousarray(np.concatenate([segs, np.zeros(1, dtype=SEGMENT_DT)]))
        _chk(lib().ma_batch_set_segments(self.h, _ptr(off), _ptr(segs)))

    def set_seeds(self, off, seeds):
        """Extracted seeds from elsewhere (CSR per read, the layout of seeds(): reverse-strand seeds mirrored onto forward
        positions) -> chain().  ma_batch_set_seeds checks them on the host and raises MaError("ma_batch_set_seeds: ...") for a
        decreasing offset array, a negative field, an empty seed, a seed beyond its read or the doubled text, an on_forward other
        than 0 / 1, an r_start outside the forward text or a delta that is not ExtractSeeds'; the batch then holds no seeds and
        stays usable."""
        off = np.ascontiguousarray(off, dtype=np.uint64)
        seeds = np.ascontiguousarray(np.concatenate([seeds, np.zeros(1, dtype=SEED_DT)]))
        _chk(lib().ma_batch_set_seeds(self.h, _ptr(off), _ptr(seeds)))

    def set_hsets(self, hset_off, hseed_off, hset_soc, seeds):
        """Harmonized sets from elsewhere (the layout of hsets()) -> dp().  ma_batch_set_hsets checks them on the host and
        raises MaError("ma_batch_set_hsets: ...") for a seed beyond its read or the text, a negative field or a decreasing
        offset array; the batch then holds no sets and stays usable."""
        hset_off = np.ascontiguousarray(hset_off, dtype=np.uint64)
        hseed_off = np.ascontiguousarray(np.concatenate([np.asarray(hseed_off, dtype=np.uint64), np.zeros(1, dtype=np.uint64)]))
        hset_soc = np.ascontiguousarray(np.concatenate([np.asarray(hset_soc, dtype=np.uint32), np.zeros(1, dtype=np.uint32)]))
        seeds = np.ascontiguousarray(np.concatenate([np.asarray(seeds, dtype=SEED_DT), np.zeros(1, dtype=SEED_DT)]))
        _chk(lib().ma_batch_set_hsets(self.h, _ptr(hset_off), _ptr(hseed_off), _ptr(hset_soc), _ptr(seeds)))

    def socs(self, heap=False):
        """The SoC queue of every read: strips in pop order, or (heap=True) the queue's array as the sweep leaves it;
        returns (soc_off, socs, seed_off, seeds re-sorted by reference position)."""
        fn = lib().ma_batch_get_soc_heap if heap else lib().ma_batch_get_socs
        n = C.c_uint64()
        _chk(fn(self.h, C.byref(n), None, None, None, None))
        c = self.counts()
        soff = np.zeros(self.n + 1, dtype=np.uint64)
        socs = np.zeros(int(n.value) + 1, dtype=SOC_DT)
        doff = np.zeros(self.n + 1, dtype=np.uint64)
        seeds = np.zeros(c["seeds"] + 1, dtype=SEED_DT)
        _chk(fn(self.h, C.byref(n), _ptr(soff), _ptr(socs), _ptr(doff), _ptr(seeds)))
        return soff, socs[: int(n.value)], doff, seeds[: c["seeds"]]

    def set_soc_heap(self, soc_off, socs, seed_off, seeds):
        """SoC queues swept elsewhere (layout of socs(heap=True)) -> chain() only harmonizes.  The seeds are held to the contract
        of set_seeds, the strips to begin <= end <= the read's seed count and n_seeds == end - begin: MaError("ma_batch_set_soc_heap:
        ...") otherwise, and the batch then holds no seeds and no strips."""
        soc_off = np.ascontiguousarray(soc_off, dtype=np.uint64)
        seed_off = np.ascontiguousarray(seed_off, dtype=np.uint64)
        socs = np.ascontiguousarray(np.concatenate([socs, np.zeros(1, dtype=SOC_DT)]))
        seeds = np.ascontiguousarray(np.concatenate([seeds, np.zeros(1, dtype=SEED_DT)]))
        _chk(lib().ma_batch_set_soc_heap(self.h, _ptr(soc_off), _ptr(socs), _ptr(seed_off), _ptr(seeds)))

    def set_alignments(self, off, alns, ops):
        """Alignments computed elsewhere (NeedlemanWunsch order) -> the MappingQuality kernel alone."""
        off = np.ascontiguousarray(off, dtype=np.uint64)
        alns = np.ascontiguousarray(np.concatenate([alns, np.zeros(1, dtype=ALIGNMENT_DT)]))
        ops = np.ascontiguousarray(np.concatenate([np.asarray(ops, dtype=np.uint64), np.zeros(2, dtype=np.uint64)]))
        _chk(lib().ma_batch_set_alignments(self.h, _ptr(off), _ptr(alns), _ptr(ops)))

    def _alns(self, fn):
        c = self.counts()
        off = np.zeros(self.n + 1, dtype=np.uint64)
        alns = np.zeros(c["alignments"], dtype=ALIGNMENT_DT)
        ops = np.zeros(2 * c["ops_cap"] + 2, dtype=np.uint64)
        _chk(fn(self.h, _ptr(off), _ptr(alns), _ptr(ops)))
        return off, alns[: int(off[-1])], ops

    def alignments(self):
        return self._alns(lib().ma_batch_get_alignments)

    def mapq_alignments(self):
        return self._alns(lib().ma_batch_get_mapq_alignments)

    def mapq_alignments_into(self, off, alns, ops):
        """The MappingQuality records into caller-owned host arrays (HostArray: u64[n + 1], ALIGNMENT_DT[>= alignments],
        u64[>= 2 * ops_cap + 2]); returns None when they are too small (the caller grows them), else the counts."""
        c = self.counts()
        if off.n < self.n + 1 or alns.n < c["alignments"] + 1 or ops.n < 2 * c["ops_cap"] + 2:
            return None
        _chk(lib().ma_batch_get_mapq_alignments(self.h, C.c_void_p(off.ptr), C.c_void_p(alns.ptr), C.c_void_p(ops.ptr)))
        return c

    # ---- double-buffered I/O (ma_batch_stage_reads ...): upload of the next reads and download of the last results beside the kernels
    def stage_reads_flat(self, codes_ptr, offsets_ptr, n_reads):
        _chk(lib().ma_batch_stage_reads(self.h, C.c_void_p(int(codes_ptr)), C.c_void_p(int(offsets_ptr)), C.c_uint64(n_reads)))
        self._staged_n = n_reads
        self._staged_off = np.ctypeslib.as_array((C.c_uint64 * (n_reads + 1)).from_address(int(offsets_ptr))).copy()

    def use_staged_reads(self):
        _chk(lib().ma_batch_use_staged_reads(self.h))
        self.n = self._staged_n
        self.read_off, self.n_bases = self._staged_off, int(self._staged_off[-1])

    def start_mapq_download(self, off, alns, ops):
        """mapq_alignments_into without the wait: returns None when the arrays are too small, else the counts; the arrays are
        complete after finish_download()."""
        c = self.counts()
        if off.n < self.n + 1 or alns.n < c["alignments"] + 1 or ops.n < 2 * c["ops_cap"] + 2:
            return None
        _chk(lib().ma_batch_start_mapq_download(self.h, C.c_void_p(off.ptr), C.c_void_p(alns.ptr), C.c_void_p(ops.ptr)))
        return c

    def finish_download(self):
        _chk(lib().ma_batch_finish_download(self.h))

    # ---- small inversions (ma_inversions_batch)
    def inversions(self):
        """SmallInversions::execute for every read on the device, after align() / dp() / set_alignments(): mapq_alignments(),
        pair(), sam() and pair_sam() then serve the lists with the inversion records behind their parents."""
        _chk(lib().ma_inversions_batch(self.h))

    def inversion_counts(self):
        v = [C.c_uint64() for _ in range(3)]
        _chk(lib().ma_batch_inversion_counts(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("candidates", "jobs", "records"), [x.value for x in v]))

    # ---- paired reads (ma_pair_batch): reads 2k and 2k+1 of the batch are the mates of pair k
    def pair(self):
        """PairedReads::execute for every pair on the device, after align() / dp()."""
        _chk(lib().ma_pair_batch(self.h))

    def pair_counts(self):
        v = [C.c_uint64() for _ in range(4)]
        _chk(lib().ma_batch_pair_counts(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("pairs", "records", "ops", "host_pairs"), [x.value for x in v]))

    def pairs(self):
        """(pair_off, alns, ops, mate, other): pair k's records are alns[pair_off[k]:pair_off[k + 1]] (ALIGNMENT_DT, ops as
        (type, length) pairs from ops_off on); mate 1 = record of the first mate, other = index of the partner's record
        within the pair or -1."""
        c = self.pair_counts()
        off = np.zeros(c["pairs"] + 1, dtype=np.uint64)
        alns = np.zeros(c["records"], dtype=ALIGNMENT_DT)
        ops = np.zeros(2 * c["ops"] + 2, dtype=np.uint64)
        mate = np.zeros(c["records"], dtype=np.int32)
        other = np.zeros(c["records"], dtype=np.int32)
        _chk(lib().ma_batch_get_pairs(self.h, _ptr(off), _ptr(alns), _ptr(ops), _ptr(mate), _ptr(other)))
        return off, alns, ops, mate, other

    def start_pair_download(self, off, alns, ops, mate, other):
        """pairs() into caller-owned HostArrays (u64[pairs + 1], ALIGNMENT_DT[records], u64[2 * ops], i32[records] twice)
        without the wait: None when they are too small, else pair_counts(); complete after finish_download()."""
        c = self.pair_counts()
        if (off.n < c["pairs"] + 1 or alns.n < c["records"] or ops.n < 2 * c["ops"] or mate.n < c["records"]
                or other.n < c["records"]):
            return None
        _chk(lib().ma_batch_start_pair_download(self.h, C.c_void_p(off.ptr), C.c_void_p(alns.ptr), C.c_void_p(ops.ptr),
                                                C.c_void_p(mate.ptr), C.c_void_p(other.ptr)))
        return c

    # ---- SAM text (ma_sam_batch): the single-end records of the batch formatted on the device
    def set_read_text(self, names, quals=None):
        """QNAME and QUAL of the reads that were set (ma_batch_set_read_text): one str / bytes per read; quals None (QUAL "*")
        or one quality string per read, as long as the read."""
        if len(names) != self.n:
            raise MaError("set_read_text: %d names for %d reads" % (len(names), self.n))
        cat, off = _csr_text(names)
        q = None
        if quals is not None:
            if len(quals) != self.n:
                raise MaError("set_read_text: %d quality strings for %d reads" % (len(quals), self.n))
            q, qoff = _csr_text(quals)
            # the library copies one character per base: every quality string has to be as long as its read
            if self.read_off is None and int(qoff[-1]) != self.n_bases:
                raise MaError("set_read_text: %d quality characters for %d bases" % (int(qoff[-1]), self.n_bases))
            if self.read_off is not None and not np.array_equal(qoff, self.read_off):
                bad = int(np.flatnonzero(np.diff(qoff.astype(np.int64)) != np.diff(self.read_off.astype(np.int64)))[0])
                raise MaError("set_read_text: quality string %d has %d characters, its read %d bases" % (
                    bad, int(qoff[bad + 1] - qoff[bad]), int(self.read_off[bad + 1] - self.read_off[bad])))
        _chk(lib().ma_batch_set_read_text(self.h, _ptr(cat), _ptr(off), _ptr(q)))

    def sam(self, options=0):
        """FileWriter::execute for every read on the device, after align() / dp() / set_alignments(); options = SAM_* bits,
        SAM_NGMLR_TAGS (the NGMLR tag emulation; the runs of N come from Index.set_holes) among them.  Returns the bytes of
        the text."""
        _chk(lib().ma_sam_batch(self.h, C.c_uint32(options)))
        return self.sam_bytes()

    def sam_bytes(self):
        n = C.c_uint64()
        _chk(lib().ma_batch_sam_counts(self.h, C.byref(n)))
        return n.value

    def sam_text(self):
        """(rec_off, text): read r's records are text[rec_off[r]:rec_off[r + 1]] (bytes)."""
        off = np.zeros(self.n + 1, dtype=np.uint64)
        text = np.zeros(self.sam_bytes() + 1, dtype=np.uint8)
        _chk(lib().ma_batch_get_sam(self.h, _ptr(off), _ptr(text)))
        return off, text[:-1].tobytes()

    def start_sam_download(self, off, text):
        """sam_text() into caller-owned HostArrays (u64[n + 1], u8[bytes]) without the wait: None when they are too small, else
        the bytes of the text; complete after finish_download()."""
        nb = self.sam_bytes()
        if off.n < self.n + 1 or text.n < nb:
            return None
        _chk(lib().ma_batch_start_sam_download(self.h, C.c_void_p(off.ptr), C.c_void_p(text.ptr)))
        return nb

    # ---- paired-end SAM text (ma_pair_sam_batch): the records of the batch's mate pairs formatted on the device
    def pair_sam(self, options=0):
        """PairedFileWriter::execute for every pair on the device, after pair() (names / qualities: set_read_text); options =
        SAM_* bits.  Returns the bytes of the text."""
        _chk(lib().ma_pair_sam_batch(self.h, C.c_uint32(options)))
        return self.pair_sam_bytes()

    def pair_sam_bytes(self):
        np_, nb = C.c_uint64(), C.c_uint64()
        _chk(lib().ma_batch_pair_sam_counts(self.h, C.byref(np_), C.byref(nb)))
        return nb.value

    def pair_sam_text(self):
        """(pair_off, text): pair k's records are text[pair_off[k]:pair_off[k + 1]] (bytes)."""
        off = np.zeros(self.n // 2 + 1, dtype=np.uint64)
        text = np.zeros(self.pair_sam_bytes() + 1, dtype=np.uint8)
        _chk(lib().ma_batch_get_pair_sam(self.h, _ptr(off), _ptr(text)))
        return off, text[:-1].tobytes()

    def start_pair_sam_download(self, off, text):
        """pair_sam_text() into caller-owned HostArrays (u64[pairs + 1], u8[bytes]) without the wait: None when they are too
        small, else the bytes of the text; complete after finish_download()."""
        nb = self.pair_sam_bytes()
        if off.n < self.n // 2 + 1 or text.n < nb:
            return None
        _chk(lib().ma_batch_start_pair_sam_download(self.h, C.c_void_p(off.ptr), C.c_void_p(text.ptr)))
        return nb

    # ---- BGZF members of a SAM text (ma_sam_bgzf_batch): the text of sam() / pair_sam() deflated on the device
    def sam_bgzf_counts(self, pair=False):
        """(members, bytes) of the last sam_bgzf_members() / sam_bgzf()"""
        nm, nb = C.c_uint64(), C.c_uint64()
        _chk(lib().ma_batch_sam_bgzf_counts(self.h, C.c_int32(1 if pair else 0), C.byref(nm), C.byref(nb)))
        return nm.value, nb.value

    def sam_bgzf_members(self, pair=False):
        """(member_off, bytes): the text of the last sam() (pair: of the last pair_sam()) as BGZF members of 65 280 bytes of text
        each, packed back to back; member k is bytes[member_off[k]:member_off[k + 1]].  sam_text() / pair_sam_text() stay."""
        _chk(lib().ma_sam_bgzf_batch(self.h, C.c_int32(1 if pair else 0)))
        nm, nb = self.sam_bgzf_counts(pair)
        off = np.zeros(nm + 1, dtype=np.uint64)
        out = np.zeros(nb + 1, dtype=np.uint8)
        _chk(lib().ma_batch_get_sam_bgzf(self.h, C.c_int32(1 if pair else 0), _ptr(off), _ptr(out)))
        return off, out[:-1].tobytes()

    def sam_bgzf(self, pair=False):
        """the bytes of all members: written behind a header's members and closed with the 28-byte end-of-file marker they are a
        .sam.gz that samtools, zcat and gzip read"""
        return self.sam_bgzf_members(pair)[1]

    def start_sam_bgzf_download(self, off, out, pair=False):
        """deflates (ma_sam_bgzf_batch) and starts sam_bgzf_members() into caller-owned HostArrays (u64[members + 1], u8[bytes])
        without the wait: None when they are too small, else (members, bytes); complete after finish_download()."""
        _chk(lib().ma_sam_bgzf_batch(self.h, C.c_int32(1 if pair else 0)))
        nm, nb = self.sam_bgzf_counts(pair)
        if off.n < nm + 1 or out.n < nb:
            return None
        _chk(lib().ma_batch_start_sam_bgzf_download(self.h, C.c_int32(1 if pair else 0), C.c_void_p(off.ptr), C.c_void_p(out.ptr)))
        return nm, nb

    def close(self):
        if self.h:
            lib().ma_batch_destroy(self.h)
            self.h = None
