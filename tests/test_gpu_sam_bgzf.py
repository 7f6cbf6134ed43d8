"""ma_sam_bgzf_batch / ma_bgzf_deflate: a text deflated on the device into BGZF members (ma_amd/csrc/stage_deflate.h), through the
C ABI / ma_amd.api.  The yardsticks: the host statement of the same rules (ma_bgzf::deflateHost, run by the `deflate` mode of
tests/emul/sam_bgzf_test.cpp -- the kernels must give its bytes), and Python's zlib / gzip, which inflate the members back to the
text.  tests/test_sam_bgzf_host.py pins the host statement itself to zlib, under the sanitizers too."""
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from ma_testlib import ROOT, gunzip_to, read_case
from test_sam_bgzf_host import build_exe

pytestmark = pytest.mark.gpu
G = os.path.join(ROOT, "tests", "golden")
END = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0\x1b\0\x03\0\0\0\0\0\0\0\0\0"  # the 28-byte end-of-file marker
LENGTHS = [0, 1, 2, 3, 4, 5, 257, 258, 259, 65279, 65280, 65281, 130560, 130561]


def host_statement(tmp, text):
    src, out = os.path.join(str(tmp), "text"), os.path.join(str(tmp), "members")
    open(src, "wb").write(text)
    subprocess.check_call([build_exe(), "deflate", src, out], stdout=subprocess.DEVNULL)
    return open(out, "rb").read()


def check_members(off, data, text):
    """ceil(n / 65280) members of the exact form, each inflating (zlib, strict) to its 65 280 bytes of the text"""
    n = (len(text) + 65279) // 65280
    assert len(off) == n + 1 and int(off[0]) == 0 and int(off[-1]) == len(data)
    for k in range(n):
        m, part = data[int(off[k]):int(off[k + 1])], text[65280 * k:65280 * (k + 1)]
        assert m[:16] == END[:16] and struct.unpack("<H", m[16:18])[0] == len(m) - 1 and len(m) <= len(part) + 31
        d = zlib.decompressobj(-15)
        assert d.decompress(m[18:-8]) == part and d.eof and not d.unused_data
        assert struct.unpack("<II", m[-8:]) == (zlib.crc32(part), len(part))
    assert gzip.decompress(data + END) == text


def periodic(rng, n, period):
    unit = bytes(rng.integers(65, 91, size=period, dtype=np.uint8))
    if period > 1:
        unit = unit[:-1] + b"\n"
    return (unit * (n // period + 1))[:n]


def fibonacci(rng):
    counts = [1, 1]
    while len(counts) < 22:
        counts.append(counts[-1] + counts[-2])
    a = np.concatenate([np.full(c, 97 + i, dtype=np.uint8) for i, c in enumerate(counts)])
    assert len(a) == 46367
    rng.shuffle(a)
    return a.tobytes()


def contents(kind):
    """the texts of one kind of content"""
    rng = np.random.default_rng(20261020)
    if kind.startswith("period"):
        return [periodic(rng, n, int(kind[6:])) for n in LENGTHS]
    if kind == "random":
        return [bytes(rng.integers(0, 256, size=n, dtype=np.uint8)) for n in LENGTHS]
    if kind == "two values":
        return [bytes(rng.integers(0, 2, size=n, dtype=np.uint8) * 3 + 65) for n in LENGTHS]
    if kind == "all values":
        return [bytes(np.arange(n, dtype=np.uint32).astype(np.uint8)) for n in LENGTHS]
    if kind == "distance":
        block = bytes(rng.integers(0, 256, size=300, dtype=np.uint8))
        return [block + b"x" * (d - 300) + block + b"y" * 50 for d in (32768, 32769)]
    if kind == "border":
        out = []
        for before in (1, 3, 100, 257, 300):
            line = bytes(rng.integers(64, 84, size=400, dtype=np.uint8))
            s = bytes(rng.integers(48, 52, size=65280 - 1000, dtype=np.uint8)) + line
            s += bytes(rng.integers(48, 52, size=65280 - before - len(s), dtype=np.uint8))
            out.append(s + line * 3)
        return out
    if kind == "fibonacci":
        return [fibonacci(rng)]
    assert kind == "sam"
    sam = b"".join(l for l in gzip.open(os.path.join(G, "small_ref.illumina.opt4.sam.gz"), "rb").read().splitlines(True) if not l.startswith(b"@"))
    return [sam, (sam * 3)[:3 * 65280 - 7]]


KINDS = ["period1", "period2", "period3", "period4", "period5", "period64", "random", "two values", "all values", "distance", "border",
         "fibonacci", "sam"]


@pytest.fixture(scope="module")
def small(tmp_path_factory, gpu_device):
    import ma_amd
    g, reads, names = read_case(gunzip_to(os.path.join(G, "small.case.gz"), str(tmp_path_factory.mktemp("sambgzf") / "small.case")))
    idx = ma_amd.Index.build(g)
    idx.set_contig_names(names)
    yield idx, g, reads
    idx.close()


def params(preset="default"):
    import ma_amd
    P = ma_amd.Params.preset(preset)
    P.srand_seed = 1
    return P


@pytest.fixture(scope="module")
def aligned(small):
    """small.case aligned once; the SAM texts are made from it"""
    import ma_amd
    idx, g, reads = small
    b = ma_amd.Batch(idx, params(), len(reads), sum(len(r) for r in reads) + 64)
    b.set_reads(reads)
    b.set_read_text(["r%d" % i for i in range(len(reads))], None)
    b.align()
    yield b
    b.close()


@pytest.mark.parametrize("kind", KINDS)
def test_bgzf_deflate_gives_the_host_statements_bytes(small, tmp_path, kind):
    """ma_amd.bgzf_deflate over the length x content grid of the host test, three members at the most: the bytes of the host
    statement, and Python's zlib inflates every member to its part of the text"""
    import ma_amd
    sizes = []
    for text in contents(kind):
        off, data = ma_amd.bgzf_deflate(small[0], text)
        want = host_statement(tmp_path, text)
        assert data == want, "%s, %d bytes: first difference at byte %d of %d / %d" % (
            kind, len(text), next((i for i, (x, y) in enumerate(zip(data, want)) if x != y), min(len(data), len(want))), len(data), len(want))
        check_members(off, data, text)
        sizes.append(len(data))
    if kind == "random":  # stored: the text + 31 bytes per member
        assert sizes == [n + 31 * ((n + 65279) // 65280) for n in LENGTHS]
    if kind == "distance":  # in reach the second block is two matches, out of reach 300 literals
        assert sizes[0] + 250 < sizes[1]
    if kind == "sam":
        assert 3 * sizes[0] < len(contents(kind)[0])


def test_bgzf_deflate_counts_and_refuses_a_small_cap(small):
    """out == NULL only counts; a cap that is too small fails with the size needed, and the next call works"""
    import ctypes as C
    import ma_amd
    text = b"ACGT\tr1\t60\n" * 7000
    buf = np.frombuffer(text + b"\0", dtype=np.uint8)
    nm, nb = C.c_uint64(), C.c_uint64()
    call = ma_amd.lib().ma_bgzf_deflate
    assert call(small[0].h, buf.ctypes.data_as(C.c_void_p), C.c_uint64(len(text)), C.byref(nm), C.byref(nb), None, None, C.c_uint64(0)) == 0
    off, data = ma_amd.bgzf_deflate(small[0], text)
    assert (nm.value, nb.value) == (2, len(data)) and len(off) == 3
    out = np.zeros(nb.value, dtype=np.uint8)
    assert call(small[0].h, buf.ctypes.data_as(C.c_void_p), C.c_uint64(len(text)), C.byref(nm), C.byref(nb), None,
                out.ctypes.data_as(C.c_void_p), C.c_uint64(nb.value - 1)) != 0
    msg = ma_amd.lib().ma_last_error().decode()
    assert msg.startswith("ma_bgzf_deflate: ") and str(len(data)) in msg
    assert ma_amd.bgzf_deflate(small[0], text)[1] == data


@pytest.mark.parametrize("options", [0, 3, 32], ids=["options 0", "soft clip + =/X", "NGMLR tags"])
def test_small_case_sam_text_as_members(aligned, tmp_path, options):
    """small.case aligned and printed on the device: sam_bgzf() is the host statement over sam_text(), gzip reads the text back,
    and sam_text() is unchanged by the call"""
    b = aligned
    nb = b.sam(options)
    roff, text = b.sam_text()
    assert nb == len(text) > 40000
    off, data = b.sam_bgzf_members()
    assert data == host_statement(tmp_path, text)
    check_members(off, data, text)
    assert b.sam_bgzf_counts() == (len(off) - 1, len(data))
    roff2, text2 = b.sam_text()
    assert text2 == text and np.array_equal(roff, roff2)
    assert b.sam_bgzf() == data


def test_a_batch_of_no_reads_has_no_members(small):
    import ma_amd
    b = ma_amd.Batch(small[0], params(), 16, 1024)
    b.set_reads([])
    b.set_read_text([], None)
    b.align()
    assert b.sam(0) == 0
    off, data = b.sam_bgzf_members()
    assert data == b"" and [int(x) for x in off] == [0] and b.sam_bgzf_counts() == (0, 0)
    b.close()


def test_paired_golden_case_as_members(tmp_path, gpu_device):
    """f4.case under illumina, options 3, through pair_sam: sam_bgzf(pair=True) is the host statement over pair_sam_text(), gzip
    reads the reference's record lines back, and neither text changes; the single-end members are the single-end text's"""
    from test_gpu_pair_sam import paired_batch
    from test_sam_pair_dev_host import PAIR_GOLDEN
    from test_gpu_sam import Ctx
    from test_gpu_sam import params as sam_params
    g, reads, names = read_case(gunzip_to(os.path.join(G, "f4.case.gz"), str(tmp_path / "f4.case")))
    reads = reads[:len(reads) // 2 * 2]
    want = b"".join(l for l in gzip.open(os.path.join(G, PAIR_GOLDEN + ".sam.gz"), "rb").read().splitlines(True) if not l.startswith(b"@"))
    ctx = Ctx(g, names)
    b = paired_batch(ctx, sam_params("illumina"), reads, ["r%d" % i for i in range(len(reads))], None)
    assert b.pair_sam(3) == len(want)
    b.sam(0)
    single = b.sam_text()[1]
    off, data = b.sam_bgzf_members(pair=True)
    assert data == host_statement(tmp_path, want)
    check_members(off, data, want)
    assert b.pair_sam_text()[1] == want and b.sam_text()[1] == single
    soff, sdata = b.sam_bgzf_members()
    check_members(soff, sdata, single)
    assert b.sam_bgzf_counts(pair=True) == (len(off) - 1, len(data)) and b.sam_bgzf_counts() == (len(soff) - 1, len(sdata))
    b.close()
    ctx.idx.close()


def test_contract(small):
    """the call before any SAM text fails with a message; a second pending download is refused by name; after sam() again the
    members are gone; the batch stays usable after each refusal"""
    import ctypes as C
    import ma_amd
    idx, g, reads = small
    b = ma_amd.Batch(idx, params(), len(reads), sum(len(r) for r in reads) + 64)
    b.set_reads(reads)
    b.set_read_text(["r%d" % i for i in range(len(reads))], None)
    b.align()
    for pair, name in ((False, "ma_sam_batch"), (True, "ma_pair_sam_batch")):
        with pytest.raises(ma_amd.MaError, match=r"ma_sam_bgzf_batch: no SAM text to deflate \(run %s first\)" % name):
            b.sam_bgzf(pair=pair)
    with pytest.raises(ma_amd.MaError, match="ma_batch_sam_bgzf_counts: no SAM text"):
        b.sam_bgzf_counts()
    b.sam(0)
    text = b.sam_text()[1]
    with pytest.raises(ma_amd.MaError, match="ma_batch_sam_bgzf_counts: run ma_sam_bgzf_batch first"):
        b.sam_bgzf_counts()
    data = b.sam_bgzf()
    assert gzip.decompress(data + END) == text
    # one download slot
    nm, nb = b.sam_bgzf_counts()
    off, out = ma_amd.HostArray(nm + 1, np.uint64), ma_amd.HostArray(nb, np.uint8)
    assert b.start_sam_bgzf_download(ma_amd.HostArray(1, np.uint64), out) is None
    assert b.start_sam_bgzf_download(off, out) == (nm, nb)
    roff, rtext = ma_amd.HostArray(len(reads) + 1, np.uint64), ma_amd.HostArray(len(text), np.uint8)
    with pytest.raises(ma_amd.MaError, match="ma_batch_start_sam_download: the download started before was not finished"):
        b.start_sam_download(roff, rtext)
    with pytest.raises(ma_amd.MaError, match="ma_batch_start_sam_bgzf_download: the download started before was not finished"):
        ma_amd.api._chk(ma_amd.lib().ma_batch_start_sam_bgzf_download(b.h, C.c_int32(0), C.c_void_p(off.ptr), C.c_void_p(out.ptr)))
    b.finish_download()
    assert out.a[:nb].tobytes() == data and int(off.a[nm]) == nb
    assert b.start_sam_download(roff, rtext) == len(text)
    b.finish_download()
    assert rtext.a.tobytes() == text
    # the text made again: the members are gone, until they are made again
    b.sam(1)
    with pytest.raises(ma_amd.MaError, match="ma_batch_get_sam_bgzf: run ma_sam_bgzf_batch first"):
        ma_amd.api._chk(ma_amd.lib().ma_batch_get_sam_bgzf(b.h, C.c_int32(0), None, None))
    assert gzip.decompress(b.sam_bgzf() + END) == b.sam_text()[1] != text
    # new reads: no text, no members
    b.set_reads(reads[:10])
    with pytest.raises(ma_amd.MaError, match="ma_sam_bgzf_batch: no SAM text to deflate"):
        b.sam_bgzf()
    b.set_read_text(["q%d" % i for i in range(10)], None)
    b.align()
    b.sam(0)
    assert gzip.decompress(b.sam_bgzf() + END) == b.sam_text()[1]
    for h in (off, out, roff, rtext):
        h.close()
    b.close()


def test_timing_slot_7(aligned):
    """with timing on, ma_batch_kernel_ms[7] is the time of the deflate kernels"""
    b = aligned
    b.enable_timing(True)
    b.sam(0)
    b.sam_bgzf()
    ms = b.kernel_ms()
    b.enable_timing(False)
    assert 0 < ms[7] < 1000


def test_set_reads_bgzf_accepts_the_members(small):
    """the members ma_amd.bgzf_deflate makes of a FASTQ text are accepted by set_reads_bgzf: the batch is as after
    set_reads_text on that text"""
    import ma_amd
    from test_gpu_bgzf import state
    fq = open(os.path.join(G, "reader", "small24.fq"), "rb").read()
    text = fq * (2 * 65280 // len(fq) + 2)  # three members; records straddle them
    off, data = ma_amd.bgzf_deflate(small[0], text)
    assert len(off) == 4
    b, t = ma_amd.Batch(small[0], params(), 4096, 400000), ma_amd.Batch(small[0], params(), 4096, 400000)
    n = b.set_reads_bgzf(data + END)
    assert n == t.set_reads_text(text) == 24 * (len(text) // len(fq))
    assert state(b) == state(t)
    b.close()
    t.close()


def bgzf_file(path):
    """the text of a BGZF file that ends with the end-of-file marker and is members from its first byte"""
    data = open(path, "rb").read()
    assert data.endswith(END) and data.count(END) == 1
    at = 0
    while at < len(data):
        assert data[at:at + 16] == END[:16]
        at += struct.unpack("<H", data[at + 16:at + 18])[0] + 1
    assert at == len(data)
    return gzip.open(path, "rb").read()


@pytest.fixture(scope="module")
def single_end_run(tmp_path_factory, gpu_device):
    """small.case as files, and the file examples/ma_align --text-input writes for them without the option"""
    from test_gpu_sam import build_ma_align, write_small_case
    tmp = tmp_path_factory.mktemp("sambgzf_align")
    exe = build_ma_align()
    fa, rd, reads = write_small_case(tmp, True)
    plain = str(tmp / "plain.sam")
    subprocess.check_call([exe, "--text-input", fa, rd, plain, "default"])
    want = open(plain, "rb").read()
    assert want.startswith(b"@SQ\t") and want.count(b"\n") > len(reads)
    return exe, fa, rd, want


@pytest.mark.parametrize("flags", [["--text-input", "--bgzf-output"], ["--bgzf-output"], ["--host-sam", "--bgzf-output"]],
                         ids=["text input", "host parse", "host sam"])
def test_ma_align_bgzf_output_single_end(tmp_path, single_end_run, flags):
    """examples/ma_align on small.case: gzip.open of the --bgzf-output file equals the file without the flag, header included,
    and the file ends with the marker -- with --text-input, with the records parsed on the host, and with --host-sam, where
    every byte goes through the host statement"""
    exe, fa, rd, want = single_end_run
    out = str(tmp_path / "packed.sam")
    subprocess.check_call([exe] + flags + [fa, rd, out, "default"])
    assert bgzf_file(out) == want
    assert os.path.getsize(out) < len(want)  # (the random qualities do not compress)


@pytest.fixture(scope="module")
def paired_run(tmp_path_factory, gpu_device):
    """small.case as mate pairs in two FASTQ files, and the file examples/ma_align writes for them without the option"""
    from test_gpu_sam import build_ma_align
    tmp = tmp_path_factory.mktemp("sambgzf_pairs")
    exe = build_ma_align()
    g, reads, names = read_case(gunzip_to(os.path.join(G, "small.case.gz"), str(tmp / "small.case")))
    fa = str(tmp / "genome.fa")
    with open(fa, "w") as f:
        for nm, c in zip(names, g):
            f.write(">%s\n%s\n" % (nm, "".join("ACGT"[int(b)] for b in c)))
    rng = np.random.default_rng(71)
    files = [str(tmp / "reads_1.fq"), str(tmp / "reads_2.fq")]
    for m in (0, 1):
        with open(files[m], "w") as f:
            for k in range(len(reads) // 2):
                r = reads[2 * k + m]
                f.write("@p%d/%d\n%s\n+\n%s\n" % (k, m + 1, "".join("ACGTN"[int(b)] for b in r),
                                                  "".join(chr(int(q)) for q in rng.integers(35, 127, size=len(r)))))
    plain = str(tmp / "plain.sam")
    subprocess.check_call([exe, fa, files[0], plain, "illuminapaired", files[1]])
    want = open(plain, "rb").read()
    assert want.startswith(b"@SQ\t") and want.count(b"\n") > len(reads)
    return exe, fa, files, want


@pytest.mark.parametrize("flags,name", [([], "named.sam.gz"), (["--text-input", "--bgzf-output"], "text.sam"), (["--host-sam", "--bgzf-output"], "host.sam")],
                         ids=["name ends in .gz", "text input", "host sam"])
def test_ma_align_bgzf_output_paired(tmp_path, paired_run, flags, name):
    """examples/ma_align on small.case as mate pairs: an output name that ends in .gz sets the option (device path), and
    --bgzf-output with --text-input and with --host-sam; gzip.open of each equals the file without the option"""
    exe, fa, files, want = paired_run
    out = str(tmp_path / name)
    subprocess.check_call([exe] + flags + [fa, files[0], out, "illuminapaired", files[1]])
    assert bgzf_file(out) == want
