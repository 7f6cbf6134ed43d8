"""ma_batch_set_reads_bgzf: BGZF members inflated on the device (ma_amd/csrc/stage_bgzf.h) into the text the parser of
ma_batch_set_reads_text reads, through the C ABI / ma_amd.api.  The yardsticks: Python's zlib, which is not the code under test
(the tests write their BGZF themselves: zlib.compressobj(level, DEFLATED, -15, 9, strategy) per member, the 18-byte header and the
trailer around it), and set_reads_text on the same text.  tests/test_bgzf_host.py runs the same inflate routine on the CPU, under
the sanitizers too."""
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from ma_testlib import ROOT, gunzip_to, read_case
from test_bgzf_host import build_exe

pytestmark = pytest.mark.gpu
G = os.path.join(ROOT, "tests", "golden")
KINDS = [(0, zlib.Z_DEFAULT_STRATEGY, False), (-1, zlib.Z_FIXED, False), (-1, zlib.Z_DEFAULT_STRATEGY, False),
         (-1, zlib.Z_HUFFMAN_ONLY, False), (-1, zlib.Z_RLE, False), (-1, zlib.Z_DEFAULT_STRATEGY, True)]  # the host test's kinds


def deflate(text, kind=2):
    level, strategy, flush = KINDS[kind]
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    half = len(text) // 2 + 1
    if flush and half < len(text):
        return c.compress(text[:half]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(text[half:]) + c.flush()
    return c.compress(text) + c.flush()


def wrap(stream, crc, isize):
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(stream) + 25) + stream + struct.pack("<II", crc, isize)


def member(text, kind=2):
    return wrap(deflate(text, kind), zlib.crc32(text), len(text))


END = member(b"")  # the 28-byte end-of-file marker


def split(text, cuts, kinds=True, empty=True):
    """the members of text cut at the offsets given: every kind in turn, an empty member in the middle and at the end"""
    edges = [0] + sorted(set(c for c in cuts if 0 < c < len(text))) + [len(text)]
    out = [member(text[a:b], i % len(KINDS) if kinds else 2) for i, (a, b) in enumerate(zip(edges, edges[1:]))]
    if empty:
        out.insert(len(out) // 2, END)
        out.append(END)
    return out


def pieces(text, k):
    return [len(text) * i // k for i in range(1, k)]


def strict(stream):
    """zlib's strict decode of a raw deflate stream: the bytes, or None"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream, 65537)
    except zlib.error:
        return None
    return out if d.eof and not d.unused_data and not d.unconsumed_tail and len(out) <= 65536 else None


def record(rng, fastq, i, end):
    n = int(rng.integers(20, 120))
    seq = "".join("ACGTNacgtRYK"[int(x)] for x in rng.integers(0, 12, size=n))
    if fastq:
        q = "".join(chr(int(x)) for x in rng.integers(33, 127, size=n))
        return ("@r%d/%d extra%s%s%s+%s%s%s" % (i, i % 7, end, seq, end, end, q, end)).encode()
    return (">r%d some description%s%s%s%s%s" % (i, end, seq[:n // 2 + 1], end, seq[n // 2 + 1:] + "A", end)).encode()


def params():
    import ma_amd
    P = ma_amd.Params.preset("default")
    P.srand_seed = 1
    return P


@pytest.fixture(scope="module")
def small(tmp_path_factory, gpu_device):
    import ma_amd
    g, reads, names = read_case(gunzip_to(os.path.join(G, "small.case.gz"), str(tmp_path_factory.mktemp("bgzf") / "small.case")))
    idx = ma_amd.Index.build(g)
    idx.set_contig_names(names)
    yield idx, g, reads
    idx.close()


@pytest.fixture(scope="module")
def batches(small):
    """(the batch under test, the batch of the text call, the texts' reference results)"""
    import ma_amd
    b, t = ma_amd.Batch(small[0], params(), 4096, 200000), ma_amd.Batch(small[0], params(), 4096, 200000)
    yield b, t, {}
    b.close()
    t.close()


@pytest.fixture(scope="module")
def texts():
    rng = np.random.default_rng(20261020)
    return dict(small24=open(os.path.join(G, "reader", "small24.fq"), "rb").read(),
                fastq=b"".join(record(rng, True, i, "\r\n") for i in range(200)),
                fasta=b"".join(record(rng, False, i, "\n") for i in range(200)))


def state(b):
    off, codes = b.reads()
    names, quals = b.read_text()
    return b.read_counts(), off.tobytes(), codes.tobytes(), names, quals


def same_as_text(batches, text, members, head=b"", drop=0):
    """after set_reads_bgzf the batch is as after set_reads_text on the text"""
    b, t, cache = batches
    if text not in cache:
        n = t.set_reads_text(text)
        cache[text] = (n, state(t))
    assert b.set_reads_bgzf(b"".join(members), head, drop) == cache[text][0]
    assert state(b) == cache[text][1]


@pytest.mark.parametrize("name", ["small24", "fastq", "fasta"])
def test_parity_with_the_text_call(batches, texts, name):
    """small24.fq, 200 generated FASTQ records with \\r\\n ends and 200 FASTA records as 1, 63, 64, 65 and 129 members (one lane,
    one wavefront less one, exactly one, one more, three) of every kind in turn with an empty member in the middle and at the
    end; borders mid-line and, for the \\r\\n text, between the \\r and the \\n of 40 lines: read_counts(), reads() and read_text()
    equal those after set_reads_text on the same text"""
    text = texts[name]
    assert len(text) <= 65536
    for k in (1, 63, 64, 65, 129):
        same_as_text(batches, text, split(text, pieces(text, k)))
    for kind in range(len(KINDS)):  # the whole text as one member of each kind
        same_as_text(batches, text, [member(text, kind)])
    returns = [i + 1 for i in range(len(text)) if text[i:i + 2] == b"\r\n"][:40]
    if returns:
        same_as_text(batches, text, split(text, returns))
    same_as_text(batches, text, [END, END] + split(text, pieces(text, 5)) + [END])


def test_head_and_drop(batches, texts):
    """head empty / ending mid-line / alone (no members, and only an empty member); drop 0 / inside the last member / the whole
    last member / across two members; a drop larger than the inflated part is refused and the batch stays usable"""
    import ma_amd
    b, t, _ = batches
    text = texts["small24"]
    extra = text[7:1507]  # what a caller drops: the front of records that belong to its next call
    for cut in (0, 100, len(text) - 1):
        for drop in (0, 350, 600, 1050):  # the last member holds 600 bytes, the one before it 900
            whole = text[cut:] + extra[:drop]
            same_as_text(batches, text, split(whole, [len(whole) - 1500, len(whole) - 600], empty=False), text[:cut], drop)
    same_as_text(batches, text, [member(text[100:])], text[:100], 0)
    same_as_text(batches, text, [], text, 0)
    same_as_text(batches, text, [END], text, 0)
    same_as_text(batches, b"", [], b"", 0)
    same_as_text(batches, b"", [member(text)], b"", len(text))
    with pytest.raises(ma_amd.MaError, match="ma_batch_set_reads_bgzf: n_drop is larger than the inflated part of the text"):
        b.set_reads_bgzf(member(text[100:]), text[:100], len(text) - 100 + 1)
    assert b.read_counts()["reads"] == 0
    same_as_text(batches, text, [member(text)])


def last_record_start(text):
    """BatchTextReader's rule for FASTQ: the last '@' line behind offset 0 whose next-but-one line starts with '+'"""
    starts = [0] + [i + 1 for i in range(len(text)) if text[i:i + 1] == b"\n" and i + 1 < len(text)]
    for k in range(len(starts) - 3, 0, -1):
        if text[starts[k]:starts[k] + 1] == b"@" and text[starts[k + 2]:starts[k + 2] + 1] == b"+":
            return starts[k]
    return 0


def test_a_streamed_file_in_three_calls(batches, texts):
    """the FASTQ text as 700-byte members, streamed in three calls as BatchBgzfReader cuts them: the members up to the one that
    holds the last record start, drop = that member's bytes behind it, which are the next call's head: the reads of the three
    calls are the file's, in order"""
    b, t, _ = batches
    text = texts["fastq"]
    parts = [text[a:a + 700] for a in range(0, len(text), 700)]
    t.set_reads_text(text)
    want = state(t)
    runs, head, carried, names, quals, codes = [len(parts) // 3, 2 * len(parts) // 3, len(parts)], b"", [], [], [], []
    sent = 0
    for r, upto in enumerate(runs):
        chunk = carried + parts[sent:upto]
        sent = upto
        whole = head + b"".join(chunk)
        cut = last_record_start(whole) if r < 2 else len(whole)
        assert cut > len(head)
        size, m = len(head), 0
        while size + len(chunk[m]) < cut:
            size += len(chunk[m])
            m += 1
        drop = size + len(chunk[m]) - cut
        n = b.set_reads_bgzf(b"".join(member(p, (r + i) % len(KINDS)) for i, p in enumerate(chunk[:m + 1])), head, drop)
        s = state(b)
        assert n == s[0]["reads"] > 0
        names += s[3]
        quals += s[4]
        codes.append(s[2])
        head, carried = whole[cut:cut + drop], chunk[m + 1:]
    assert not head and not carried
    assert names == want[3] and quals == want[4] and b"".join(codes) == want[2]


def test_refusals(batches, texts):
    """the table of tests/emul/bgzf_dev_test.cpp `reasons` (one stream per reason behind a good member): the device's message is
    inflateHost's, byte for byte; afterwards the batch holds no reads and the next good call works.  Of several violations the
    lowest member is named, whichever wavefront sees it; gzip.compress's bytes are refused as plain gzip; a violation in the
    text is reported with its line and offset in the text"""
    import ma_amd
    b, t, _ = batches
    text = texts["small24"]
    table = [l.split(" ", 1) for l in subprocess.check_output([build_exe(), "reasons", "print"]).decode().splitlines()]
    assert len(table) == 19 and len(set(m for _, m in table)) == 19
    good = [member(text[a:a + 40]) for a in range(0, 40 * 130, 40)]
    bad_crc = lambda i: wrap(deflate(text[40 * i:40 * i + 40]), zlib.crc32(text[40 * i:40 * i + 40]) ^ 4, 40)
    bad_len = lambda i: wrap(deflate(text[40 * i:40 * i + 40]), zlib.crc32(text[40 * i:40 * i + 40]), 41)
    several = [(good[:3] + [bad_crc(3)] + good[4:70] + [bad_len(70)] + good[71:], "member 3 (byte %d): CRC mismatch" % sum(map(len, good[:3]))),
               (good[:3] + [bad_len(3)] + good[4:70] + [bad_crc(70)] + good[71:], "member 3 (byte %d): length mismatch" % sum(map(len, good[:3]))),
               (good[:129] + [bad_crc(129)], "member 129 (byte %d): CRC mismatch" % sum(map(len, good[:129]))),
               ([gzip.compress(text)], "member 0 (byte 0): a gzip member without the BGZF size field: single-member gzip stays with GzFileStream")]
    cases = [(bytes.fromhex(h), m) for h, m in table] + [(b"".join(ms), "ma_batch_set_reads_bgzf: " + m) for ms, m in several]
    for data, want in cases:
        with pytest.raises(ma_amd.MaError) as e:
            b.set_reads_bgzf(data)
        assert str(e.value).startswith(want) and want.startswith("ma_batch_set_reads_bgzf: member ")
        assert b.read_counts() == dict(reads=0, bases=0, name_bytes=0, has_qual=0)
        same_as_text(batches, text, split(text, pieces(text, 3)))
    # a violation in the text: the message of the text call with this call's words in front
    broken = text.replace(b"\n+", b"\n-", 3).replace(b"\n-", b"\n+", 2)  # the third record's + line
    assert broken != text
    with pytest.raises(ma_amd.MaError) as e:
        t.set_reads_text(broken)
    want = str(e.value).replace("ma_batch_set_reads_text: ", "ma_batch_set_reads_bgzf: text: ")
    assert " line 11 " in want
    for head in (0, 50):
        with pytest.raises(ma_amd.MaError) as e:
            b.set_reads_bgzf(b"".join(split(broken[head:], pieces(broken[head:], 4))), broken[:head])
        assert str(e.value) == want
        assert b.read_counts()["reads"] == 0
    with pytest.raises(ma_amd.MaError, match=r"ma_batch_set_reads_bgzf: text: line 1 \(byte 0\): the text starts with neither"):
        b.set_reads_bgzf(member(text[1:]))
    same_as_text(batches, text, [member(text)])


def test_capacity(small, texts):
    """more reads than the batch holds: "batch capacity exceeded", the exception carries the reads of the text; the next call works"""
    import ma_amd
    b = ma_amd.Batch(small[0], params(), 8, 200000)
    with pytest.raises(ma_amd.MaError, match="ma_batch_set_reads_bgzf: batch capacity exceeded") as e:
        b.set_reads_bgzf(member(texts["small24"]))
    assert e.value.n_reads == 24 and b.read_counts()["reads"] == 0
    eight = b"".join(texts["small24"].splitlines(True)[:32])
    assert b.set_reads_bgzf(member(eight)) == 8
    b.close()


def test_mutants_have_zlibs_verdict(batches, texts):
    """60 single-bit flips of the deflate bytes of a three-member stream (stored, fixed, dynamic) with the trailer left alone
    (family A) and 60 with the trailer recomputed where zlib still decodes (family B): the call refuses the member exactly when
    Python zlib's strict decode + CRC + ISIZE does, and where it does not, it does with the decoded text what set_reads_text
    does with it -- the same reads or the same refusal, which names a line and a byte of the text.  At least a third of B passes
    the inflate.  (tests/test_bgzf_host.py runs the same routine over 3 600 mutants under the sanitizers.)"""
    import ma_amd
    b, t, _ = batches
    text = texts["small24"]
    third = [text[:1500], text[1500:3000], text[3000:]]
    streams = [deflate(p, k) for p, k in zip(third, (0, 1, 2))]
    rng = np.random.default_rng(20261020)
    passed = {False: 0, True: 0}
    for k in range(120):
        family_b = k >= 60
        which = int(rng.integers(0, 3))
        bit = int(rng.integers(0, 8 * len(streams[which])))
        mutant = bytearray(streams[which])
        mutant[bit // 8] ^= 1 << (bit % 8)
        decoded = strict(bytes(mutant))
        crc, isize = zlib.crc32(third[which]), len(third[which])
        if family_b and decoded is not None:
            crc, isize = zlib.crc32(decoded), len(decoded)
        accept = decoded is not None and len(decoded) == isize and zlib.crc32(decoded) == crc
        data = b"".join(wrap(bytes(mutant), crc, isize) if i == which else wrap(streams[i], zlib.crc32(third[i]), len(third[i])) for i in range(3))
        whole = b"".join(decoded if i == which else third[i] for i in range(3)) if accept else None
        try:
            got = (b.set_reads_bgzf(data), state(b))
        except ma_amd.MaError as e:
            got = str(e)
        if not accept:
            offset = sum(len(wrap(streams[i], 0, 0)) for i in range(which))
            assert isinstance(got, str) and got.startswith("ma_batch_set_reads_bgzf: member %d (byte %d): " % (which, offset)), (k, got)
            continue
        passed[family_b] += 1
        try:
            want = (t.set_reads_text(whole), state(t))
        except ma_amd.MaError as e:
            want = str(e).replace("ma_batch_set_reads_text: ", "ma_batch_set_reads_bgzf: text: ")
        assert got == want, (k, got if isinstance(got, str) else got[0], want if isinstance(want, str) else want[0])
    print("mutants that pass the inflate: family A %d of 60, family B %d of 60" % (passed[False], passed[True]))
    assert 3 * passed[True] >= 60


def test_end_to_end_sam(small):
    """the reads of small.case as FASTQ text in 3 000-byte members -> set_reads_bgzf -> align -> sam(): the bytes and the record
    offsets of the same batch set through set_reads_text"""
    import ma_amd
    idx, g, reads = small
    rng = np.random.default_rng(70)
    text = b"".join(("@r%d\n%s\n+\n%s\n" % (i, "".join("ACGTN"[int(x)] for x in r), "".join(chr(int(q)) for q in rng.integers(35, 127, size=len(r))))).encode()
                    for i, r in enumerate(reads))
    n_bases = sum(len(r) for r in reads)
    a, z = ma_amd.Batch(idx, params(), len(reads), n_bases + 64), ma_amd.Batch(idx, params(), len(reads), n_bases + 64)
    assert a.set_reads_text(text) == len(reads)
    assert z.set_reads_bgzf(b"".join(split(text, range(3000, len(text), 3000)))) == len(reads)
    a.align()
    z.align()
    for bits in (0, 31):
        assert a.sam(bits) == z.sam(bits) > 0
        (ao, at), (zo, zt) = a.sam_text(), z.sam_text()
        assert at == zt and np.array_equal(ao, zo)
    a.close()
    z.close()


def test_ma_align_text_input_on_a_bgzip_file(tmp_path, gpu_device):
    """examples/ma_align --text-input on the reads of small.case written as BGZF (60 000 bytes of text per member, the end-of-file
    marker behind them; BatchBgzfReader + BatchAligner::executeBgzfSam) writes, byte for byte, the file it writes from the plain
    text; the same text as plain gzip is an error that names bgzip"""
    from test_gpu_reads_text import build_ma_align, write_small_case
    exe = build_ma_align()
    fa, rd, reads = write_small_case(tmp_path, True)
    text = open(rd, "rb").read()
    bgz, plain_gz = str(tmp_path / "reads.fq.gz"), str(tmp_path / "plain.fq.gz")
    with open(bgz, "wb") as f:
        f.write(b"".join(split(text, range(60000, len(text), 60000), kinds=False)))
    with open(plain_gz, "wb") as f:
        f.write(gzip.compress(text))
    a, z = str(tmp_path / "text.sam"), str(tmp_path / "bgzf.sam")
    subprocess.check_call([exe, "--text-input", fa, rd, a])
    subprocess.check_call([exe, "--text-input", fa, bgz, z])
    got, want = open(z, "rb").read(), open(a, "rb").read()
    assert got == want and got.count(b"\n") > len(reads)
    p = subprocess.run([exe, "--text-input", fa, plain_gz, str(tmp_path / "o.sam")], stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"compressed" in p.stderr and b"bgzip" in p.stderr
