#!/usr/bin/env python3
"""The inflate kernels of ma_batch_set_mates_bgzf beside those of ma_batch_set_reads_bgzf on the SAME members, one batch object,
alternating: their HIP-event time (ma_batch_kernel_ms [6]: k_bgzf_inflate + k_bgzf_crc) and the wall time of the whole call.  The
paired call gets the members of R1 and of R2 as its two sides, the single-end call the two chains concatenated (one FASTQ text
of twice as many reads): the same members in the same joint table, so the same launch -- what differs is the parse behind it.
The texts are FASTQ of random reads, written as BGZF through zlib at the default level, 65 280 bytes of text per member.
usage: python tools/mates_bgzf_inflate_ms.py [pairs=131072] [read length=150] [repeats=5]"""
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ma_amd

pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
length = int(sys.argv[2]) if len(sys.argv) > 2 else 150
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
rng = np.random.default_rng(1)


def bgzf(mate):
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(pairs, length))]
    quals = rng.integers(35, 127, size=(pairs, length), dtype=np.uint8)
    text = b"".join(b"@r%d/%d\n%s\n+\n%s\n" % (i, mate, bases[i].tobytes(), quals[i].tobytes()) for i in range(pairs))
    members = []
    for at in range(0, len(text), 65280):
        part = text[at:at + 65280]
        c = zlib.compressobj(-1, zlib.DEFLATED, -15, 8)
        stream = c.compress(part) + c.flush()
        members.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(stream) + 25) + stream +
                       struct.pack("<II", zlib.crc32(part), len(part)))
    return len(text), len(members), b"".join(members)


(n1, m1, z1), (n2, m2, z2) = bgzf(1), bgzf(2)
idx = ma_amd.Index.build([rng.integers(0, 4, size=200000, dtype=np.uint8)])
b = ma_amd.Batch(idx, ma_amd.Params.preset("default"), 2 * pairs, 2 * pairs * length + 64)
b.enable_timing(True)
out = dict(pairs=pairs, read_len=length, text_bytes=[n1, n2], bgzf_bytes=[len(z1), len(z2)], members=[m1, m2], mates_inflate_kernels_ms=[],
           reads_inflate_kernels_ms=[], set_mates_bgzf_wall_ms=[], set_reads_bgzf_wall_ms=[])
for r in range(repeats + 1):  # (the first turn allocates)
    t0 = time.perf_counter()
    assert b.set_mates_bgzf(z1, z2)[0] == pairs
    t1 = time.perf_counter()
    mates_ms = float(b.kernel_ms()[6])
    t2 = time.perf_counter()
    assert b.set_reads_bgzf(z1 + z2) == 2 * pairs
    t3 = time.perf_counter()
    reads_ms = float(b.kernel_ms()[6])
    if r:
        out["mates_inflate_kernels_ms"].append(round(mates_ms, 3))
        out["reads_inflate_kernels_ms"].append(round(reads_ms, 3))
        out["set_mates_bgzf_wall_ms"].append(round(1e3 * (t1 - t0), 3))
        out["set_reads_bgzf_wall_ms"].append(round(1e3 * (t3 - t2), 3))
print(json.dumps(out))
b.close()
idx.close()
