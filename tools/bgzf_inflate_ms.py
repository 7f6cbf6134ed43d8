#!/usr/bin/env python3
"""The inflate kernels of ma_batch_set_reads_bgzf on ONE batch: their HIP-event time (ma_batch_kernel_ms [6]: k_bgzf_inflate +
k_bgzf_crc) and the wall time of the whole call, beside the wall time of ma_batch_set_reads_text on the same text.  The text is
FASTQ of random reads, written as BGZF through zlib at the default level, 65 280 bytes of text per member as bgzip cuts them.
usage: python tools/bgzf_inflate_ms.py [reads=262144] [read length=150] [repeats=5]"""
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

reads = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
length = int(sys.argv[2]) if len(sys.argv) > 2 else 150
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
rng = np.random.default_rng(1)
bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(reads, length))]
quals = rng.integers(35, 127, size=(reads, length), dtype=np.uint8)
text = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, bases[i].tobytes(), quals[i].tobytes()) for i in range(reads))
members = []
for at in range(0, len(text), 65280):
    part = text[at:at + 65280]
    c = zlib.compressobj(-1, zlib.DEFLATED, -15, 8)
    stream = c.compress(part) + c.flush()
    members.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(stream) + 25) + stream +
                   struct.pack("<II", zlib.crc32(part), len(part)))
data = b"".join(members)
idx = ma_amd.Index.build([rng.integers(0, 4, size=200000, dtype=np.uint8)])
b = ma_amd.Batch(idx, ma_amd.Params.preset("default"), reads, reads * length + 64)
b.enable_timing(True)
out = dict(reads=reads, read_len=length, text_bytes=len(text), bgzf_bytes=len(data), members=len(members), inflate_kernels_ms=[],
           set_reads_bgzf_wall_ms=[], set_reads_text_wall_ms=[])
for r in range(repeats + 1):  # (the first turn allocates)
    t0 = time.perf_counter()
    assert b.set_reads_bgzf(data) == reads
    t1 = time.perf_counter()
    kernel = float(b.kernel_ms()[6])
    t2 = time.perf_counter()
    assert b.set_reads_text(text) == reads
    t3 = time.perf_counter()
    if r:
        out["inflate_kernels_ms"].append(round(kernel, 3))
        out["set_reads_bgzf_wall_ms"].append(round(1e3 * (t1 - t0), 3))
        out["set_reads_text_wall_ms"].append(round(1e3 * (t3 - t2), 3))
print(json.dumps(out))
b.close()
idx.close()
