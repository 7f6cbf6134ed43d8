#!/usr/bin/env python3
"""Generates tests/golden/extract_lists.seeds.gz: the compiled reference's own ExtractSeeds::execute (SegmentVector::forEachSeed,
Segment::forEachSeed with FMIndex::bwt_sa, setDeltaOfSeed) on the hand-made segment list of tests/extract_lists.py, once per
(min_seed_len, max_ambiguity) of extract_lists.PARAMS, through oracle/_ref/ref_dump_extract (oracle/ref_dump_extract.cpp).

Needs oracle/_ref/ref_dump_extract (make -C oracle ref, where the reference's sources exist; Makefile.ref compiles with -DNDEBUG).
The output is data only: one line per seed the reference printed.  The generated batch of 256 * 2048 + 1 seeds is not recorded.
Made-up row ranges are legal input for the reference too (bwt_sa walks from any row); a case the reference dies on shows as the
last read of a short dump: this script then names it, and it has to leave the golden (say so in extract_lists.py's header).
Run:  python tests/golden/make_extract_golden.py
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import extract_lists as ex  # noqa
from ma_testlib import REF_DUMP, write_case  # noqa
from make_golden import gz  # noqa

REF_DUMP_EXTRACT = REF_DUMP + "_extract"


def main():
    if not os.path.exists(REF_DUMP_EXTRACT):
        sys.exit("oracle/_ref/ref_dump_extract missing: run `make -C oracle ref` where the reference's sources exist")
    ex.check()
    batch = ex.case_batch()
    names, reads = batch[0], batch[1]
    out = ex.golden_path()[:-3]
    if os.path.exists(out):
        os.remove(out)
    with tempfile.TemporaryDirectory() as tmp:
        case, segs = os.path.join(tmp, "extract.case"), os.path.join(tmp, "extract.segs")
        write_case(case, list(ex.genome()), reads)
        ex.write_segs_file(segs, batch)
        for k, (min_len, max_amb) in enumerate(ex.PARAMS):
            rc = subprocess.call([REF_DUMP_EXTRACT, case, segs, out, str(min_len), str(max_amb)])
            done = sum(1 for line in open(out) if line.startswith("SEED "))
            if rc != 0 or done != (k + 1) * len(reads):
                sys.exit("the reference ended with status %d on case %s (min_seed_len %d, max_ambiguity %d)"
                         % (rc, names[min(done - k * len(reads), len(names) - 1)], min_len, max_amb))
    n = sum(1 for line in open(out) if line.startswith("d "))
    gz(out)
    print("%s: %d reads x %d parameter sets, %d seeds, %d bytes" % (os.path.basename(out) + ".gz", len(reads), len(ex.PARAMS), n,
                                                                  os.path.getsize(out + ".gz")))


if __name__ == "__main__":
    main()
