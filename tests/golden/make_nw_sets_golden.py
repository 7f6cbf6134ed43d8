#!/usr/bin/env python3
"""Generates the nw_sets.* goldens: the compiled reference's own NeedlemanWunsch::execute + MappingQuality::execute on the
hand-made harmonized sets of tests/nw_sets.py (ref_dump nwsets), for the preset's scoring and for one that makes kswcpp swap
its two gap models.

The binary is oracle/_ref/ref_dump_nw: ref_dump with the reference's alignment.cpp, needlemanWunsch.cpp and mappingQuality.cpp in
one translation unit, so that all three read the scoring this script sets (oracle/ref_dump_nw.cpp has the reason: in the
plain build each of them keeps the defaults of its own copy of the reference's global parameters).  With the default scoring
plain ref_dump must write the same bytes, which is asserted here.

Needs oracle/_ref/ref_dump (make -C oracle ref, where the reference's sources exist; Makefile.ref compiles with -DNDEBUG).  The
outputs are data only: the ALN and MQ lines of the reference's dump.  A case the reference dies on shows as the last read of a
short dump: this script then names it, and it has to leave nw_sets.py.  Run:  python tests/golden/make_nw_sets_golden.py
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import nw_sets as ns  # noqa
from ma_testlib import REF_DUMP, have_ref, write_case  # noqa

REF_DUMP_NW = REF_DUMP + "_nw"
from make_golden import gz  # noqa


def main():
    if not have_ref() or not os.path.exists(REF_DUMP_NW):
        sys.exit("oracle/_ref/ref_dump or ref_dump_nw missing: run `make -C oracle ref` where the reference's sources exist")
    ns.check()
    names, reads, hset_off, hseed_off, hset_soc, seeds = ns.case_batch()
    with tempfile.TemporaryDirectory() as tmp:
        case, sets = os.path.join(tmp, "nw_sets.case"), os.path.join(tmp, "nw_sets.sets")
        write_case(case, list(ns.genome()), reads)
        ns.write_sets_file(sets, reads, hset_off, hseed_off, hset_soc, seeds)
        for scoring, sc in ns.SCORINGS.items():
            out = ns.golden_path(scoring)[:-3]
            rc = subprocess.call([REF_DUMP_NW, "nwsets", case, "default", sets, out] + [str(v) for v in (sc or ())])
            done = sum(1 for line in open(out) if line.startswith("MQ "))
            if rc != 0 or done != len(reads):
                sys.exit("the reference ended with status %d on case %s (%d of %d reads dumped)" % (rc, names[min(done, len(names) - 1)],
                                                                                              done, len(reads)))
            if sc is None:
                plain = os.path.join(tmp, "plain.pipe")
                subprocess.check_call([REF_DUMP, "nwsets", case, "default", sets, plain])
                assert open(plain, "rb").read() == open(out, "rb").read(), "ref_dump and ref_dump_nw differ under the default scoring"
            gz(out)
            print("%s: %d reads, %d sets, %d bytes" % (os.path.basename(out) + ".gz", len(reads), len(hset_soc),
                                                       os.path.getsize(out + ".gz")))


if __name__ == "__main__":
    main()
