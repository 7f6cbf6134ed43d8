#!/usr/bin/env python3
"""Generates the harm_sets.* goldens: the compiled reference's own StripOfConsiderationSeeds::execute + Harmonization::execute on
the hand-made seeds of tests/harm_sets.py (ref_dump chainseeds), one file per parameter set that the reference's
ParameterSetManager can express (harm_sets.ORACLE_ONLY names the others).

Needs oracle/_ref/ref_dump (make -C oracle ref, where the reference's sources exist; Makefile.ref compiles with -DNDEBUG).  The
outputs are data only: the R, HARM, h and g lines of the reference's dump.  A case the reference dies on shows as the last read
of a short dump: this script then names it, and it has to leave harm_sets.py.  Run:  python tests/golden/make_harm_sets_golden.py
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import harm_sets as hs  # noqa
from ma_testlib import REF_DUMP, have_ref, write_case  # noqa
from make_golden import gz  # noqa


def reference_dump(pset, tmp):
    """The reference's dump of a parameter set's batch as text; ends the program naming the case if the reference ended early."""
    names, reads, read_lens, seed_off, seeds = hs.case_batch(pset)
    case, sf, out = (os.path.join(tmp, "harm_sets.%s.%s" % (pset, e)) for e in ("case", "seeds", "pipe"))
    write_case(case, list(hs.genome()), reads)
    hs.write_seeds_file(sf, seed_off, seeds)
    rc = subprocess.call([REF_DUMP, "chainseeds", case, hs.PARAM_SETS[pset][0], str(hs.SRAND_SEED), sf, out] + hs.param_args(pset))
    done = sum(1 for line in open(out) if line.startswith("HARM ")) if os.path.exists(out) else 0
    if rc != 0 or done != len(reads):
        sys.exit("the reference ended with status %d on case %s of set %s (%d of %d reads dumped)" % (rc, names[min(done, len(names) - 1)], pset,
                                                                                                  done, len(reads)))
    return out


def main():
    if not have_ref():
        sys.exit("oracle/_ref/ref_dump missing: run `make -C oracle ref` where the reference's sources exist")
    hs.check()
    with tempfile.TemporaryDirectory() as tmp:
        for pset in hs.PARAM_SETS:
            if pset in hs.ORACLE_ONLY:
                continue
            out = reference_dump(pset, tmp)
            dst = hs.golden_path(pset)[:-3]
            os.replace(out, dst)
            gz(dst)
            print("%s: %d reads, %d bytes" % (os.path.basename(dst) + ".gz", len(hs.cases_of(pset)), os.path.getsize(dst + ".gz")))


if __name__ == "__main__":
    main()
