// TEST INFRASTRUCTURE ONLY -- ref_dump with the reference's Alignment, NeedlemanWunsch and MappingQuality sources compiled into
// the SAME translation unit (oracle/_ref/ref_dump_nw, Makefile.ref), for `nwsets` with a scoring that is not the default.
//
// Why: the reference declares its global parameters as `const std::shared_ptr<GlobalParameter> pGlobalParams` in a header
// (ms/util/parameter.h:1064).  A const object at namespace scope has internal linkage, so every translation unit gets a
// GlobalParameter of its own.  ref_dump sets match / mismatch / gap / extend in ITS copy: NeedlemanWunsch's constructor is
// inline and reads that copy for kswcpp, while Alignment::append (alignment.cpp) and MappingQuality::execute
// (mappingQuality.cpp), compiled into libma_ref.so, keep scoring with the defaults of theirs -- a dump in which the DP runs
// under one scoring and the alignments are scored under another.  Here the three sources see the one copy ref_dump sets, which is
// what "global" means; with the default scoring both binaries write the same bytes (make_nw_sets_golden.py asserts it).
// Nothing of the reference is copied: its sources are included where they lie.
#include "container/alignment.cpp"
#include "module/mappingQuality.cpp"
#include "module/needlemanWunsch.cpp"

#include "ref_dump.cpp"
