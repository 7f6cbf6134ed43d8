// batch_state_test.cpp -- the rules of ma_amd/host/ma_batch_state.h on the host: a state is driven through a full pass, then every
// row of the header's call table is applied to it, and the COMPLETE set of valid products is compared after "enter", after
// "enter + finish" and after "enter + an early return" (nothing more happens) with the sets written out below.  The expected sets
// are literals: nothing here is computed by the header under test.
//   build: g++ -std=c++17 -Wall -I ma_amd/host tests/emul/batch_state_test.cpp -o batch_state_test
#include "ma_batch_state.h"

#include <functional>
#include <stdio.h>
#include <string>
#include <vector>

using namespace ma_state;

static const char* const NAME[ N_PRODUCTS ] = { "names", "seeded", "extracted", "chained", "aligned", "inversions", "sam", "sam_bgzf", "pairs", "pair_sam", "pair_sam_bgzf" };

static std::string setOf( const BatchState& s )
{
    std::string out;
    for( int p = 0; p < N_PRODUCTS; p++ )
        if( s.has( Product( p ) ) )
            out += ( out.empty( ) ? "" : " " ) + std::string( NAME[ p ] );
    return out;
}

static int failures = 0;
static void expect( const std::string& what, const std::string& got, const std::string& want )
{
    if( got == want )
        return;
    failures++;
    printf( "FAIL %s:\n  got  {%s}\n  want {%s}\n", what.c_str( ), got.c_str( ), want.c_str( ) );
}
static void expect( const std::string& what, bool ok )
{
    if( !ok )
    {
        failures++;
        printf( "FAIL %s\n", what.c_str( ) );
    }
}

// every stage, the names, the inversions, the pairs, both texts and their members, with a count of each
static BatchState fullPass( )
{
    BatchState s;
    s.newReads( );
    s.drop( SEEDED ), s.nSegs = 11, s.finish( SEEDED );
    s.drop( EXTRACTED ), s.nSeeds = 12, s.finish( EXTRACTED );
    s.drop( CHAINED ), s.nHsets = 13, s.nHseeds = 14, s.finish( CHAINED );
    s.drop( ALIGNED ), s.nJobSlots = 15, s.finish( ALIGNED );
    s.drop( NAMES ), s.hasQual = true, s.nameBytes = 16, s.finish( NAMES );
    s.drop( INVERSIONS ), s.invCands = 17, s.invJobsN = 18, s.invRecs = 19, s.invOps = 20, s.finish( INVERSIONS );
    s.drop( PAIRS ), s.pairRecs = 21, s.pairNOps = 22, s.pairOnHost = 23, s.finish( PAIRS );
    s.drop( SAM ), s.sam.bytes = 24, s.finish( SAM );
    s.drop( PAIR_SAM ), s.pairSam.bytes = 25, s.finish( PAIR_SAM );
    s.drop( SAM_BGZF ), s.sam.zMembers = 26, s.sam.zBytes = 27, s.finish( SAM_BGZF );
    s.drop( PAIR_SAM_BGZF ), s.pairSam.zMembers = 28, s.pairSam.zBytes = 29, s.finish( PAIR_SAM_BGZF );
    return s;
}

struct Row
{
    const char* call;
    std::function<void( BatchState& )> enter, finish; // finish: what the call does on success (none: the call establishes nothing)
    const char* afterEnter; // = after an early return
    const char* afterFinish;
};

#define ALL_STAGES "seeded extracted chained aligned"
static const char* const FULL = "names " ALL_STAGES " inversions sam sam_bgzf pairs pair_sam pair_sam_bgzf";

// the table of ma_batch_state.h, each row on a batch that has been through the full pass
static const std::vector<Row> ROWS = {
    { "new reads (host arrays, staged, device arrays)", []( BatchState& s ) { s.newReads( ); }, []( BatchState& ) {}, "", "" },
    { "new reads (text, mates text, BGZF)", []( BatchState& s ) { s.newReads( ); }, []( BatchState& s ) { s.finish( NAMES ); }, "", "names" },
    { "new reads (refused text)", []( BatchState& s ) { s.newReads( ); }, nullptr, "", "" },
    { "ma_batch_set_read_text", []( BatchState& s ) { s.drop( NAMES ); }, []( BatchState& s ) { s.finish( NAMES ); },
      ALL_STAGES " inversions pairs", "names " ALL_STAGES " inversions pairs" },
    { "ma_seed_batch, ma_batch_set_segments", []( BatchState& s ) { s.drop( SEEDED ); }, []( BatchState& s ) { s.finish( SEEDED ); }, "names", "names seeded" },
    { "ma_extract_seeds_batch, ma_batch_set_seeds", []( BatchState& s ) { s.drop( EXTRACTED ); }, []( BatchState& s ) { s.finish( EXTRACTED ); },
      "names seeded", "names seeded extracted" },
    { "ma_batch_set_soc_heap", []( BatchState& s ) { s.drop( EXTRACTED ); }, []( BatchState& s ) { s.finish( EXTRACTED ), s.giveSocs( ); },
      "names seeded", "names seeded extracted" },
    { "ma_chain_batch, ma_batch_set_hsets", []( BatchState& s ) { s.drop( CHAINED ); }, []( BatchState& s ) { s.finish( CHAINED ); },
      "names seeded extracted", "names seeded extracted chained" },
    { "ma_batch_set_hsets, refused", []( BatchState& s ) { s.drop( CHAINED ); }, nullptr, "names seeded extracted", "names seeded extracted" },
    { "ma_dp_batch, ma_batch_set_alignments", []( BatchState& s ) { s.drop( ALIGNED ); }, []( BatchState& s ) { s.finish( ALIGNED ); },
      "names seeded extracted chained", "names " ALL_STAGES },
    // the first asymmetry: the lists the inversions scan stay
    { "ma_inversions_batch", []( BatchState& s ) { s.drop( INVERSIONS ); }, []( BatchState& s ) { s.finish( INVERSIONS ); },
      "names " ALL_STAGES, "names " ALL_STAGES " inversions" },
    // the second: the single-end text does not read the picks
    { "ma_pair_batch", []( BatchState& s ) { s.drop( PAIRS ); }, []( BatchState& s ) { s.finish( PAIRS ); },
      "names " ALL_STAGES " inversions sam sam_bgzf", "names " ALL_STAGES " inversions sam sam_bgzf pairs" },
    { "ma_sam_batch", []( BatchState& s ) { s.drop( SAM ); }, []( BatchState& s ) { s.finish( SAM ); },
      "names " ALL_STAGES " inversions pairs pair_sam pair_sam_bgzf", "names " ALL_STAGES " inversions sam pairs pair_sam pair_sam_bgzf" },
    { "ma_pair_sam_batch", []( BatchState& s ) { s.drop( PAIR_SAM ); }, []( BatchState& s ) { s.finish( PAIR_SAM ); },
      "names " ALL_STAGES " inversions sam sam_bgzf pairs", "names " ALL_STAGES " inversions sam sam_bgzf pairs pair_sam" },
    { "ma_sam_bgzf_batch (single-end text)", []( BatchState& s ) { s.drop( membersOf( SAM ) ); }, []( BatchState& s ) { s.finish( membersOf( SAM ) ); },
      "names " ALL_STAGES " inversions sam pairs pair_sam pair_sam_bgzf", FULL },
    { "ma_sam_bgzf_batch (pairs' text)", []( BatchState& s ) { s.drop( membersOf( PAIR_SAM ) ); }, []( BatchState& s ) { s.finish( membersOf( PAIR_SAM ) ); },
      "names " ALL_STAGES " inversions sam sam_bgzf pairs pair_sam", FULL },
};

int main( )
{
    expect( "a new state", setOf( BatchState( ) ), "" );
    expect( "the full pass", setOf( fullPass( ) ), FULL );
    for( const Row& r : ROWS )
    {
        BatchState s = fullPass( );
        r.enter( s );
        expect( std::string( r.call ) + ": enter (= enter + early return)", setOf( s ), r.afterEnter );
        if( r.finish )
            r.finish( s );
        expect( std::string( r.call ) + ": enter + finish", setOf( s ), r.afterFinish );
    }

    // the counts go with their product, and with no other
    {
        BatchState s = fullPass( );
        s.drop( PAIRS );
        expect( "ma_pair_batch zeroes the pairs' counts and the counts of their text",
                s.pairRecs == 0 && s.pairNOps == 0 && s.pairOnHost == 0 && s.pairSam.bytes == 0 && s.pairSam.zMembers == 0 && s.pairSam.zBytes == 0 );
        expect( "ma_pair_batch keeps the single-end text's counts and the inversions'",
                s.sam.bytes == 24 && s.sam.zMembers == 26 && s.sam.zBytes == 27 && s.invRecs == 19 && s.invOps == 20 && s.invFinal( ) );
        s.drop( SAM );
        expect( "ma_sam_batch zeroes the bytes of its text and of the members", s.sam.bytes == 0 && s.sam.zMembers == 0 && s.sam.zBytes == 0 );
        s = fullPass( );
        s.drop( SAM_BGZF );
        expect( "ma_sam_bgzf_batch zeroes the members' counts alone", s.sam.bytes == 24 && s.sam.zMembers == 0 && s.sam.zBytes == 0 && s.pairSam.zMembers == 28 );
        s.drop( INVERSIONS );
        expect( "ma_inversions_batch puts the list view back and keeps the lists' counts",
                !s.invFinal( ) && s.invCands == 0 && s.invJobsN == 0 && s.invRecs == 0 && s.invOps == 0 && s.nHsets == 13 && s.nJobSlots == 15 );
        s.finish( INVERSIONS );
        expect( "inversions that kept no record leave the view on the MappingQuality lists", s.has( INVERSIONS ) && !s.invFinal( ) );
        s.drop( ALIGNED );
        expect( "ma_dp_batch zeroes the job slots and keeps the sets", s.nJobSlots == 0 && s.nHsets == 13 && s.nHseeds == 14 );
        s.drop( CHAINED );
        expect( "ma_chain_batch zeroes the sets and keeps the seeds", s.nHsets == 0 && s.nHseeds == 0 && s.nSeeds == 12 );
        s.giveSocs( );
        s.drop( EXTRACTED );
        expect( "ma_extract_seeds_batch zeroes the seeds, forgets given SoC queues and keeps the segments", s.nSeeds == 0 && !s.socGiven && s.nSegs == 11 );
        s.markSegments( true );
        s.drop( SEEDED );
        expect( "ma_seed_batch zeroes the segments and their mark and keeps the names", s.nSegs == 0 && !s.segMarked && s.hasQual && s.nameBytes == 16 );
        s = fullPass( );
        s.drop( NAMES );
        expect( "ma_batch_set_read_text zeroes the names' counts and both texts', not the pairs'",
                !s.hasQual && s.nameBytes == 0 && s.sam.bytes == 0 && s.pairSam.bytes == 0 && s.sam.zBytes == 0 && s.pairSam.zBytes == 0 && s.pairRecs == 21 );
        s = fullPass( );
        s.newReads( );
        expect( "new reads zero every count", s.nSegs == 0 && s.nSeeds == 0 && s.nHsets == 0 && s.nHseeds == 0 && s.nJobSlots == 0 && s.invRecs == 0 &&
                                                  s.pairRecs == 0 && s.sam.bytes == 0 && s.pairSam.bytes == 0 && s.nameBytes == 0 && !s.hasQual && !s.socGiven );
    }

    // a hand-in call makes the stage jump to the product handed in, from wherever the batch was
    {
        BatchState s;
        s.newReads( );
        s.drop( CHAINED ), s.finish( CHAINED );
        expect( "ma_batch_set_hsets on new reads", setOf( s ), "seeded extracted chained" );
        s.drop( CHAINED );
        expect( "... and refused afterwards: at most EXTRACTED", setOf( s ), "seeded extracted" );
        s.newReads( );
        s.drop( ALIGNED ), s.finish( ALIGNED );
        expect( "ma_batch_set_alignments on new reads", setOf( s ), ALL_STAGES );
        s.newReads( );
        s.drop( EXTRACTED ), s.finish( EXTRACTED ), s.giveSocs( );
        expect( "ma_batch_set_soc_heap on new reads", setOf( s ), "seeded extracted" );
        expect( "... gives the SoC queues", s.socGiven );
        s.drop( EXTRACTED ), s.finish( EXTRACTED );
        expect( "ma_batch_set_seeds takes them back", !s.socGiven );
    }
    if( failures )
    {
        printf( "batch_state: %d failures\n", failures );
        return 1;
    }
    printf( "batch_state ok: %d rows\n", (int)ROWS.size( ) );
    return 0;
}
