// ma_batch_state.h -- what a ma_batch holds that is VALID, written ONCE: which call makes which product, and which products a
// call takes away.  libma_amd.so (ma_amd/csrc/pipeline.hip and its launch_*.h) keeps one BatchState per batch and touches the
// validity of a product through drop( ) / newReads( ) / finish( ) only; tests/emul/batch_state_test.cpp drives the same functions on
// the host.  Plain C++: no HIP, no containers, no strings.
//
// The products and their order -- dropping one drops everything to its right:
//
//   reads ─ names
//   reads ─ SEEDED ─ EXTRACTED ─ CHAINED ─ ALIGNED ─ inversion view ─┬─ single-end text (needs names) ─ its BGZF members
//                                                                   └─ pairs ─ pairs' text (needs names) ─ its BGZF members
//
// Every entry point that makes product X follows one pattern:
//   enter   drop( X ), after the argument checks that must not disturb the batch and before the first device write or counter reset
//   finish  finish( X ) on success
//   an early `return 1` in between needs no bookkeeping: the batch is left at "X and what depends on it are gone"
//
//   call                                          drops on entry                      establishes on success
//   every form of new reads                       everything (newReads)               the reads; a text form: NAMES;
//                                                                                     ma_batch_set_mates_bgzf: the mates' rest
//   ma_batch_set_read_text                        NAMES: both texts and members       NAMES
//   ma_seed_batch, ma_batch_set_segments          SEEDED and later                    SEEDED
//   ma_extract_seeds_batch, ma_batch_set_seeds    EXTRACTED and later (socGiven too)  EXTRACTED
//   ma_batch_set_soc_heap                         as ma_batch_set_seeds               EXTRACTED + giveSocs
//   ma_chain_batch, ma_batch_set_hsets            CHAINED and later                   CHAINED
//   ma_batch_set_hsets, refused                   CHAINED and later                   nothing
//   ma_dp_batch, ma_batch_set_alignments          ALIGNED and later                   ALIGNED
//   ma_inversions_batch                           INVERSIONS and later, not ALIGNED   INVERSIONS
//   ma_pair_batch                                 PAIRS, PAIR_SAM (+ members);        PAIRS
//                                                 not SAM, not INVERSIONS
//   ma_sam_batch / ma_pair_sam_batch              that text and its members           that text
//   ma_sam_bgzf_batch                             that text's members                 those members
//
// The reads themselves have no flag: a batch has the reads that were installed last (ma_batch::d_roff says whether any were).
// INVERSIONS is "ma_inversions_batch ran on these lists"; the list view every later stage reads exists from ALIGNED on (the
// MappingQuality lists until an inversion record is kept: invFinal).  A hand-in call (ma_batch_set_segments / _seeds / _soc_heap /
// _hsets / _alignments) makes the stage jump to the product handed in, whatever the stage was: finish( ) of a stage marks the
// stages before it too, and what those hold is not specified -- the hand-in calls reset the device counters the earlier stages
// left (the segment count among them) -- and not modelled here.
//
// The counts that mean something only while a product is valid live here and are zeroed by its drop; the code that makes the
// product writes them before finish( ).
#pragma once
#include <initializer_list>
#include <stdint.h>

namespace ma_state
{
enum Product : int
{
    NAMES, // the reads' names and qualities
    SEEDED, // the four stages, in order
    EXTRACTED,
    CHAINED,
    ALIGNED,
    INVERSIONS,
    SAM, // the single-end text, its BGZF members
    SAM_BGZF,
    PAIRS,
    PAIR_SAM, // the pairs' text, its BGZF members
    PAIR_SAM_BGZF,
    N_PRODUCTS
};

constexpr unsigned bit( Product p )
{
    return 1u << p;
}
// the members of a text (SAM, PAIR_SAM)
constexpr Product membersOf( Product text )
{
    return Product( text + 1 );
}

// what depends DIRECTLY on a product: the diagram above, edge by edge
constexpr unsigned NEXT[ N_PRODUCTS ] = {
    /* NAMES */ bit( SAM ) | bit( PAIR_SAM ),
    /* SEEDED */ bit( EXTRACTED ),
    /* EXTRACTED */ bit( CHAINED ),
    /* CHAINED */ bit( ALIGNED ),
    /* ALIGNED */ bit( INVERSIONS ),
    /* INVERSIONS */ bit( SAM ) | bit( PAIRS ),
    /* SAM */ bit( SAM_BGZF ),
    /* SAM_BGZF */ 0,
    /* PAIRS */ bit( PAIR_SAM ),
    /* PAIR_SAM */ bit( PAIR_SAM_BGZF ),
    /* PAIR_SAM_BGZF */ 0 };

// a product and everything that depends on it (every edge points to a later product: one pass in order closes the set)
constexpr unsigned withDependents( Product p )
{
    unsigned m = bit( p );
    for( int q = p; q < N_PRODUCTS; q++ )
        if( m & ( 1u << q ) )
            m |= NEXT[ q ];
    return m;
}

struct TextCounts
{
    uint64_t bytes = 0, zMembers = 0, zBytes = 0; // of the text; of its members
};

struct BatchState
{
    unsigned valid = 0; // bit( p ) for every valid product
    // NAMES
    bool hasQual = false;
    uint64_t nameBytes = 0;
    // the reads came from ma_batch_set_mates_bgzf: the two inflated texts are still in the text buffer, and ma_batch_get_mates_rest
    // serves what of each lies beyond the last pair (offset and bytes).  No product: nothing depends on it; every form of new
    // reads takes it away (newReads: ma_batch_set_reads, _set_reads_device, _use_staged_reads, _set_reads_text, _set_reads_bgzf,
    // _set_mates_text, _set_mates_bgzf, refused or not).  ma_batch_set_read_text does not: it replaces names and qualities, not
    // the reads, and does not touch the text buffer the rest lies in
    bool matesRest = false;
    uint64_t restAt[ 2 ] = { 0, 0 }, restBytes[ 2 ] = { 0, 0 };
    // SEEDED: segments; the pool may hold segments that carry a position instead of rows (seeding.h: text mode)
    uint64_t nSegs = 0;
    bool segMarked = false;
    // EXTRACTED: seeds; the SoC queues were swept elsewhere (ma_batch_set_soc_heap) and ma_chain_batch only harmonizes
    uint64_t nSeeds = 0;
    bool socGiven = false;
    // CHAINED (ma_batch_set_alignments: nHsets = the alignments handed in)
    uint64_t nHsets = 0, nHseeds = 0;
    // ALIGNED
    uint64_t nJobSlots = 0;
    // INVERSIONS
    uint64_t invCands = 0, invJobsN = 0, invRecs = 0, invOps = 0;
    // PAIRS
    uint64_t pairRecs = 0, pairNOps = 0, pairOnHost = 0;
    // SAM / SAM_BGZF, PAIR_SAM / PAIR_SAM_BGZF
    TextCounts sam, pairSam;

    bool has( Product p ) const
    {
        return ( valid & bit( p ) ) != 0;
    }
    // the list view is on the final lists of ma_inversions_batch, which kept at least one record
    bool invFinal( ) const
    {
        return has( INVERSIONS ) && invRecs != 0;
    }
    TextCounts& text( Product t )
    {
        return t == SAM ? sam : pairSam;
    }

    // enter: p and everything that depends on it are gone, their counts with them
    void drop( Product p )
    {
        const unsigned gone = withDependents( p );
        valid &= ~gone;
        if( gone & bit( NAMES ) )
            hasQual = false, nameBytes = 0;
        if( gone & bit( SEEDED ) )
            nSegs = 0, segMarked = false;
        if( gone & bit( EXTRACTED ) )
            nSeeds = 0, socGiven = false;
        if( gone & bit( CHAINED ) )
            nHsets = nHseeds = 0;
        if( gone & bit( ALIGNED ) )
            nJobSlots = 0;
        if( gone & bit( INVERSIONS ) )
            invCands = invJobsN = invRecs = invOps = 0;
        if( gone & bit( PAIRS ) )
            pairRecs = pairNOps = pairOnHost = 0;
        for( Product t : { SAM, PAIR_SAM } )
        {
            if( gone & bit( t ) )
                text( t ).bytes = 0;
            if( gone & bit( membersOf( t ) ) )
                text( t ).zMembers = text( t ).zBytes = 0;
        }
    }
    // the batch gets other reads: nothing of the reads before is left
    void newReads( )
    {
        drop( NAMES );
        drop( SEEDED );
        matesRest = false;
        restAt[ 0 ] = restAt[ 1 ] = restBytes[ 0 ] = restBytes[ 1 ] = 0;
    }
    // ma_batch_set_mates_bgzf on success, behind finish( NAMES ): where in the text buffer the records beyond the last pair are
    void keepMatesRest( const uint64_t at[ 2 ], const uint64_t bytes[ 2 ] )
    {
        matesRest = true;
        restAt[ 0 ] = at[ 0 ], restAt[ 1 ] = at[ 1 ];
        restBytes[ 0 ] = bytes[ 0 ], restBytes[ 1 ] = bytes[ 1 ];
    }
    // finish: p is valid; a stage brings the stages before it
    void finish( Product p )
    {
        valid |= bit( p );
        if( p >= SEEDED && p <= ALIGNED )
            valid |= ( bit( p ) - 1 ) & ~( bit( SEEDED ) - 1 );
    }
    // ma_batch_set_soc_heap behind finish( EXTRACTED ); ma_seed_batch's text mode behind drop( SEEDED ), seg_materialise after it
    void giveSocs( )
    {
        socGiven = true;
    }
    void markSegments( bool marked )
    {
        segMarked = marked;
    }
};
} // namespace ma_state
