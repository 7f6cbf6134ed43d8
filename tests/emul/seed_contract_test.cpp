// seed_contract_test.cpp -- the contract of ma_batch_set_seeds and ma_batch_set_soc_heap (ma_amd/host/ma_seed_contract.h) on the host,
// clause by clause: a small batch that keeps it, then one violation at a time with the message the library would give, and the
// seeds the contract must NOT refuse (a match across a contig border, across the strand junction, a mirrored seed at both ends of
// the text).  Prints "seed_contract ok: N refusals, M accepted" as its last line; a mismatch ends it with exit status 1.
#include "ma_seed_contract.h"
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

static int fails = 0, refusals = 0, accepted = 0;

// three contigs of 100, 40 and 60 bases: F = 200, n = 400; reads of 50, 30 and 0 bases
static const uint64_t CSTART[ 3 ] = { 0, 100, 140 }, F = 200, ROFF[ 4 ] = { 0, 50, 80, 80 };

static ma_seed seed( int64_t q, int64_t len, int64_t r, uint32_t fwd, uint64_t qlen )
{
    ma_seed s;
    memset( &s, 0, sizeof( s ) );
    s.q_start = q, s.len = len, s.r_start = r, s.ambiguity = 1, s.on_forward = fwd;
    const uint64_t contig = r >= 140 ? 2 : ( r >= 100 ? 1 : 0 );
    s.delta = r + ( (int64_t)qlen - q ) + (int64_t)( ( qlen + 1 ) * contig );
    return s;
}
struct Batch
{
    std::vector<uint64_t> off{ 0, 3, 5, 5 };
    std::vector<ma_seed> seeds{ seed( 0, 20, 10, 1, 50 ), seed( 25, 25, 120, 1, 50 ), seed( 5, 10, 150, 0, 50 ), seed( 0, 30, 0, 1, 30 ),
                                seed( 29, 1, 199, 0, 30 ) };
    std::vector<uint64_t> socOff{ 0, 2, 3, 3 };
    std::vector<ma_soc> socs;
    Batch( )
    {
        socs.resize( 3 );
        memset( socs.data( ), 0, 3 * sizeof( ma_soc ) );
        socs[ 0 ].begin = 0, socs[ 0 ].end = 2, socs[ 0 ].n_seeds = 2;
        socs[ 1 ].begin = 2, socs[ 1 ].end = 3, socs[ 1 ].n_seeds = 1;
        socs[ 2 ].begin = 0, socs[ 2 ].end = 2, socs[ 2 ].n_seeds = 2;
    }
    std::string seedsMsg( ) const
    {
        return ma_contract::seeds_violation( off.data( ), seeds.data( ), 3, ROFF, CSTART, 3, F );
    }
    std::string socsMsg( ) const
    {
        return ma_contract::socs_violation( socOff.data( ), socs.data( ), off.data( ), 3 );
    }
};

static void expect( const char* what, const std::string& got, const std::string& want )
{
    if( got != want )
    {
        printf( "FAILED %s: \"%s\", expected \"%s\"\n", what, got.c_str( ), want.c_str( ) );
        fails++;
    }
    else if( want.empty( ) )
        accepted++;
    else
        refusals++;
}
static void seedCase( const char* what, const std::function<void( Batch& )>& change, const std::string& want )
{
    Batch b;
    change( b );
    expect( what, b.seedsMsg( ), want );
}
static void socCase( const char* what, const std::function<void( Batch& )>& change, const std::string& want )
{
    Batch b;
    change( b );
    expect( what, b.socsMsg( ), want );
}

int main( )
{
    seedCase( "the batch as it is", []( Batch& ) {}, "" );
    seedCase( "no seeds at all", []( Batch& b ) { b.off = { 0, 0, 0, 0 }; }, "" );
    // ---- offsets
    seedCase( "offsets start behind 0", []( Batch& b ) { b.off[ 0 ] = 1; }, "seed_off does not start at 0" );
    seedCase( "offsets decrease", []( Batch& b ) { b.off[ 2 ] = 2; }, "seed_off decreases at read 1" );
    seedCase( "offsets decrease at the last read", []( Batch& b ) { b.off[ 3 ] = 4; }, "seed_off decreases at read 2" );
    // ---- fields
    seedCase( "negative q_start", []( Batch& b ) { b.seeds[ 1 ].q_start = -1; }, "negative field (read 0, seed 1)" );
    seedCase( "negative len", []( Batch& b ) { b.seeds[ 3 ].len = -5; }, "negative field (read 1, seed 0)" );
    seedCase( "negative r_start", []( Batch& b ) { b.seeds[ 0 ].r_start = -1; }, "negative field (read 0, seed 0)" );
    seedCase( "negative delta", []( Batch& b ) { b.seeds[ 4 ].delta = -1; }, "negative field (read 1, seed 1)" );
    seedCase( "len 0", []( Batch& b ) { b.seeds[ 2 ].len = 0; }, "empty seed (read 0, seed 2)" );
    seedCase( "one base beyond the read", []( Batch& b ) { b.seeds[ 1 ].len = 26; }, "seed ends beyond its read of 50 bases (read 0, seed 1)" );
    seedCase( "q_start beyond the read", []( Batch& b ) { b.seeds[ 4 ].q_start = 31; }, "seed ends beyond its read of 30 bases (read 1, seed 1)" );
    seedCase( "a seed of a read without bases", []( Batch& b ) { b.off[ 3 ] = 6, b.seeds.push_back( seed( 0, 1, 10, 1, 0 ) ); },
              "seed ends beyond its read of 0 bases (read 2, seed 0)" );
    seedCase( "on_forward 2", []( Batch& b ) { b.seeds[ 0 ].on_forward = 2; }, "on_forward is neither 0 nor 1 (read 0, seed 0)" );
    seedCase( "r_start at F", []( Batch& b ) { b.seeds[ 0 ] = seed( 0, 20, 200, 1, 50 ); }, "r_start outside the forward text of 200 bases (read 0, seed 0)" );
    seedCase( "an un-mirrored reverse seed", []( Batch& b ) { b.seeds[ 2 ] = seed( 5, 10, 249, 0, 50 ); },
              "r_start outside the forward text of 200 bases (read 0, seed 2)" );
    seedCase( "a mirrored seed that starts before the text's end and ends behind it", []( Batch& b ) { b.seeds[ 2 ] = seed( 5, 10, 8, 0, 50 ); },
              "seed ends beyond the doubled text of 400 bases (read 0, seed 2)" );
    // ---- delta
    seedCase( "delta one too large", []( Batch& b ) { b.seeds[ 1 ].delta++; }, "delta is 197, ExtractSeeds computes 196 (read 0, seed 1)" );
    seedCase( "delta without the contig's share", []( Batch& b ) { b.seeds[ 1 ].delta -= 51; }, "delta is 145, ExtractSeeds computes 196 (read 0, seed 1)" );
    seedCase( "delta of the un-mirrored position", []( Batch& b ) { b.seeds[ 4 ].delta += 1; }, "delta is 263, ExtractSeeds computes 262 (read 1, seed 1)" );
    // ---- what the reference's extraction can produce and the contract therefore takes
    seedCase( "a seed across a contig border", []( Batch& b ) { b.seeds[ 0 ] = seed( 0, 20, 90, 1, 50 ); }, "" );
    seedCase( "a seed across the strand junction", []( Batch& b ) { b.seeds[ 0 ] = seed( 0, 20, 190, 1, 50 ); }, "" );
    seedCase( "a forward seed on the last base", []( Batch& b ) { b.seeds[ 0 ] = seed( 0, 1, 199, 1, 50 ); }, "" );
    seedCase( "a mirrored seed that ends on the last base of the doubled text", []( Batch& b ) { b.seeds[ 2 ] = seed( 5, 10, 9, 0, 50 ); }, "" );
    seedCase( "a mirrored seed at the junction", []( Batch& b ) { b.seeds[ 2 ] = seed( 5, 10, 199, 0, 50 ); }, "" );
    seedCase( "first base of a contig", []( Batch& b ) { b.seeds[ 0 ] = seed( 0, 20, 100, 1, 50 ), b.seeds[ 1 ] = seed( 0, 20, 140, 1, 50 ); }, "" );
    seedCase( "duplicated seeds", []( Batch& b ) { b.seeds[ 1 ] = b.seeds[ 0 ]; }, "" );
    // ---- strips
    socCase( "the strips as they are", []( Batch& ) {}, "" );
    socCase( "no strips", []( Batch& b ) { b.socOff = { 0, 0, 0, 0 }; }, "" );
    socCase( "strip offsets start behind 0", []( Batch& b ) { b.socOff[ 0 ] = 1; }, "soc_off does not start at 0" );
    socCase( "strip offsets decrease", []( Batch& b ) { b.socOff[ 2 ] = 1; }, "soc_off decreases at read 1" );
    socCase( "more strips than seeds", []( Batch& b ) { b.socOff = { 0, 0, 3, 3 }; }, "more strips than seeds (read 1)" );
    socCase( "a strip of a read without seeds", []( Batch& b ) { b.socOff = { 0, 2, 2, 3 }; }, "more strips than seeds (read 2)" );
    socCase( "begin behind end", []( Batch& b ) { b.socs[ 1 ].begin = 3, b.socs[ 1 ].end = 2; }, "strip outside the read's 3 seeds (read 0, strip 1)" );
    socCase( "end behind the read's seeds", []( Batch& b ) { b.socs[ 2 ].end = 3, b.socs[ 2 ].n_seeds = 3; }, "strip outside the read's 2 seeds (read 1, strip 0)" );
    socCase( "n_seeds is not the range", []( Batch& b ) { b.socs[ 0 ].n_seeds = 3; }, "n_seeds is not end - begin (read 0, strip 0)" );
    socCase( "an empty strip", []( Batch& b ) { b.socs[ 1 ].begin = 3, b.socs[ 1 ].n_seeds = 0; }, "" );
    if( fails )
        return 1;
    printf( "seed_contract ok: %d refusals, %d accepted\n", refusals, accepted );
    return 0;
}
