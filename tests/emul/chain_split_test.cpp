// chain_split_test.cpp -- the host-checkable parts of the short-read chain stage (ma_amd/csrc/chain.h), stand-alone:
//   1. chain_read_one (what k_chain_split answers for a read of at most one seed) against chain_read itself, record by record,
//      over the parameter grid;
//   2. chain_scratch_carve (one scratch block per read): alignment, no two arrays of a read and no two reads overlap, and every
//      array can be written in full;
//   3. GlibcRand as a counter into a table of the first K draws, K shrunk to 4, against the ring-only generator and libc's
//      rand( ) for 10 000 draws.
// Prints "chain_split ok: ..." as its last line; any mismatch ends it with a message and exit status 1.
#include "../../ma_amd/csrc/chain.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace ma;

static int fails = 0;
#define CHECK( c, ... )                                                                                                          \
    do                                                                                                                           \
    {                                                                                                                            \
        if( !( c ) )                                                                                                             \
        {                                                                                                                        \
            printf( "FAILED %s:%d %s: ", __FILE__, __LINE__, #c );                                                               \
            printf( __VA_ARGS__ );                                                                                               \
            printf( "\n" );                                                                                                      \
            if( ++fails > 20 )                                                                                                   \
                exit( 1 );                                                                                                       \
        }                                                                                                                        \
    } while( 0 )

// glibc srandom_r + 310 discards (stdlib/random_r.c): the state after srand( seed )
static void srand_ring( u32 seed, u32 ring[ 31 ] )
{
    if( seed == 0 )
        seed = 1;
    i32 word = (i32)seed;
    ring[ 0 ] = (u32)word;
    for( int i = 1; i < 31; i++ )
    {
        const long hi = word / 127773, lo = word % 127773;
        word = (i32)( 16807 * lo - 2836 * hi );
        if( word < 0 )
            word += 2147483647;
        ring[ i ] = (u32)word;
    }
    int f = 3, r = 0;
    for( int i = 0; i < 310; i++ )
    {
        ring[ f ] += ring[ r ];
        if( ++f >= 31 )
            f = 0;
        if( ++r >= 31 )
            r = 0;
    }
}

// ---- 1. one-seed answers
struct OneOut
{
    u32 nsets = 0, err = 0;
    unsigned long long poolUsed = 0;
    std::vector<HSet> sets;
    std::vector<ma_seed> local, pool;
};
static const u32 SET_SLOTS = 24, LOCAL_SLOTS = 3, POOL_SLOTS = 8;
static void prepare( OneOut& o )
{
    o.sets.resize( SET_SLOTS );
    o.local.resize( LOCAL_SLOTS );
    o.pool.resize( POOL_SLOTS );
    memset( o.sets.data( ), 0xAB, SET_SLOTS * sizeof( HSet ) );
    memset( o.local.data( ), 0xCD, LOCAL_SLOTS * sizeof( ma_seed ) );
    memset( o.pool.data( ), 0xEF, POOL_SLOTS * sizeof( ma_seed ) );
}
static ChainOut sink( OneOut& o, u32 setCap, u32 n, bool withLocal )
{
    ChainOut O;
    O.pool = o.pool.data( );
    O.pool_cap = POOL_SLOTS;
    O.pool_used = &o.poolUsed;
    O.sets = o.sets.data( );
    O.set_cap = setCap;
    O.local = withLocal ? o.local.data( ) : nullptr;
    O.local_cap = withLocal ? 3 * n : 0;
    return O;
}
static u64 one_seed_grid( )
{
    const u64 cstart[ 2 ] = { 0, 600000 }, clen[ 2 ] = { 600000, 400000 };
    IndexView X{ };
    X.cstart = cstart, X.clen = clen, X.n_contigs = 2, X.F = 1000000, X.n = 2000000;
    u32 ring[ 31 ];
    srand_ring( 1, ring );
    u32 table[ MA_RNG_TAB_WORDS( MA_RNG_TAB ) ];
    fill_rand_table( ring, table, MA_RNG_TAB );
    u64 cases = 0, kept = 0, dropped = 0, writtenButDropped = 0;
    for( int nSeeds = 0; nSeeds <= 1; nSeeds++ )
    for( int fwd = 0; fwd <= 1; fwd++ )
    for( u64 len : { 1ull, 11ull, 150ull } )
    for( u32 hsm : { 0u, 18u } )
    for( double rel : { 0.0, 0.5 } )
    for( u64 gsd : { 1000ull, 5000000ull } ) // genome_size_disable below / above the text's 2 000 000 positions
    for( u32 minSoc : { 0u, 1u } )
    for( u32 maxSoc : { 0u, 1u, 10u } )
    for( u32 noHeur : { 0u, 1u } )
    for( u32 switchQ : { 0u, 100u, 1000u } ) // below, above the read's length: the `repeat` bookkeeping
    for( double diffTol : { 0.0001, 0.01 } ) // 150 * tol below / above a seed of length 1
    for( u32 qlen : { 150u, 12u } )
    for( int withLocal = 1; withLocal >= 0; withLocal-- )
    {
        if( len > qlen )
            continue;
        ChainParams P;
        P.max_num_soc = maxSoc, P.min_num_soc = minSoc, P.harm_score_min = hsm, P.max_score_lookahead = 3, P.switch_qlen = switchQ;
        P.min_delta_dist = 16, P.sv_penalty = 100, P.match = 2, P.gap = 4, P.extend = 2, P.disable_heuristics = noHeur, P.soc_width = 0;
        P.genome_size_disable = gsd, P.harm_score_min_rel = rel, P.soc_score_decrease_tol = 0.1, P.score_diff_tol = diffTol;
        P.max_delta_dist = 0.1, P.libm_probe = 0;
        memcpy( P.rng_ring, ring, sizeof( ring ) );
        P.rng_tab_n = MA_RNG_TAB, P.rng_tab = table;
        ma_seed s;
        memset( &s, 0, sizeof( s ) );
        s.q_start = (i64)( qlen - len ), s.len = (i64)len, s.ambiguity = 1, s.on_forward = (u32)fwd;
        // a forward seed on the second contig; a reverse-strand one at its mirrored position (r_start >= F)
        s.r_start = fwd ? 700123 : (i64)( X.n - 700123 - len );
        s.delta = s.r_start - s.q_start + 150;
        const u32 setCap = 2 * maxSoc;
        // chain_read on scratch carved for this read
        OneOut want, got;
        prepare( want ), prepare( got );
        std::vector<uint8_t> scratch( (size_t)( 7 + 1 + 1 ) * MA_CHAIN_SCRATCH_B + 8 );
        ChainScratch C = chain_scratch_carve( scratch.data( ), 7, (u32)nSeeds ); // (vector storage: aligned for every type)
        if( nSeeds )
            C.work[ 0 ] = s;
        want.nsets = chain_read( X, P, C, (u32)nSeeds, qlen, sink( want, setCap, (u32)nSeeds, withLocal != 0 ), want.err );
        got.nsets = chain_read_one( X, P, &s, (u32)nSeeds, qlen, sink( got, setCap, (u32)nSeeds, withLocal != 0 ), got.err );
        const bool same = want.nsets == got.nsets && want.err == got.err && want.poolUsed == got.poolUsed &&
                          !memcmp( want.sets.data( ), got.sets.data( ), SET_SLOTS * sizeof( HSet ) ) &&
                          !memcmp( want.local.data( ), got.local.data( ), LOCAL_SLOTS * sizeof( ma_seed ) ) &&
                          !memcmp( want.pool.data( ), got.pool.data( ), POOL_SLOTS * sizeof( ma_seed ) );
        CHECK( same, "n %d fwd %d len %llu hsm %u rel %g gsd %llu min %u max %u noHeur %u switch %u tol %g qlen %u local %d: nsets %u / %u err %u / %u",
               nSeeds, fwd, (unsigned long long)len, hsm, rel, (unsigned long long)gsd, minSoc, maxSoc, noHeur, switchQ, diffTol, qlen, withLocal,
               want.nsets, got.nsets, want.err, got.err );
        cases++;
        kept += want.nsets;
        dropped += nSeeds && !want.nsets;
        HSet untouched;
        memset( &untouched, 0xAB, sizeof( untouched ) );
        writtenButDropped += !want.nsets && setCap && memcmp( &want.sets[ 0 ], &untouched, sizeof( HSet ) ) != 0;
        if( want.nsets && nSeeds && !fwd && withLocal ) // the un-mirroring reached the output
            CHECK( (u64)want.local[ 0 ].r_start == X.n - (u64)s.r_start - 1 && want.sets[ 0 ].soc == 0, "reverse seed" );
    }
    // the grid reaches every outcome: kept, dropped before emit, and emitted but taken back by the repeat loop
    CHECK( kept > 0 && dropped > 0 && writtenButDropped > 0, "kept %llu dropped %llu written-but-dropped %llu", (unsigned long long)kept,
           (unsigned long long)dropped, (unsigned long long)writtenButDropped );
    return cases;
}

// ---- 2. the carving
struct Range
{
    uintptr_t b, e;
    size_t align;
    const char* name;
};
static std::vector<Range> ranges_of( const ChainScratch& C, u64 n )
{
#define R( f, T, k ) Range{ (uintptr_t)C.f, (uintptr_t)C.f + ( k ) * n * sizeof( T ), alignof( T ), #f }
    return { R( work, ma_seed, 1 ), R( maxima, SoCEntry, 1 ), R( mm, RefMinMax, 1 ), R( setA, ma_seed, 1 ), R( setB, ma_seed, 1 ),
             R( outA, ma_seed, 1 ), R( sh1, Shadow, 1 ), R( sh2, Shadow, 1 ), R( vX, double, 3 ), R( vY, double, 3 ), R( med, double, 6 ),
             R( inl, i32, 3 ), R( best, i32, 3 ) };
#undef R
}
static u64 carving( )
{
    const u32 counts[] = { 0, 1, 2, 3, 17, 1000, 0, 1, 3 };
    const size_t nReads = sizeof( counts ) / sizeof( counts[ 0 ] );
    u64 total = 0;
    for( u32 c : counts )
        total += c;
    CHECK( MA_CHAIN_SCRATCH_B == 4 * sizeof( ma_seed ) + sizeof( SoCEntry ) + sizeof( RefMinMax ) + 2 * sizeof( Shadow ) + 12 * 8 + 6 * 4,
           "B %zu", (size_t)MA_CHAIN_SCRATCH_B );
    // (+ 1 seed as in ma_chain_batch; the buffer comes from operator new: aligned for every type, and ASan guards its ends)
    std::vector<uint8_t> buf( (size_t)( total + 1 ) * MA_CHAIN_SCRATCH_B );
    const uintptr_t lo = (uintptr_t)buf.data( ), hi = lo + buf.size( );
    std::vector<Range> all;
    u64 off = 0, checked = 0;
    for( size_t r = 0; r < nReads; r++ )
    {
        const u64 n = counts[ r ];
        const ChainScratch C = chain_scratch_carve( buf.data( ), off, (u32)n );
        const std::vector<Range> rs = ranges_of( C, n );
        u64 bytes = 0;
        for( size_t i = 0; i < rs.size( ); i++ )
        {
            CHECK( rs[ i ].b % rs[ i ].align == 0, "read %zu array %s misaligned", r, rs[ i ].name );
            CHECK( rs[ i ].b >= lo + off * MA_CHAIN_SCRATCH_B && rs[ i ].e <= lo + ( off + n ) * MA_CHAIN_SCRATCH_B && rs[ i ].e <= hi,
                   "read %zu array %s leaves the read's block", r, rs[ i ].name );
            for( size_t j = 0; j < i; j++ )
                CHECK( rs[ i ].e <= rs[ j ].b || rs[ j ].e <= rs[ i ].b, "read %zu arrays %s and %s overlap", r, rs[ i ].name, rs[ j ].name );
            bytes += rs[ i ].e - rs[ i ].b;
            // every byte of the array written with a tag of its own
            memset( (void*)rs[ i ].b, (int)( 1 + ( r * 13 + i ) % 250 ), rs[ i ].e - rs[ i ].b );
            checked++;
        }
        CHECK( bytes == n * MA_CHAIN_SCRATCH_B, "read %zu: arrays hold %llu bytes", r, (unsigned long long)bytes );
        for( const Range& x : rs )
            all.push_back( x );
        off += n;
    }
    // no write of one array landed in another (of the same read or of another read)
    for( size_t k = 0; k < all.size( ); k++ )
        for( uintptr_t p = all[ k ].b; p < all[ k ].e; p++ )
            if( *(const uint8_t*)p != (uint8_t)( 1 + k % 250 ) )
            {
                CHECK( false, "array %zu (%s) was overwritten", k, all[ k ].name );
                break;
            }
    return checked;
}

// ---- 3. the draw table
static u64 draws( )
{
    u64 n = 0;
    for( u32 seed : { 1u, 42u, 0u, 123456789u } )
    {
        u32 ring[ 31 ];
        srand_ring( seed, ring );
        for( u32 K : { 4u, 1u, 256u } )
        {
            std::vector<u32> tab( MA_RNG_TAB_WORDS( K ) );
            fill_rand_table( ring, tab.data( ), K );
            GlibcRand plain, tabled;
            plain.init( ring );
            tabled.init( ring, tab.data( ), K );
            srand( seed );
            for( int i = 0; i < 10000; i++, n++ )
            {
                const i32 a = plain.next( ), b = tabled.next( ), c = (i32)rand( );
                if( a != b || a != c )
                {
                    CHECK( false, "seed %u K %u draw %d: ring %d table %d libc %d", seed, K, i, a, b, c );
                    break;
                }
            }
        }
    }
    return n;
}

int main( )
{
    const u64 a = one_seed_grid( );
    const u64 b = carving( );
    const u64 c = draws( );
    if( fails )
        return 1;
    printf( "chain_split ok: %llu one-seed cases, %llu arrays carved, %llu draws\n", (unsigned long long)a, (unsigned long long)b,
            (unsigned long long)c );
    return 0;
}
