// harm_census.cpp -- the chain stage (ma_amd/csrc/chain.h) on hand-made seeds (tests/harm_sets.py), stand-alone on the CPU:
// chain_read on every read of a case file + seeds file, the harmonized sets in the HARM lines of the pipe dump, and behind
// every read a line "B name=count ..." of the branches the read ran (CH_HIT / CH_HIT_IF in chain.h count here and expand to
// nothing everywhere else).  Every read runs three ways, which must agree record by record:
//   plain      chain_read sweeps for itself (k_chain, k_chain_list)
//   preswept   soc_windows over prefix sums on seeds sorted by delta beforehand, then chain_read with the strips given
//              (k_sort_seeds_wave + k_soc_windows + k_chain)
//   queue      soc_dump_read's heap layout and re-sorted seeds, then chain_read on the given queue (ma_batch_set_soc_heap)
// The branch counts are those of the plain run.  Every array has exactly the size the product carves for the read, so the
// sanitized build reports a read that leaves them.
//
// usage: harm_census <case> <seeds> <out> [name=value ...]     (names: the fields of ChainParams, srand_seed)
#include <map>
#include <string>
static std::map<std::string, unsigned long long> g_hits;
static bool g_count = false;
#define CH_HIT( name ) ( g_count ? (void)g_hits[ #name ]++ : (void)0 )
#define CH_HIT_IF( cond, name ) ( ( g_count && ( cond ) ) ? (void)g_hits[ #name ]++ : (void)0 )
#include "../../ma_amd/csrc/chain.h"
#include "../../oracle/dump_format.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace ma;

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

struct Result
{
    u32 nsets = 0, err = 0;
    std::vector<u32> soc;
    std::vector<std::vector<ma_seed>> sets;
    bool operator==( const Result& o ) const
    {
        if( nsets != o.nsets || err != o.err || soc != o.soc || sets.size( ) != o.sets.size( ) )
            return false;
        for( size_t k = 0; k < sets.size( ); k++ )
            if( sets[ k ].size( ) != o.sets[ k ].size( ) ||
                ( !sets[ k ].empty( ) && memcmp( sets[ k ].data( ), o.sets[ k ].data( ), sets[ k ].size( ) * sizeof( ma_seed ) ) ) )
                return false;
        return true;
    }
};

// the thirteen arrays of a read of n seeds, each of the size the product gives it
struct Scratch
{
    std::vector<ma_seed> work, setA, setB, outA;
    std::vector<SoCEntry> mx;
    std::vector<RefMinMax> mm;
    std::vector<Shadow> sh1, sh2;
    std::vector<double> vX, vY, med;
    std::vector<i32> inl, best;
    explicit Scratch( u32 n )
        : work( n ), setA( n ), setB( n ), outA( n ), mx( n ), mm( n ), sh1( n ), sh2( n ), vX( 3 * n ), vY( 3 * n ), med( 6 * n ), inl( 3 * n ),
          best( 3 * n )
    {}
    ChainScratch view( )
    {
        return ChainScratch{ work.data( ), mx.data( ), mm.data( ), setA.data( ), setB.data( ), outA.data( ), sh1.data( ),
                             sh2.data( ), vX.data( ), vY.data( ), med.data( ), inl.data( ), best.data( ) };
    }
};

enum Mode
{
    PLAIN,
    PRESWEPT,
    QUEUE
};

static Result run( const IndexView& X, const ChainParams& P, const std::vector<ma_seed>& seeds, u32 qlen, Mode mode )
{
    const u32 n = (u32)seeds.size( );
    Scratch S( n );
    std::copy( seeds.begin( ), seeds.end( ), S.work.begin( ) );
    const u32 setCap = 2 * P.max_num_soc;
    std::vector<HSet> sets( setCap );
    std::vector<ma_seed> pool( 3 * (size_t)n + 1 ), local( 3 * (size_t)n );
    unsigned long long used = 0;
    ChainOut O;
    O.pool = pool.data( ), O.pool_cap = pool.size( ), O.pool_used = &used, O.sets = sets.data( ), O.set_cap = setCap;
    O.local = local.data( ), O.local_cap = 3 * n;
    Result R;
    const ChainScratch C = S.view( );
    if( mode == PLAIN )
        R.nsets = chain_read( X, P, C, n, qlen, O, R.err );
    else if( mode == PRESWEPT )
    {
        // what the wave sort leaves: the permutation std::sort gives (the kernels are held to it by test_gpu_chain_seeds.py)
        if( n )
            ss::sort( S.work.data( ), (i64)n, SeedByDelta( ) );
        std::vector<u64> prefix( 2 * ( (size_t)n + 2 ) );
        const u32 nPre = n ? soc_windows( X, P, S.work.data( ), n, qlen, S.mx.data( ), S.mm.data( ), S.setA.data( ), true, n >= 2 ? prefix.data( ) : nullptr )
                           : 0;
        R.nsets = chain_read( X, P, C, n, qlen, O, R.err, nullptr, 0, true, nPre, false );
    }
    else
    {
        std::vector<ma_soc> heap( n );
        const u32 nq = soc_dump_read( X, P, S.work.data( ), n, qlen, S.mx.data( ), S.mm.data( ), heap.data( ), true );
        R.nsets = chain_read( X, P, C, n, qlen, O, R.err, heap.data( ), nq );
    }
    for( u32 k = 0; k < R.nsets && k < setCap; k++ )
    {
        const HSet& h = sets[ k ];
        const ma_seed* src = ( h.off & MA_HSET_LOCAL ) ? local.data( ) + ( h.off & ~MA_HSET_LOCAL ) : pool.data( ) + h.off;
        R.soc.push_back( h.soc );
        R.sets.emplace_back( src, src + h.cnt );
    }
    return R;
}

int main( int argc, char** argv )
{
    if( argc < 4 )
    {
        fprintf( stderr, "usage: harm_census <case> <seeds> <out> [name=value ...]\n" );
        return 2;
    }
    CaseFile c = readCase( argv[ 1 ] );
    ChainSeedsFile sf = readChainSeeds( argv[ 2 ] );
    if( sf.seedOff.size( ) != c.reads.size( ) + 1 )
    {
        fprintf( stderr, "seeds file and case differ in their number of reads\n" );
        return 2;
    }
    static_assert( sizeof( NwSetsSeed ) == sizeof( ma_seed ), "seed record" );
    std::vector<u64> cstart, clen;
    u64 F = 0;
    for( auto& g : c.contigs )
    {
        cstart.push_back( F );
        clen.push_back( g.size( ) );
        F += g.size( );
    }
    IndexView X{ };
    X.cstart = cstart.data( ), X.clen = clen.data( ), X.n_contigs = (u32)cstart.size( ), X.F = F, X.n = 2 * F;
    // the "default" preset (parameter.h:704-880)
    ChainParams P;
    P.max_num_soc = 30, P.min_num_soc = 1, P.harm_score_min = 18, P.max_score_lookahead = 3, P.switch_qlen = 800, P.min_delta_dist = 16;
    P.sv_penalty = 100, P.match = 2, P.gap = 4, P.extend = 2, P.disable_heuristics = 0, P.soc_width = 0, P.genome_size_disable = 10000000;
    P.harm_score_min_rel = 0.002, P.soc_score_decrease_tol = 0.1, P.score_diff_tol = 0.0001, P.max_delta_dist = 0.1, P.libm_probe = 0;
    u32 srandSeed = 1, tabN = MA_RNG_TAB;
    for( int a = 4; a < argc; a++ )
    {
        const char* eq = strchr( argv[ a ], '=' );
        if( !eq )
        {
            fprintf( stderr, "not name=value: %s\n", argv[ a ] );
            return 2;
        }
        const std::string k( argv[ a ], eq - argv[ a ] );
        const double v = atof( eq + 1 );
#define U32( f )                                                                                                                   \
    if( k == #f )                                                                                                                  \
    {                                                                                                                              \
        P.f = (u32)strtoul( eq + 1, nullptr, 10 );                                                                                 \
        continue;                                                                                                                  \
    }
#define F64( f )                                                                                                                   \
    if( k == #f )                                                                                                                  \
    {                                                                                                                              \
        P.f = v;                                                                                                                   \
        continue;                                                                                                                  \
    }
        U32( max_num_soc ) U32( min_num_soc ) U32( harm_score_min ) U32( max_score_lookahead ) U32( switch_qlen ) U32( min_delta_dist )
        U32( sv_penalty ) U32( match ) U32( gap ) U32( extend ) U32( disable_heuristics ) U32( soc_width ) U32( libm_probe )
        F64( harm_score_min_rel ) F64( soc_score_decrease_tol ) F64( score_diff_tol ) F64( max_delta_dist )
#undef U32
#undef F64
        if( k == "genome_size_disable" )
            P.genome_size_disable = strtoull( eq + 1, nullptr, 10 );
        else if( k == "srand_seed" )
            srandSeed = (u32)strtoul( eq + 1, nullptr, 10 );
        else if( k == "rng_tab_n" ) // (the product: MA_RNG_TAB)
            tabN = (u32)strtoul( eq + 1, nullptr, 10 );
        else
        {
            fprintf( stderr, "unknown parameter %s\n", k.c_str( ) );
            return 2;
        }
    }
    srand_ring( srandSeed, P.rng_ring );
    std::vector<u32> table( MA_RNG_TAB_WORDS( tabN ) );
    fill_rand_table( P.rng_ring, table.data( ), tabN );
    P.rng_tab_n = tabN, P.rng_tab = table.data( );

    FILE* f = fopen( argv[ 3 ], "w" );
    if( !f )
        return 2;
    int bad = 0;
    for( size_t i = 0; i < c.reads.size( ); i++ )
    {
        const u32 qlen = (u32)c.reads[ i ].size( );
        std::vector<ma_seed> seeds( sf.seedOff[ i + 1 ] - sf.seedOff[ i ] );
        if( !seeds.empty( ) )
            memcpy( seeds.data( ), &sf.seeds[ sf.seedOff[ i ] ], seeds.size( ) * sizeof( ma_seed ) );
        g_hits.clear( );
        g_count = true;
        const Result plain = run( X, P, seeds, qlen, PLAIN );
        g_count = false;
        const Result pre = run( X, P, seeds, qlen, PRESWEPT ), que = run( X, P, seeds, qlen, QUEUE );
        if( !( pre == plain ) || !( que == plain ) )
        {
            fprintf( stderr, "read %zu: the %s run differs from the plain one (%u / %u sets)\n", i, pre == plain ? "queue" : "preswept",
                     pre == plain ? que.nsets : pre.nsets, plain.nsets );
            bad = 1;
        }
        fprintf( f, "R %zu %u\nHARM %u\n", i, qlen, plain.nsets );
        for( size_t k = 0; k < plain.sets.size( ); k++ )
        {
            fprintf( f, "h %u %zu\n", plain.soc[ k ], plain.sets[ k ].size( ) );
            for( const ma_seed& x : plain.sets[ k ] )
                fprintf( f, "g %llu %llu %llu %u %d %llu\n", (unsigned long long)x.q_start, (unsigned long long)x.len, (unsigned long long)x.r_start,
                         x.ambiguity, (int)x.on_forward, (unsigned long long)x.delta );
        }
        fprintf( f, "B err=%u", plain.err );
        for( auto& h : g_hits )
            fprintf( f, " %s=%llu", h.first.c_str( ), h.second );
        fprintf( f, "\n" );
    }
    fclose( f );
    return bad;
}
