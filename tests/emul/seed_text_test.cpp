// The text mode of the maxSpan runs (ma_amd/csrc/seeding.h: seed_step, template flag TXT) compiled for the CPU and compared with the
// plain state machine on the same index: the segments of every read must be the same records once the ones that carry a position
// are given their rows back (seed_materialise), with fewer extend_backward calls.  Both forms of the compare are run -- base by
// base, and the word-wise one of the kernel (FAST), whose buffers are padded here as the kernel's are.
//   seed_text_test <case> <min_ambiguity>      prints "steps off <a> on <b> blocks off <c> on <d> marked <e> segments <f>"
//   seed_text_test <case> prop                 extend_backward on size-1 intervals against the text comparison
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../ma_amd/csrc/seeding.h"
#include "../../oracle/dump_format.h"
#include "../../oracle/ma_oracle.h"
#include <string>
#include <vector>

using namespace ma;

struct Run
{
    std::vector<ma_segment> segs;
    u64 steps = 0, blocks = 0;
};

template <bool TXT, bool FAST> static bool seedRead( const IndexView& X, const SeedParams& SP, const uint8_t* q, u32 qlen, Run& R )
{
    const u32 seg_cap = 2 * qlen + 8;
    std::vector<ma_segment> stage( seg_cap ), none( 1 );
    std::vector<u32> stack( 2 * MA_SEED_STACK );
    SeedScratch SS{ stage.data( ), seg_cap, none.data( ), none.data( ), 0, SP.min_seed_size_drop, stack.data( ) };
    SeedLane L;
    seed_begin_read( L, q, qlen );
    seed_read_serial<TXT, FAST>( L, SP, SS, X );
    if( L.err )
        return false;
    R.segs.assign( stage.begin( ), stage.begin( ) + L.nseg ); // before seed_finish's drop rule: every segment is compared
    R.steps = L.steps, R.blocks = L.blocks;
    return true;
}

static bool sameSeg( const ma_segment& a, const ma_segment& b )
{
    return a.q_start == b.q_start && a.q_size == b.q_size && a.sa_start == b.sa_start && a.sa_start_rc == b.sa_start_rc && a.sa_size == b.sa_size;
}

static int propCheck( const IndexView& X )
{
    // the rows of the suffixes at n - 1, F and F - 1: LF steps from row 0 (the empty suffix at n)
    std::vector<i64> rows = { X.primary, 0 };
    {
        i64 k = 0;
        for( u64 pos = X.n; pos > X.F - 1; pos-- )
        {
            k = inv_psi( X, k ); // the row of the suffix at pos - 1
            if( pos - 1 == X.n - 1 || pos - 1 == X.F || pos - 1 == X.F - 1 )
                rows.push_back( k );
        }
    }
    {
        u32 st;
        if( bwt_sa( X, X.primary, st ) != 0 || bwt_sa( X, rows[ 2 ], st ) != (i64)X.n - 1 || bwt_sa( X, rows[ 3 ], st ) != (i64)X.F ||
            bwt_sa( X, rows[ 4 ], st ) != (i64)X.F - 1 )
        {
            fprintf( stderr, "prop: the special rows are not where they should be\n" );
            return 1;
        }
    }
    u64 x = 88172645463325252ull;
    for( int i = 0; i < 100000; i++ )
    {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        rows.push_back( (i64)( x % ( X.n + 1 ) ) );
    }
    u64 ones = 0;
    for( i64 k : rows )
    {
        u32 st;
        const u64 p = k == 0 ? X.n : (u64)bwt_sa( X, k, st ); // (row 0: the empty suffix; its sample is the reference's -1)
        for( u32 c = 0; c < 4; c++ )
        {
            const i64 ik[ 3 ] = { k, 0, 1 };
            i64 ok[ 3 ];
            u32 nb;
            extend_backward( X, ik, c, ok, nb );
            const bool text = p > 0 && text_base( X, p - 1 ) == c;
            if( ok[ 2 ] != ( text ? 1 : 0 ) || ( text && (u64)bwt_sa( X, ok[ 0 ], st ) != p - 1 ) )
            {
                fprintf( stderr, "prop: row %lld (position %llu) base %u: extend_backward size %lld, text says %d\n", (long long)k,
                         (unsigned long long)p, c, (long long)ok[ 2 ], (int)text );
                return 1;
            }
            ones += text;
        }
        // the mirror the right step rests on: the text is its own reverse complement
        if( p > 0 && p < X.n && text_base( X, p - 1 ) != 3u - text_base( X, X.n - p ) )
        {
            fprintf( stderr, "prop: position %llu: the text is not its own reverse complement\n", (unsigned long long)p );
            return 1;
        }
    }
    printf( "prop ok: %zu rows, %llu extensions of size 1\n", rows.size( ), (unsigned long long)ones );
    return 0;
}

int main( int argc, char** argv )
{
    if( argc < 3 )
    {
        fprintf( stderr, "usage: seed_text_test <case> <min_ambiguity | prop>\n" );
        return 2;
    }
    CaseFile cs = readCase( argv[ 1 ] );
    std::vector<uint64_t> lens;
    std::vector<uint8_t> cat;
    for( auto& v : cs.contigs )
    {
        lens.push_back( v.size( ) );
        cat.insert( cat.end( ), v.begin( ), v.end( ) );
    }
    ma_or_index* ox = ma_or_index_build( (int32_t)lens.size( ), lens.data( ), cat.data( ) );
    IndexView X;
    std::vector<u64> cstart( lens.size( ) );
    u64 o = 0;
    for( size_t i = 0; i < lens.size( ); i++ )
    {
        cstart[ i ] = o;
        o += lens[ i ];
    }
    u64 L2[ 5 ], n;
    i64 primary;
    ma_or_index_meta( ox, L2, &primary, &n );
    // the pack as the device holds it: 8-byte aligned, 16 bytes of padding (their value must not matter: all ones)
    std::vector<u64> pac( ( n / 2 + 3 ) / 4 / 8 + 4, ~0ull );
    memcpy( pac.data( ), ma_or_index_pac( ox ), ( n / 2 + 3 ) / 4 );
    X.bwt = ma_or_index_bwt( ox );
    X.sa = ma_or_index_sa( ox );
    X.pac = (const uint8_t*)pac.data( );
    X.cstart = cstart.data( );
    X.clen = lens.data( );
    X.n = n;
    X.F = n / 2;
    X.primary = primary;
    for( int i = 0; i < 5; i++ )
        X.L2[ i ] = L2[ i ];
    X.n_contigs = (i32)lens.size( );
    if( std::string( argv[ 2 ] ) == "prop" )
        return propCheck( X );

    ma_or_params OP;
    ma_or_params_default( &OP );
    SeedParams SP;
    SP.technique = 0;
    SP.min_seed_len = OP.min_seed_len;
    SP.min_amb = (u32)atoi( argv[ 2 ] );
    SP.max_amb = OP.max_ambiguity;
    SP.min_seed_size_drop = OP.min_seed_size_drop;
    SP.disable_heuristics = OP.disable_heuristics;
    SP.rel_min_seed_size_amount = OP.rel_min_seed_size_amount;
    SP.genome_size_disable = OP.genome_size_disable;
    u64 stOff = 0, stOn = 0, blOff = 0, blOn = 0, marked = 0, nseg = 0;
    for( size_t ri = 0; ri < cs.reads.size( ); ri++ )
    {
        const u32 qlen = (u32)cs.reads[ ri ].size( );
        // the read as k_seed holds it in LDS: 4-byte aligned, readable up to the next multiple of 8 (padding: a value no base has)
        std::vector<u32> qbuf( ( qlen + 7 ) / 8 * 2 + 1, 0xeeeeeeeeu );
        memcpy( qbuf.data( ), cs.reads[ ri ].data( ), qlen );
        const uint8_t* q = (const uint8_t*)qbuf.data( );
        Run off, on, fast;
        if( !seedRead<false, false>( X, SP, q, qlen, off ) || !seedRead<true, false>( X, SP, q, qlen, on ) || !seedRead<true, true>( X, SP, q, qlen, fast ) )
        {
            fprintf( stderr, "read %zu: seeding overflow\n", ri );
            return 1;
        }
        bool same = off.segs.size( ) == on.segs.size( ) && on.segs.size( ) == fast.segs.size( ) && on.steps == fast.steps && on.blocks == fast.blocks;
        for( size_t k = 0; same && k < off.segs.size( ); k++ )
        {
            same = sameSeg( on.segs[ k ], fast.segs[ k ] ); // the two forms of the compare: the same records, marked ones included
            if( on.segs[ k ].sa_start < 0 )
            {
                marked++;
                u32 st;
                same = same && on.segs[ k ].sa_size == 1 && off.segs[ k ].sa_size == 1 && -1 - on.segs[ k ].sa_start == bwt_sa( X, off.segs[ k ].sa_start, st );
                seed_materialise( X, q, on.segs[ k ] );
            }
            same = same && sameSeg( on.segs[ k ], off.segs[ k ] );
        }
        if( !same )
        {
            fprintf( stderr, "read %zu (%u bases): segments differ: %zu / %zu / %zu\n", ri, qlen, off.segs.size( ), on.segs.size( ), fast.segs.size( ) );
            for( size_t k = 0; k < off.segs.size( ) && k < on.segs.size( ); k++ )
                fprintf( stderr, "  off %lld %lld %lld %lld %lld   on %lld %lld %lld %lld %lld\n", (long long)off.segs[ k ].q_start,
                         (long long)off.segs[ k ].q_size, (long long)off.segs[ k ].sa_start, (long long)off.segs[ k ].sa_start_rc,
                         (long long)off.segs[ k ].sa_size, (long long)on.segs[ k ].q_start, (long long)on.segs[ k ].q_size,
                         (long long)on.segs[ k ].sa_start, (long long)on.segs[ k ].sa_start_rc, (long long)on.segs[ k ].sa_size );
            return 1;
        }
        stOff += off.steps, stOn += on.steps, blOff += off.blocks, blOn += on.blocks, nseg += off.segs.size( );
    }
    printf( "steps off %llu on %llu blocks off %llu on %llu marked %llu segments %llu\n", (unsigned long long)stOff, (unsigned long long)stOn,
            (unsigned long long)blOff, (unsigned long long)blOn, (unsigned long long)marked, (unsigned long long)nseg );
    return 0;
}
