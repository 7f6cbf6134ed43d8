// CPU-only check of the routing of DP jobs to kernel classes (ma_amd/csrc/ksw_launch.h: ksw_route_job, ksw_size_route), compiled
// for the host (hipcc --cuda-host-only; no GPU is touched).
//   dp_route_test dump <out>
//       a fixed population of jobs through the host path of ma_ksw_ext_batch (byte arrays -> ksw_route_job -> ksw_size_route), under
//       grp = 1 / 1033 x band_long = 0 / 1: per job its inputs and its class under each setting, per block of 250 jobs the KswSizing
//       the launches would be planned with.  tests/golden/make_dp_route_golden.py stores this as tests/golden/dp_route.txt.gz.
//   dp_route_test check <fixture>
//       the same again, compared with the fixture line by line; every one of the KSW_N_CLASSES classes must occur; and every job once
//       more the way k_dp_enum reaches the router (ksw_route_slot: a DpJob whose bases come from the batch's reads and the 2-bit packed
//       reference, both strands, forward and reversed in place), which must give the same KswRoute as the byte path.
//       Prints what it compared; exits non-zero on a difference.
#include "../../ma_amd/csrc/ksw_launch.h"

#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace ma;

struct Job
{
    ma_ksw_job j; // the byte path's view
    DpJob d; // the pipeline's view of the same job
    int kind; // 0 matching, 1 few mismatches, 2 random
};
struct Batch
{
    std::vector<Job> jobs;
    std::vector<uint8_t> qBytes, tBytes; // DP order, back to back
    std::vector<uint8_t> reads, pac; // the pipeline's arrays
    IndexView X;
};

static i32 pickLen( std::mt19937_64& rng )
{
    // 1 .. 9000, with most of the weight where the class boundaries are (32, 64, 126, 254, the ring slots of the exact kernels)
    switch( rng( ) % 8 )
    {
    case 0: return 1 + (i32)( rng( ) % 40 );
    case 1: return 1 + (i32)( rng( ) % 70 );
    case 2: return 30 + (i32)( rng( ) % 110 );
    case 3: return 100 + (i32)( rng( ) % 170 );
    case 4: return 200 + (i32)( rng( ) % 500 );
    case 5: return 1 + (i32)( rng( ) % 2500 );
    case 6: return 600 + (i32)( rng( ) % 2000 );
    default: return 1 + (i32)( rng( ) % 9000 );
    }
}

static void makeBatch( Batch& B, size_t n )
{
    std::mt19937_64 rng( 20261017ull );
    const i32 bands[ 3 ] = { 64, 512, 1024 };
    std::vector<std::vector<uint8_t>> Q( n ), T( n );
    u64 textLen = 16;
    for( size_t i = 0; i < n; i++ )
    {
        Job J;
        memset( &J, 0, sizeof( J ) );
        const i32 ql = pickLen( rng );
        // targets: about the query's length (a gap between two seeds) or independent of it (an end extension into padded reference)
        i32 tl = rng( ) % 2 ? pickLen( rng ) : ql + (i32)( rng( ) % 41 ) - 10;
        tl = tl < 1 ? 1 : ( tl > 9000 ? 9000 : tl );
        J.kind = (int)( rng( ) % 3 );
        Q[ i ].resize( ql );
        T[ i ].resize( tl );
        for( auto& c : T[ i ] )
            c = (uint8_t)( rng( ) % 4 );
        for( i32 k = 0; k < ql; k++ )
            Q[ i ][ k ] = J.kind == 2 || k >= tl ? (uint8_t)( rng( ) % 4 ) : T[ i ][ k ];
        if( J.kind == 1 )
        {
            // a few substitutions near the start, and sometimes one base more in the query
            const int m = 1 + (int)( rng( ) % 9 );
            for( int k = 0; k < m; k++ )
            {
                const size_t at = rng( ) % std::min<size_t>( ql, 200 );
                Q[ i ][ at ] = (uint8_t)( ( Q[ i ][ at ] + 1 + rng( ) % 3 ) % 4 );
            }
            if( rng( ) % 3 == 0 && ql > 20 )
            {
                const size_t at = 5 + rng( ) % 10;
                Q[ i ].insert( Q[ i ].begin( ) + at, (uint8_t)( rng( ) % 4 ) );
                Q[ i ].pop_back( );
            }
        }
        J.j.qlen = ql, J.j.tlen = tl;
        J.j.w = bands[ rng( ) % 3 ];
        J.j.zdrop = rng( ) % 3 == 0 ? -1 : 100 + (i32)( rng( ) % 300 );
        const u64 f = rng( ) % 5; // global, left, left with the cigar reversed, right, right with the cigar reversed
        J.j.flag = f == 0 ? 0 : ( KSW_EZ_EXTZ_ONLY | ( f >= 3 ? KSW_EZ_RIGHT : 0 ) | ( f % 2 == 0 ? KSW_EZ_REV_CIGAR : 0 ) );
        if( f == 0 && rng( ) % 2 )
            J.j.zdrop = -1; // what NeedlemanWunsch::ksw passes for a gap between two seeds
        J.j.q_off = B.qBytes.size( ), J.j.t_off = B.tBytes.size( );
        B.qBytes.insert( B.qBytes.end( ), Q[ i ].begin( ), Q[ i ].end( ) );
        B.tBytes.insert( B.tBytes.end( ), T[ i ].begin( ), T[ i ].end( ) );
        // the same job as a slot of the pipeline: the query inside a read, the target inside a window of the reference
        const u32 qo = (u32)( rng( ) % 7 ), ro = (u32)( rng( ) % 7 );
        J.d.rev = (u32)( rng( ) % 2 );
        J.d.read_off = B.reads.size( );
        J.d.q_from = qo, J.d.q_to = qo + (u32)ql;
        J.d.r_from = ro, J.d.r_to = ro + (u32)tl;
        J.d.w = J.j.w, J.d.zdrop = J.j.zdrop, J.d.flag = J.j.flag;
        B.reads.resize( B.reads.size( ) + qo + ql + 3, 0 );
        for( i32 k = 0; k < ql; k++ )
            B.reads[ J.d.read_off + ( J.d.rev ? J.d.q_to - 1 - (u32)k : J.d.q_from + (u32)k ) ] = Q[ i ][ k ];
        J.d.win_begin = textLen; // (forward position of the target for now: the strand is chosen below, when the text's length is known)
        textLen += (u64)tl + 8;
        B.jobs.push_back( J );
    }
    B.qBytes.resize( B.qBytes.size( ) + 16, 0 );
    B.tBytes.resize( B.tBytes.size( ) + 16, 0 );
    // the packed reference: forward strand of textLen bases; jobs with an odd index lie on the reverse strand
    const u64 F = ( textLen + 3 ) / 4 * 4;
    B.pac.assign( F / 4, 0 );
    memset( &B.X, 0, sizeof( B.X ) );
    B.X.F = F, B.X.n = 2 * F;
    for( size_t i = 0; i < n; i++ )
    {
        DpJob& d = B.jobs[ i ].d;
        const u64 pos = d.win_begin, tl = d.r_to - d.r_from;
        const u64 start = i % 2 ? 2 * F - pos - tl : pos; // text position of the first base of the window's job part
        d.win_begin = start - d.r_from;
        for( u64 k = 0; k < tl; k++ )
        {
            const u64 p = d.win_begin + ( d.rev ? d.r_to - 1 - k : d.r_from + k ); // where the kernels read base k (stage_dp.h)
            const u64 fwd = p < F ? p : 2 * F - 1 - p;
            const u32 code = p < F ? T[ i ][ k ] : 3u - T[ i ][ k ];
            B.pac[ fwd >> 2 ] = (uint8_t)( ( B.pac[ fwd >> 2 ] & ~( 3u << ( ( ~fwd & 3 ) << 1 ) ) ) | code << ( ( ~fwd & 3 ) << 1 ) );
        }
    }
    B.X.pac = B.pac.data( );
}

static KswScoring settingOf( int c )
{
    KswScoring SC{ 2, 4, 4, 2, 24, 1 };
    SC.grp = c & 2 ? 1033 : 1;
    SC.band_mis = KSW_BAND_MAXMIS;
    SC.band_long = c & 1;
    return SC;
}

// the host path: what ksw_batch_impl<ByteFetchPipe> (prims.hip) does with every job
static KswRoute routeBytes( const KswScoring& SC, const Batch& B, const ma_ksw_job& j )
{
    const uint8_t *qp = B.qBytes.data( ) + j.q_off, *tp = B.tBytes.data( ) + j.t_off;
    auto qf = [ & ]( i32 k ) -> u32 { return qp[ k ]; };
    auto tf = [ & ]( i32 k ) -> u32 { return tp[ k ]; };
    return ksw_route_job( SC, j.qlen, j.tlen, j.w, j.zdrop, j.flag, qf, tf, false );
}
static void hostPath( const KswScoring& SC, const Batch& B, size_t from, size_t to, std::vector<int>& cls, KswSizing& S )
{
    for( size_t i = from; i < to; i++ )
        ksw_size_job( S, B.jobs[ i ].j.qlen, B.jobs[ i ].j.tlen, B.jobs[ i ].j.w );
    for( int k = 0; k < KSW_N_CLASSES; k++ )
        S.cls[ k ] = S.pc[ k ] = S.cigc[ k ] = 0;
    for( size_t i = from; i < to; i++ )
    {
        const KswRoute R = routeBytes( SC, B, B.jobs[ i ].j );
        cls[ i ] = R.cls;
        ksw_size_route( S, R );
    }
}

static u64 fnv( const uint8_t* p, size_t n )
{
    u64 h = 1469598103934665603ull;
    for( size_t i = 0; i < n; i++ )
        h = ( h ^ p[ i ] ) * 1099511628211ull;
    return h;
}

#define N_JOBS 4000
#define BLOCK 250
static std::vector<std::string> record( const Batch& B, u64 seen[ KSW_N_CLASSES ] )
{
    std::vector<std::string> out;
    std::vector<int> cls[ 4 ];
    std::vector<KswSizing> sizing[ 4 ];
    for( int c = 0; c < 4; c++ )
    {
        cls[ c ].assign( B.jobs.size( ), -1 );
        for( size_t from = 0; from < B.jobs.size( ); from += BLOCK )
        {
            KswSizing S;
            hostPath( settingOf( c ), B, from, std::min( from + BLOCK, B.jobs.size( ) ), cls[ c ], S );
            sizing[ c ].push_back( S );
        }
    }
    char buf[ 512 ];
    for( size_t i = 0; i < B.jobs.size( ); i++ )
    {
        const ma_ksw_job& j = B.jobs[ i ].j;
        snprintf( buf, sizeof( buf ), "J %zu %d %d %d %d %d %d %016llx %016llx %d %d %d %d", i, j.qlen, j.tlen, j.w, j.zdrop, j.flag, B.jobs[ i ].kind,
                  (unsigned long long)fnv( B.qBytes.data( ) + j.q_off, j.qlen ), (unsigned long long)fnv( B.tBytes.data( ) + j.t_off, j.tlen ), cls[ 0 ][ i ],
                  cls[ 1 ][ i ], cls[ 2 ][ i ], cls[ 3 ][ i ] );
        out.push_back( buf );
        for( int c = 0; c < 4; c++ )
            seen[ cls[ c ][ i ] ]++;
    }
    for( int c = 0; c < 4; c++ )
        for( size_t b = 0; b < sizing[ c ].size( ); b++ )
        {
            const KswSizing& S = sizing[ c ][ b ];
            std::string s = "S grp=" + std::to_string( settingOf( c ).grp ) + " band_long=" + std::to_string( settingOf( c ).band_long ) + " block=" + std::to_string( b );
            auto add = [ & ]( const char* name, u64 v ) { s += std::string( " " ) + name + "=" + std::to_string( v ); };
            add( "state", S.state ), add( "h", S.h ), add( "p", S.p ), add( "cig", S.cig ), add( "qlen", S.qlen );
            add( "pRedo", S.pRedo ), add( "cigRedo", S.cigRedo ), add( "bandlN", S.bandlN );
            for( int k = 0; k < KSW_N_CLASSES; k++ )
                s += " " + std::to_string( k ) + ":" + std::to_string( S.cls[ k ] ) + "/" + std::to_string( S.pc[ k ] ) + "/" + std::to_string( S.cigc[ k ] );
            out.push_back( s );
        }
    return out;
}

int main( int argc, char** argv )
{
    if( argc < 3 )
    {
        fprintf( stderr, "usage: dp_route_test dump <out> | check <fixture>\n" );
        return 2;
    }
    Batch B;
    makeBatch( B, N_JOBS );
    u64 seen[ KSW_N_CLASSES ] = { };
    const std::vector<std::string> lines = record( B, seen );
    if( std::string( argv[ 1 ] ) == "dump" )
    {
        FILE* f = fopen( argv[ 2 ], "w" );
        if( !f )
            return 2;
        for( auto& l : lines )
            fprintf( f, "%s\n", l.c_str( ) );
        fclose( f );
        return 0;
    }
    int bad = 0;
    // ---- the fixture: the routing and the sizes as they were recorded
    {
        FILE* f = fopen( argv[ 2 ], "r" );
        if( !f )
            return 2;
        std::vector<char> buf( 1 << 16 );
        size_t at = 0;
        u64 fixtureSeen[ KSW_N_CLASSES ] = { };
        while( fgets( buf.data( ), (int)buf.size( ), f ) )
        {
            std::string l( buf.data( ) );
            while( !l.empty( ) && ( l.back( ) == '\n' || l.back( ) == '\r' ) )
                l.pop_back( );
            if( at >= lines.size( ) || l != lines[ at ] )
            {
                if( bad++ < 10 )
                    printf( "line %zu differs\n  fixture: %s\n  router:  %s\n", at + 1, l.c_str( ), at < lines.size( ) ? lines[ at ].c_str( ) : "(none)" );
            }
            if( l[ 0 ] == 'J' )
            {
                // the last four fields: the job's class under the four settings
                size_t p = l.size( );
                for( int c = 0; c < 4; c++ )
                {
                    p = l.rfind( ' ', p - 1 );
                    const int k = atoi( l.c_str( ) + p + 1 );
                    if( k >= 0 && k < KSW_N_CLASSES )
                        fixtureSeen[ k ]++;
                }
            }
            at++;
        }
        fclose( f );
        if( at != lines.size( ) )
        {
            printf( "the fixture has %zu lines, the router gives %zu\n", at, lines.size( ) );
            bad++;
        }
        printf( "fixture: %zu lines compared; jobs per class (four settings):", at );
        for( int k = 0; k < KSW_N_CLASSES; k++ )
        {
            printf( " %llu", (unsigned long long)fixtureSeen[ k ] );
            if( fixtureSeen[ k ] == 0 )
            {
                printf( "\nclass %d does not occur in the fixture\n", k );
                bad++;
            }
        }
        printf( "\n" );
    }
    // ---- the device's way to the router against the host's, job by job
    {
        size_t n = 0;
        for( int c = 0; c < 4; c++ )
            for( const Job& J : B.jobs )
            {
                const KswScoring SC = settingOf( c );
                const KswRoute a = routeBytes( SC, B, J.j ), b = ksw_route_slot( SC, B.X, B.reads.data( ), J.d );
                n++;
                if( a.cls != b.cls || a.cig != b.cig || a.p != b.p || a.pk != b.pk || a.redo != b.redo || a.bandlN != b.bandlN || a.ext != b.ext || a.pExt != b.pExt )
                    if( bad++ < 10 )
                        printf( "job %zu (grp %d, band_long %d): class %d through the byte path, %d through the job slot\n", (size_t)( &J - B.jobs.data( ) ), SC.grp,
                                SC.band_long, a.cls, b.cls );
            }
        printf( "job slots: %zu routes compared\n", n );
    }
    printf( bad ? "dp_route_test: %d differences\n" : "dp_route_test ok\n", bad );
    return bad ? 1 : 0;
}
