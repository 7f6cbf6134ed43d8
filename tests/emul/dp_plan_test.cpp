// CPU-only check of the launch planning of the DP stage (ma_amd/csrc/ksw_launch.h: ksw_plan_stage), compiled for the host
// (hipcc --cuda-host-only; no GPU is touched).
//   dp_plan_test dump <out> <dp_route.txt>
//       plans the stage of every input below and writes, per stage, one header line
//           P <sizing> grp= lists= big= side= B= perCu= : total= base=,,, used=,,, ldsPk= ldsLds= bandAfter= n=
//       and one line per launch, in issue order, with every field of its row
//           L <family> inst= lane= waves= lds= queue= list= nDev= jb=n/mode/cls/tier/pSplit/qSplit stride= p_cap= out1=list:entries out2=list:entries
//             outCtr= nMore= ws=stride/state_cap/h_cap/p_cap/cig_cap/use_lds
//       A counter prints as next+WORD, big+WORD, nRedo or -, a list as lists+INDEX (times list_stride) or -.
//       tests/golden/make_dp_plan_golden.py stores this as tests/golden/dp_plan.txt.gz.
//   dp_plan_test check <fixture> <dp_route.txt>
//       the same again, compared with the fixture line by line; and the fixture must reach the planning's paths (see `reach` below).
//       Prints what it compared; exits non-zero on a difference.
// Inputs: the KswSizing of every block of tests/golden/dp_route.txt (16 blocks x grp 1 / 1033 x band_long 0 / 1), the same with every
// job count times 2000 (launches ask for full sets of waves), three hand-made long-read sizings, and one of a population that went
// through ksw_size_job alone (no lists: the shape of ma_ksw_batch and ksw_bytes_device); each without side streams / with three /
// with three and the event `band` / with stream[ 2 ] alone, a budget of 24 GB / 256 / 64 / 40 MB, 32 / 8 waves per CU; the last sizing
// with and without lists, the hand-made ones with and without queues for huge tiers.
#include "../../ma_amd/csrc/ksw_launch.h"

#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace ma;

struct Input
{
    std::string name;
    KswSizing S;
    i32 grp;
    bool routed; // the sizing of a routed population: planned with lists only
    bool handMade; // also planned without nextBig
};

static u64 field( const std::string& l, const char* key )
{
    const size_t p = l.find( std::string( " " ) + key + "=" );
    return p == std::string::npos ? 0 : strtoull( l.c_str( ) + p + strlen( key ) + 2, nullptr, 10 );
}

static bool inputs( const char* routeTxt, std::vector<Input>& in )
{
    FILE* f = fopen( routeTxt, "r" );
    if( !f )
        return false;
    std::vector<char> buf( 1 << 16 );
    std::vector<Input> routed;
    while( fgets( buf.data( ), (int)buf.size( ), f ) )
    {
        const std::string l( buf.data( ) );
        if( l[ 0 ] != 'S' )
            continue;
        Input I{ "route", KswSizing( ), (i32)field( l, "grp" ), true, false };
        I.name += "/grp" + std::to_string( I.grp ) + "/bl" + std::to_string( field( l, "band_long" ) ) + "/" + std::to_string( field( l, "block" ) );
        KswSizing& S = I.S;
        S.state = field( l, "state" ), S.h = field( l, "h" ), S.p = field( l, "p" ), S.cig = field( l, "cig" ), S.qlen = field( l, "qlen" );
        S.pRedo = field( l, "pRedo" ), S.cigRedo = field( l, "cigRedo" ), S.bandlN = field( l, "bandlN" );
        for( int k = 0; k < KSW_N_CLASSES; k++ )
        {
            unsigned long long a = 0, b = 0, c = 0;
            const size_t p = l.find( " " + std::to_string( k ) + ":" );
            if( p == std::string::npos || sscanf( l.c_str( ) + p, " %*d:%llu/%llu/%llu", &a, &b, &c ) != 3 )
                return false;
            S.cls[ k ] = a, S.pc[ k ] = b, S.cigc[ k ] = c;
        }
        routed.push_back( I );
    }
    fclose( f );
    in = routed;
    for( Input I : routed ) // a batch of 2000 such blocks: the counts grow, the largest job of a class stays
    {
        I.name += "x2000";
        for( u64& c : I.S.cls )
            c *= 2000;
        in.push_back( I );
    }
    auto cls = []( KswSizing& S, int k, u64 n, u64 p, u64 cig ) { S.cls[ k ] = n, S.pc[ k ] = p, S.cigc[ k ] = cig; };
    {
        // 10 kb reads: gap fills of all widths, junk extensions of thousands of bases on k_ksw_pk<5>, most long extensions on the band of
        // 120, a few jobs of 10 kb x 10 kb for k_ksw (state + H: 150 KB, so in HBM)
        Input I{ "10kb", KswSizing( ), 1033, true, true };
        KswSizing& S = I.S;
        S.state = 90048, S.h = 40064, S.p = 41ull << 20, S.cig = 20002, S.qlen = 10000, S.pRedo = 6500000, S.cigRedo = 16000, S.bandlN = 6000;
        cls( S, KSW_CLS_PK0, 40000, 60000, 900 ), cls( S, KSW_CLS_PK1, 9000, 200000, 2500 ), cls( S, KSW_CLS_PK2, 5000, 400000, 4000 );
        cls( S, KSW_CLS_PK3, 8500, 6500000, 16000 ), cls( S, KSW_CLS_LDS, 40, 41ull << 20, 20002 );
        cls( S, KSW_CLS_EXT1, 50000, 76816, 700 ), cls( S, KSW_CLS_EXT2, 9000, 230416, 1000 );
        cls( S, KSW_CLS_NARROW_L, 3000, 0, 500 ), cls( S, KSW_CLS_NARROW_R, 3000, 0, 500 ), cls( S, KSW_CLS_GRP2_L, 8000, 0, 200 ), cls( S, KSW_CLS_GRP2_R, 8000, 0, 200 );
        cls( S, KSW_CLS_GRP4_L, 12000, 0, 100 ), cls( S, KSW_CLS_GRP4_R, 12000, 0, 100 ), cls( S, KSW_CLS_BANDL_L, 60000, 0, 14000 ), cls( S, KSW_CLS_BANDL_R, 60000, 0, 14000 );
        in.push_back( I );
    }
    {
        // 50 kb reads: end extensions with a 49 kb query and 27 MB of direction bytes among the jobs of k_ksw_pk<5>, one 49 kb query
        // with a narrow band among 10^5 gap fills of k_ksw_pk<1>
        Input I{ "50kb", KswSizing( ), 1033, true, true };
        KswSizing& S = I.S;
        S.state = 450000, S.h = 200000, S.p = 60ull << 20, S.cig = 100000, S.qlen = 49000, S.pRedo = 27ull << 20, S.cigRedo = 60000, S.bandlN = 7900;
        cls( S, KSW_CLS_PK0, 100000, 800000, 51000 ), cls( S, KSW_CLS_PK1, 20000, 300000, 6000 ), cls( S, KSW_CLS_PK2, 8000, 800000, 9000 );
        cls( S, KSW_CLS_PK3, 6000, 27ull << 20, 60000 ), cls( S, KSW_CLS_LDS, 12, 60ull << 20, 100000 );
        cls( S, KSW_CLS_EXT1, 20000, 76816, 700 ), cls( S, KSW_CLS_EXT2, 5000, 230416, 1000 );
        cls( S, KSW_CLS_GRP2_L, 3000, 0, 200 ), cls( S, KSW_CLS_GRP4_R, 5000, 0, 100 ), cls( S, KSW_CLS_BANDL_L, 30000, 0, 17000 ), cls( S, KSW_CLS_BANDL_R, 30000, 0, 17000 );
        in.push_back( I );
    }
    {
        // one class of 10^5 small jobs plus a single huge one (40 MB of direction bytes, a 50 kb query), and a few extensions
        Input I{ "small+huge", KswSizing( ), 1033, true, true };
        KswSizing& S = I.S;
        S.state = 4000, S.h = 1600, S.p = 40ull << 20, S.cig = 100002, S.qlen = 50000, S.pRedo = 20000, S.cigRedo = 700;
        cls( S, KSW_CLS_PK2, 100001, 40ull << 20, 100002 ), cls( S, KSW_CLS_EXT1, 100, 38416, 400 );
        in.push_back( I );
    }
    {
        // jobs that ksw_size_job alone has seen: classes 0 .. 4, the largest of 4 500 x 4 500 (state + H of k_ksw: 58 KB, so in LDS)
        Input I{ "sized", KswSizing( ), 1033, false, false };
        std::mt19937_64 rng( 20261021ull );
        for( int i = 0; i < 3000; i++ )
        {
            const i32 q = 1 + (i32)( rng( ) % ( i % 3 ? 300 : 4500 ) ), t = i % 2 ? q + (i32)( rng( ) % 40 ) : 1 + (i32)( rng( ) % 4500 );
            ksw_size_job( I.S, q, t < 4500 ? t : 4500, i % 5 ? 64 : 1024 );
        }
        ksw_size_job( I.S, 4500, 4500, 1024 );
        in.push_back( I );
    }
    return true;
}

static std::string ctrName( int w )
{
    return w == KSW_NONE ? "-" : ( w < KSW_CT_BIG ? "next+" + std::to_string( w ) : ( w < KSW_CT_NREDO ? "big+" + std::to_string( w - KSW_CT_BIG ) : "nRedo" ) );
}
static std::string listName( int i )
{
    return i == KSW_NONE ? "-" : "lists+" + std::to_string( i );
}
static const char* const FAMILY[ 6 ] = { "pk", "ext", "grp", "band4", "band1", "lds" };
static const u64 BUDGET_MB[ 4 ] = { 24576, 256, 64, 40 };

static void printStage( const KswStagePlan& P, std::vector<std::string>& out )
{
    char buf[ 1024 ];
    snprintf( buf, sizeof( buf ), " : total=%llu base=%llu,%llu,%llu,%llu used=%d,%d,%d,%d ldsPk=%u ldsLds=%u bandAfter=%d n=%d", (unsigned long long)P.total,
              (unsigned long long)P.laneBase[ 0 ], (unsigned long long)P.laneBase[ 1 ], (unsigned long long)P.laneBase[ 2 ], (unsigned long long)P.laneBase[ 3 ],
              (int)P.laneUsed[ 0 ], (int)P.laneUsed[ 1 ], (int)P.laneUsed[ 2 ], (int)P.laneUsed[ 3 ], P.ldsPk, P.ldsLds, P.bandAfter, P.n );
    out.back( ) += buf;
    for( int i = 0; i < P.n; i++ )
    {
        const KswLaunch& L = P.launch[ i ];
        snprintf( buf, sizeof( buf ), "L %s inst=%d lane=%d waves=%u lds=%u queue=%s list=%s nDev=%s jb=%u/%d/%d/%d/%llu/%d stride=%llu p_cap=%llu out1=%s:%u out2=%s:%u outCtr=%s nMore=%s ws=%llu/%llu/%llu/%llu/%llu/%u",
                  FAMILY[ L.family ], L.inst, L.lane, L.waves, L.lds, ctrName( L.queue ).c_str( ), listName( L.list ).c_str( ), ctrName( L.nDev ).c_str( ), L.jb.n, L.jb.mode,
                  L.jb.cls, L.jb.tier, (unsigned long long)L.jb.pSplit, L.jb.qSplit, (unsigned long long)L.stride, (unsigned long long)L.p_cap, listName( L.out1 ).c_str( ), L.nOut1,
                  listName( L.out2 ).c_str( ), L.nOut2, ctrName( L.outCtr ).c_str( ), ctrName( L.nMore ).c_str( ), (unsigned long long)L.ws.stride,
                  (unsigned long long)L.ws.state_cap, (unsigned long long)L.ws.h_cap, (unsigned long long)L.ws.p_cap, (unsigned long long)L.ws.cig_cap, L.ws.use_lds );
        out.push_back( buf );
    }
}

// side: 0 no side streams, 1 all three, 2 all three and the event `band`, 3 stream[ 2 ] alone
static KswStagePlan planStage( const Input& I, bool lists, bool nextBig, int side, u64 B, u64 perCu )
{
    KswScoring SC{ 2, 4, 4, 2, 24, 1 };
    SC.grp = I.grp;
    u64 nSlots = 0;
    for( u64 c : I.S.cls )
        nSlots += c;
    return ksw_plan_stage( I.S, SC, (u32)nSlots, lists, nextBig, side == 1 || side == 2, side != 0, side == 2, B, perCu );
}

static std::vector<std::string> record( const std::vector<Input>& in )
{
    std::vector<std::string> out;
    for( const Input& I : in )
        for( int lists = 1; lists >= ( I.routed ? 1 : 0 ); lists-- )
            for( int big = 1; big >= ( I.handMade ? 0 : 1 ); big-- )
                for( int side = 0; side < 4; side++ )
                    for( u64 mb : BUDGET_MB )
                        for( u64 perCu : { 32, 8 } )
                        {
                            out.push_back( "P " + I.name + " grp=" + std::to_string( I.grp ) + " lists=" + std::to_string( lists ) + " big=" + std::to_string( big ) +
                                           " side=" + std::to_string( side ) + " B=" + std::to_string( mb ) + " perCu=" + std::to_string( perCu ) );
                            printStage( planStage( I, lists != 0, big != 0, side, mb << 20, perCu ), out );
                        }
    return out;
}

// What the fixture must reach, counted from its own lines: every kernel family, tiers 1 and 2, all four lanes, the event `band` recorded
// and not recorded in stages that run the band of 120, the rule "over 2 GB: take the whole budget" firing and not firing in the
// concurrent and in the sequential layout, an LDS limit above 48 KB, k_ksw with its state in LDS and in HBM, a launch whose waves
// the budget cut (waves == budget of its region / stride, below the waves it would ask for).
struct Reach
{
    u64 family[ 6 ] = { }, tier[ 3 ] = { }, lane[ 4 ] = { }, bandOn = 0, bandOff = 0, whole[ 2 ][ 2 ] = { }, ldsPk = 0, ldsLds = 0, kswLds[ 2 ] = { }, cut = 0;
    // the current stage
    u64 B = 0, perCu = 0;
    bool conc = false;
    int bandAfter = -1;
    bool sawBand1 = false;
    void endStage( )
    {
        if( sawBand1 )
            ( bandAfter >= 0 ? bandOn : bandOff )++;
        sawBand1 = false;
    }
    bool line( const std::string& l )
    {
        if( l[ 0 ] == 'P' )
        {
            endStage( );
            unsigned long long total, b[ 4 ];
            unsigned pk, ld;
            int used[ 4 ], n;
            const size_t p = l.find( " : " );
            if( p == std::string::npos || sscanf( l.c_str( ) + p, " : total=%llu base=%llu,%llu,%llu,%llu used=%d,%d,%d,%d ldsPk=%u ldsLds=%u bandAfter=%d n=%d", &total, b, b + 1,
                                                  b + 2, b + 3, used, used + 1, used + 2, used + 3, &pk, &ld, &bandAfter, &n ) != 13 )
                return false;
            B = field( l, "B" ) << 20, perCu = field( l, "perCu" );
            conc = field( l, "lists" ) && ( field( l, "side" ) == 1 || field( l, "side" ) == 2 );
            if( total )
                whole[ conc ][ ( conc ? total : b[ 1 ] - b[ 0 ] ) > ( 2ull << 30 ) ]++;
            ldsPk += pk > 48 * 1024, ldsLds += ld > 48 * 1024;
            return true;
        }
        char fam[ 16 ];
        int lanei, tieri;
        unsigned waves, useLds;
        unsigned long long stride;
        const size_t pj = l.find( " jb=" ), ps = l.find( " stride=" ), pw = l.find( " ws=" );
        if( l[ 0 ] != 'L' || pj == std::string::npos || ps == std::string::npos || pw == std::string::npos || sscanf( l.c_str( ), "L %15s inst=%*d lane=%d waves=%u", fam, &lanei, &waves ) != 3 ||
            sscanf( l.c_str( ) + pj, " jb=%*u/%*d/%*d/%d/", &tieri ) != 1 || sscanf( l.c_str( ) + ps, " stride=%llu", &stride ) != 1 ||
            sscanf( l.c_str( ) + pw, " ws=%*u/%*u/%*u/%*u/%*u/%u", &useLds ) != 1 || lanei < 0 || lanei > 3 || tieri < 0 || tieri > 2 )
            return false;
        int f = 0;
        while( f < 6 && strcmp( fam, FAMILY[ f ] ) )
            f++;
        if( f == 6 )
            return false;
        family[ f ]++, tier[ tieri ]++, lane[ lanei ]++;
        sawBand1 |= f == KSW_FAM_BAND1;
        if( f == KSW_FAM_LDS )
            kswLds[ useLds != 0 ]++;
        const u64 share[ 4 ] = { B / 4, 5 * B / 12, B / 3, B / 4 }, budget = conc ? share[ lanei ] : B;
        cut += stride && waves == budget / stride && waves < 256 * perCu;
        return true;
    }
    int missing( )
    {
        endStage( );
        int bad = 0;
        auto want = [ & ]( const char* what, u64 n ) {
            printf( " %s %llu", what, (unsigned long long)n );
            if( n == 0 )
                bad++;
        };
        printf( "fixture reaches:" );
        for( int f = 0; f < 6; f++ )
            want( FAMILY[ f ], family[ f ] );
        want( "tier1", tier[ 1 ] ), want( "tier2", tier[ 2 ] );
        want( "lane0", lane[ 0 ] ), want( "lane1", lane[ 1 ] ), want( "lane2", lane[ 2 ] ), want( "lane3", lane[ 3 ] );
        want( "bandEventOn", bandOn ), want( "bandEventOff", bandOff );
        want( "wholeBudget/sequential", whole[ 0 ][ 1 ] ), want( "ownSize/sequential", whole[ 0 ][ 0 ] ), want( "wholeBudget/concurrent", whole[ 1 ][ 1 ] ), want( "ownSize/concurrent", whole[ 1 ][ 0 ] );
        want( "ldsLimitPk", ldsPk ), want( "ldsLimitKsw", ldsLds ), want( "kswInLds", kswLds[ 1 ] ), want( "kswInHbm", kswLds[ 0 ] ), want( "wavesCut", cut );
        printf( "\n" );
        return bad;
    }
};

int main( int argc, char** argv )
{
    std::vector<Input> in;
    if( argc < 4 || !inputs( argv[ 3 ], in ) )
    {
        fprintf( stderr, "usage: dp_plan_test dump <out> <dp_route.txt> | check <fixture> <dp_route.txt>\n" );
        return 2;
    }
    const std::vector<std::string> lines = record( in );
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
    FILE* f = fopen( argv[ 2 ], "r" );
    if( !f )
        return 2;
    int bad = 0;
    std::vector<char> buf( 1 << 16 );
    size_t at = 0;
    Reach R;
    while( fgets( buf.data( ), (int)buf.size( ), f ) )
    {
        std::string l( buf.data( ) );
        while( !l.empty( ) && ( l.back( ) == '\n' || l.back( ) == '\r' ) )
            l.pop_back( );
        if( at >= lines.size( ) || l != lines[ at ] )
            if( bad++ < 10 )
                printf( "line %zu differs\n  fixture: %s\n  planned: %s\n", at + 1, l.c_str( ), at < lines.size( ) ? lines[ at ].c_str( ) : "(none)" );
        if( !R.line( l ) && bad++ < 10 )
            printf( "line %zu of the fixture does not parse: %s\n", at + 1, l.c_str( ) );
        at++;
    }
    fclose( f );
    if( at != lines.size( ) )
    {
        printf( "the fixture has %zu lines, the planning gives %zu\n", at, lines.size( ) );
        bad++;
    }
    printf( "fixture: %zu lines compared, %zu inputs\n", at, in.size( ) );
    bad += R.missing( );
    printf( bad ? "dp_plan_test: %d differences\n" : "dp_plan_test ok\n", bad );
    return bad ? 1 : 0;
}
