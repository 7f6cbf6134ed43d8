// CPU test program of the small-inversion logic the device stage runs (ma_amd/host/ma_inv_dev.h: scanDrops, stretchJob,
// assemble, kept, place), on the host, against
//   - SmallInversions::DropScan / forAllDropPos of ma_amd/host/ma_modules.h, the host module's restatement (the yardstick), on
//     every record of the reference's f4 dumps under four values of "Z Drop Inversions";
//   - the inversion records of those dumps themselves: assemble, fed with a record's own ops collapsed to an M / I / D cigar and
//     the bases of the case, rebuilds the record (bounds, score, ops, flags, mapq bits, strip index);
//   - hand-made records, the smallest shapes that can go wrong, with the expected stretches spelled out.
// Modes:  golden <case> <dump> <paired 0|1> <zd of the dump>   |   handmade
#include "../../ma_amd/csrc/nw.h"
#include "ma_inv_dev.h"
#include "inv_common.h"

typedef std::vector<ma_inv::Stretch> Stretches;

static Stretches sharedScan( const ma_params& rP, const ma_sam::FlatList& rList, uint32_t k )
{
    Stretches v;
    ma_inv::scanDrops( ma_inv::params( rP ), rList, k, [ & ]( const ma_inv::Stretch& s ) { v.push_back( s ); } );
    return v;
}
// the yardstick: SmallInversions::forAllDropPos on an Alignment container of the same record
static Stretches yardstickScan( const ma_params& rP, const Input& rIn, size_t uiUnit, uint32_t k )
{
    ParameterSetManager xParams;
    *xParams.getSelected( ) = rP;
    SmallInversions xModule( xParams );
    Stretches v;
    xModule.forAllDropPos( [ & ]( nucSeqIndex a, nucSeqIndex b, nucSeqIndex c, nucSeqIndex d ) { v.push_back( ma_inv::Stretch{ a, b, c, d } ); },
                           *( *rIn.containers( uiUnit ) )[ k ] );
    return v;
}
static bool same( const Stretches& a, const Stretches& b )
{
    if( a.size( ) != b.size( ) )
        return false;
    for( size_t i = 0; i < a.size( ); i++ )
        if( a[ i ].startQ != b[ i ].startQ || a[ i ].startR != b[ i ].startR || a[ i ].endQ != b[ i ].endQ || a[ i ].endR != b[ i ].endR )
            return false;
    return true;
}

static ma::NwParams nwParams( const ma_params& P ) // (the fields Alignment::append reads)
{
    ma::NwParams N{ };
    N.sv_penalty = (u32)P.sv_penalty;
    N.match = (u32)P.match, N.mismatch = (u32)P.mismatch, N.gap = (u32)P.gap, N.extend = (u32)P.extend;
    return N;
}
struct Built
{
    ma::AlnHeader h;
    std::vector<u64> ops;
    bool bOk, bKept;
};
struct Appender
{
    const ma::NwParams& P;
    ma::AlnBuilder& A;
    void append( uint32_t type, uint64_t size )
    {
        ma::aln_append( P, A, type, size );
    }
};
// assemble + kept + place over a cigar, the query from uiStartQ on and the window's codes
static Built build( const ma_params& rP, const std::vector<uint32_t>& vCigar, const uint8_t* pQuery, const std::vector<uint8_t>& vWindow,
                    const ma_alignment& rParent, const ma_inv::Stretch& rS, const ma_inv::Job& rJob )
{
    Built b;
    memset( &b.h, 0, sizeof( b.h ) );
    b.ops.assign( ma_inv::opsBound( rJob ), 0 ); // (exactly the bound: the sanitizer build sees a word too many)
    b.h.ops_cap = (u32)b.ops.size( );
    u32 err = 0;
    ma::AlnBuilder ab;
    ab.h = &b.h, ab.ops = b.ops.data( ), ab.err = &err;
    const ma::NwParams N = nwParams( rP );
    Appender xApp{ N, ab };
    b.bOk = ma_inv::assemble(
        (uint32_t)vCigar.size( ), [ & ]( uint32_t i ) { return vCigar[ i ]; }, [ & ]( uint64_t i ) { return pQuery[ rS.startQ + i ]; },
        [ & ]( uint64_t i ) { return vWindow.at( i ); }, xApp );
    ma::aln_flush( ab );
    check( err == 0, "ops beyond the bound" );
    b.ops.resize( b.h.n_ops );
    b.bKept = b.bOk && ma_inv::kept( ma_inv::params( rP ), b.h.score );
    if( b.bKept )
        ma_inv::place( b.h, rParent, rS, rJob );
    return b;
}
static uint8_t textCode( const Input& rIn, uint64_t p ) // Pack::vExtractSubsection: the doubled text
{
    const uint64_t F = rIn.vGenome.size( );
    return p < F ? rIn.vGenome[ p ] : (uint8_t)( 3 - rIn.vGenome[ 2 * F - 1 - p ] );
}

static int golden( const char* sCase, const char* sDump, bool bPaired, int iZd )
{
    const Input in = fromF4Dump( sCase, sDump, bPaired );
    ma_params P;
    ma_params_default( &P );
    const uint64_t F = in.vGenome.size( ), N = 2 * F;
    size_t nRecords = 0, nStretches = 0, nInversions = 0, nFiltered = 0, nCompared = 0;
    for( size_t u = 0; u < in.vReads.size( ); u++ )
    {
        const ma_sam::FlatList l = in.list( u );
        // 1. shared scan == the host module's, on every record, under four thresholds
        for( uint32_t k = 0; k < l.size( ); k++ )
            for( int zd : { 1, 40, 100, 100000 } )
            {
                P.zdrop_inversion = zd;
                const Stretches a = sharedScan( P, l, k );
                check( same( a, yardstickScan( P, in, u, k ) ), "read " + std::to_string( u ) + " record " + std::to_string( k ) + " zd " +
                                                                    std::to_string( zd ) + ": scanDrops and DropScan differ" );
                nCompared++;
                check( zd != 100000 || a.empty( ), "a drop of 100000" );
            }
        // 2. at the dump's threshold: the records behind a parent are its stretches' records, in stretch order; each is rebuilt
        P.zdrop_inversion = iZd;
        const ma_inv::Params IP = ma_inv::params( P );
        uint32_t k = 0;
        while( k < l.size( ) )
        {
            const uint32_t uiParent = k++;
            const ma_alignment& rParent = l.alns[ uiParent ];
            nRecords++;
            for( const ma_inv::Stretch& s : sharedScan( P, l, uiParent ) )
            {
                nStretches++;
                ma_inv::Job j;
                check( ma_inv::stretchJob( IP, s, in.vReads[ u ].vCodes.size( ), N, F, j ) == ma_inv::OK, "a stretch of the reference's own record is refused" );
                const bool bHere = k < l.size( ) && l.alns[ k ].supplementary && !l.alns[ k ].secondary && l.alns[ k ].mapq == 0 &&
                                   (uint64_t)l.alns[ k ].begin_q == s.startQ && (uint64_t)l.alns[ k ].begin_ref == j.winBegin;
                if( !bHere )
                {
                    nFiltered++; // (the score filter dropped it: the DP is not run here)
                    continue;
                }
                const ma_alignment& rInv = l.alns[ k ];
                // the record's own ops as the cigar kswcpp returned: match / mismatch runs merge into M
                std::vector<uint32_t> vCigar;
                for( uint32_t o = 0; o < rInv.n_ops; o++ )
                {
                    const uint64_t t = l.opType( k, o ), len = l.opLen( k, o );
                    const uint32_t sym = t == ma_inv::OP_INSERTION ? 1u : ( t == ma_inv::OP_DELETION ? 2u : 0u );
                    check( t != ma_inv::OP_SEED, "an inversion record with a seed op" );
                    if( !vCigar.empty( ) && ( vCigar.back( ) & 0xf ) == sym )
                        vCigar.back( ) += (uint32_t)len << 4;
                    else
                        vCigar.push_back( (uint32_t)len << 4 | sym );
                }
                std::vector<uint8_t> vWindow( (size_t)j.tlen );
                for( size_t i = 0; i < vWindow.size( ); i++ )
                    vWindow[ i ] = textCode( in, j.winBegin + i );
                const Built b = build( P, vCigar, in.vReads[ u ].vCodes.data( ), vWindow, rParent, s, j );
                const std::string sAt = "read " + std::to_string( u ) + " record " + std::to_string( k );
                check( b.bOk && b.bKept, sAt + ": the reference's inversion record is not kept" );
                check( b.h.begin_ref == (u64)rInv.begin_ref && b.h.end_ref == (u64)rInv.end_ref && b.h.begin_q == (u64)rInv.begin_q &&
                           b.h.end_q == (u64)rInv.end_q,
                       sAt + ": bounds" );
                check( b.h.score == rInv.score, sAt + ": score" );
                check( b.h.supplementary == 1 && b.h.secondary == 0 && memcmp( &b.h.mapq, &rInv.mapq, 8 ) == 0, sAt + ": flags / mapq bits" );
                check( b.h.soc_index == rInv.soc_index, sAt + ": strip index" );
                check( b.h.n_ops == rInv.n_ops, sAt + ": number of ops" );
                for( uint32_t o = 0; o < rInv.n_ops; o++ )
                    check( ma::op_type( b.ops[ o ] ) == l.opType( k, o ) && ma::op_len( b.ops[ o ] ) == l.opLen( k, o ), sAt + ": op " + std::to_string( o ) );
                nInversions++;
                k++;
            }
        }
    }
    printf( "golden ok: %zu records, %zu scans compared, %zu stretches, %zu inversion records rebuilt, %zu without a record\n", nRecords, nCompared,
            nStretches, nInversions, nFiltered );
    return 0;
}

// ---- hand-made records --------------------------------------------------------------------------------------------------
struct Hand
{
    Input in;
    Hand( )
    {
        in.addContig( "c", 4000 );
        Rng g( 7 );
        for( int i = 0; i < 4000; i++ )
            in.vGenome.push_back( (uint8_t)below( g, 4 ) );
        ReadData q;
        q.sName = "q";
        q.vCodes.assign( 400, 0 );
        in.vReads.push_back( q );
        in.vOff.assign( 1, 0 );
    }
    uint32_t add( uint64_t uiBeginQ, uint64_t uiBeginR, std::vector<std::pair<uint32_t, uint64_t>> vOps )
    {
        ma_alignment a{ };
        a.begin_q = a.end_q = (int64_t)uiBeginQ, a.begin_ref = a.end_ref = (int64_t)uiBeginR;
        a.ops_off = in.vOps.size( ) / 2, a.n_ops = (uint32_t)vOps.size( ), a.soc_index = 3;
        for( auto& o : vOps )
        {
            in.vOps.push_back( o.first ), in.vOps.push_back( o.second );
            a.end_q += o.first != ma_inv::OP_DELETION ? (int64_t)o.second : 0;
            a.end_ref += o.first != ma_inv::OP_INSERTION ? (int64_t)o.second : 0;
        }
        in.vAlns.push_back( a );
        in.vOff.assign( { 0, in.vAlns.size( ) } );
        return (uint32_t)in.vAlns.size( ) - 1;
    }
};

static int handmade( )
{
    using namespace ma_inv;
    ma_params P;
    ma_params_default( &P ); // match 2, mismatch 4, gap 4, extend 2, harm_score_min 18
    Hand H;
    const uint64_t F = 4000, N = 8000;
    // a drop of 20 + 100 - 30 * 2 = 60 behind 10 matches: ( match 10, mismatch 30 ) scores 20, then -100, 30 away
    const uint32_t kNoSeed = H.add( 5, 1000, { { OP_MATCH, 10 }, { OP_MISMATCH, 30 }, { OP_MATCH, 20 } } );
    const uint32_t kBehindLast = H.add( 5, 1000, { { OP_SEED, 20 }, { OP_MATCH, 10 }, { OP_MISMATCH, 30 } } );
    const uint32_t kBeforeFirst = H.add( 5, 1000, { { OP_MATCH, 10 }, { OP_MISMATCH, 30 }, { OP_SEED, 20 } } );
    const uint32_t kTwo = H.add( 0, 1000, { { OP_SEED, 20 }, { OP_MATCH, 10 }, { OP_MISMATCH, 30 }, { OP_SEED, 20 }, { OP_MATCH, 10 },
                                            { OP_MISMATCH, 30 }, { OP_SEED, 20 } } );
    // a drop of 40 + 68 - 50 * 2 = 8 behind a seed of 20: ( deletion 10, deletion 40 ) scores 16, then -68, 50 away; the same with insertions
    const uint32_t kNoQuery = H.add( 0, 1000, { { OP_SEED, 20 }, { OP_DELETION, 10 }, { OP_DELETION, 40 }, { OP_SEED, 20 } } );
    const uint32_t kNoWindow = H.add( 0, 1000, { { OP_SEED, 20 }, { OP_INSERTION, 10 }, { OP_INSERTION, 40 }, { OP_SEED, 20 } } );
    const uint32_t kReverse = H.add( 0, 5000, { { OP_SEED, 20 }, { OP_MATCH, 10 }, { OP_MISMATCH, 30 }, { OP_SEED, 20 } } );
    const uint32_t kExact = H.add( 0, 1000, { { OP_SEED, 20 }, { OP_MATCH, 10 }, { OP_MISMATCH, 20 }, { OP_SEED, 20 } } ); // drop 60 + 20 - 40 = 40
    const ma_sam::FlatList l = H.in.list( 0 );
    auto scan = [ & ]( uint32_t k, int zd ) {
        P.zdrop_inversion = zd;
        const Stretches a = sharedScan( P, l, k );
        check( same( a, yardstickScan( P, H.in, 0, k ) ), "hand-made record " + std::to_string( k ) + ": scanDrops and DropScan differ" );
        return a;
    };
    auto is = []( const Stretches& v, std::vector<ma_inv::Stretch> w ) { return same( v, w ); };
    check( scan( kNoSeed, 1 ).empty( ), "no seed op: no stretch is ever reported" );
    check( scan( kBehindLast, 1 ).empty( ), "a drop behind the last seed is never reported" );
    check( is( scan( kBeforeFirst, 60 ), { { 5, 1000, 45, 1040 } } ), "the stretch before the first seed starts at the record's begin" );
    check( scan( kBeforeFirst, 61 ).empty( ), "the drop is 60: not >= 61" );
    check( is( scan( kTwo, 60 ), { { 20, 1020, 60, 1060 }, { 80, 1080, 120, 1120 } } ), "two stretches, in the order of the walk" );
    check( is( scan( kExact, 40 ), { { 20, 1020, 50, 1050 } } ) && scan( kExact, 41 ).empty( ), "the drop is compared with >=" );
    check( is( scan( kNoQuery, 8 ), { { 20, 1020, 20, 1070 } } ) && scan( kNoQuery, 9 ).empty( ), "deletions only: qlen 0" );
    check( is( scan( kNoWindow, 8 ), { { 20, 1020, 70, 1020 } } ), "insertions only: tlen 0" );
    const ma_inv::Params IP = params( P );
    Job j;
    // the windows
    check( stretchJob( IP, Stretch{ 20, 1020, 60, 1060 }, 400, N, F, j ) == OK && j.winBegin == 8000 - 1061 && j.winEnd == 8000 - 1021 && j.qlen == 40 &&
               j.tlen == 40 && j.w == P.bandwidth_ext && j.zdrop == P.zdrop && j.flag == 0 && j.hasDp( ),
           "the reverse-strand window of a forward stretch" );
    check( stretchJob( IP, scan( kReverse, 60 ).at( 0 ), 400, N, F, j ) == OK && j.winBegin == 8000 - 5061 && j.winEnd <= F && j.hasDp( ),
           "a parent on the reverse strand has its window on the forward strand" );
    check( stretchJob( IP, Stretch{ 20, 1020, 20, 1070 }, 400, N, F, j ) == OK && j.qlen == 0 && j.tlen == 50 && !j.hasDp( ), "qlen 0: no DP" );
    Job j0 = j;
    check( stretchJob( IP, Stretch{ 20, 1020, 70, 1020 }, 400, N, F, j ) == OK && j.qlen == 50 && j.tlen == 0 && !j.hasDp( ), "tlen 0: no DP" );
    check( stretchJob( IP, Stretch{ 20, 1020, 401, 1060 }, 400, N, F, j ) == ERR_BEYOND_READ, "a stretch beyond its read" );
    check( stretchJob( IP, Stretch{ 20, 1020, 60, 8000 }, 400, N, F, j ) == ERR_OUTSIDE_TEXT, "a stretch beyond the text" );
    check( stretchJob( IP, Stretch{ 20, 3990, 60, 4010 }, 400, N, F, j ) == ERR_BRIDGING, "a window on both strands" );
    // the score filter: k matches score 2 k; harm_score_min * match = 36
    const ma_alignment& rParent = l.alns[ kTwo ];
    for( uint32_t n : { 18u, 19u } )
    {
        const Stretch s{ 20, 1020, 20 + n, 1020 + n };
        check( stretchJob( IP, s, 400, N, F, j ) == OK, "job" );
        std::vector<uint8_t> vWindow( n, 0 ); // (the read is all A)
        const Built b = build( P, { n << 4 }, H.in.vReads[ 0 ].vCodes.data( ), vWindow, rParent, s, j );
        check( b.bOk && b.h.score == 2 * (int64_t)n && b.bKept == ( n == 19 ), "score " + std::to_string( 2 * n ) + " against harm_score_min * match = 36" );
        if( b.bKept )
            check( b.h.begin_q == 20 && b.h.end_q == 39 && b.h.begin_ref == j.winBegin && b.h.end_ref == j.winBegin + 19 && b.h.supplementary == 1 &&
                       b.h.secondary == 0 && b.h.mapq == 0 && b.h.soc_index == 3 && b.h.n_ops == 1 && b.ops[ 0 ] == ma::op_pack( OP_MATCH, 19 ),
                   "the kept record's place" );
    }
    {
        // M runs split base by base, runs merge, indels as they are: 3M 2I 2M 1D over AAA.. against A A C | A A
        const Stretch s{ 20, 1020, 27, 1026 };
        check( stretchJob( IP, s, 400, N, F, j ) == OK, "job" );
        ma_params Pd = P;
        Pd.disable_heuristics = 1;
        const Built b = build( Pd, { 3u << 4, 2u << 4 | 1, 2u << 4, 1u << 4 | 2 }, H.in.vReads[ 0 ].vCodes.data( ), { 0, 0, 1, 0, 0, 3 }, rParent, s, j );
        check( b.bOk && b.bKept && b.h.n_ops == 5 && b.ops[ 0 ] == ma::op_pack( OP_MATCH, 2 ) && b.ops[ 1 ] == ma::op_pack( OP_MISMATCH, 1 ) &&
                   b.ops[ 2 ] == ma::op_pack( OP_INSERTION, 2 ) && b.ops[ 3 ] == ma::op_pack( OP_MATCH, 2 ) && b.ops[ 4 ] == ma::op_pack( OP_DELETION, 1 ) &&
                   b.h.score == 4 - 4 - 8 + 4 - 6 && b.h.end_q == 27 && b.h.end_ref == j.winBegin + 6,
               "match / mismatch split, merged runs, Alignment's score" );
        check( !build( Pd, { 3u << 4 | 3 }, H.in.vReads[ 0 ].vCodes.data( ), { 0, 0, 0 }, rParent, s, j ).bOk, "a symbol that is none of M I D" );
        // disable_heuristics keeps the empty record of a job without DP; the heuristics drop it
        const Stretch e{ 20, 1020, 20, 1070 };
        const Built d = build( Pd, { }, H.in.vReads[ 0 ].vCodes.data( ), { }, rParent, e, j0 );
        check( d.bKept && d.h.n_ops == 0 && d.h.begin_q == 20 && d.h.end_q == 20 && d.h.begin_ref == j0.winBegin && d.h.end_ref == j0.winBegin &&
                   d.h.score == 0 && d.h.supplementary == 1,
               "disable_heuristics keeps an empty record" );
        check( !build( P, { }, H.in.vReads[ 0 ].vCodes.data( ), { }, rParent, e, j0 ).bKept, "the heuristics drop an empty record" );
    }
    printf( "handmade ok\n" );
    return 0;
}

int main( int argc, char** argv )
{
    try
    {
        if( argc == 6 && !strcmp( argv[ 1 ], "golden" ) )
            return golden( argv[ 2 ], argv[ 3 ], atoi( argv[ 4 ] ) != 0, atoi( argv[ 5 ] ) );
        if( argc == 2 && !strcmp( argv[ 1 ], "handmade" ) )
            return handmade( );
        fprintf( stderr, "usage: inv_dev_test golden <case> <f4 dump> <paired> <zd> | handmade\n" );
        return 2;
    }
    catch( const std::exception& e )
    {
        fprintf( stderr, "FAILED: %s\n", e.what( ) );
        return 1;
    }
}
