// CPU-only checks of the NGMLR tag emulation of the record formatter the device stage runs (ma_amd/host/ma_sam_dev.h:
// ma_sam::formatRead( sink, options | NGMLR_TAGS, contigs, read, list, ref ) over its counting and its writing sink) against the
// yardstick, ma_amd's FileWriter with bEmulateNgmlrTags (ma_amd/host/ma_sam.h), and the SAM goldens the compiled reference wrote.
//   sam_tags_dev_test golden <case> <pipe dump> <golden.sam> <options>   the records of a pipeline dump: shared formatter ==
//                                                                         FileWriter == the record lines of the golden
//   sam_tags_dev_test random <seed> <lists>                               seeded random record lists over a two-contig genome with
//                                                                         holes under all 32 option sets with the tag bit, plus the
//                                                                         deterministic cases; the census is asserted
//   sam_tags_dev_test floats <seed> <n>                                   the %f formatter against snprintf
//   sam_tags_dev_test dump <dump> <out> <options>                         the yardstick of tests/test_gpu_sam_tags.py: FileWriter's
//                                                                         text of a dump (format MASAMT01: that of sam_dev_test
//                                                                         plus genome bases and holes) to <out>, the per-read
//                                                                         offsets (u64) to <out>.off; an exception is printed as
//                                                                         "ERROR: <text>" (exit code 3)
//   sam_tags_dev_test case <name> <out>                                   writes one of the deterministic cases as a dump (the GPU
//                                                                         test injects it through ma_batch_set_alignments)
// options: the MA_SAM_* bits of include/ma_amd.h.  Every count of the counting sink is checked against the bytes written; the
// writing sink gets a buffer of exactly that size, the reads hold exactly their bases and pac exactly the forward strand, so
// that an AddressSanitizer build of this program sees any byte touched outside of them.
#include "sam_dev_common.h"

#include <map>

// the yardstick: FileWriter::execute over all reads, on fresh Alignment containers (it swaps their ops); throws what it throws
static std::string yardstick( const Input& rIn, uint32_t uiOptions, std::vector<uint64_t>* pOff = nullptr )
{
    return fileWriterText( rIn, uiOptions, pOff );
}
// the shared formatter: counting sink, then the writing sink into exactly that many bytes
static DevResult shared( const Input& rIn, uint32_t uiOptions )
{
    const DevContigs xC( rIn );
    const std::vector<uint8_t> vPac = rIn.pac( );
    const ma_sam::Ref xRef{ vPac.data( ), rIn.vHoleStart.data( ), rIn.vHoleLen.data( ), rIn.vHoleStart.size( ), rIn.forward( ) };
    return countThenWrite( rIn.vReads.size( ), [ & ]( auto& rSink, size_t r ) {
        ma_sam::formatRead( rSink, uiOptions, xC.xView, rIn.vReads[ r ].view( ), rIn.list( r ), xRef );
    } );
}

// ---- golden pass ---------------------------------------------------------------------------------------------------------
static int golden( int argc, char** argv )
{
    if( argc < 6 )
        return 2;
    const Input in = fromPipeDump( argv[ 2 ], argv[ 3 ] );
    const uint32_t uiOptions = (uint32_t)atoi( argv[ 5 ] );
    const std::string sGolden = goldenRecords( argv[ 4 ] );
    const std::string sYard = yardstick( in, uiOptions );
    const DevResult xDev = shared( in, uiOptions );
    if( xDev.uiErrors )
        throw std::runtime_error( "the shared formatter reports errors on the golden records" );
    compare( xDev.sText, sYard, "shared formatter against FileWriter" );
    compare( xDev.sText, sGolden, "shared formatter against the golden" );
    printf( "golden ok: %zu reads, %zu records, %zu bytes\n", in.vReads.size( ), in.vAlns.size( ), sYard.size( ) );
    return 0;
}

// ---- generated records ---------------------------------------------------------------------------------------------------
// two contigs; holes: 150 bases 40 bases into contig 0, 120 bases further on, 30 bases, one touching the contig border
static Input genome( Rng& g, uint64_t uiLen0 = 3000, uint64_t uiLen1 = 2500 )
{
    Input in;
    in.vNames = { "ctgA", "second_contig" };
    in.vStarts = { 0, uiLen0 };
    in.vLengths = { uiLen0, uiLen1 };
    for( uint64_t i = 0; i < uiLen0 + uiLen1; i++ )
        in.vGenome.push_back( (uint8_t)below( g, 4 ) );
    in.vHoleStart = { 40, 700, 1500, uiLen0 - 90 };
    in.vHoleLen = { 150, 120, 30, 90 };
    in.vOff.assign( 1, 0 );
    return in;
}

typedef std::vector<std::pair<uint64_t, uint64_t>> Ops;
// appends one read with the records given: each (ops, reverse strand, forward start, secondary, supplementary, begin_q);
// the read is as long as its longest record needs plus uiTail
struct RecSpec
{
    Ops vOps;
    bool bRev;
    uint64_t uiForwardStart;
    bool bSecondary, bSupplementary;
    uint64_t uiBeginQ;
    double fMapq;
    int64_t iScore;
};
static void spans( const Ops& v, uint64_t& r, uint64_t& q )
{
    r = q = 0;
    for( auto& o : v )
    {
        r += o.first != 3 ? o.second : 0;
        q += o.first != 4 ? o.second : 0;
    }
}
static void addRead( Input& in, Rng& g, const std::vector<RecSpec>& vRecs, uint64_t uiTail, bool bQual, const std::string& sName )
{
    const uint64_t F = in.forward( );
    uint64_t uiLen = 0;
    for( auto& s : vRecs )
    {
        uint64_t r, q;
        spans( s.vOps, r, q );
        uiLen = std::max( uiLen, s.uiBeginQ + q );
        ma_alignment a{ };
        a.begin_ref = (int64_t)( s.bRev ? 2 * F - ( s.uiForwardStart + r ) : s.uiForwardStart ), a.end_ref = a.begin_ref + (int64_t)r;
        a.begin_q = (int64_t)s.uiBeginQ, a.end_q = (int64_t)( s.uiBeginQ + q );
        a.score = s.iScore, a.mapq = s.fMapq, a.secondary = s.bSecondary, a.supplementary = s.bSupplementary;
        a.ops_off = in.vOps.size( ) / 2, a.n_ops = (uint32_t)s.vOps.size( );
        for( auto& o : s.vOps )
            in.vOps.push_back( o.first ), in.vOps.push_back( o.second );
        in.vAlns.push_back( a );
    }
    ReadData q;
    q.sName = sName;
    q.bQual = bQual;
    for( uint64_t i = 0; i < uiLen + uiTail; i++ )
    {
        q.vCodes.push_back( (uint8_t)( below( g, 16 ) == 0 ? 4 : below( g, 4 ) ) );
        if( bQual )
            q.vQual.push_back( (uint8_t)( '!' + below( g, 94 ) ) );
    }
    in.vReads.push_back( q );
    in.vOff.push_back( in.vAlns.size( ) );
}
static void finish( Input& in )
{
    in.vOps.push_back( 0 ), in.vOps.push_back( 0 );
}
static Ops withRun( const char* sRun ) // 20 matches, the run of single insertions / deletions of 2 / 3 bases, a mismatch, 15 seeds
{
    Ops v{ { 1, 20 } };
    for( const char* p = sRun; *p; p++ )
        v.emplace_back( *p == 'I' ? 3 : 4, *p == 'I' ? 2 : 3 );
    v.emplace_back( 2, 1 );
    v.emplace_back( 0, 15 );
    return v;
}
static Ops singleBaseOps( uint32_t n ) // no two neighbours of one type; an insertion next to a deletion every eight
{
    static const uint64_t aType[ 8 ] = { 1, 0, 2, 3, 4, 1, 2, 4 };
    Ops v;
    for( uint32_t j = 0; j < n; j++ )
        v.emplace_back( aType[ j % 8 ], 1 );
    return v;
}

// the deterministic cases, by name (tests/test_gpu_sam_tags.py injects the same ones on the device)
static Input caseOf( const std::string& sName )
{
    Rng g( 20261019 );
    if( sName == "long" ) // one record of 0x10000 ops per strand over 200 kb
    {
        Input in = genome( g, 120000, 80000 );
        for( int iRev = 0; iRev < 2; iRev++ )
            addRead( in, g, { { singleBaseOps( 0x10000 ), iRev != 0, 5000, false, false, 100, 0.5, 4321 } }, 50, true, iRev ? "long-" : "long+" );
        finish( in );
        return in;
    }
    Input in = genome( g );
    if( sName == "runs" ) // the four I/D runs (and two longer ones) on both strands
    {
        for( const char* sRun : { "DI", "ID", "IDI", "IDID", "DIDID", "IID" } )
            for( int iRev = 0; iRev < 2; iRev++ )
                addRead( in, g, { { withRun( sRun ), iRev != 0, 300 + 100 * below( g, 20 ), false, false, below( g, 5 ), 0.25, 77 } }, below( g, 9 ), iRev != 0,
                         std::string( sRun ) + ( iRev ? "-" : "+" ) );
    }
    else if( sName == "sisters" ) // three reverse-strand sisters with runs: the swap shows in those before a record only
    {
        const std::vector<RecSpec> v{ { withRun( "ID" ), true, 400, false, false, 0, 0.5, 10 },
                                      { withRun( "DI" ), true, 900, false, true, 40, 0.125, -3 },
                                      { withRun( "IDI" ), true, 2200, false, true, 80, std::numeric_limits<double>::quiet_NaN( ), 0 } };
        addRead( in, g, v, 7, true, "three" );
        // a secondary one and one of op length 0 among them, a forward one
        std::vector<RecSpec> w = v;
        w[ 1 ].bSecondary = true;
        w.push_back( { Ops{ { 1, 0 }, { 4, 0 } }, true, 1000, false, false, 3, 1.0, 5 } );
        w.push_back( { withRun( "ID" ), false, 3100, false, false, 3, 0.75, 5 } );
        addRead( in, g, w, 0, false, "five" );
    }
    else if( sName == "span0" ) // all insertions: 0 reference bases, 0 matches; all deletions: 0 query bases
    {
        addRead( in, g, { { Ops{ { 3, 12 } }, false, 250, false, false, 2, 0.5, -30 } }, 3, true, "ins" );
        addRead( in, g, { { Ops{ { 4, 9 } }, true, 250, false, false, 2, 0.5, -20 }, { Ops{ { 1, 30 } }, false, 600, false, true, 0, 0.5, 30 } }, 3, true,
                 "del" );
    }
    else if( sName == "edges" ) // begin_ref 10 (the wrap-around), behind and before holes, under a hole, the genome's last base
    {
        addRead( in, g, { { Ops{ { 1, 50 }, { 2, 3 }, { 4, 2 }, { 2, 2 }, { 1, 30 } }, false, 10, false, false, 0, 0.5, 60 } }, 0, true, "wrap" );
        addRead( in, g, { { Ops{ { 1, 60 } }, false, 190, false, false, 0, 0.5, 60 } }, 40, true, "behind_hole" ); // SV 1
        addRead( in, g, { { Ops{ { 1, 60 } }, false, 640, false, false, 0, 0.5, 60 } }, 0, false, "before_hole" ); // SV 3
        addRead( in, g, { { Ops{ { 0, 50 }, { 2, 4 }, { 1, 50 } }, false, 1460, false, false, 0, 0.5, 60 } }, 400, true, "over_hole" ); // SV 0
        addRead( in, g, { { Ops{ { 1, 50 }, { 3, 1 }, { 1, 50 } }, true, in.forward( ) - 100, false, false, 0, 0.5, 60 } }, 0, true, "last_base-" );
        addRead( in, g, { { Ops{ { 1, 50 }, { 4, 1 }, { 1, 49 } }, false, in.forward( ) - 100, false, false, 0, 0.5, 60 } }, 0, true, "last_base+" );
        addRead( in, g, { { Ops{ { 1, 40 } }, true, 2910, false, false, 0, 0.5, 60 } }, 0, true, "border_hole-" );
    }
    else
        throw std::runtime_error( "unknown case " + sName );
    finish( in );
    return in;
}

struct Census
{
    std::map<std::string, size_t> m;
    void count( const std::string& s, bool b = true )
    {
        m[ s ] += b ? 1 : 0;
    }
};
// what the records of an input hold (under the tag option alone: a record is printed when its ops have a length)
static void census( const Input& in, Census& c )
{
    const uint64_t F = in.forward( );
    auto runs = [ & ]( const ma_alignment& a ) { // the I/D runs of the record as a string, ops of other types as '.'
        std::string s;
        for( uint32_t j = 0; j < a.n_ops; j++ )
        {
            const uint64_t t = in.vOps[ 2 * ( a.ops_off + j ) ];
            s.push_back( t == 3 ? 'I' : t == 4 ? 'D' : '.' );
        }
        return "." + s + ".";
    };
    auto nonZero = [ & ]( const ma_alignment& a ) {
        for( uint32_t j = 0; j < a.n_ops; j++ )
            if( in.vOps[ 2 * ( a.ops_off + j ) + 1 ] )
                return true;
        return false;
    };
    auto swaps = [ & ]( const ma_alignment& a ) { return (uint64_t)a.begin_ref >= F && ( runs( a ).find( "ID" ) != std::string::npos || runs( a ).find( "DI" ) != std::string::npos ); };
    const ma_sam::Ref xRef{ nullptr, in.vHoleStart.data( ), in.vHoleLen.data( ), in.vHoleStart.size( ), F };
    for( size_t r = 0; r + 1 < in.vOff.size( ); r++ )
        for( uint64_t k = in.vOff[ r ]; k < in.vOff[ r + 1 ]; k++ )
        {
            const ma_alignment& a = in.vAlns[ k ];
            const bool bRev = (uint64_t)a.begin_ref >= F, bPrinted = nonZero( a );
            const std::string s = runs( a );
            if( bRev && bPrinted )
                for( const char* sRun : { "DI", "ID", "IDI", "IDID" } )
                    c.count( std::string( "reverse " ) + sRun, s.find( std::string( "." ) + sRun + "." ) != std::string::npos );
            c.count( "reverse", bRev && bPrinted );
            c.count( "forward", !bRev && bPrinted );
            c.count( "begin_ref < 100", bPrinted && a.begin_ref < 100 );
            c.count( "0x10000 ops", a.n_ops >= 0x10000 );
            c.count( "NaN mapq", a.mapq != a.mapq );
            c.count( "negative score", a.score < 0 );
            uint64_t uiAt = (uint64_t)a.begin_ref, uiSpanR = 0, uiSpanQ = 0;
            for( uint32_t j = 0; j < a.n_ops; j++ )
            {
                const uint64_t t = in.vOps[ 2 * ( a.ops_off + j ) ], l = in.vOps[ 2 * ( a.ops_off + j ) + 1 ];
                if( bPrinted && j > 0 && t == 2 && l > 0 && in.vOps[ 2 * ( a.ops_off + j - 1 ) ] == 4 && !swaps( a ) )
                    c.count( "deletion then mismatch" );
                c.count( "mismatch section longer than 1", bPrinted && t == 2 && l > 1 );
                c.count( "hole under a match", bPrinted && t <= 1 && xRef.holeBasesDoubled( uiAt, l ) > 0 );
                uiAt += t != 3 ? l : 0, uiSpanR += t != 3 ? l : 0, uiSpanQ += t != 4 ? l : 0;
            }
            c.count( "span 0", bPrinted && ( uiSpanR == 0 || uiSpanQ == 0 ) );
            // sisters
            bool bSwappedBefore = false, bUnswappedBehind = false;
            for( uint64_t s2 = in.vOff[ r ]; s2 < in.vOff[ r + 1 ]; s2++ )
            {
                const ma_alignment& o = in.vAlns[ s2 ];
                if( s2 == k || !bPrinted )
                    continue;
                c.count( "secondary sister", o.secondary != 0 );
                if( o.secondary )
                    continue;
                c.count( "sister of op length 0", !nonZero( o ) );
                bSwappedBefore |= s2 < k && nonZero( o ) && swaps( o );
                bUnswappedBehind |= s2 > k && swaps( o );
            }
            c.count( "swapped sister before, unswapped behind", bSwappedBefore && bUnswappedBehind );
        }
}
static void censusOfText( const std::string& sText, Census& c )
{
    for( const char* sTag : { "\tSV:i:0\t", "\tSV:i:1\t", "\tSV:i:2\t", "\tSV:i:3\t", "\tSA:Z:", "\tCG:B:I,", "\tXI:f:-nan\t", "\tXI:f:1.000000\t", "\tAS:i:-" } )
        c.count( std::string( "text " ) + ( sTag + 1 ), sText.find( sTag ) != std::string::npos );
}

static Input randomInput( Rng& g, size_t uiLists )
{
    Input in = genome( g );
    const uint64_t F = in.forward( );
    static const uint64_t aStarts[] = { 0, 5, 10, 99, 100, 190, 191, 580, 640, 700, 820, 1400, 1490, 1530, 2800, 2910, 3000, 3001 };
    for( size_t r = 0; r < uiLists; r++ )
    {
        std::vector<RecSpec> vRecs;
        const unsigned kind = (unsigned)below( g, 12 ); // 0: empty list, 1: alignments of length 0 only, else 1 - 4 records
        const size_t nA = kind == 0 ? 0 : 1 + below( g, 4 );
        for( size_t k = 0; k < nA; k++ )
        {
            RecSpec s;
            const uint32_t n = (uint32_t)( kind == 1 ? below( g, 3 ) : 1 + below( g, 12 ) );
            for( uint32_t j = 0; j < n; j++ )
            {
                // matches more often than the rest; now and then an op without length
                const uint64_t t = below( g, 3 ) == 0 ? 1 : below( g, 5 );
                s.vOps.emplace_back( t, kind == 1 || below( g, 12 ) == 0 ? 0 : t <= 1 ? 1 + below( g, 60 ) : 1 + below( g, 4 ) );
            }
            if( kind != 1 && below( g, 3 ) == 0 ) // a run of alternating insertions and deletions spliced in
            {
                static const char* aRuns[] = { "DI", "ID", "IDI", "IDID", "DID", "DIDI", "IDIDI" };
                Ops vRun = withRun( aRuns[ below( g, 7 ) ] );
                s.vOps.insert( s.vOps.begin( ) + (long)below( g, s.vOps.size( ) + 1 ), vRun.begin( ), vRun.end( ) );
            }
            uint64_t sr, sq;
            spans( s.vOps, sr, sq );
            s.bRev = below( g, 2 ) != 0;
            s.uiForwardStart = below( g, 3 ) == 0 ? aStarts[ below( g, sizeof( aStarts ) / sizeof( aStarts[ 0 ] ) ) ] : below( g, F - sr + 1 );
            if( s.uiForwardStart + sr > F )
                s.uiForwardStart = F - sr;
            s.bSecondary = below( g, 4 ) == 0, s.bSupplementary = below( g, 4 ) == 0;
            s.uiBeginQ = below( g, 3 ) == 0 ? 0 : below( g, 30 );
            const unsigned m = (unsigned)below( g, 8 );
            s.fMapq = m == 0 ? std::numeric_limits<double>::quiet_NaN( ) : m == 1 ? 0.0 : m == 2 ? 1.0 : (double)below( g, 1000001 ) / 1000000.0;
            s.iScore = (int64_t)below( g, 2000 ) - 300;
            vRecs.push_back( s );
        }
        std::string sName;
        for( uint64_t i = 0, n = 1 + below( g, 20 ); i < n; i++ )
            sName.push_back( (char)( '!' + below( g, 94 ) ) );
        addRead( in, g, vRecs, below( g, 3 ) == 0 ? 0 : below( g, 40 ), below( g, 2 ) != 0, sName );
    }
    finish( in );
    return in;
}

static void checkAllOptions( const Input& in, const std::string& sWhat, Census& c, size_t& uiBytes )
{
    census( in, c );
    for( uint32_t uiOptions = MA_SAM_NGMLR_TAGS; uiOptions <= ma_sam::ALL_OPTIONS; uiOptions++ )
    {
        if( in.vAlns.size( ) < 4 && ( uiOptions & ( MA_SAM_NO_SECONDARY | MA_SAM_NO_SUPPLEMENTARY | MA_SAM_EQX_CIGAR ) ) )
            continue; // (the two records of 0x10000 ops: the bits that bear on them)
        const std::string sYard = yardstick( in, uiOptions );
        const DevResult xDev = shared( in, uiOptions );
        if( xDev.uiErrors )
            throw std::runtime_error( sWhat + ": errors on well-formed records" );
        compare( xDev.sText, sYard, sWhat + ", options " + std::to_string( uiOptions ) );
        censusOfText( sYard, c );
        c.count( "options " + std::to_string( uiOptions ) );
        if( in.vAlns.size( ) < 4 )
            c.count( ( uiOptions & MA_SAM_NO_CG_TAG ) ? "0x10000 ops without the CG tag" : "0x10000 ops with the CG tag",
                     ( sYard.find( "\tCG:B:I," ) != std::string::npos ) == ( ( uiOptions & MA_SAM_NO_CG_TAG ) == 0 ) );
        uiBytes += sYard.size( );
    }
}

// the error kinds: a bridging record gives the reference's text, ops that cover a base too many or too few are refused
static void errors( )
{
    Rng g( 5 );
    for( int iCase = 0; iCase < 5; iCase++ )
    {
        Input in = genome( g );
        const uint64_t F = in.forward( );
        addRead( in, g, { { Ops{ { 1, 30 } }, false, 300, false, false, 0, 0.5, 1 }, { Ops{ { 1, 40 }, { 2, 1 }, { 1, 9 } }, iCase == 4, 1000, false, true, 0, 0.5, 1 } }, 20,
                 true, "e" );
        finish( in );
        ma_alignment& a = in.vAlns[ 1 ];
        uint32_t uiWant = ma_sam::ERR_OPS_COVERAGE;
        if( iCase == 0 ) // across the strands
            a.begin_ref = (int64_t)F - 20, a.end_ref = (int64_t)F + 30, uiWant = ma_sam::ERR_BRIDGING;
        else if( iCase == 1 ) // beyond the doubled text
            a.begin_ref = (int64_t)( 2 * F ) - 20, a.end_ref = (int64_t)( 2 * F ) + 30, uiWant = ma_sam::ERR_BRIDGING;
        else if( iCase == 2 ) // one reference base too many
            in.vOps[ 2 * a.ops_off + 1 ] += 1, a.end_q += 1;
        else if( iCase == 3 ) // one too few
            a.end_ref += 1;
        else // the query's
            a.end_q -= 1;
        // (the host reads outside its buffer on the others)
        const std::string sHost = uiWant == ma_sam::ERR_BRIDGING ? errorOf( [ & ] { yardstick( in, MA_SAM_NGMLR_TAGS ); } ) : "";
        const DevResult xDev = shared( in, MA_SAM_NGMLR_TAGS );
        char aText[ 96 ];
        ma_sam::errorText( aText, xDev.uiKind, xDev.iValue );
        if( xDev.uiErrors != 1 || xDev.uiKind != uiWant || xDev.uiRecord != 1 )
            throw std::runtime_error( "error case " + std::to_string( iCase ) + ": kind " + std::to_string( xDev.uiKind ) + ", " + std::to_string( xDev.uiErrors ) + " errors" );
        if( uiWant == ma_sam::ERR_BRIDGING && ( sHost != aText || sHost != "(vExtractSubsection) Try to extract bridging sequence. This is impossible." ) )
            throw std::runtime_error( "bridging text: host '" + sHost + "', shared '" + aText + "'" );
        if( shared( in, 0 ).uiErrors ) // without the tags the record prints as it always did
            throw std::runtime_error( "error reported without the tag option" );
    }
}

static int randomPass( int argc, char** argv )
{
    if( argc < 4 )
        return 2;
    Rng g( strtoull( argv[ 2 ], nullptr, 10 ) );
    const size_t uiLists = (size_t)atoi( argv[ 3 ] );
    size_t uiBytes = 0, uiRounds = 0;
    Census c;
    for( const char* sCase : { "runs", "sisters", "span0", "edges", "long" } )
        checkAllOptions( caseOf( sCase ), sCase, c, uiBytes );
    for( size_t done = 0; done < uiLists; done += 250, uiRounds++ )
        checkAllOptions( randomInput( g, 250 ), "random round " + std::to_string( uiRounds ), c, uiBytes );
    errors( );
    // the six-argument entry without the bit is the five-argument one
    {
        const Input in = randomInput( g, 50 );
        for( uint32_t uiOptions : { 0u, 3u, 31u } )
            compare( shared( in, uiOptions ).sText, yardstick( in, uiOptions ), "no tags, options " + std::to_string( uiOptions ) );
    }
    printf( "random ok: %zu lists x 32 option sets, %zu bytes\n", uiRounds * 250, uiBytes );
    for( auto& e : c.m )
        printf( "  %-44s %zu\n", e.first.c_str( ), e.second );
    std::vector<std::string> vNeeded{ "reverse DI", "reverse ID", "reverse IDI", "reverse IDID", "swapped sister before, unswapped behind", "deletion then mismatch",
                                      "mismatch section longer than 1", "text SV:i:0\t", "text SV:i:1\t", "text SV:i:2\t", "text SV:i:3\t", "begin_ref < 100",
                                      "hole under a match", "sister of op length 0", "secondary sister", "0x10000 ops with the CG tag",
                                      "0x10000 ops without the CG tag", "span 0", "text XI:f:-nan\t", "text SA:Z:", "reverse", "forward", "NaN mapq", "text AS:i:-" };
    for( uint32_t o = MA_SAM_NGMLR_TAGS; o <= ma_sam::ALL_OPTIONS; o++ )
        vNeeded.push_back( "options " + std::to_string( o ) );
    for( auto& s : vNeeded )
        if( c.m[ s ] == 0 )
            throw std::runtime_error( "the census lacks: " + s );
    return 0;
}

// ---- the %f formatter ------------------------------------------------------------------------------------------------------
static void checkFloat( float f, size_t& n )
{
    char aWant[ 64 ], aGot[ 64 ];
    snprintf( aWant, sizeof( aWant ), "%f", (double)f );
    ma_sam::WriteSink xOut{ aGot };
    ma_sam::detail::putFloat( xOut, f );
    aGot[ xOut.n ] = 0;
    ma_sam::CountSink xCount;
    ma_sam::detail::putFloat( xCount, f );
    if( strcmp( aWant, aGot ) != 0 || xCount.n != xOut.n )
        throw std::runtime_error( std::string( "%f: want " ) + aWant + ", got " + aGot );
    n++;
}
static int floats( int argc, char** argv )
{
    if( argc < 4 )
        return 2;
    size_t n = 0;
    for( uint32_t b = 1; b <= 4096; b++ )
        for( uint32_t a = 0; a <= b; a++ )
        {
            checkFloat( (float)a / (float)b, n );
            checkFloat( 100.0f * (float)a / (float)b, n );
        }
    Rng g( strtoull( argv[ 2 ], nullptr, 10 ) );
    const size_t uiRandom = (size_t)strtoull( argv[ 3 ], nullptr, 10 );
    for( size_t i = 0; i < uiRandom; i++ )
    {
        // any bit pattern of [0, 128): exponent fields 0 (subnormals) .. 133
        const uint32_t uiBits = (uint32_t)( below( g, 134 ) << 23 ) | (uint32_t)below( g, 1u << 23 );
        float f;
        memcpy( &f, &uiBits, 4 );
        checkFloat( f, n );
    }
    for( float f : { 0.0f, 1.0f, 0.9999995f, 0.99999994f, 99.9999999f, 0.0000005f, 0.00000049999f, 0.5f, 1e10f, 1.8446744e19f, 3e38f, 16777216.0f,
                     1.1e12f, 2.1990233e12f, 4.3980465e12f } )
        checkFloat( f, n );
    // the ratios as the host computes them, the 0 / 0 the host's division makes among them
    for( uint64_t uiNum : { 0ull, 1ull, 7ull, 149ull, 150ull, 1ull << 40, ~0ull } )
        for( uint64_t uiDen : { 0ull, 1ull, 3ull, 150ull, 151ull, ( 1ull << 24 ) + 1, ~0ull } )
            for( int iTimes100 = 0; iTimes100 < 2; iTimes100++ )
            {
                volatile float fNum = iTimes100 ? 100.0f * (float)uiNum : (float)uiNum, fDen = (float)uiDen;
                const std::string sWant = std::to_string( fNum / fDen );
                char aGot[ 64 ];
                ma_sam::WriteSink xOut{ aGot };
                ma_sam::detail::putRatio( xOut, iTimes100 != 0, uiNum, uiDen );
                if( sWant != std::string( aGot, xOut.n ) )
                    throw std::runtime_error( "ratio " + std::to_string( uiNum ) + " / " + std::to_string( uiDen ) + ": want " + sWant + ", got " +
                                              std::string( aGot, xOut.n ) );
                n++;
            }
    printf( "floats ok: %zu values\n", n );
    return 0;
}

// ---- dumps -----------------------------------------------------------------------------------------------------------------
static void writeDump( const Input& in, const char* sPath ) // (reads of one kind: all with qualities or all without)
{
    FILE* f = fopen( sPath, "wb" );
    if( !f )
        throw std::runtime_error( std::string( "cannot write " ) + sPath );
    auto wr = [ & ]( const void* p, size_t n ) { fwrite( p, 1, n, f ); };
    auto u32 = [ & ]( uint32_t v ) { wr( &v, 4 ); };
    auto u64 = [ & ]( uint64_t v ) { wr( &v, 8 ); };
    wr( "MASAMT01", 8 );
    u32( (uint32_t)in.vNames.size( ) );
    for( size_t i = 0; i < in.vNames.size( ); i++ )
    {
        u32( (uint32_t)in.vNames[ i ].size( ) );
        wr( in.vNames[ i ].data( ), in.vNames[ i ].size( ) );
        u64( in.vStarts[ i ] ), u64( in.vLengths[ i ] );
    }
    u64( in.vGenome.size( ) );
    wr( in.vGenome.data( ), in.vGenome.size( ) );
    u64( in.vHoleStart.size( ) );
    for( size_t i = 0; i < in.vHoleStart.size( ); i++ )
        u64( in.vHoleStart[ i ] ), u64( in.vHoleLen[ i ] );
    u32( (uint32_t)in.vReads.size( ) ), u32( 1 );
    for( auto& q : in.vReads )
    {
        u32( (uint32_t)q.sName.size( ) );
        wr( q.sName.data( ), q.sName.size( ) );
        u32( (uint32_t)q.vCodes.size( ) );
        wr( q.vCodes.data( ), q.vCodes.size( ) );
        std::vector<uint8_t> vQ = q.vQual;
        vQ.resize( q.vCodes.size( ), (uint8_t)'#' ); // (a read the case left without qualities gets some)
        wr( vQ.data( ), vQ.size( ) );
    }
    wr( in.vOff.data( ), in.vOff.size( ) * 8 );
    wr( in.vAlns.data( ), in.vAlns.size( ) * sizeof( ma_alignment ) );
    u64( in.vOps.size( ) / 2 - 1 );
    wr( in.vOps.data( ), ( in.vOps.size( ) - 2 ) * 8 );
    fclose( f );
}

static int dump( int argc, char** argv )
{
    if( argc < 5 )
        return 2;
    Input in;
    {
        DumpFile f( argv[ 2 ] );
        readDump( f, in, "MASAMT01", true, 1 );
    }
    return writeYardstick( argv[ 3 ], [ & ]( std::vector<uint64_t>* pOff ) { return yardstick( in, (uint32_t)atoi( argv[ 4 ] ), pOff ); } );
}

int main( int argc, char** argv )
{
    if( argc < 2 )
        return 2;
    const std::string sMode = argv[ 1 ];
    try
    {
        if( sMode == "golden" )
            return golden( argc, argv );
        if( sMode == "random" )
            return randomPass( argc, argv );
        if( sMode == "floats" )
            return floats( argc, argv );
        if( sMode == "dump" )
            return dump( argc, argv );
        if( sMode == "case" && argc >= 4 )
        {
            writeDump( caseOf( argv[ 2 ] ), argv[ 3 ] );
            return 0;
        }
    }
    catch( const std::exception& e )
    {
        fprintf( stderr, "sam_tags_dev_test %s: %s\n", sMode.c_str( ), e.what( ) );
        return 1;
    }
    return 2;
}
