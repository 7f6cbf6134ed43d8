// CPU-only checks of the record formatter the device stage runs (ma_amd/host/ma_sam_dev.h: ma_sam::formatRead over its counting
// and its writing sink) and of the host's flat writer on top of it (flat::formatRead of ma_amd/host/ma_flat_sam.h) against the
// yardstick, FileWriter::execute of ma_amd/host/ma_sam.h on fresh Alignment containers, and the SAM goldens.
//   sam_dev_test golden <case> <pipe dump> <golden.sam> <options>   the records of a pipeline dump: the formatter under both
//                                                                    sinks, the flat writer, the yardstick and the record
//                                                                    lines of the golden must agree byte for byte
//   sam_dev_test random <seed> <lists>                               seeded random record lists under every option combination
//   sam_dev_test special                                             cigars of 65 535 / 65 536 ops (CG tag), the two error texts
//   sam_dev_test dump <dump> <out> <options>                         mode 2, the yardstick of tests/test_gpu_sam.py: writes
//                                                                    FileWriter's text of a dump to <out> and the
//                                                                    per-read offsets (u64) to <out>.off; a formatter
//                                                                    exception is printed as "ERROR: <text>" (exit code 3)
// options: the MA_SAM_* bits of include/ma_amd.h.  Every count of the counting sink is checked against the bytes written; the
// writing sink gets a buffer of exactly that size and the reads hold exactly their bases, so that an AddressSanitizer build of
// this program sees any byte touched outside of them.
#include "sam_dev_common.h"

// the yardstick: FileWriter::execute over all reads (throws what it throws).  The five-argument formatRead does not know the
// tag bit, so the yardstick runs without it.
static std::string yardstick( const Input& rIn, uint32_t uiOptions, std::vector<uint64_t>* pOff = nullptr )
{
    return fileWriterText( rIn, uiOptions & ~(uint32_t)MA_SAM_NGMLR_TAGS, pOff );
}
// the host's flat writer: flat::formatRead, the adapter of ma_flat_sam.h, over all reads (throws what it throws)
static std::string adapter( const Input& rIn, uint32_t uiOptions )
{
    ma_amd::flat::Arena xOut;
    const ma_amd::flat::ContigTable xContigs = rIn.flatContigs( );
    for( size_t r = 0; r < rIn.vReads.size( ); r++ )
        ma_amd::flat::formatRead( xOut, formatOf( uiOptions ), xContigs, rIn.vReads[ r ].flatView( ), rIn.vAlns.data( ) + rIn.vOff[ r ],
                                  (size_t)( rIn.vOff[ r + 1 ] - rIn.vOff[ r ] ), rIn.vOps.data( ) );
    return std::string( xOut.data( ), xOut.size( ) );
}
// the shared formatter: counting sink, then the writing sink into exactly that many bytes
static DevResult shared( const Input& rIn, uint32_t uiOptions )
{
    const DevContigs xC( rIn );
    return countThenWrite( rIn.vReads.size( ), [ & ]( auto& rSink, size_t r ) {
        ma_sam::formatRead( rSink, uiOptions, xC.xView, rIn.vReads[ r ].view( ), rIn.list( r ) );
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
    compare( adapter( in, uiOptions ), sYard, "flat::formatRead against FileWriter" );
    printf( "golden ok: %zu reads, %zu records, %zu bytes\n", in.vReads.size( ), in.vAlns.size( ), sYard.size( ) );
    return 0;
}

// ---- random pass ---------------------------------------------------------------------------------------------------------
static Input randomInput( Rng& g, size_t uiLists )
{
    static const uint64_t aLens[] = { 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257 };
    Input in;
    const size_t nC = 1 + below( g, 3 );
    for( size_t i = 0; i < nC; i++ )
    {
        // two contigs share a name
        const std::string sName = i == 2 ? in.vNames[ 0 ] : std::string( 1 + below( g, 12 ), (char)( 'a' + below( g, 26 ) ) );
        in.addContig( sName, 300 + nearBoundary( g, 2000000000ull ) );
    }
    const uint64_t F = in.forward( );
    in.vOff.assign( 1, 0 );
    for( size_t r = 0; r < uiLists; r++ )
    {
        ReadData q;
        const uint64_t len = aLens[ below( g, sizeof( aLens ) / sizeof( aLens[ 0 ] ) ) ];
        for( uint64_t i = 0, n = 1 + below( g, 40 ); i < n; i++ )
            q.sName.push_back( (char)( '!' + below( g, 94 ) ) );
        q.bQual = below( g, 2 ) != 0;
        for( uint64_t i = 0; i < len; i++ )
        {
            q.vCodes.push_back( (uint8_t)( below( g, 8 ) == 0 ? 4 + below( g, 3 ) : below( g, 4 ) ) ); // codes above 3 among them
            if( q.bQual )
                q.vQual.push_back( (uint8_t)( '!' + below( g, 94 ) ) );
        }
        const unsigned kind = (unsigned)below( g, 10 ); // 0: empty list, 1: alignments of length 0 only, else: 1 - 4 records
        const size_t nA = kind == 0 ? 0 : 1 + below( g, 4 );
        for( size_t k = 0; k < nA; k++ )
        {
            ma_alignment a{ };
            const bool bRev = below( g, 2 ) != 0;
            const size_t c = below( g, nC );
            const uint64_t cs = in.vStarts[ c ], cl = in.vLengths[ c ];
            const uint64_t span = 1 + below( g, 300 );
            const uint64_t fs = cs + nearBoundary( g, cl - span ), fe = fs + span; // forward interval [fs, fe) inside the contig
            a.begin_ref = (int64_t)( bRev ? 2 * F - fe : fs );
            a.end_ref = (int64_t)( bRev ? 2 * F - fs : fe );
            a.begin_q = (int64_t)below( g, len + 1 );
            a.end_q = a.begin_q + (int64_t)below( g, len + 1 - (uint64_t)a.begin_q );
            a.score = (int64_t)below( g, 1000 );
            a.secondary = below( g, 4 ) == 0, a.supplementary = below( g, 4 ) == 0;
            const unsigned m = (unsigned)below( g, 8 );
            a.mapq = m == 0 ? std::numeric_limits<double>::quiet_NaN( ) : m == 1 ? 0.0 : m == 2 ? 1.0 : (double)below( g, 1000001 ) / 1000000.0;
            a.ops_off = in.vOps.size( ) / 2;
            a.n_ops = (uint32_t)( kind == 1 ? below( g, 3 ) : 1 + below( g, 12 ) );
            for( uint32_t j = 0; j < a.n_ops; j++ )
            {
                in.vOps.push_back( below( g, 5 ) );
                in.vOps.push_back( kind == 1 ? 0 : below( g, 3 ) == 0 ? nearBoundary( g, 2000000000ull ) : below( g, 150 ) );
            }
            in.vAlns.push_back( a );
        }
        in.vReads.push_back( q );
        in.vOff.push_back( in.vAlns.size( ) );
    }
    in.vOps.push_back( 0 ), in.vOps.push_back( 0 );
    return in;
}

static int randomPass( int argc, char** argv )
{
    if( argc < 4 )
        return 2;
    Rng g( strtoull( argv[ 2 ], nullptr, 10 ) );
    const size_t uiLists = (size_t)atoi( argv[ 3 ] );
    size_t uiBytes = 0, uiRounds = 0;
    for( size_t done = 0; done < uiLists; done += 200, uiRounds++ )
    {
        const Input in = randomInput( g, 200 ); // (a new contig table every 200 lists)
        for( uint32_t uiOptions = 0; uiOptions <= ma_sam::ALL_OPTIONS; uiOptions++ )
        {
            const std::string sYard = yardstick( in, uiOptions );
            const DevResult xDev = shared( in, uiOptions );
            if( xDev.uiErrors )
                throw std::runtime_error( "errors on records that lie inside their reads" );
            compare( xDev.sText, sYard, "options " + std::to_string( uiOptions ) );
            compare( adapter( in, uiOptions ), sYard, "flat::formatRead, options " + std::to_string( uiOptions ) );
            uiBytes += sYard.size( );
        }
    }
    printf( "random ok: %zu lists x 32 option sets, %zu bytes\n", uiRounds * 200, uiBytes );
    return 0;
}

// ---- special pass --------------------------------------------------------------------------------------------------------
static Input longCigar( uint32_t uiOps, bool bRev )
{
    Input in;
    in.addContig( "chrL", 200000 );
    ReadData q;
    q.sName = "long";
    q.bQual = true;
    for( uint32_t i = 0; i < 70000; i++ )
        q.vCodes.push_back( (uint8_t)( ( i * 7 + i / 3 ) % 5 ) ), q.vQual.push_back( (uint8_t)( '!' + i % 90 ) );
    ma_alignment a{ };
    uint64_t qlen = 0, rlen = 0;
    for( uint32_t j = 0; j < uiOps; j++ ) // single-base ops, no two neighbours of one type
    {
        const uint64_t t = j % 4 == 3 ? ( j % 8 == 3 ? 3 : 4 ) : j % 4;
        in.vOps.push_back( t ), in.vOps.push_back( 1 );
        qlen += t != 4, rlen += t != 3;
    }
    a.begin_q = 100, a.end_q = (int64_t)( 100 + qlen );
    a.begin_ref = (int64_t)( bRev ? 2 * 200000 - ( 5000 + rlen ) : 5000 ), a.end_ref = a.begin_ref + (int64_t)rlen;
    a.n_ops = uiOps, a.mapq = 0.5;
    in.vAlns = { a };
    in.vOff = { 0, 1 };
    in.vReads = { q };
    return in;
}
static int special( )
{
    for( uint32_t uiOps : { 65535u, 65536u } )
        for( int iRev = 0; iRev < 2; iRev++ )
            for( uint32_t uiOptions : { 0u, (uint32_t)MA_SAM_NO_CG_TAG, (uint32_t)MA_SAM_EQX_CIGAR, (uint32_t)( MA_SAM_NO_CG_TAG | MA_SAM_EQX_CIGAR | MA_SAM_SOFT_CLIP ) } )
            {
                const Input in = longCigar( uiOps, iRev != 0 );
                const std::string sYard = yardstick( in, uiOptions );
                compare( shared( in, uiOptions ).sText, sYard, "long cigar" );
                compare( adapter( in, uiOptions ), sYard, "long cigar through flat::formatRead" );
                const bool bTag = sYard.find( "\tCG:B:I," ) != std::string::npos;
                if( bTag != ( uiOps >= 0x10000 && !( uiOptions & MA_SAM_NO_CG_TAG ) ) )
                    throw std::runtime_error( "CG tag present / absent against expectation" );
            }
    // a record that ends beyond its read: the yardstick throws, the shared formatter reports the same text, touches nothing
    // beyond the read and writes what it counted; the flat writer throws the same text
    for( int iRev = 0; iRev < 2; iRev++ )
        for( uint32_t uiOptions : { 0u, (uint32_t)MA_SAM_EQX_CIGAR } )
        {
            Input in = longCigar( 10, iRev != 0 );
            in.vReads[ 0 ].vCodes.resize( 150 ), in.vReads[ 0 ].vQual.resize( 150 );
            in.vAlns[ 0 ].begin_q = 120, in.vAlns[ 0 ].end_q = 153;
            const std::string sWant = errorOf( [ & ] { yardstick( in, uiOptions ); } );
            const std::string sAdapter = errorOf( [ & ] { adapter( in, uiOptions ); } );
            const DevResult xDev = shared( in, uiOptions );
            char aText[ 64 ];
            ma_sam::errorText( aText, xDev.uiKind, xDev.iValue );
            if( xDev.uiErrors != 1 || sWant.empty( ) || sWant != aText )
                throw std::runtime_error( "error text: want '" + sWant + "', got '" + ( xDev.uiErrors ? aText : "(none)" ) + "'" );
            if( sWant != ( iRev ? "Index out of range (compCharAt)" : "Query length is off by -3." ) )
                throw std::runtime_error( "unexpected text of the yardstick: " + sWant );
            if( sAdapter != sWant )
                throw std::runtime_error( "error text of flat::formatRead: want '" + sWant + "', got '" + sAdapter + "'" );
        }
    // soft clipping prints the whole read: no error even then (the yardstick does not throw either)
    {
        Input in = longCigar( 10, true );
        in.vReads[ 0 ].vCodes.resize( 150 ), in.vReads[ 0 ].vQual.resize( 150 );
        in.vAlns[ 0 ].begin_q = 120, in.vAlns[ 0 ].end_q = 153;
        const DevResult xDev = shared( in, MA_SAM_SOFT_CLIP );
        if( xDev.uiErrors )
            throw std::runtime_error( "error reported under soft clipping" );
        compare( xDev.sText, yardstick( in, MA_SAM_SOFT_CLIP ), "soft clipping beyond the read" );
        compare( adapter( in, MA_SAM_SOFT_CLIP ), xDev.sText, "soft clipping beyond the read through flat::formatRead" );
    }
    // a pack without contigs can only yield unmapped records: the flat writer prints them without looking at its table
    {
        Input in = longCigar( 10, false );
        in.vNames.clear( ), in.vStarts.clear( ), in.vLengths.clear( ), in.vAlns.clear( );
        in.vOff = { 0, 0 };
        compare( adapter( in, 0 ), yardstick( in, 0 ), "unmapped read, no contigs" );
    }
    printf( "special ok\n" );
    return 0;
}

// ---- mode 2: the yardstick's text of a dump --------------------------------------------------------------------------------
static int dump( int argc, char** argv )
{
    if( argc < 5 )
        return 2;
    Input in;
    {
        DumpFile f( argv[ 2 ] );
        readDump( f, in, "MASAMD01", false, 1 );
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
        if( sMode == "special" )
            return special( );
        if( sMode == "dump" )
            return dump( argc, argv );
    }
    catch( const std::exception& e )
    {
        fprintf( stderr, "sam_dev_test %s: %s\n", sMode.c_str( ), e.what( ) );
        return 1;
    }
    return 2;
}
