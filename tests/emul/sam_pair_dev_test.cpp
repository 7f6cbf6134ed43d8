// CPU-only checks of the paired-end record formatter the device stage runs (ma_amd/host/ma_sam_dev.h: ma_sam::formatPair over
// its counting and its writing sink) and of the host's flat writer on top of it (flat::formatPair of ma_amd/host/ma_flat_sam.h)
// against the yardstick, PairedFileWriter::execute of ma_amd/host/ma_sam.h on fresh Alignment containers, and the paired SAM
// golden.
//   sam_pair_dev_test golden <case> <f4 dump> <golden.sam> <options>   the "P" / "p" records of an f4 dump of the compiled
//                                                                       reference: the formatter under both sinks, the flat
//                                                                       writer, the yardstick and the record lines of the
//                                                                       golden must agree byte for byte
//   sam_pair_dev_test random <seed> <pairs>                            seeded random pairs under every option combination
//   sam_pair_dev_test special                                          cigars of 65 535 / 65 536 ops inside a pair (CG tag),
//                                                                       the two error texts for either mate
//   sam_pair_dev_test dump <dump> <out> <options>                      the yardstick of tests/test_gpu_pair_sam.py: writes
//                                                                       PairedFileWriter's text of a dump (the arrays of
//                                                                       ma_batch_get_pairs) to <out> and the per-pair offsets
//                                                                       (u64) to <out>.off; a formatter exception is printed
//                                                                       as "ERROR: <text>" (exit code 3)
// options: the MA_SAM_* bits of include/ma_amd.h.  Every count of the counting sink is checked against the bytes written; the
// writing sink gets a buffer of exactly that size and the reads hold exactly their bases, so that an AddressSanitizer build of
// this program sees any byte touched outside of them.
#include "sam_dev_common.h"

struct PairInput : Input // vReads: 2 per pair, vOff: pairs + 1
{
    std::vector<int32_t> vMate, vOther;
    size_t pairs( ) const
    {
        return vOff.size( ) - 1;
    }
};

// the yardstick: PairedFileWriter::execute over all pairs, the containers' xStats set from mate and other (throws what it
// throws).  formatPair does not know the tag bit, which the paired writer refuses: the yardstick runs without it.
static std::string yardstick( const PairInput& rIn, uint32_t uiOptions, std::vector<uint64_t>* pOff = nullptr )
{
    return writerText<PairedFileWriter>( rIn, uiOptions & ma_sam::PAIR_OPTIONS, rIn.pairs( ), pOff,
                                         [ & ]( PairedFileWriter& rWriter, std::shared_ptr<Pack> pPack, size_t p ) {
                                             auto pV = rIn.containers( p );
                                             for( size_t k = 0; k < pV->size( ); k++ )
                                             {
                                                 const uint64_t o = rIn.vOff[ p ] + k;
                                                 ( *pV )[ k ]->xStats.bFirst = rIn.vMate[ o ] != 0;
                                                 if( rIn.vOther[ o ] >= 0 )
                                                     ( *pV )[ k ]->xStats.pOther = ( *pV )[ (size_t)rIn.vOther[ o ] ];
                                             }
                                             rWriter.execute( rIn.vReads[ 2 * p ].container( ), rIn.vReads[ 2 * p + 1 ].container( ), pV, pPack );
                                         } );
}
// the host's flat writer: flat::formatPair, the adapter of ma_flat_sam.h, over all pairs (throws what it throws)
static std::string adapter( const PairInput& rIn, uint32_t uiOptions )
{
    ma_amd::flat::Arena xOut;
    const ma_amd::flat::ContigTable xContigs = rIn.flatContigs( );
    for( size_t p = 0; p < rIn.pairs( ); p++ )
    {
        const uint64_t o = rIn.vOff[ p ];
        ma_amd::flat::formatPair( xOut, formatOf( uiOptions ), xContigs, rIn.vReads[ 2 * p ].flatView( ), rIn.vReads[ 2 * p + 1 ].flatView( ),
                                  rIn.vAlns.data( ) + o, (size_t)( rIn.vOff[ p + 1 ] - o ), rIn.vOps.data( ), rIn.vMate.data( ) + o, rIn.vOther.data( ) + o );
    }
    return std::string( xOut.data( ), xOut.size( ) );
}
// the shared formatter: counting sink, then the writing sink into exactly that many bytes
static DevResult shared( const PairInput& rIn, uint32_t uiOptions )
{
    const DevContigs xC( rIn );
    return countThenWrite( rIn.pairs( ), [ & ]( auto& rSink, size_t p ) {
        const ma_sam::FlatPairList xL{ rIn.list( p ), rIn.vMate.data( ) + rIn.vOff[ p ], rIn.vOther.data( ) + rIn.vOff[ p ] };
        ma_sam::formatPair( rSink, uiOptions, xC.xView, rIn.vReads[ 2 * p ].view( ), rIn.vReads[ 2 * p + 1 ].view( ), xL );
    } );
}

// ---- golden pass ---------------------------------------------------------------------------------------------------------
static PairInput fromF4Dump( const char* sCase, const char* sDump )
{
    PairInput in;
    static_cast<Input&>( in ) = fromCase( sCase );
    if( in.vReads.size( ) % 2 )
        in.vReads.pop_back( );
    std::ifstream f( sDump );
    std::string line;
    long unit = -1;
    while( std::getline( f, line ) )
    {
        std::istringstream ss( line );
        std::string tag;
        ss >> tag;
        if( tag == "P" )
        {
            long u;
            ss >> u;
            if( u != unit + 1 )
                throw std::runtime_error( "the dump's pairs are not in order" );
            unit = u;
            in.vOff.push_back( in.vAlns.size( ) );
        }
        else if( tag == "p" )
        {
            ma_alignment a;
            memset( &a, 0, sizeof( a ) );
            int first, other;
            size_t nops;
            std::string sMq;
            ss >> first >> other >> a.begin_ref >> a.end_ref >> a.begin_q >> a.end_q >> a.score >> a.soc_index >> a.secondary >> a.supplementary >>
                sMq >> nops;
            a.mapq = sMq == "nan" ? NAN : strtod( sMq.c_str( ), nullptr );
            a.n_ops = (uint32_t)nops;
            a.ops_off = in.vOps.size( ) / 2;
            readOps( ss, nops, in.vOps );
            in.vAlns.push_back( a );
            in.vMate.push_back( first );
            in.vOther.push_back( other );
        }
    }
    in.vOff.push_back( in.vAlns.size( ) );
    if( in.pairs( ) * 2 != in.vReads.size( ) )
        throw std::runtime_error( "the dump has " + std::to_string( in.pairs( ) ) + " pairs, the case " + std::to_string( in.vReads.size( ) ) + " reads" );
    in.vOps.push_back( 0 ), in.vOps.push_back( 0 );
    in.vMate.push_back( 0 ), in.vOther.push_back( 0 );
    return in;
}

static int golden( int argc, char** argv )
{
    if( argc < 6 )
        return 2;
    const PairInput in = fromF4Dump( argv[ 2 ], argv[ 3 ] );
    const uint32_t uiOptions = (uint32_t)atoi( argv[ 5 ] );
    const std::string sGolden = goldenRecords( argv[ 4 ] );
    const std::string sYard = yardstick( in, uiOptions );
    const DevResult xDev = shared( in, uiOptions );
    if( xDev.uiErrors )
        throw std::runtime_error( "the shared formatter reports errors on the golden records" );
    compare( xDev.sText, sYard, "shared formatter against PairedFileWriter" );
    compare( xDev.sText, sGolden, "shared formatter against the golden" );
    compare( adapter( in, uiOptions ), sYard, "flat::formatPair against PairedFileWriter" );
    printf( "golden ok: %zu pairs, %zu records, %zu bytes\n", in.pairs( ), in.vAlns.size( ), sYard.size( ) );
    return 0;
}

// ---- random pass ---------------------------------------------------------------------------------------------------------
struct Census
{
    size_t picked[ 4 ] = { 0, 0, 0, 0 }, lists = 0, emptied = 0, firstFiltered = 0, zeroLength = 0, otherContig = 0, sameName = 0, capped = 0,
           nan = 0, noRecords = 0, unequalMates = 0;
};

// one record of a mate of uiLen bases (the record lies inside the mate); iStrand 0 / 1 forward / reverse, else either
static ma_alignment randomRecord( Rng& g, PairInput& in, uint64_t uiLen, int iStrand, size_t uiContig, bool bZero, Census& rC )
{
    const uint64_t F = in.forward( );
    ma_alignment a{ };
    const bool bRev = iStrand < 0 ? below( g, 2 ) != 0 : iStrand != 0;
    const uint64_t cs = in.vStarts[ uiContig ], cl = in.vLengths[ uiContig ];
    const uint64_t span = 1 + below( g, 300 );
    const uint64_t fs = cs + nearBoundary( g, cl - span ), fe = fs + span; // forward interval [fs, fe) inside the contig
    a.begin_ref = (int64_t)( bRev ? 2 * F - fe : fs );
    a.end_ref = (int64_t)( bRev ? 2 * F - fs : fe );
    a.begin_q = (int64_t)below( g, uiLen + 1 );
    a.end_q = a.begin_q + (int64_t)below( g, uiLen + 1 - (uint64_t)a.begin_q );
    a.score = (int64_t)below( g, 1000 );
    const unsigned m = (unsigned)below( g, 8 );
    // (2.0 and 1.01 exceed 255 after scaling: the paired writer's cap)
    a.mapq = m == 0 ? std::numeric_limits<double>::quiet_NaN( ) : m == 1 ? 0.0 : m == 2 ? 1.0 : m == 3 ? 2.0 : m == 4 ? 1.01 : (double)below( g, 1000001 ) / 1000000.0;
    rC.nan += m == 0, rC.capped += m == 3 || m == 4;
    a.ops_off = in.vOps.size( ) / 2;
    a.n_ops = (uint32_t)( bZero ? below( g, 3 ) : 1 + below( g, 12 ) );
    for( uint32_t j = 0; j < a.n_ops; j++ )
    {
        in.vOps.push_back( below( g, 5 ) );
        in.vOps.push_back( bZero ? 0 : j == 0 ? 1 + below( g, 150 ) : below( g, 3 ) == 0 ? nearBoundary( g, 2000000000ull ) : below( g, 150 ) );
    }
    rC.zeroLength += bZero;
    return a;
}

static PairInput randomInput( Rng& g, size_t uiPairs, Census& rC )
{
    static const uint64_t aLens[] = { 0, 1, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257 }; // (0: an empty mate)
    const size_t nLens = sizeof( aLens ) / sizeof( aLens[ 0 ] );
    PairInput in;
    const size_t nC = 1 + below( g, 3 );
    for( size_t i = 0; i < nC; i++ )
    {
        // two contigs share a name
        const std::string sName = i == 2 ? in.vNames[ 0 ] : std::string( 1 + below( g, 12 ), (char)( 'a' + below( g, 26 ) ) );
        in.addContig( sName, 300 + nearBoundary( g, 2000000000ull ) );
    }
    const bool bQual = below( g, 2 ) != 0; // (a run has qualities or has none)
    in.vOff.assign( 1, 0 );
    for( size_t p = 0; p < uiPairs; p++ )
    {
        uint64_t aLen[ 2 ];
        aLen[ 0 ] = aLens[ below( g, nLens ) ];
        aLen[ 1 ] = below( g, 3 ) == 0 ? aLen[ 0 ] : aLens[ below( g, nLens ) ];
        rC.unequalMates += aLen[ 0 ] != aLen[ 1 ];
        for( int m = 0; m < 2; m++ )
        {
            ReadData q;
            for( uint64_t i = 0, n = 1 + below( g, 40 ); i < n; i++ )
                q.sName.push_back( (char)( '!' + below( g, 94 ) ) );
            q.bQual = bQual;
            for( uint64_t i = 0; i < aLen[ m ]; i++ )
            {
                q.vCodes.push_back( (uint8_t)( below( g, 8 ) == 0 ? 4 + below( g, 3 ) : below( g, 4 ) ) ); // codes above 3 among them
                if( q.bQual )
                    q.vQual.push_back( (uint8_t)( '!' + below( g, 94 ) ) );
            }
            in.vReads.push_back( q );
        }
        // 0: no records, 1-4: a picked pair on strand combination kind - 1, 5-9: one mate's list
        const unsigned kind = (unsigned)below( g, 10 );
        if( kind == 0 )
            rC.noRecords++;
        else if( kind <= 4 )
        {
            const size_t c1 = below( g, nC ), c2 = below( g, 3 ) == 0 ? below( g, nC ) : c1;
            rC.picked[ kind - 1 ]++;
            rC.otherContig += c1 != c2;
            rC.sameName += c1 != c2 && in.vNames[ c1 ] == in.vNames[ c2 ];
            const bool bZero = below( g, 12 ) == 0; // (a picked record of length 0 is skipped as any other)
            in.vAlns.push_back( randomRecord( g, in, aLen[ 0 ], ( kind - 1 ) & 1, c1, bZero, rC ) );
            in.vAlns.push_back( randomRecord( g, in, aLen[ 1 ], ( ( kind - 1 ) >> 1 ) & 1, c2, false, rC ) );
            in.vMate.push_back( 1 ), in.vMate.push_back( 0 );
            in.vOther.push_back( 1 ), in.vOther.push_back( 0 );
        }
        else
        {
            const int iFirst = (int)below( g, 2 );
            const size_t nA = 1 + below( g, 5 );
            // 5: every record secondary or supplementary (options 4 | 8 empty the list), 6: record 0 filtered, a later one
            // printed, 7: record 0 of length 0, else: any
            rC.lists++;
            rC.emptied += kind == 5, rC.firstFiltered += kind == 6 && nA > 1;
            for( size_t k = 0; k < nA; k++ )
            {
                ma_alignment a = randomRecord( g, in, aLen[ iFirst ? 0 : 1 ], -1, below( g, nC ), kind == 7 && k == 0, rC );
                a.secondary = below( g, 4 ) == 0, a.supplementary = below( g, 4 ) == 0;
                if( kind == 5 )
                    ( below( g, 2 ) ? a.secondary : a.supplementary ) = 1;
                if( kind == 6 )
                {
                    if( k == 0 )
                        a.secondary = 1, a.supplementary = below( g, 2 ) != 0;
                    else if( k == 1 )
                        a.secondary = a.supplementary = 0;
                }
                in.vAlns.push_back( a );
                in.vMate.push_back( iFirst );
                in.vOther.push_back( -1 );
            }
        }
        in.vOff.push_back( in.vAlns.size( ) );
    }
    in.vOps.push_back( 0 ), in.vOps.push_back( 0 );
    in.vMate.push_back( 0 ), in.vOther.push_back( 0 );
    return in;
}

static int randomPass( int argc, char** argv )
{
    if( argc < 4 )
        return 2;
    Rng g( strtoull( argv[ 2 ], nullptr, 10 ) );
    const size_t uiPairs = (size_t)atoi( argv[ 3 ] );
    size_t uiBytes = 0, uiRounds = 0, uiWithQual = 0;
    Census xC;
    for( size_t done = 0; done < uiPairs; done += 200, uiRounds++ )
    {
        const PairInput in = randomInput( g, 200, xC ); // (a new contig table every 200 pairs)
        uiWithQual += in.vReads[ 0 ].bQual;
        for( uint32_t uiOptions = 0; uiOptions <= ma_sam::ALL_OPTIONS; uiOptions++ )
        {
            const std::string sYard = yardstick( in, uiOptions );
            const DevResult xDev = shared( in, uiOptions );
            if( xDev.uiErrors )
                throw std::runtime_error( "errors on records that lie inside their reads" );
            compare( xDev.sText, sYard, "options " + std::to_string( uiOptions ) );
            compare( adapter( in, uiOptions ), sYard, "flat::formatPair, options " + std::to_string( uiOptions ) );
            uiBytes += sYard.size( );
        }
    }
    printf( "random ok: %zu pairs x 32 option sets, %zu bytes\n", uiRounds * 200, uiBytes );
    printf( "picked by strands %zu %zu %zu %zu, lists %zu (emptied by 12: %zu, record 0 filtered: %zu), zero-length records %zu, partner on "
            "another contig %zu (of the same name %zu), mapq capped %zu, NaN %zu, no records %zu, mates of different lengths %zu, rounds "
            "with qualities %zu of %zu\n",
            xC.picked[ 0 ], xC.picked[ 1 ], xC.picked[ 2 ], xC.picked[ 3 ], xC.lists, xC.emptied, xC.firstFiltered, xC.zeroLength, xC.otherContig,
            xC.sameName, xC.capped, xC.nan, xC.noRecords, xC.unequalMates, uiWithQual, uiRounds );
    if( uiRounds >= 10 )
    {
        const size_t aWant[] = { xC.picked[ 0 ], xC.picked[ 1 ], xC.picked[ 2 ], xC.picked[ 3 ], xC.emptied, xC.firstFiltered, xC.zeroLength,
                                 xC.otherContig, xC.sameName, xC.capped, xC.nan, xC.noRecords, xC.unequalMates, uiWithQual, uiRounds - uiWithQual };
        for( size_t w : aWant )
            if( w == 0 )
                throw std::runtime_error( "a shape the pass is to cover never came up" );
    }
    return 0;
}

// ---- special pass --------------------------------------------------------------------------------------------------------
// a picked pair: the first mate a 70 kb read with uiOps single-base ops, the second a plain 150 bp record
static PairInput longCigarPair( uint32_t uiOps, bool bRev, bool bLongIsFirst )
{
    PairInput in;
    in.addContig( "chrL", 200000 ), in.addContig( "chrM", 1000 );
    const uint64_t F = 201000;
    ReadData q, s;
    q.sName = "long", s.sName = "short";
    q.bQual = s.bQual = true;
    for( uint32_t i = 0; i < 70000; i++ )
        q.vCodes.push_back( (uint8_t)( ( i * 7 + i / 3 ) % 5 ) ), q.vQual.push_back( (uint8_t)( '!' + i % 90 ) );
    for( uint32_t i = 0; i < 150; i++ )
        s.vCodes.push_back( (uint8_t)( ( i * 5 + i / 7 ) % 4 ) ), s.vQual.push_back( (uint8_t)( '#' + i % 60 ) );
    ma_alignment a{ }, b{ };
    uint64_t qlen = 0, rlen = 0;
    for( uint32_t j = 0; j < uiOps; j++ ) // single-base ops, no two neighbours of one type
    {
        const uint64_t t = j % 4 == 3 ? ( j % 8 == 3 ? 3 : 4 ) : j % 4;
        in.vOps.push_back( t ), in.vOps.push_back( 1 );
        qlen += t != 4, rlen += t != 3;
    }
    a.begin_q = 100, a.end_q = (int64_t)( 100 + qlen );
    a.begin_ref = (int64_t)( bRev ? 2 * F - ( 5000 + rlen ) : 5000 ), a.end_ref = a.begin_ref + (int64_t)rlen;
    a.n_ops = uiOps, a.mapq = 0.5;
    b.begin_q = 0, b.end_q = 150, b.n_ops = 1, b.ops_off = uiOps, b.mapq = 0.5;
    b.begin_ref = (int64_t)( bRev ? 200100 : 2 * F - 200400 ), b.end_ref = b.begin_ref + 150;
    in.vOps.push_back( 0 ), in.vOps.push_back( 150 );
    in.vOps.push_back( 0 ), in.vOps.push_back( 0 );
    if( bLongIsFirst )
        in.vAlns = { a, b }, in.vReads = { q, s };
    else
        in.vAlns = { b, a }, in.vReads = { s, q };
    in.vMate = { 1, 0, 0 }, in.vOther = { 1, 0, 0 };
    in.vOff = { 0, 2 };
    return in;
}
static int special( )
{
    for( uint32_t uiOps : { 65535u, 65536u } )
        for( int iRev = 0; iRev < 2; iRev++ )
            for( int iFirst = 0; iFirst < 2; iFirst++ )
                for( uint32_t uiOptions : { 0u, (uint32_t)MA_SAM_NO_CG_TAG, (uint32_t)MA_SAM_EQX_CIGAR, (uint32_t)( MA_SAM_NO_CG_TAG | MA_SAM_EQX_CIGAR | MA_SAM_SOFT_CLIP ) } )
                {
                    const PairInput in = longCigarPair( uiOps, iRev != 0, iFirst != 0 );
                    const std::string sYard = yardstick( in, uiOptions );
                    compare( shared( in, uiOptions ).sText, sYard, "long cigar" );
                    compare( adapter( in, uiOptions ), sYard, "long cigar through flat::formatPair" );
                    const bool bTag = sYard.find( "\tCG:B:I," ) != std::string::npos;
                    if( bTag != ( uiOps >= 0x10000 && !( uiOptions & MA_SAM_NO_CG_TAG ) ) )
                        throw std::runtime_error( "CG tag present / absent against expectation" );
                }
    // a record that ends beyond its OWN mate -- the other mate is longer, so that only the own length tells -- in the first
    // and in the second mate: the yardstick throws, the shared formatter reports the same text for that record, touches
    // nothing beyond the read and writes what it counted; the flat writer throws the same text
    for( int iBadMate = 0; iBadMate < 2; iBadMate++ )
        for( int iRev = 0; iRev < 2; iRev++ )
            for( uint32_t uiOptions : { 0u, (uint32_t)MA_SAM_EQX_CIGAR } )
            {
                PairInput in = longCigarPair( 10, iRev != 0, iBadMate == 0 ); // the 70 kb mate is the bad one, cut to 150 bases
                in.vReads[ iBadMate ].vCodes.resize( 150 ), in.vReads[ iBadMate ].vQual.resize( 150 );
                in.vReads[ 1 - iBadMate ].vCodes.resize( 400, 2 ), in.vReads[ 1 - iBadMate ].vQual.resize( 400, (uint8_t)'I' );
                in.vAlns[ iBadMate ].begin_q = 120, in.vAlns[ iBadMate ].end_q = 153;
                const std::string sWant = errorOf( [ & ] { yardstick( in, uiOptions ); } );
                const std::string sAdapter = errorOf( [ & ] { adapter( in, uiOptions ); } );
                const DevResult xDev = shared( in, uiOptions );
                char aText[ 64 ];
                ma_sam::errorText( aText, xDev.uiKind, xDev.iValue );
                if( xDev.uiErrors != 1 || sWant.empty( ) || sWant != aText || xDev.uiRecord != (uint32_t)iBadMate )
                    throw std::runtime_error( "error text: want '" + sWant + "', got '" + ( xDev.uiErrors ? aText : "(none)" ) + "' for record " +
                                              std::to_string( xDev.uiRecord ) );
                if( sWant != ( iRev ? "Index out of range (compCharAt)" : "Query length is off by -3." ) )
                    throw std::runtime_error( "unexpected text of the yardstick: " + sWant );
                if( sAdapter != sWant )
                    throw std::runtime_error( "error text of flat::formatPair: want '" + sWant + "', got '" + sAdapter + "'" );
                // soft clipping prints the whole read: no error even then (the yardstick does not throw either)
                const DevResult xSoft = shared( in, uiOptions | MA_SAM_SOFT_CLIP );
                if( xSoft.uiErrors )
                    throw std::runtime_error( "error reported under soft clipping" );
                compare( xSoft.sText, yardstick( in, uiOptions | MA_SAM_SOFT_CLIP ), "soft clipping beyond the read" );
                compare( adapter( in, uiOptions | MA_SAM_SOFT_CLIP ), xSoft.sText, "soft clipping beyond the read through flat::formatPair" );
            }
    // a pack without contigs can only yield unmapped records: the flat writer prints them without looking at its table
    {
        PairInput in = longCigarPair( 10, false, true );
        in.vNames.clear( ), in.vStarts.clear( ), in.vLengths.clear( ), in.vAlns.clear( );
        in.vOff = { 0, 0 };
        compare( adapter( in, 0 ), yardstick( in, 0 ), "pair without records, no contigs" );
    }
    printf( "special ok\n" );
    return 0;
}

// ---- the yardstick's text of a dump ----------------------------------------------------------------------------------------
static int dump( int argc, char** argv )
{
    if( argc < 5 )
        return 2;
    PairInput in;
    {
        DumpFile f( argv[ 2 ] );
        readDump( f, in, "MASAMP01", false, 2 );
        const size_t nA = in.vAlns.size( );
        in.vMate.resize( nA + 1 ), in.vOther.resize( nA + 1 );
        f.rd( in.vMate.data( ), nA * 4 );
        f.rd( in.vOther.data( ), nA * 4 );
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
        fprintf( stderr, "sam_pair_dev_test %s: %s\n", sMode.c_str( ), e.what( ) );
        return 1;
    }
    return 2;
}
