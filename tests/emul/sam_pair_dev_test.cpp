// CPU-only checks of the paired-end record formatter the device stage runs (ma_amd/host/ma_sam_dev.h: ma_sam::formatPair over
// its counting and its writing sink) against the yardstick, flat::formatPair of ma_amd/host/ma_flat_sam.h, and the paired SAM
// golden.
//   sam_pair_dev_test golden <case> <f4 dump> <golden.sam> <options>   the "P" / "p" records of an f4 dump of the compiled
//                                                                       reference: both formatters and the record lines of
//                                                                       the golden must agree byte for byte
//   sam_pair_dev_test random <seed> <pairs>                            seeded random pairs under every option combination
//   sam_pair_dev_test special                                          cigars of 65 535 / 65 536 ops inside a pair (CG tag),
//                                                                       the two error texts for either mate
//   sam_pair_dev_test dump <dump> <out> <options>                      the yardstick of tests/test_gpu_pair_sam.py: writes
//                                                                       flat::formatPair's text of a dump (the arrays of
//                                                                       ma_batch_get_pairs) to <out> and the per-pair offsets
//                                                                       (u64) to <out>.off; a formatter exception is printed
//                                                                       as "ERROR: <text>" (exit code 3)
// options: the MA_SAM_* bits of include/ma_amd.h.  Every count of the counting sink is checked against the bytes written; the
// writing sink gets a buffer of exactly that size and the reads hold exactly their bases, so that an AddressSanitizer build of
// this program sees any byte touched outside of them.
#include "../../oracle/dump_format.h"
#include "ma_flat_sam.h"
#include "ma_sam_dev.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <random>
#include <sstream>

using namespace ma_amd;

struct ReadData
{
    std::string sName;
    std::vector<uint8_t> vCodes, vQual;
    bool bQual = false;
};
struct Input
{
    flat::Contigs xContigs;
    std::vector<ReadData> vReads; // 2 per pair
    std::vector<uint64_t> vOff; // pairs + 1
    std::vector<ma_alignment> vAlns;
    std::vector<uint64_t> vOps; // (type, length) pairs
    std::vector<int32_t> vMate, vOther;
    size_t pairs( ) const
    {
        return vOff.size( ) - 1;
    }
};

static flat::SamFormat formatOf( uint32_t uiOptions )
{
    flat::SamFormat f;
    f.bSoftClip = ( uiOptions & MA_SAM_SOFT_CLIP ) != 0;
    f.bOutputMCigar = ( uiOptions & MA_SAM_EQX_CIGAR ) == 0;
    f.bNoSecondary = ( uiOptions & MA_SAM_NO_SECONDARY ) != 0;
    f.bNoSupplementary = ( uiOptions & MA_SAM_NO_SUPPLEMENTARY ) != 0;
    f.bCGTag = ( uiOptions & MA_SAM_NO_CG_TAG ) == 0;
    return f;
}

// the contig table as ma_sam_dev.h reads it
struct DevContigs
{
    std::vector<char> vNames;
    std::vector<uint64_t> vNameOff;
    ma_sam::Contigs view( const flat::Contigs& r )
    {
        vNames.clear( );
        vNameOff.assign( 1, 0 );
        for( auto& s : r.vNames )
        {
            vNames.insert( vNames.end( ), s.begin( ), s.end( ) );
            vNameOff.push_back( vNames.size( ) );
        }
        return ma_sam::Contigs{ vNames.data( ), vNameOff.data( ), r.vStarts.data( ), r.vLengths.data( ), (uint32_t)r.vStarts.size( ) };
    }
};

// the yardstick: flat::formatPair over all pairs (throws what it throws).  An empty mate has no quality string, as in the host
// layer (NucSeq::xQuality empty -> no qualities): its QUAL is "*".
static std::string yardstick( const Input& rIn, uint32_t uiOptions, std::vector<uint64_t>* pOff = nullptr )
{
    flat::Arena xOut;
    const flat::SamFormat xF = formatOf( uiOptions );
    if( pOff )
        pOff->assign( 1, 0 );
    for( size_t p = 0; p < rIn.pairs( ); p++ )
    {
        flat::ReadView v[ 2 ];
        for( int m = 0; m < 2; m++ )
        {
            const ReadData& q = rIn.vReads[ 2 * p + m ];
            v[ m ].sName = q.sName.data( ), v[ m ].uiNameLen = q.sName.size( );
            v[ m ].pCodes = q.vCodes.data( ), v[ m ].pQuality = q.bQual && !q.vQual.empty( ) ? q.vQual.data( ) : nullptr, v[ m ].uiLength = q.vCodes.size( );
        }
        const uint64_t o = rIn.vOff[ p ];
        flat::formatPair( xOut, xF, rIn.xContigs, v[ 0 ], v[ 1 ], rIn.vAlns.data( ) + o, (size_t)( rIn.vOff[ p + 1 ] - o ), rIn.vOps.data( ),
                          rIn.vMate.data( ) + o, rIn.vOther.data( ) + o );
        if( pOff )
            pOff->push_back( xOut.size( ) );
    }
    return std::string( xOut.data( ), xOut.size( ) );
}

struct DevResult
{
    std::string sText;
    uint32_t uiErrors = 0, uiKind = 0, uiRecord = 0;
    size_t uiPair = 0;
    int64_t iValue = 0;
};
// the shared formatter: counting sink, then the writing sink into exactly that many bytes
static DevResult shared( const Input& rIn, uint32_t uiOptions )
{
    DevContigs xNames;
    const ma_sam::Contigs xC = xNames.view( rIn.xContigs );
    DevResult xRes;
    for( size_t p = 0; p < rIn.pairs( ); p++ )
    {
        const ReadData &q1 = rIn.vReads[ 2 * p ], &q2 = rIn.vReads[ 2 * p + 1 ];
        const ma_sam::Read xQ1{ q1.sName.data( ), q1.sName.size( ), q1.vCodes.data( ), q1.bQual && !q1.vQual.empty( ) ? q1.vQual.data( ) : nullptr, q1.vCodes.size( ) };
        const ma_sam::Read xQ2{ q2.sName.data( ), q2.sName.size( ), q2.vCodes.data( ), q2.bQual && !q2.vQual.empty( ) ? q2.vQual.data( ) : nullptr, q2.vCodes.size( ) };
        const uint64_t o = rIn.vOff[ p ];
        const ma_sam::FlatPairList xL{ { rIn.vAlns.data( ) + o, (uint32_t)( rIn.vOff[ p + 1 ] - o ), rIn.vOps.data( ) },
                                       rIn.vMate.data( ) + o,
                                       rIn.vOther.data( ) + o };
        ma_sam::CountSink xCount;
        ma_sam::formatPair( xCount, uiOptions, xC, xQ1, xQ2, xL );
        if( xCount.nErrors && !xRes.uiErrors )
            xRes.uiKind = xCount.firstKind, xRes.iValue = xCount.firstValue, xRes.uiRecord = xCount.firstRecord, xRes.uiPair = p;
        xRes.uiErrors += xCount.nErrors;
        std::unique_ptr<char[]> pBuf( new char[ xCount.n ] ); // (exactly: the sanitizer build sees a byte too many)
        ma_sam::WriteSink xWrite{ pBuf.get( ) };
        ma_sam::formatPair( xWrite, uiOptions, xC, xQ1, xQ2, xL );
        if( xWrite.n != xCount.n )
            throw std::runtime_error( "pair " + std::to_string( p ) + ": the counting sink says " + std::to_string( xCount.n ) + " bytes, " +
                                      std::to_string( xWrite.n ) + " were written" );
        xRes.sText.append( pBuf.get( ), xWrite.n );
    }
    return xRes;
}

static void compare( const std::string& sGot, const std::string& sWant, const std::string& sWhat )
{
    if( sGot == sWant )
        return;
    size_t i = 0;
    while( i < sGot.size( ) && i < sWant.size( ) && sGot[ i ] == sWant[ i ] )
        i++;
    const size_t b = sWant.rfind( '\n', i ) == std::string::npos ? 0 : sWant.rfind( '\n', i ) + 1;
    throw std::runtime_error( sWhat + ": texts differ at byte " + std::to_string( i ) + "\n want: " + sWant.substr( b, 300 ) + "\n got:  " +
                              sGot.substr( b < sGot.size( ) ? b : 0, 300 ) );
}

// ---- golden pass ---------------------------------------------------------------------------------------------------------
static Input fromF4Dump( const char* sCase, const char* sDump )
{
    CaseFile c = readCase( sCase );
    Input in;
    uint64_t off = 0;
    for( size_t i = 0; i < c.contigs.size( ); i++ )
    {
        in.xContigs.vNames.push_back( c.names[ i ] );
        in.xContigs.vStarts.push_back( off );
        in.xContigs.vLengths.push_back( c.contigs[ i ].size( ) );
        off += c.contigs[ i ].size( );
    }
    for( size_t r = 0; r < c.reads.size( ); r++ )
    {
        ReadData q;
        q.sName = "r" + std::to_string( r );
        q.vCodes = c.reads[ r ];
        in.vReads.push_back( q );
    }
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
            for( size_t k = 0; k < nops; k++ )
            {
                std::string op;
                ss >> op;
                const size_t colon = op.find( ':' );
                in.vOps.push_back( (uint64_t)atoi( op.substr( 0, colon ).c_str( ) ) );
                in.vOps.push_back( strtoull( op.c_str( ) + colon + 1, nullptr, 10 ) );
            }
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
    const Input in = fromF4Dump( argv[ 2 ], argv[ 3 ] );
    const uint32_t uiOptions = (uint32_t)atoi( argv[ 5 ] );
    std::ifstream f( argv[ 4 ] );
    std::string line, sGolden;
    while( std::getline( f, line ) )
        if( line.empty( ) || line[ 0 ] != '@' )
            sGolden += line + "\n";
    const std::string sYard = yardstick( in, uiOptions );
    const DevResult xDev = shared( in, uiOptions );
    if( xDev.uiErrors )
        throw std::runtime_error( "the shared formatter reports errors on the golden records" );
    compare( xDev.sText, sYard, "shared formatter against flat::formatPair" );
    compare( xDev.sText, sGolden, "shared formatter against the golden" );
    printf( "golden ok: %zu pairs, %zu records, %zu bytes\n", in.pairs( ), in.vAlns.size( ), sYard.size( ) );
    return 0;
}

// ---- random pass ---------------------------------------------------------------------------------------------------------
typedef std::mt19937_64 Rng;
static uint64_t below( Rng& g, uint64_t n ) // [0, n)
{
    return n ? g( ) % n : 0;
}
// a number next to a decimal boundary (9/10, 99/100, ... 10^9), or any
static uint64_t nearBoundary( Rng& g, uint64_t uiMax )
{
    if( below( g, 4 ) == 0 )
        return below( g, uiMax + 1 );
    uint64_t p = 10;
    for( uint64_t e = below( g, 9 ); e > 0; e-- )
        p *= 10;
    const uint64_t v = p - 2 + below( g, 4 ); // p-2 .. p+1
    return v > uiMax ? uiMax : v;
}

struct Census
{
    size_t picked[ 4 ] = { 0, 0, 0, 0 }, lists = 0, emptied = 0, firstFiltered = 0, zeroLength = 0, otherContig = 0, sameName = 0, capped = 0,
           nan = 0, noRecords = 0, unequalMates = 0;
};

// one record of a mate of uiLen bases (the record lies inside the mate); iStrand 0 / 1 forward / reverse, else either
static ma_alignment randomRecord( Rng& g, Input& in, uint64_t uiLen, int iStrand, size_t uiContig, bool bZero, Census& rC )
{
    const uint64_t F = in.xContigs.forwardSize( );
    ma_alignment a{ };
    const bool bRev = iStrand < 0 ? below( g, 2 ) != 0 : iStrand != 0;
    const uint64_t cs = in.xContigs.vStarts[ uiContig ], cl = in.xContigs.vLengths[ uiContig ];
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

static Input randomInput( Rng& g, size_t uiPairs, Census& rC )
{
    static const uint64_t aLens[] = { 0, 1, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257 }; // (0: an empty mate)
    const size_t nLens = sizeof( aLens ) / sizeof( aLens[ 0 ] );
    Input in;
    const size_t nC = 1 + below( g, 3 );
    uint64_t off = 0;
    for( size_t i = 0; i < nC; i++ )
    {
        // two contigs share a name
        in.xContigs.vNames.push_back( i == 2 ? in.xContigs.vNames[ 0 ] : std::string( 1 + below( g, 12 ), (char)( 'a' + below( g, 26 ) ) ) );
        in.xContigs.vStarts.push_back( off );
        in.xContigs.vLengths.push_back( 300 + nearBoundary( g, 2000000000ull ) );
        off += in.xContigs.vLengths.back( );
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
            rC.sameName += c1 != c2 && in.xContigs.vNames[ c1 ] == in.xContigs.vNames[ c2 ];
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
        const Input in = randomInput( g, 200, xC ); // (a new contig table every 200 pairs)
        uiWithQual += in.vReads[ 0 ].bQual;
        for( uint32_t uiOptions = 0; uiOptions <= ma_sam::ALL_OPTIONS; uiOptions++ )
        {
            const std::string sYard = yardstick( in, uiOptions );
            const DevResult xDev = shared( in, uiOptions );
            if( xDev.uiErrors )
                throw std::runtime_error( "errors on records that lie inside their reads" );
            compare( xDev.sText, sYard, "options " + std::to_string( uiOptions ) );
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
static Input longCigarPair( uint32_t uiOps, bool bRev, bool bLongIsFirst )
{
    Input in;
    in.xContigs.vNames = { "chrL", "chrM" };
    in.xContigs.vStarts = { 0, 200000 };
    in.xContigs.vLengths = { 200000, 1000 };
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
                    const Input in = longCigarPair( uiOps, iRev != 0, iFirst != 0 );
                    const std::string sYard = yardstick( in, uiOptions );
                    compare( shared( in, uiOptions ).sText, sYard, "long cigar" );
                    const bool bTag = sYard.find( "\tCG:B:I," ) != std::string::npos;
                    if( bTag != ( uiOps >= 0x10000 && !( uiOptions & MA_SAM_NO_CG_TAG ) ) )
                        throw std::runtime_error( "CG tag present / absent against expectation" );
                }
    // a record that ends beyond its OWN mate -- the other mate is longer, so that only the own length tells -- in the first
    // and in the second mate: the yardstick throws, the shared formatter reports the same text for that record, touches
    // nothing beyond the read and writes what it counted
    for( int iBadMate = 0; iBadMate < 2; iBadMate++ )
        for( int iRev = 0; iRev < 2; iRev++ )
            for( uint32_t uiOptions : { 0u, (uint32_t)MA_SAM_EQX_CIGAR } )
            {
                Input in = longCigarPair( 10, iRev != 0, iBadMate == 0 ); // the 70 kb mate is the bad one, cut to 150 bases
                in.vReads[ iBadMate ].vCodes.resize( 150 ), in.vReads[ iBadMate ].vQual.resize( 150 );
                in.vReads[ 1 - iBadMate ].vCodes.resize( 400, 2 ), in.vReads[ 1 - iBadMate ].vQual.resize( 400, (uint8_t)'I' );
                in.vAlns[ iBadMate ].begin_q = 120, in.vAlns[ iBadMate ].end_q = 153;
                std::string sWant;
                try
                {
                    yardstick( in, uiOptions );
                }
                catch( const std::exception& e )
                {
                    sWant = e.what( );
                }
                const DevResult xDev = shared( in, uiOptions );
                char aText[ 64 ];
                ma_sam::errorText( aText, xDev.uiKind, xDev.iValue );
                if( xDev.uiErrors != 1 || sWant.empty( ) || sWant != aText || xDev.uiRecord != (uint32_t)iBadMate )
                    throw std::runtime_error( "error text: want '" + sWant + "', got '" + ( xDev.uiErrors ? aText : "(none)" ) + "' for record " +
                                              std::to_string( xDev.uiRecord ) );
                if( sWant != ( iRev ? "Index out of range (compCharAt)" : "Query length is off by -3." ) )
                    throw std::runtime_error( "unexpected text of the yardstick: " + sWant );
                // soft clipping prints the whole read: no error even then (the yardstick does not throw either)
                const DevResult xSoft = shared( in, uiOptions | MA_SAM_SOFT_CLIP );
                if( xSoft.uiErrors )
                    throw std::runtime_error( "error reported under soft clipping" );
                compare( xSoft.sText, yardstick( in, uiOptions | MA_SAM_SOFT_CLIP ), "soft clipping beyond the read" );
            }
    printf( "special ok\n" );
    return 0;
}

// ---- the yardstick's text of a dump ----------------------------------------------------------------------------------------
static int dump( int argc, char** argv )
{
    if( argc < 5 )
        return 2;
    FILE* f = fopen( argv[ 2 ], "rb" );
    if( !f )
        throw std::runtime_error( std::string( "cannot open " ) + argv[ 2 ] );
    auto rd = [ & ]( void* p, size_t n ) {
        if( n && fread( p, 1, n, f ) != n )
            throw std::runtime_error( "dump too short" );
    };
    auto u32 = [ & ]( ) {
        uint32_t v;
        rd( &v, 4 );
        return v;
    };
    auto u64 = [ & ]( ) {
        uint64_t v;
        rd( &v, 8 );
        return v;
    };
    char magic[ 8 ];
    rd( magic, 8 );
    if( memcmp( magic, "MASAMP01", 8 ) )
        throw std::runtime_error( "bad dump magic" );
    Input in;
    for( uint32_t i = 0, n = u32( ); i < n; i++ )
    {
        std::string s( u32( ), ' ' );
        rd( &s[ 0 ], s.size( ) );
        in.xContigs.vNames.push_back( s );
        in.xContigs.vStarts.push_back( u64( ) );
        in.xContigs.vLengths.push_back( u64( ) );
    }
    const uint32_t nR = u32( ), bQual = u32( );
    if( nR % 2 )
        throw std::runtime_error( "odd number of reads" );
    for( uint32_t r = 0; r < nR; r++ )
    {
        ReadData q;
        q.sName.assign( u32( ), ' ' );
        rd( &q.sName[ 0 ], q.sName.size( ) );
        q.vCodes.resize( u32( ) );
        rd( q.vCodes.data( ), q.vCodes.size( ) );
        q.bQual = bQual != 0;
        if( q.bQual )
        {
            q.vQual.resize( q.vCodes.size( ) );
            rd( q.vQual.data( ), q.vQual.size( ) );
        }
        in.vReads.push_back( q );
    }
    const size_t nP = nR / 2;
    in.vOff.resize( nP + 1 );
    rd( in.vOff.data( ), ( nP + 1 ) * 8 );
    const size_t nA = in.vOff[ nP ];
    in.vAlns.resize( nA );
    rd( in.vAlns.data( ), nA * sizeof( ma_alignment ) );
    in.vOps.resize( 2 * u64( ) + 2 );
    rd( in.vOps.data( ), ( in.vOps.size( ) - 2 ) * 8 );
    in.vMate.resize( nA + 1 ), in.vOther.resize( nA + 1 );
    rd( in.vMate.data( ), nA * 4 );
    rd( in.vOther.data( ), nA * 4 );
    fclose( f );
    std::vector<uint64_t> vOff;
    std::string sText;
    try
    {
        sText = yardstick( in, (uint32_t)atoi( argv[ 4 ] ), &vOff );
    }
    catch( const std::exception& e )
    {
        printf( "ERROR: %s\n", e.what( ) );
        return 3;
    }
    FILE* o = fopen( argv[ 3 ], "wb" );
    fwrite( sText.data( ), 1, sText.size( ), o );
    fclose( o );
    o = fopen( ( std::string( argv[ 3 ] ) + ".off" ).c_str( ), "wb" );
    fwrite( vOff.data( ), 8, vOff.size( ), o );
    fclose( o );
    return 0;
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
