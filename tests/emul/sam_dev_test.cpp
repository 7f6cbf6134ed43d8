// CPU-only checks of the record formatter the device stage runs (ma_amd/host/ma_sam_dev.h: ma_sam::formatRead over its counting
// and its writing sink) against the yardstick, flat::formatRead of ma_amd/host/ma_flat_sam.h, and the SAM goldens.
//   sam_dev_test golden <case> <pipe dump> <golden.sam> <options>   the records of a pipeline dump: both formatters and the
//                                                                    record lines of the golden must agree byte for byte
//   sam_dev_test random <seed> <lists>                               seeded random record lists under every option combination
//   sam_dev_test special                                             cigars of 65 535 / 65 536 ops (CG tag), the two error texts
//   sam_dev_test dump <dump> <out> <options>                         mode 2, the yardstick of tests/test_gpu_sam.py: writes
//                                                                    flat::formatRead's text of a dump to <out> and the
//                                                                    per-read offsets (u64) to <out>.off; a formatter
//                                                                    exception is printed as "ERROR: <text>" (exit code 3)
// options: the MA_SAM_* bits of include/ma_amd.h.  Every count of the counting sink is checked against the bytes written; the
// writing sink gets a buffer of exactly that size and the reads hold exactly their bases, so that an AddressSanitizer build of
// this program sees any byte touched outside of them.
#include "../../oracle/dump_format.h"
#include "ma_flat_sam.h"
#include "ma_sam_dev.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <cstring>
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
    std::vector<ReadData> vReads;
    std::vector<uint64_t> vOff; // n + 1
    std::vector<ma_alignment> vAlns;
    std::vector<uint64_t> vOps; // (type, length) pairs
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

// the yardstick: flat::formatRead over all reads (throws what it throws)
static std::string yardstick( const Input& rIn, uint32_t uiOptions, std::vector<uint64_t>* pOff = nullptr )
{
    flat::Arena xOut;
    const flat::SamFormat xF = formatOf( uiOptions );
    if( pOff )
        pOff->assign( 1, 0 );
    for( size_t r = 0; r < rIn.vReads.size( ); r++ )
    {
        const ReadData& q = rIn.vReads[ r ];
        flat::ReadView v;
        v.sName = q.sName.data( ), v.uiNameLen = q.sName.size( );
        v.pCodes = q.vCodes.data( ), v.pQuality = q.bQual ? q.vQual.data( ) : nullptr, v.uiLength = q.vCodes.size( );
        flat::formatRead( xOut, xF, rIn.xContigs, v, rIn.vAlns.data( ) + rIn.vOff[ r ], (size_t)( rIn.vOff[ r + 1 ] - rIn.vOff[ r ] ), rIn.vOps.data( ) );
        if( pOff )
            pOff->push_back( xOut.size( ) );
    }
    return std::string( xOut.data( ), xOut.size( ) );
}

struct DevResult
{
    std::string sText;
    uint32_t uiErrors = 0, uiKind = 0;
    int64_t iValue = 0;
};
// the shared formatter: counting sink, then the writing sink into exactly that many bytes
static DevResult shared( const Input& rIn, uint32_t uiOptions )
{
    DevContigs xNames;
    const ma_sam::Contigs xC = xNames.view( rIn.xContigs );
    DevResult xRes;
    for( size_t r = 0; r < rIn.vReads.size( ); r++ )
    {
        const ReadData& q = rIn.vReads[ r ];
        const ma_sam::Read xQ{ q.sName.data( ), q.sName.size( ), q.vCodes.data( ), q.bQual ? q.vQual.data( ) : nullptr, q.vCodes.size( ) };
        const ma_sam::FlatList xL{ rIn.vAlns.data( ) + rIn.vOff[ r ], (uint32_t)( rIn.vOff[ r + 1 ] - rIn.vOff[ r ] ), rIn.vOps.data( ) };
        ma_sam::CountSink xCount;
        ma_sam::formatRead( xCount, uiOptions, xC, xQ, xL );
        if( xCount.nErrors && !xRes.uiErrors )
            xRes.uiKind = xCount.firstKind, xRes.iValue = xCount.firstValue;
        xRes.uiErrors += xCount.nErrors;
        std::unique_ptr<char[]> pBuf( new char[ xCount.n ] ); // (exactly: the sanitizer build sees a byte too many)
        ma_sam::WriteSink xWrite{ pBuf.get( ) };
        ma_sam::formatRead( xWrite, uiOptions, xC, xQ, xL );
        if( xWrite.n != xCount.n )
            throw std::runtime_error( "read " + std::to_string( r ) + ": the counting sink says " + std::to_string( xCount.n ) + " bytes, " +
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
static Input fromPipeDump( const char* sCase, const char* sPipe )
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
    struct Rec
    {
        unsigned long long br, er, bq, eq;
        long long score;
        std::vector<uint64_t> ops;
    };
    std::vector<std::vector<ma_alignment>> vPerRead( c.reads.size( ) );
    std::vector<std::vector<std::vector<uint64_t>>> vPerReadOps( c.reads.size( ) );
    std::vector<Rec> alns;
    std::ifstream f( sPipe );
    std::string line;
    long read = -1;
    while( std::getline( f, line ) )
    {
        std::istringstream is( line );
        std::string tag;
        is >> tag;
        if( tag == "R" )
        {
            is >> read;
            alns.clear( );
        }
        else if( tag == "a" )
        {
            Rec r;
            unsigned soc;
            size_t n;
            is >> r.br >> r.er >> r.bq >> r.eq >> r.score >> soc >> n;
            for( size_t k = 0; k < n; k++ )
            {
                std::string t;
                is >> t;
                const size_t colon = t.find( ':' );
                r.ops.push_back( (uint64_t)atoi( t.substr( 0, colon ).c_str( ) ) );
                r.ops.push_back( strtoull( t.substr( colon + 1 ).c_str( ), nullptr, 10 ) );
            }
            alns.push_back( r );
        }
        else if( tag == "m" )
        {
            unsigned long long br, er, bq, eq;
            long long score;
            int sec, sup;
            std::string sQ;
            is >> br >> er >> bq >> eq >> score >> sec >> sup >> sQ;
            ma_alignment a{ };
            a.begin_ref = (int64_t)br, a.end_ref = (int64_t)er, a.begin_q = (int64_t)bq, a.end_q = (int64_t)eq, a.score = score;
            a.secondary = sec != 0, a.supplementary = sup != 0, a.mapq = strtod( sQ.c_str( ), nullptr );
            std::vector<uint64_t> ops;
            for( auto& r : alns ) // the MQ record is one of the NW alignments
                if( r.br == br && r.er == er && r.bq == bq && r.eq == eq && r.score == score )
                {
                    ops = r.ops;
                    break;
                }
            a.n_ops = (uint32_t)( ops.size( ) / 2 );
            vPerRead[ (size_t)read ].push_back( a );
            vPerReadOps[ (size_t)read ].push_back( ops );
        }
    }
    in.vOff.assign( 1, 0 );
    for( size_t r = 0; r < c.reads.size( ); r++ )
    {
        for( size_t k = 0; k < vPerRead[ r ].size( ); k++ )
        {
            ma_alignment a = vPerRead[ r ][ k ];
            a.ops_off = in.vOps.size( ) / 2;
            in.vOps.insert( in.vOps.end( ), vPerReadOps[ r ][ k ].begin( ), vPerReadOps[ r ][ k ].end( ) );
            in.vAlns.push_back( a );
        }
        in.vOff.push_back( in.vAlns.size( ) );
    }
    in.vOps.push_back( 0 ), in.vOps.push_back( 0 );
    return in;
}

static int golden( int argc, char** argv )
{
    if( argc < 6 )
        return 2;
    const Input in = fromPipeDump( argv[ 2 ], argv[ 3 ] );
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
    compare( xDev.sText, sYard, "shared formatter against flat::formatRead" );
    compare( xDev.sText, sGolden, "shared formatter against the golden" );
    printf( "golden ok: %zu reads, %zu records, %zu bytes\n", in.vReads.size( ), in.vAlns.size( ), sYard.size( ) );
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

static Input randomInput( Rng& g, size_t uiLists )
{
    static const uint64_t aLens[] = { 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257 };
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
    const uint64_t F = off;
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
            const uint64_t cs = in.xContigs.vStarts[ c ], cl = in.xContigs.vLengths[ c ];
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
    in.xContigs.vNames = { "chrL" };
    in.xContigs.vStarts = { 0 };
    in.xContigs.vLengths = { 200000 };
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
                const bool bTag = sYard.find( "\tCG:B:I," ) != std::string::npos;
                if( bTag != ( uiOps >= 0x10000 && !( uiOptions & MA_SAM_NO_CG_TAG ) ) )
                    throw std::runtime_error( "CG tag present / absent against expectation" );
            }
    // a record that ends beyond its read: the yardstick throws, the shared formatter reports the same text, touches nothing
    // beyond the read and writes what it counted
    for( int iRev = 0; iRev < 2; iRev++ )
        for( uint32_t uiOptions : { 0u, (uint32_t)MA_SAM_EQX_CIGAR } )
        {
            Input in = longCigar( 10, iRev != 0 );
            in.vReads[ 0 ].vCodes.resize( 150 ), in.vReads[ 0 ].vQual.resize( 150 );
            in.vAlns[ 0 ].begin_q = 120, in.vAlns[ 0 ].end_q = 153;
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
            if( xDev.uiErrors != 1 || sWant.empty( ) || sWant != aText )
                throw std::runtime_error( "error text: want '" + sWant + "', got '" + ( xDev.uiErrors ? aText : "(none)" ) + "'" );
            if( sWant != ( iRev ? "Index out of range (compCharAt)" : "Query length is off by -3." ) )
                throw std::runtime_error( "unexpected text of the yardstick: " + sWant );
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
    }
    printf( "special ok\n" );
    return 0;
}

// ---- mode 2: the yardstick's text of a dump --------------------------------------------------------------------------------
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
    if( memcmp( magic, "MASAMD01", 8 ) )
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
    in.vOff.resize( nR + 1 );
    rd( in.vOff.data( ), ( nR + 1 ) * 8 );
    in.vAlns.resize( in.vOff[ nR ] );
    rd( in.vAlns.data( ), in.vAlns.size( ) * sizeof( ma_alignment ) );
    in.vOps.resize( 2 * u64( ) + 2 );
    rd( in.vOps.data( ), ( in.vOps.size( ) - 2 ) * 8 );
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
        fprintf( stderr, "sam_dev_test %s: %s\n", sMode.c_str( ), e.what( ) );
        return 1;
    }
    return 2;
}
