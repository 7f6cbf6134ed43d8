// CPU-only checks of the rules the device's BGZF deflate runs (ma_amd/host/ma_deflate_dev.h: ma_bgzf::deflateHost over the routines
// the kernels call) against the yardstick, zlib (<zlib.h>), which is never the code under test: zlib inflates what deflateHost
// wrote, and zlib's deflate on the same 65 280-byte chunks gives the sizes to compare with.
//   sam_bgzf_test roundtrip <seed>        the length x content grid below: the header bytes, BSIZE, CRC32, ISIZE and the size bound of
//                                         every member, the member count, zlib's strict inflate and ma_bgzf::inflateHost over the
//                                         chain with the end-of-file marker; twice the same bytes; a repeated 200-byte line
//                                         compresses to under a tenth
//   sam_bgzf_test codes <seed> <n>        n random histograms per alphabet and limit: the lengths are a complete code within the limit
//   sam_bgzf_test golden <sam.gz> ...     the record lines of every file: round trip, and per file one line
//                                         "<file> text <n> ours <a> fixed1 <b> huffman <c> level1 <d> level6 <e>"
//   sam_bgzf_test deflate <in> <out>      the members of a file's bytes (the GPU tests compare the kernels with this)
//   sam_bgzf_test writers <small.case> <small.pipe> <f4.case> <f4 dump> <out>
//                                         the host writers over the flat records of the reference's dumps, once plain and once with
//                                         SamOptions::bBgzf, to <out>.<writer>.sam / .sam.gz: BatchFileWriter (options 0 and soft
//                                         clip + =/X; the flat formatter, and with the NGMLR tags its per-read writer), FileWriter
//                                         per read, BatchPairedFileWriter (the caller inflates and compares)
// Every buffer holds exactly its bytes, so that an AddressSanitizer build of this program sees any byte touched outside of them.
#include "ma_batch_nodes.h"
#include "ma_deflate_dev.h"
#include "sam_dev_common.h"
#include <algorithm>
#include <fstream>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>
#include <zlib.h>

typedef std::string Bytes;

static Bytes slurp( const std::string& sPath )
{
    std::ifstream xIn( sPath, std::ios::binary );
    if( !xIn )
        throw std::runtime_error( "cannot read " + sPath );
    std::stringstream xAll;
    xAll << xIn.rdbuf( );
    return xAll.str( );
}
static Bytes gunzipFile( const std::string& sPath )
{
    gzFile f = gzopen( sPath.c_str( ), "rb" );
    if( !f )
        throw std::runtime_error( "cannot read " + sPath );
    Bytes sOut;
    char aBuf[ 65536 ];
    int n;
    while( ( n = gzread( f, aBuf, sizeof( aBuf ) ) ) > 0 )
        sOut.append( aBuf, (size_t)n );
    gzclose( f );
    return sOut;
}
static Bytes recordLines( const Bytes& sSam )
{
    Bytes sOut;
    size_t i = 0;
    while( i < sSam.size( ) )
    {
        size_t j = sSam.find( '\n', i );
        j = j == Bytes::npos ? sSam.size( ) : j + 1;
        if( sSam[ i ] != '@' )
            sOut.append( sSam, i, j - i );
        i = j;
    }
    return sOut;
}
static void check( bool b, const std::string& sWhat )
{
    if( !b )
        throw std::runtime_error( sWhat );
}

// ---- zlib: the yardstick --------------------------------------------------------------------------------------------------------
static size_t zlibChunks( const Bytes& sText, int iLevel, int iStrategy ) // raw deflate per chunk + 26 bytes of frame
{
    size_t uiTotal = 0;
    for( size_t i = 0; i < sText.size( ); i += ma_bgzf::DEFLATE_CHUNK )
    {
        const size_t n = std::min<size_t>( ma_bgzf::DEFLATE_CHUNK, sText.size( ) - i );
        z_stream z;
        memset( &z, 0, sizeof( z ) );
        check( deflateInit2( &z, iLevel, Z_DEFLATED, -15, 9, iStrategy ) == Z_OK, "deflateInit2" );
        std::vector<Bytef> vOut( deflateBound( &z, (uLong)n ) + 64 );
        z.next_in = (Bytef*)sText.data( ) + i;
        z.avail_in = (uInt)n;
        z.next_out = vOut.data( );
        z.avail_out = (uInt)vOut.size( );
        check( deflate( &z, Z_FINISH ) == Z_STREAM_END, "deflate" );
        uiTotal += z.total_out + 26;
        deflateEnd( &z );
    }
    return uiTotal;
}
static Bytes zlibStrict( const uint8_t* p, size_t n, size_t uiExpect ) // raw inflate: the stream must end with its last byte
{
    z_stream z;
    memset( &z, 0, sizeof( z ) );
    check( inflateInit2( &z, -15 ) == Z_OK, "inflateInit2" );
    Bytes sOut( uiExpect + 1, '\0' );
    z.next_in = (Bytef*)p;
    z.avail_in = (uInt)n;
    z.next_out = (Bytef*)&sOut[ 0 ];
    z.avail_out = (uInt)sOut.size( );
    const int rc = inflate( &z, Z_FINISH );
    const bool bOk = rc == Z_STREAM_END && z.avail_in == 0;
    sOut.resize( z.total_out );
    inflateEnd( &z );
    check( bOk, "zlib refuses the stream (rc " + std::to_string( rc ) + ")" );
    return sOut;
}

// ---- deflateHost and everything the issue asks of its members ---------------------------------------------------------------------
struct Deflated
{
    std::vector<uint64_t> vOff;
    Bytes sBytes;
};
static Deflated deflated( const Bytes& sText )
{
    Deflated d;
    const uint64_t uiMembers = ma_bgzf::deflateMembers( sText.size( ) );
    d.vOff.assign( uiMembers + 1, ~0ull );
    std::vector<uint8_t> vOut( ma_bgzf::deflateBound( sText.size( ) ) ); // exactly the documented room
    const uint64_t n = ma_bgzf::deflateHost( (const uint8_t*)sText.data( ), sText.size( ), vOut.data( ), d.vOff.data( ) );
    check( n <= vOut.size( ), "deflateHost wrote more than its bound" );
    d.sBytes.assign( (const char*)vOut.data( ), n );
    return d;
}
static size_t roundTrip( const Bytes& sText, const std::string& sName )
{
    try
    {
        const Deflated d = deflated( sText );
        const Deflated d2 = deflated( sText );
        check( d.sBytes == d2.sBytes && d.vOff == d2.vOff, "two runs differ" );
        const size_t uiMembers = ( sText.size( ) + 65279 ) / 65280;
        check( d.vOff.size( ) == uiMembers + 1 && d.vOff[ 0 ] == 0 && d.vOff[ uiMembers ] == d.sBytes.size( ), "member count or offsets" );
        static const uint8_t aHead[ 16 ] = { 0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0 };
        for( size_t k = 0; k < uiMembers; k++ )
        {
            const Bytes sPart = sText.substr( k * 65280, 65280 );
            check( d.vOff[ k + 1 ] > d.vOff[ k ] + 26, "member " + std::to_string( k ) + ": size" );
            const size_t uiSize = d.vOff[ k + 1 ] - d.vOff[ k ];
            const uint8_t* const p = (const uint8_t*)d.sBytes.data( ) + d.vOff[ k ];
            check( memcmp( p, aHead, 16 ) == 0, "member " + std::to_string( k ) + ": header bytes" );
            check( (size_t)p[ 16 ] + 256 * (size_t)p[ 17 ] == uiSize - 1, "member " + std::to_string( k ) + ": BSIZE" );
            check( uiSize <= sPart.size( ) + 31 && uiSize <= 65536, "member " + std::to_string( k ) + ": larger than text + 31" );
            check( ma_bgzf::le32( p + uiSize - 8 ) == (uint32_t)crc32( crc32( 0L, Z_NULL, 0 ), (const Bytef*)sPart.data( ), (uInt)sPart.size( ) ),
                   "member " + std::to_string( k ) + ": CRC32" );
            check( ma_bgzf::le32( p + uiSize - 4 ) == sPart.size( ), "member " + std::to_string( k ) + ": ISIZE" );
            check( zlibStrict( p + 18, uiSize - 26, sPart.size( ) ) == sPart, "member " + std::to_string( k ) + ": zlib inflates other bytes" );
        }
        // the whole chain with the end-of-file marker through the strict form of the inflate side
        Bytes sFile = d.sBytes;
        sFile.resize( sFile.size( ) + ma_bgzf::EOF_BYTES );
        ma_bgzf::writeEof( (uint8_t*)&sFile[ d.sBytes.size( ) ] );
        static const uint8_t aEof[ 28 ] = { 0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
        check( memcmp( sFile.data( ) + d.sBytes.size( ), aEof, 28 ) == 0, "end-of-file marker" );
        ma_bgzf::Result r;
        check( ma_bgzf::inflateHost( (const uint8_t*)sFile.data( ), sFile.size( ), NULL, &r ) == 0 && r.uiBytes == sText.size( ) &&
                   r.uiMembers == uiMembers + 1,
               "inflateHost: headers" );
        std::vector<uint8_t> vBack( sText.size( ) );
        check( ma_bgzf::inflateHost( (const uint8_t*)sFile.data( ), sFile.size( ), vBack.data( ), &r ) == 0, "inflateHost refuses: " +
                                                                                                             std::string( ma_bgzf::errorText( r.uiReason ) ) );
        check( Bytes( vBack.begin( ), vBack.end( ) ) == sText, "inflateHost gives other bytes" );
        return d.sBytes.size( );
    }
    catch( const std::exception& e )
    {
        throw std::runtime_error( sName + " (" + std::to_string( sText.size( ) ) + " bytes): " + e.what( ) );
    }
}

static const size_t aLengths[] = { 0, 1, 2, 3, 4, 5, 257, 258, 259, 65279, 65280, 65281, 130560, 130561 };
static Bytes periodic( size_t n, size_t uiPeriod, Rng& r )
{
    Bytes sUnit( uiPeriod, '\0' );
    for( char& c : sUnit )
        c = (char)( 'A' + r( ) % 26 );
    if( uiPeriod > 1 )
        sUnit[ uiPeriod - 1 ] = '\n'; // (so that the unit is no shorter period)
    Bytes s( n, '\0' );
    for( size_t i = 0; i < n; i++ )
        s[ i ] = sUnit[ i % uiPeriod ];
    return s;
}
static Bytes randomBytes( size_t n, Rng& r, unsigned uiValues = 256 )
{
    Bytes s( n, '\0' );
    for( char& c : s )
        c = (char)( r( ) % uiValues );
    return s;
}
static int roundtripMode( uint64_t uiSeed )
{
    Rng r( uiSeed );
    size_t uiTexts = 0;
    for( size_t n : aLengths )
    {
        for( size_t uiPeriod : { 1, 2, 3, 4, 5, 64 } )
            roundTrip( periodic( n, uiPeriod, r ), "period " + std::to_string( uiPeriod ) ), uiTexts++;
        roundTrip( randomBytes( n, r ), "random" ), uiTexts++;
        roundTrip( randomBytes( n, r, 2 ), "two values" ), uiTexts++;
        Bytes sAll( n, '\0' );
        for( size_t i = 0; i < n; i++ )
            sAll[ i ] = (char)( i & 255 );
        roundTrip( sAll, "all byte values" ), uiTexts++;
    }
    // a random block repeated at distance exactly 32 768 (in reach) and 32 769 (just out of reach)
    // (between the two there is one repeated byte: it takes one entry of the table and leaves the block's in it)
    {
        const Bytes sBlock = randomBytes( 300, r );
        size_t aSize[ 2 ];
        for( size_t i = 0; i < 2; i++ )
        {
            const Bytes s = sBlock + Bytes( 32768 + i - 300, 'x' ) + sBlock + Bytes( 50, 'y' );
            aSize[ i ] = roundTrip( s, "distance " + std::to_string( 32768 + i ) );
            uiTexts++;
        }
        // in reach, the second block is two matches (258 + 42); out of reach it is 300 literals of eight bits
        check( aSize[ 0 ] + 250 < aSize[ 1 ], "distance 32768 / 32769: " + std::to_string( aSize[ 0 ] ) + " / " + std::to_string( aSize[ 1 ] ) + " bytes" );
    }
    // matches that would run across a member's end: a period over the border, and a line whose repeat starts 3 / 100 bytes before it
    for( size_t uiBefore : { 1, 3, 100, 257, 300 } )
    {
        const Bytes sLine = randomBytes( 400, r, 20 );
        Bytes s = randomBytes( 65280 - 1000, r, 4 );
        s += sLine;
        s += randomBytes( 65280 - uiBefore - s.size( ), r, 4 );
        s += sLine + sLine + sLine;
        roundTrip( s, "match across the border, " + std::to_string( uiBefore ) + " before" ), uiTexts++;
    }
    {
        // 22 distinct bytes with Fibonacci counts 1 1 2 .. 17 711: an unrestricted Huffman tree is deeper than 15 levels
        Bytes s;
        size_t a = 1, b = 1;
        for( int i = 0; i < 22; i++ )
        {
            s.append( a, (char)( 'a' + i ) );
            const size_t c = a + b;
            a = b, b = c;
        }
        check( s.size( ) == 46367, "Fibonacci text" );
        std::shuffle( s.begin( ), s.end( ), r );
        const size_t n = roundTrip( s, "Fibonacci counts" );
        check( n < s.size( ) / 2, "Fibonacci counts: stored?" );
        uiTexts++;
    }
    {
        Bytes sLine = randomBytes( 199, r, 64 );
        for( char& c : sLine )
            c = (char)( c + 48 );
        sLine += '\n';
        Bytes s;
        while( s.size( ) < 65280 )
            s += sLine;
        s.resize( 65280 );
        const size_t n = roundTrip( s, "repeated line" );
        check( 10 * n < s.size( ), "a repeated 200-byte line takes " + std::to_string( n ) + " bytes: more than a tenth" );
        uiTexts++;
    }
    printf( "roundtrip ok: %zu texts\n", uiTexts );
    return 0;
}

// ---- the code construction alone ----------------------------------------------------------------------------------------------
static int codesMode( uint64_t uiSeed, size_t uiRounds )
{
    Rng r( uiSeed );
    ma_bgzf::DeflateWork W;
    size_t uiLimited = 0;
    for( size_t k = 0; k < uiRounds; k++ )
    {
        const uint32_t aBase[ 3 ] = { ma_bgzf::A_LITLEN, ma_bgzf::A_DIST, ma_bgzf::A_CODELEN };
        const uint32_t aSize[ 3 ] = { ma_bgzf::N_LITLEN, ma_bgzf::N_DIST, ma_bgzf::N_CODELEN };
        const uint32_t aLimit[ 3 ] = { 15, 15, 7 };
        const int a = (int)( k % 3 );
        memset( &W, 0, sizeof( W ) );
        const uint32_t uiUsed = (uint32_t)( r( ) % ( aSize[ a ] + 1 ) );
        const int iShape = (int)( r( ) % 4 );
        uint64_t uiFib[ 2 ] = { 1, 1 };
        for( uint32_t i = 0; i < uiUsed; i++ )
        {
            uint32_t c;
            if( iShape == 0 )
                c = 1 + (uint32_t)( r( ) % 1000 );
            else if( iShape == 1 )
                c = 1u << ( r( ) % 17 );
            else if( iShape == 2 )
                c = 1;
            else
            {
                c = (uint32_t)std::min<uint64_t>( uiFib[ 0 ], 60000 );
                const uint64_t t = uiFib[ 0 ] + uiFib[ 1 ];
                uiFib[ 0 ] = uiFib[ 1 ], uiFib[ 1 ] = t;
            }
            W.aCount[ aBase[ a ] + r( ) % aSize[ a ] ] = c;
        }
        ma_bgzf::padAlphabet( W, aBase[ a ], aSize[ a ] );
        const uint32_t m = ma_bgzf::rankAll( W, aBase[ a ], aSize[ a ] );
        check( m >= 2 && m == ma_bgzf::usedOf( W, aBase[ a ], aSize[ a ] ), "codes: used symbols" );
        ma_bgzf::lengthsOf( W, aBase[ a ], aSize[ a ], m, aLimit[ a ] );
        uint64_t uiKraft = 0;
        uint32_t uiLongest = 0;
        for( uint32_t s = 0; s < aSize[ a ]; s++ )
        {
            const uint32_t l = W.aLength[ aBase[ a ] + s ];
            check( ( l != 0 ) == ( W.aCount[ aBase[ a ] + s ] != 0 ) && l <= aLimit[ a ], "codes: a length of " + std::to_string( l ) );
            if( l )
                uiKraft += 1ull << ( 15 - l );
            uiLongest = std::max( uiLongest, l );
        }
        check( uiKraft == 1ull << 15, "codes: not a complete code (round " + std::to_string( k ) + ")" );
        // rarer symbols never have shorter codes
        for( uint32_t i = 1; i < m; i++ )
            check( W.aLength[ aBase[ a ] + W.aOrder[ i - 1 ] ] >= W.aLength[ aBase[ a ] + W.aOrder[ i ] ], "codes: order" );
        uiLimited += uiLongest == aLimit[ a ] ? 1 : 0;
    }
    check( 10 * uiLimited >= uiRounds, "codes: the limit was hardly ever reached" );
    printf( "codes ok: %zu histograms, %zu at the limit\n", uiRounds, uiLimited );
    return 0;
}

static int goldenMode( int argc, char** argv )
{
    size_t aTotal[ 6 ] = { 0, 0, 0, 0, 0, 0 };
    for( int i = 2; i < argc; i++ )
    {
        const Bytes sText = recordLines( gunzipFile( argv[ i ] ) );
        const size_t a[ 6 ] = { sText.size( ),
                                roundTrip( sText, argv[ i ] ),
                                zlibChunks( sText, 1, Z_FIXED ),
                                zlibChunks( sText, 1, Z_HUFFMAN_ONLY ),
                                zlibChunks( sText, 1, Z_DEFAULT_STRATEGY ),
                                zlibChunks( sText, 6, Z_DEFAULT_STRATEGY ) };
        printf( "%s text %zu ours %zu fixed1 %zu huffman %zu level1 %zu level6 %zu\n", argv[ i ], a[ 0 ], a[ 1 ], a[ 2 ], a[ 3 ], a[ 4 ], a[ 5 ] );
        for( int k = 0; k < 6; k++ )
            aTotal[ k ] += a[ k ];
    }
    printf( "golden ok: %d files text %zu ours %zu fixed1 %zu huffman %zu level1 %zu level6 %zu\n", argc - 2, aTotal[ 0 ], aTotal[ 1 ], aTotal[ 2 ],
            aTotal[ 3 ], aTotal[ 4 ], aTotal[ 5 ] );
    return 0;
}

static int deflateMode( const std::string& sIn, const std::string& sOut )
{
    const Deflated d = deflated( slurp( sIn ) );
    std::ofstream xOut( sOut, std::ios::binary );
    xOut.write( d.sBytes.data( ), (std::streamsize)d.sBytes.size( ) );
    check( (bool)xOut, "cannot write " + sOut );
    printf( "deflate ok: %zu members, %zu bytes\n", d.vOff.size( ) - 1, d.sBytes.size( ) );
    return 0;
}

// ---- the host writers -----------------------------------------------------------------------------------------------------------
// the pair records ("P" / "p" lines) of the reference's f4 dump; mate and other beside them
struct PairInput : Input
{
    std::vector<int32_t> vMate, vOther;
};
static PairInput pairsOfDump( const char* sCase, const char* sDump )
{
    PairInput in;
    static_cast<Input&>( in ) = fromCase( sCase );
    if( in.vReads.size( ) % 2 )
        in.vReads.pop_back( );
    std::ifstream f( sDump );
    std::string line;
    while( std::getline( f, line ) )
    {
        std::istringstream ss( line );
        std::string tag;
        ss >> tag;
        if( tag == "P" )
            in.vOff.push_back( in.vAlns.size( ) );
        else if( tag == "p" )
        {
            ma_alignment a;
            memset( &a, 0, sizeof( a ) );
            int first, other;
            size_t nops;
            std::string sMq;
            ss >> first >> other >> a.begin_ref >> a.end_ref >> a.begin_q >> a.end_q >> a.score >> a.soc_index >> a.secondary >> a.supplementary >> sMq >> nops;
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
    check( ( in.vOff.size( ) - 1 ) * 2 == in.vReads.size( ), "the dump's pairs are not the case's reads" );
    in.vOps.push_back( 0 ), in.vOps.push_back( 0 );
    in.vMate.push_back( 0 ), in.vOther.push_back( 0 );
    return in;
}
template <typename T> static void fill( ma_amd::engine::HostBuf<T>& rBuf, const std::vector<T>& v )
{
    memcpy( rBuf.need( v.size( ) + 2 ), v.data( ), v.size( ) * sizeof( T ) );
}
// the batch a device run would return for the records of rIn
static std::shared_ptr<AlignedBatch> batchOf( const Input& rIn, const PairInput* pPairs )
{
    auto pResult = std::make_shared<ma_amd::engine::BatchResult>( );
    pResult->uiReads = rIn.vReads.size( );
    if( pPairs == nullptr )
    {
        fill( pResult->vMqOff, rIn.vOff ), fill( pResult->vMq, rIn.vAlns ), fill( pResult->vMqOps, rIn.vOps );
        pResult->uiMqAlignments = rIn.vAlns.size( );
    }
    else
    {
        pResult->bPairs = true;
        fill( pResult->vMqOff, std::vector<uint64_t>( rIn.vReads.size( ) + 1, 0 ) );
        fill( pResult->vPairOff, rIn.vOff ), fill( pResult->vPair, rIn.vAlns ), fill( pResult->vPairOps, rIn.vOps );
        fill( pResult->vPairMate, pPairs->vMate ), fill( pResult->vPairOther, pPairs->vOther );
        pResult->uiPairRecords = rIn.vAlns.size( );
    }
    auto pBatch = std::make_shared<AlignedBatch>( );
    pBatch->pReads = std::make_shared<ReadVector>( );
    for( const ReadData& rRead : rIn.vReads )
        pBatch->pReads->push_back( rRead.container( ) );
    pBatch->pResult = pResult;
    return pBatch;
}
static void spill( const std::string& sPath, const std::string& sBytes )
{
    std::ofstream xOut( sPath, std::ios::binary );
    xOut.write( sBytes.data( ), (std::streamsize)sBytes.size( ) );
    check( (bool)xOut, "cannot write " + sPath );
}
// WRITE( parameters, stream ) runs a writer to its end; once plain, once with the option
template <typename WRITE> static void bothWays( const std::string& sOut, uint32_t uiOptions, WRITE write )
{
    for( int iBgzf = 0; iBgzf < 2; iBgzf++ )
    {
        ParameterSetManager xParams;
        xParams.xSam = optionsOf( uiOptions );
        xParams.xSam.bBgzf = iBgzf != 0;
        auto pStream = std::make_shared<StringOutStream>( );
        write( xParams, std::static_pointer_cast<OutStream>( pStream ) );
        spill( sOut + ( iBgzf ? ".sam.gz" : ".sam" ), pStream->sText );
    }
}
static int writersMode( char** argv )
{
    const Input xSingle = fromPipeDump( argv[ 2 ], argv[ 3 ] );
    const PairInput xPairs = pairsOfDump( argv[ 4 ], argv[ 5 ] );
    const std::string sOut = argv[ 6 ];
    const auto pPack = xSingle.pack( );
    const auto pBatch = batchOf( xSingle, nullptr );
    for( uint32_t uiOptions : { 0u, 3u, (uint32_t)MA_SAM_NGMLR_TAGS } )
        bothWays( sOut + ".batch" + std::to_string( uiOptions ), uiOptions, [ & ]( const ParameterSetManager& rParams, std::shared_ptr<OutStream> pStream ) {
            BatchFileWriter xWriter( rParams, pStream, pPack );
            xWriter.execute( pBatch->pReads, pBatch, pPack );
            xWriter.write( *pBatch, pPack ); // (a second batch behind the first)
        } ); // (the stream closes with the writer)
    bothWays( sOut + ".perread", 0, [ & ]( const ParameterSetManager& rParams, std::shared_ptr<OutStream> pStream ) {
        FileWriter xWriter( rParams, pStream, pPack );
        FileWriter xSecond( rParams, std::shared_ptr<FileWriter>( &xWriter, []( FileWriter* ) {} ) ); // a second writer on the same stream
        for( size_t r = 0; r < xSingle.vReads.size( ); r++ )
            ( r % 2 ? xSecond : xWriter ).execute( xSingle.vReads[ r ].container( ), xSingle.containers( r ), pPack );
        xWriter.finishStream( );
        xWriter.finishStream( ); // (the marker is written once)
    } );
    const auto pPairPack = xPairs.pack( );
    const auto pPairBatch = batchOf( xPairs, &xPairs );
    bothWays( sOut + ".pairs", 3, [ & ]( const ParameterSetManager& rParams, std::shared_ptr<OutStream> pStream ) {
        BatchPairedFileWriter xWriter( rParams, pStream, pPairPack );
        xWriter.execute( *pPairBatch );
    } );
    // members of a device batch onto a plain stream are refused
    {
        auto pResult = std::make_shared<ma_amd::engine::BatchResult>( );
        pResult->uiReads = xSingle.vReads.size( ), pResult->bSam = pResult->bSamBgzf = true;
        auto pMembers = std::make_shared<AlignedBatch>( );
        pMembers->pReads = pBatch->pReads, pMembers->pResult = pResult;
        ParameterSetManager xParams;
        BatchFileWriter xWriter( xParams, std::static_pointer_cast<OutStream>( std::make_shared<StringOutStream>( ) ), pPack );
        const std::string sRefusal = errorOf( [ & ]( ) { xWriter.write( *pMembers, pPack ); } );
        check( sRefusal.find( "the writer's stream is plain" ) != std::string::npos, "members onto a plain stream: \"" + sRefusal + "\"" );
    }
    printf( "writers ok: %zu reads, %zu pairs\n", xSingle.vReads.size( ), xPairs.vOff.size( ) - 1 );
    return 0;
}

int main( int argc, char** argv )
{
    try
    {
        const std::string sMode = argc > 1 ? argv[ 1 ] : "";
        if( sMode == "roundtrip" && argc == 3 )
            return roundtripMode( std::stoull( argv[ 2 ] ) );
        if( sMode == "codes" && argc == 4 )
            return codesMode( std::stoull( argv[ 2 ] ), std::stoull( argv[ 3 ] ) );
        if( sMode == "golden" && argc >= 3 )
            return goldenMode( argc, argv );
        if( sMode == "deflate" && argc == 4 )
            return deflateMode( argv[ 2 ], argv[ 3 ] );
        if( sMode == "writers" && argc == 7 )
            return writersMode( argv );
        fprintf( stderr, "usage: sam_bgzf_test roundtrip <seed> | codes <seed> <n> | golden <sam.gz> ... | deflate <in> <out> | writers <case> <pipe> <f4 case> <f4 dump> <out>\n" );
        return 2;
    }
    catch( const std::exception& e )
    {
        fprintf( stderr, "FAILED: %s\n", e.what( ) );
        return 1;
    }
}
