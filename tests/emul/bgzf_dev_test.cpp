// CPU-only checks of the rules the device's BGZF inflate runs (ma_amd/host/ma_bgzf_dev.h: ma_bgzf::inflateHost over the routine
// the kernels call) and of BatchBgzfReader (ma_amd/host/ma_batch_nodes.h) against the yardstick, zlib (<zlib.h>), which is not
// the code under test.  The program writes its BGZF itself: deflateInit2( level, Z_DEFLATED, -15, 9, strategy ) per member, the
// 18-byte header and the trailer around it.
//   bgzf_dev_test kinds <seed>            members of every kind (stored, fixed, dynamic, Huffman only, RLE, several blocks) at 0 1
//                                         2 257 258 259 32767 32768 32769 65536 bytes of read text and of one repeated byte,
//                                         a match of length 258 at distance 32768, a chain of members with empty ones: the
//                                         text equals zlib's
//   bgzf_dev_test handmade                hand-assembled dynamic headers: a distance set of one code, of no code, the repeats
//                                         16 / 17 / 18 across the literal/distance border, a block that is its end code alone
//   bgzf_dev_test mutants <seed> <n>      per kind n single-bit flips of the deflate bytes with the trailer left alone (A: the
//                                         verdict equals zlib's strict decode + CRC + ISIZE) and n with the trailer recomputed
//                                         where zlib still decodes (B: accepted with zlib's bytes, else refused)
//   bgzf_dev_test reasons [print]         one hand-made stream per reason: member, byte and wording of the refusal
//   bgzf_dev_test crc <seed>              crcOf / crcCombine and the kernel's 64-lane fold against zlib's crc32
//   bgzf_dev_test reader <bytes> <fq>     BatchBgzfReader's batches over <fq> compressed at members of 1, 7, 300 and 65280 bytes
//                                         of text and over a generated FASTA of long records: their texts concatenate to the
//                                         file and start at record starts; plain gzip throws and names GzFileStream
// zlib's strict decode: inflateInit2( -15 ), Z_STREAM_END, no input left, at most 65536 bytes.  Every buffer holds exactly its
// bytes, so that an AddressSanitizer build of this program sees any byte touched outside of them.
#include "ma_batch_nodes.h"
#include "ma_bgzf_dev.h"
#include <fstream>
#include <random>
#include <zlib.h>

using namespace libMA;
typedef std::string Bytes;
typedef std::mt19937_64 Rng;

static size_t pick( Rng& r, size_t n )
{
    return (size_t)( r( ) % n );
}
static Bytes slurp( const std::string& sPath )
{
    std::ifstream xIn( sPath, std::ios::binary );
    if( !xIn )
        throw std::runtime_error( "cannot read " + sPath );
    std::stringstream xAll;
    xAll << xIn.rdbuf( );
    return xAll.str( );
}

// ---- zlib: the writer of the test's members and the yardstick ---------------------------------------------------------------------
static Bytes deflateRaw( const Bytes& sText, int iLevel, int iStrategy, size_t uiFlushAt = 0 )
{
    z_stream z;
    memset( &z, 0, sizeof( z ) );
    if( deflateInit2( &z, iLevel, Z_DEFLATED, -15, 9, iStrategy ) != Z_OK )
        throw std::runtime_error( "deflateInit2" );
    Bytes sOut( deflateBound( &z, (uLong)sText.size( ) ) + 64, '\0' );
    z.next_out = (Bytef*)&sOut[ 0 ];
    z.avail_out = (uInt)sOut.size( );
    z.next_in = (Bytef*)sText.data( );
    if( uiFlushAt > 0 && uiFlushAt < sText.size( ) )
    {
        z.avail_in = (uInt)uiFlushAt;
        if( deflate( &z, Z_FULL_FLUSH ) != Z_OK )
            throw std::runtime_error( "deflate: flush" );
    }
    z.avail_in = (uInt)( sText.size( ) - z.total_in );
    if( deflate( &z, Z_FINISH ) != Z_STREAM_END )
        throw std::runtime_error( "deflate: finish" );
    sOut.resize( z.total_out );
    deflateEnd( &z );
    return sOut;
}
static void le( Bytes& s, uint32_t v, int n )
{
    for( int i = 0; i < n; i++ )
        s += (char)( ( v >> ( 8 * i ) ) & 0xff );
}
// a BGZF member around a deflate stream; sOther: subfields in front of BC.  (BSIZE is 16 bits: the caller checks fits( ).)
static Bytes member( const Bytes& sDeflate, uint32_t uiCrc, uint32_t uiIsize, const Bytes& sOther = "" )
{
    Bytes s( "\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff", 10 );
    le( s, (uint32_t)sOther.size( ) + 6, 2 );
    s += sOther;
    s += "BC";
    le( s, 2, 2 );
    le( s, (uint32_t)( 12 + sOther.size( ) + 6 + sDeflate.size( ) + 8 - 1 ), 2 );
    s += sDeflate;
    le( s, uiCrc, 4 );
    le( s, uiIsize, 4 );
    return s;
}
static bool fits( const Bytes& sDeflate )
{
    return 12 + 6 + sDeflate.size( ) + 8 <= 65536;
}
static uint32_t zcrc( const Bytes& s )
{
    return (uint32_t)crc32( crc32( 0L, Z_NULL, 0 ), (const Bytef*)s.data( ), (uInt)s.size( ) );
}
static Bytes memberOfText( const Bytes& sText, int iLevel = Z_DEFAULT_COMPRESSION, int iStrategy = Z_DEFAULT_STRATEGY, size_t uiFlushAt = 0 )
{
    return member( deflateRaw( sText, iLevel, iStrategy, uiFlushAt ), zcrc( sText ), (uint32_t)sText.size( ) );
}
static const Bytes& endMarker( ) // the 28 bytes bgzip ends a file with
{
    static const Bytes s = member( Bytes( "\x03\x00", 2 ), 0, 0 );
    return s;
}
struct Decoded
{
    bool bOk;
    Bytes sOut;
};
static Decoded zlibStrict( const Bytes& sDeflate )
{
    z_stream z;
    memset( &z, 0, sizeof( z ) );
    if( inflateInit2( &z, -15 ) != Z_OK )
        throw std::runtime_error( "inflateInit2" );
    Bytes sOut( 65537, '\0' );
    z.next_in = (Bytef*)sDeflate.data( );
    z.avail_in = (uInt)sDeflate.size( );
    z.next_out = (Bytef*)&sOut[ 0 ];
    z.avail_out = (uInt)sOut.size( );
    const int iRet = inflate( &z, Z_FINISH );
    Decoded d;
    d.bOk = iRet == Z_STREAM_END && z.avail_in == 0 && z.total_out <= 65536;
    sOut.resize( z.total_out );
    d.sOut = d.bOk ? sOut : Bytes( );
    inflateEnd( &z );
    return d;
}

// ---- the code under test ----------------------------------------------------------------------------------------------------------
// ma_bgzf::inflate on a deflate stream that is to give uiIsize bytes
static Decoded oursDeflate( const Bytes& sDeflate, uint32_t uiIsize, uint32_t* pReason = nullptr )
{
    std::unique_ptr<uint8_t[]> pIn( new uint8_t[ sDeflate.size( ) ] ), pOut( new uint8_t[ uiIsize ] ); // (exactly their bytes)
    memcpy( pIn.get( ), sDeflate.data( ), sDeflate.size( ) );
    ma_bgzf::HostTables xTables;
    memset( xTables.a, 0, sizeof( xTables.a ) );
    const ma_bgzf::ByteSource xSrc = { pIn.get( ), (uint32_t)sDeflate.size( ) };
    ma_bgzf::ByteSink xSink = { pOut.get( ) };
    const uint32_t uiReason = ma_bgzf::inflate( xSrc, xSink, xTables, uiIsize );
    if( pReason )
        *pReason = uiReason;
    Decoded d;
    d.bOk = uiReason == ma_bgzf::OK;
    if( d.bOk )
        d.sOut.assign( (const char*)pOut.get( ), uiIsize );
    return d;
}
struct Hosted
{
    bool bOk;
    Bytes sOut;
    ma_bgzf::Result xResult;
    std::string sMessage;
};
static Hosted oursStream( const Bytes& sData )
{
    Hosted h;
    std::unique_ptr<uint8_t[]> pIn( new uint8_t[ sData.size( ) ] );
    memcpy( pIn.get( ), sData.data( ), sData.size( ) );
    h.bOk = ma_bgzf::inflateHost( pIn.get( ), sData.size( ), nullptr, &h.xResult ) == 0;
    if( h.bOk )
    {
        std::unique_ptr<uint8_t[]> pOut( new uint8_t[ h.xResult.uiBytes ] );
        h.bOk = ma_bgzf::inflateHost( pIn.get( ), sData.size( ), pOut.get( ), &h.xResult ) == 0;
        if( h.bOk )
            h.sOut.assign( (const char*)pOut.get( ), h.xResult.uiBytes );
    }
    if( !h.bOk )
    {
        char aMessage[ 320 ];
        ma_bgzf::message( aMessage, sizeof( aMessage ), h.xResult.uiMember, h.xResult.uiByte, h.xResult.uiReason );
        h.sMessage = aMessage;
    }
    return h;
}

// ---- texts and member kinds -------------------------------------------------------------------------------------------------------
static Bytes fastq( Rng& r, size_t uiBytes )
{
    Bytes s;
    for( size_t k = 0; s.size( ) < uiBytes; k++ )
    {
        const size_t n = 60 + pick( r, 90 );
        Bytes sBases, sQual;
        for( size_t i = 0; i < n; i++ )
        {
            sBases += "ACGT"[ pick( r, 4 ) ];
            sQual += (char)( 'F' - (int)pick( r, pick( r, 8 ) ? 3 : 30 ) );
        }
        s += "@read" + std::to_string( k ) + "/" + std::to_string( pick( r, 1000 ) ) + " extra\n" + sBases + "\n+\n" + sQual + "\n";
    }
    s.resize( uiBytes );
    return s;
}
enum Kind
{
    STORED,
    FIXED,
    DYNAMIC,
    HUFFMAN,
    RLE,
    BLOCKS,
    N_KINDS
};
static const char* const aKindName[ N_KINDS ] = { "stored", "fixed", "dynamic", "huffman-only", "rle", "blocks" };
static Bytes deflateKind( const Bytes& sText, int iKind )
{
    switch( iKind )
    {
        case STORED:
            return deflateRaw( sText, 0, Z_DEFAULT_STRATEGY );
        case FIXED:
            return deflateRaw( sText, Z_DEFAULT_COMPRESSION, Z_FIXED );
        case HUFFMAN:
            return deflateRaw( sText, Z_DEFAULT_COMPRESSION, Z_HUFFMAN_ONLY );
        case RLE:
            return deflateRaw( sText, Z_DEFAULT_COMPRESSION, Z_RLE );
        case BLOCKS:
            return deflateRaw( sText, Z_DEFAULT_COMPRESSION, Z_DEFAULT_STRATEGY, sText.size( ) / 2 + 1 );
        default:
            return deflateRaw( sText, Z_DEFAULT_COMPRESSION, Z_DEFAULT_STRATEGY );
    }
}

// ---- hand-assembled deflate -------------------------------------------------------------------------------------------------------
struct BitWriter
{
    Bytes s;
    uint32_t uiAcc = 0;
    int nAcc = 0;
    void put( uint32_t v, int n ) // n bits, the lowest first
    {
        for( int i = 0; i < n; i++ )
        {
            uiAcc |= ( ( v >> i ) & 1u ) << nAcc;
            if( ++nAcc == 8 )
                s += (char)uiAcc, uiAcc = 0, nAcc = 0;
        }
    }
    void code( uint32_t c, int n ) // a Huffman code: the highest bit first
    {
        for( int i = n - 1; i >= 0; i-- )
            put( ( c >> i ) & 1u, 1 );
    }
    Bytes done( )
    {
        if( nAcc )
            s += (char)uiAcc, uiAcc = 0, nAcc = 0;
        return s;
    }
};
static std::vector<uint32_t> canonical( const std::vector<int>& vLen ) // RFC 1951, 3.2.2
{
    std::vector<uint32_t> vCount( 17, 0 ), vNext( 17, 0 ), vCode( vLen.size( ), 0 );
    for( int l : vLen )
        vCount[ l ]++;
    vCount[ 0 ] = 0;
    uint32_t c = 0;
    for( int l = 1; l <= 16; l++ )
        vNext[ l ] = c = ( c + vCount[ l - 1 ] ) << 1;
    for( size_t i = 0; i < vLen.size( ); i++ )
        if( vLen[ i ] )
            vCode[ i ] = vNext[ vLen[ i ] ]++;
    return vCode;
}
static const int aLenBase[ 29 ] = { 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258 };
static const int aLenExtra[ 29 ] = { 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0 };
static const int aDistBase[ 30 ] = { 1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                     193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577 };
static const int aDistExtra[ 30 ] = { 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13 };
// the symbols of one block under given code lengths
struct BlockCodes
{
    std::vector<int> vLit, vDist;
    std::vector<uint32_t> vLitCode, vDistCode;
    BlockCodes( const std::vector<int>& rLit, const std::vector<int>& rDist )
        : vLit( rLit ), vDist( rDist ), vLitCode( canonical( rLit ) ), vDistCode( canonical( rDist ) )
    {}
    void symbol( BitWriter& w, int s ) const
    {
        if( vLit[ s ] == 0 )
            throw std::runtime_error( "test: a symbol without a code" );
        w.code( vLitCode[ s ], vLit[ s ] );
    }
    void match( BitWriter& w, int iLen, int iDist ) const
    {
        int l = 28, d = 29;
        while( aLenBase[ l ] > iLen )
            l--;
        if( iLen == 258 )
            l = 28;
        else if( l == 28 )
            l = 27;
        while( aDistBase[ d ] > iDist )
            d--;
        symbol( w, 257 + l );
        w.put( (uint32_t)( iLen - aLenBase[ l ] ), aLenExtra[ l ] );
        if( vDist[ d ] == 0 )
            throw std::runtime_error( "test: a distance without a code" );
        w.code( vDistCode[ d ], vDist[ d ] );
        w.put( (uint32_t)( iDist - aDistBase[ d ] ), aDistExtra[ d ] );
    }
};
static BlockCodes fixedCodes( )
{
    std::vector<int> vLit( 288 ), vDist( 30, 5 );
    for( int s = 0; s < 288; s++ )
        vLit[ s ] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
    return BlockCodes( vLit, vDist );
}
// The header of a dynamic block: the lengths are sent by the code-length symbols vOps (symbol, value of its extra bits), which
// must expand to rLit followed by rDist unless bCheck is off; the code-length codes get the lengths 1, 2, ..., k - 1, k - 1 in
// the order of their first use (a complete set), or vForced if that is given (19 lengths by symbol).
typedef std::vector<std::pair<int, int>> Ops;
static void dynamicHeader( BitWriter& w, bool bLast, size_t nLit, size_t nDist, const Ops& vOps, const std::vector<int>& vForced = { } )
{
    static const int aOrder[ 19 ] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
    std::vector<int> vCl( 19, 0 );
    if( !vForced.empty( ) )
        vCl = vForced;
    else
    {
        std::vector<int> vUsed;
        for( const auto& rOp : vOps )
            if( std::find( vUsed.begin( ), vUsed.end( ), rOp.first ) == vUsed.end( ) )
                vUsed.push_back( rOp.first );
        for( size_t i = 0; i < vUsed.size( ); i++ )
            vCl[ vUsed[ i ] ] = (int)std::min( i + 1, vUsed.size( ) - 1 );
    }
    const std::vector<uint32_t> vCode = canonical( vCl );
    w.put( bLast ? 1 : 0, 1 );
    w.put( 2, 2 );
    w.put( (uint32_t)( nLit - 257 ), 5 );
    w.put( (uint32_t)( nDist - 1 ), 5 );
    w.put( 15, 4 );
    for( int i = 0; i < 19; i++ )
        w.put( (uint32_t)vCl[ aOrder[ i ] ], 3 );
    for( const auto& rOp : vOps )
    {
        w.code( vCode[ rOp.first ], vCl[ rOp.first ] );
        if( rOp.first >= 16 )
            w.put( (uint32_t)rOp.second, rOp.first == 16 ? 2 : rOp.first == 17 ? 3 : 7 );
    }
}
static std::vector<int> expand( const Ops& vOps )
{
    std::vector<int> v;
    for( const auto& rOp : vOps )
    {
        if( rOp.first < 16 )
            v.push_back( rOp.first );
        else
            v.insert( v.end( ), (size_t)( rOp.first == 18 ? 11 : 3 ) + rOp.second, rOp.first == 16 ? v.back( ) : 0 );
    }
    return v;
}
static Ops zeros( size_t n ) // a run of n >= 3 zero lengths
{
    Ops v;
    while( n >= 11 )
    {
        const size_t k = std::min<size_t>( n, 138 ) - ( n > 138 && n - 138 < 3 ? 3 : 0 );
        v.push_back( { 18, (int)( k - 11 ) } );
        n -= k;
    }
    if( n >= 3 )
        v.push_back( { 17, (int)( n - 3 ) } ), n = 0;
    while( n-- )
        v.push_back( { 0, 0 } );
    return v;
}
static Ops operator+( Ops a, const Ops& b )
{
    a.insert( a.end( ), b.begin( ), b.end( ) );
    return a;
}
// a whole dynamic block out of its lengths as vOps sends them, and what it holds: literals ('A'..), or { -len, dist } matches
struct Hand
{
    std::string sName;
    Bytes sDeflate;
};
static Hand handBlock( const std::string& sName, size_t nLit, size_t nDist, const Ops& vOps, const std::vector<std::pair<int, int>>& vData )
{
    const std::vector<int> vAll = expand( vOps );
    if( vAll.size( ) != nLit + nDist )
        throw std::runtime_error( "test: " + sName + ": the lengths do not fill the block" );
    const BlockCodes xCodes( std::vector<int>( vAll.begin( ), vAll.begin( ) + nLit ), std::vector<int>( vAll.begin( ) + nLit, vAll.end( ) ) );
    BitWriter w;
    dynamicHeader( w, true, nLit, nDist, vOps );
    for( const auto& rItem : vData )
        if( rItem.first >= 0 )
            xCodes.symbol( w, rItem.first );
        else
            xCodes.match( w, -rItem.first, rItem.second );
    xCodes.symbol( w, 256 );
    return Hand{ sName, w.done( ) };
}

static int fail( const std::string& s )
{
    printf( "FAIL %s\n", s.c_str( ) );
    return 1;
}
// ours on the stream alone and, where a member holds it, through inflateHost: both as zlib's strict decode
static int sameAsZlib( const std::string& sWhat, const Bytes& sDeflate, bool bMustAccept, const Bytes* pText = nullptr )
{
    const Decoded z = zlibStrict( sDeflate );
    if( bMustAccept && !z.bOk )
        return fail( sWhat + ": zlib refuses the test's own stream" );
    if( pText && z.sOut != *pText )
        return fail( sWhat + ": zlib does not give the text back" );
    uint32_t uiReason = 0;
    const Decoded o = oursDeflate( sDeflate, (uint32_t)z.sOut.size( ), &uiReason );
    if( o.bOk != z.bOk || o.sOut != z.sOut )
        return fail( sWhat + ": zlib " + ( z.bOk ? "accepts" : "refuses" ) + ", inflate says '" + ma_bgzf::errorText( uiReason ) + "'" +
                     ( o.bOk ? " with other bytes" : "" ) );
    if( z.bOk && fits( sDeflate ) )
    {
        const Hosted h = oursStream( member( sDeflate, zcrc( z.sOut ), (uint32_t)z.sOut.size( ) ) );
        if( !h.bOk || h.sOut != z.sOut )
            return fail( sWhat + ": as a member: " + h.sMessage );
    }
    return 0;
}

static int kinds( uint64_t uiSeed )
{
    Rng r( uiSeed );
    static const size_t aSizes[] = { 0, 1, 2, 257, 258, 259, 32767, 32768, 32769, 65536 };
    size_t nStreams = 0, nMembers = 0;
    for( size_t uiSize : aSizes )
        for( int iData = 0; iData < 3; iData++ )
        {
            // read text; one repeated byte (matches at distance 1); short periods (overlapping copies of every small distance)
            Bytes sText = iData == 0 ? fastq( r, uiSize ) : Bytes( uiSize, 'A' );
            if( iData == 2 )
                for( size_t i = 0; i < uiSize; i++ )
                    sText[ i ] = (char)( 'a' + i % ( 2 + i / 700 % 9 ) );
            for( int iKind = 0; iKind < N_KINDS; iKind++ )
            {
                const Bytes sDeflate = deflateKind( sText, iKind );
                if( sameAsZlib( std::string( aKindName[ iKind ] ) + " " + std::to_string( uiSize ) + " bytes, data " + std::to_string( iData ), sDeflate,
                                true, &sText ) )
                    return 1;
                nStreams++;
                nMembers += fits( sDeflate ) ? 1 : 0;
            }
        }
    // a match of length 258 at distance 32768 (zlib's deflate never looks that far back): fixed codes by hand
    {
        const BlockCodes xFixed = fixedCodes( );
        BitWriter w;
        w.put( 1, 1 );
        w.put( 1, 2 );
        Bytes sText;
        for( size_t i = 0; i < 32768; i++ )
        {
            sText += (char)pick( r, 256 );
            xFixed.symbol( w, (uint8_t)sText.back( ) );
        }
        xFixed.match( w, 258, 32768 );
        xFixed.match( w, 3, 1 );
        xFixed.symbol( w, 256 );
        sText += sText.substr( 0, 258 ) + Bytes( 3, sText[ 257 ] );
        if( sameAsZlib( "length 258 at distance 32768", w.done( ), true, &sText ) )
            return 1;
        nStreams++, nMembers++;
    }
    // a chain: members of every kind with empty ones in front, in the middle and at the end
    {
        Bytes sData = endMarker( ), sAll;
        for( int iKind = 0; iKind < N_KINDS; iKind++ )
        {
            const Bytes sText = fastq( r, 1 + pick( r, 3000 ) );
            sData += member( deflateKind( sText, iKind ), zcrc( sText ), (uint32_t)sText.size( ), iKind == FIXED ? Bytes( "XY\x03\x00" "abc", 7 ) : Bytes( ) );
            sAll += sText;
            if( iKind == DYNAMIC )
                sData += endMarker( ) + memberOfText( Bytes( ), 0 );
        }
        sData += endMarker( );
        const Hosted h = oursStream( sData );
        if( !h.bOk || h.sOut != sAll || h.xResult.uiMembers != N_KINDS + 4 )
            return fail( "a chain of members: " + h.sMessage );
    }
    printf( "kinds ok: %zu streams equal, %zu of them also as members\n", nStreams, nMembers );
    return 0;
}

static int handmade( )
{
    std::vector<Hand> v;
    const Ops A1 = { { 1, 0 } }, A2 = { { 2, 0 } }, A3 = { { 3, 0 } };
    // 'A' 1 bit, end and length 3 2 bits; ONE distance code (distance 1) of length 1: an incomplete set zlib accepts
    v.push_back( handBlock( "one distance code", 258, 1, zeros( 65 ) + A1 + zeros( 190 ) + A2 + A2 + A1, { { 65, 0 }, { -3, 1 } } ) );
    // no distance code at all, literals only
    v.push_back( handBlock( "no distance code", 257, 1, zeros( 65 ) + A1 + zeros( 190 ) + A1 + Ops{ { 0, 0 } }, { { 65, 0 }, { 65, 0 } } ) );
    // repeat 16 across the border: 253 has 3, then five more 3s: 254 255 256 and the distances 0 1
    v.push_back( handBlock( "repeat 16 across the border", 257, 5, zeros( 65 ) + A2 + A2 + zeros( 186 ) + A3 + Ops{ { 16, 2 } } + A2 + A2 + A2,
                            { { 65, 0 }, { 66, 0 }, { 253, 0 }, { 255, 0 } } ) );
    // repeat 17 across the border: 258 259 and the distances 0 1 are 0; the distances 2 3 have a bit
    v.push_back( handBlock( "repeat 17 across the border", 260, 4, zeros( 65 ) + A1 + zeros( 190 ) + A2 + A2 + Ops{ { 17, 1 } } + A1 + A1,
                            { { 65, 0 }, { 65, 0 }, { 65, 0 }, { 65, 0 }, { -3, 3 }, { -3, 4 } } ) );
    // repeat 18 across the border: 258 .. 269 and the distances 0 1 2 are 0; the distances 3 4 have a bit
    v.push_back( handBlock( "repeat 18 across the border", 270, 5, zeros( 65 ) + A1 + zeros( 190 ) + A2 + A2 + Ops{ { 18, 4 } } + A1 + A1,
                            { { 65, 0 }, { 65, 0 }, { 65, 0 }, { 65, 0 }, { 65, 0 }, { -3, 4 }, { -3, 5 } } ) );
    // the block that is its end code alone: ONE literal/length code of length 1
    v.push_back( handBlock( "the end code alone", 257, 1, zeros( 256 ) + A1 + Ops{ { 0, 0 } }, { } ) );
    size_t nAccepted = 0;
    for( const Hand& h : v )
    {
        if( sameAsZlib( h.sName, h.sDeflate, false ) )
            return 1;
        nAccepted += zlibStrict( h.sDeflate ).bOk ? 1 : 0;
    }
    if( !zlibStrict( v[ 0 ].sDeflate ).bOk || zlibStrict( v[ 0 ].sDeflate ).sOut != "AAAA" || nAccepted + 1 < v.size( ) )
        return fail( "zlib refuses the hand-made streams: the test assembles them wrongly" );
    // the same sets with the unused code met: refused by both
    {
        const std::vector<int> vLit = [ & ] {
            std::vector<int> x( 258, 0 );
            x[ 65 ] = 1, x[ 256 ] = 2, x[ 257 ] = 2;
            return x;
        }( );
        BitWriter w;
        dynamicHeader( w, true, 258, 1, zeros( 65 ) + A1 + zeros( 190 ) + A2 + A2 + A1 );
        const BlockCodes xCodes( vLit, { 1 } );
        xCodes.symbol( w, 65 );
        xCodes.symbol( w, 257 );
        w.put( 1, 1 ); // the other 1-bit distance pattern: no code
        xCodes.symbol( w, 256 );
        const Bytes s = w.done( );
        if( zlibStrict( s ).bOk || sameAsZlib( "the unused pattern of a one-code distance set", s, false ) )
            return fail( "the unused pattern of a one-code distance set" );
    }
    printf( "handmade ok: %zu streams, %zu accepted\n", v.size( ) + 1, nAccepted );
    return 0;
}

static int mutants( uint64_t uiSeed, size_t n )
{
    Rng r( uiSeed );
    const Bytes sText = fastq( r, 9000 );
    for( int iKind = 0; iKind < N_KINDS; iKind++ )
    {
        const Bytes sDeflate = deflateKind( sText, iKind );
        size_t nAcceptedA = 0, nAcceptedB = 0;
        for( size_t k = 0; k < 2 * n; k++ )
        {
            const bool bFamilyB = k >= n;
            Bytes sMutant = sDeflate;
            const size_t uiBit = pick( r, 8 * sMutant.size( ) );
            sMutant[ uiBit / 8 ] = (char)( sMutant[ uiBit / 8 ] ^ ( 1 << ( uiBit % 8 ) ) );
            const Decoded z = zlibStrict( sMutant );
            uint32_t uiCrc = zcrc( sText ), uiIsize = (uint32_t)sText.size( );
            if( bFamilyB && z.bOk )
                uiCrc = zcrc( z.sOut ), uiIsize = (uint32_t)z.sOut.size( );
            const bool bWant = z.bOk && z.sOut.size( ) == uiIsize && zcrc( z.sOut ) == uiCrc;
            const Hosted h = oursStream( member( sMutant, uiCrc, uiIsize ) );
            const std::string sWhat = std::string( aKindName[ iKind ] ) + " family " + ( bFamilyB ? "B" : "A" ) + " bit " + std::to_string( uiBit );
            if( h.bOk != bWant )
                return fail( sWhat + ": the yardstick " + ( bWant ? "accepts" : "refuses" ) + ", inflateHost says '" + h.sMessage + "'" );
            if( h.bOk && h.sOut != z.sOut )
                return fail( sWhat + ": accepted with other bytes" );
            ( bFamilyB ? nAcceptedB : nAcceptedA ) += h.bOk ? 1 : 0;
        }
        printf( "%s: A %zu of %zu accepted, B %zu of %zu accepted\n", aKindName[ iKind ], nAcceptedA, n, nAcceptedB, n );
        if( 3 * nAcceptedB < n )
            return fail( std::string( aKindName[ iKind ] ) + ": fewer than a third of family B accepted" );
    }
    printf( "mutants ok: %zu per family and kind, %d kinds, 0 different\n", n, (int)N_KINDS );
    return 0;
}

static int reasons( bool bPrint )
{
    Rng r( 7 );
    const Bytes sText = fastq( r, 500 ), sGood = memberOfText( sText ), sDeflate = deflateRaw( sText, Z_DEFAULT_COMPRESSION, Z_DEFAULT_STRATEGY );
    const uint32_t uiCrc = zcrc( sText ), uiIsize = (uint32_t)sText.size( );
    const BlockCodes xFixed = fixedCodes( );
    auto fixedStart = [ & ]( BitWriter& w ) {
        w.put( 1, 1 );
        w.put( 1, 2 );
    };
    auto dynamic = [ & ]( size_t nLit, size_t nDist, const Ops& vOps, const std::vector<int>& vForced = { } ) {
        BitWriter w;
        dynamicHeader( w, true, nLit, nDist, vOps, vForced );
        w.put( 0, 16 );
        return w.done( );
    };
    const Ops A1 = { { 1, 0 } }, A2 = { { 2, 0 } };
    struct Case
    {
        uint32_t uiReason;
        Bytes sMember;
    };
    std::vector<Case> v;
    {
        // plain gzip: what gzip.compress writes
        Bytes s( "\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff", 10 );
        s += sDeflate;
        le( s, uiCrc, 4 );
        le( s, uiIsize, 4 );
        v.push_back( { ma_bgzf::ERR_NOT_BGZF, s } );
    }
    v.push_back( { ma_bgzf::ERR_TRUNCATED, sGood.substr( 0, sGood.size( ) - 1 ) } );
    v.push_back( { ma_bgzf::ERR_ISIZE, member( sDeflate, uiCrc, 65537 ) } );
    v.push_back( { ma_bgzf::ERR_BTYPE, member( Bytes( "\x07", 1 ), 0, 0 ) } );
    v.push_back( { ma_bgzf::ERR_STORED_LEN, member( Bytes( "\x01\x01\x00\x00\x00" "A", 6 ), zcrc( "A" ), 1 ) } );
    v.push_back( { ma_bgzf::ERR_SYMBOL_COUNT, member( dynamic( 287, 1, A1 + A1 ), 0, 0 ) } );
    v.push_back( { ma_bgzf::ERR_CODELEN_SET, member( dynamic( 257, 1, A1 + A1, std::vector<int>( 19, 1 ) ), 0, 0 ) } );
    v.push_back( { ma_bgzf::ERR_REPEAT_FIRST, member( dynamic( 257, 1, Ops{ { 16, 0 }, { 0, 0 } } ), 0, 0 ) } );
    v.push_back( { ma_bgzf::ERR_REPEAT_OVER, member( dynamic( 257, 1, Ops{ { 18, 127 }, { 18, 127 }, { 0, 0 } } ), 0, 0 ) } );
    v.push_back( { ma_bgzf::ERR_NO_EOB, member( dynamic( 257, 1, A1 + A1 + zeros( 256 ) ), 0, 0 ) } );
    v.push_back( { ma_bgzf::ERR_LITLEN_SET, member( dynamic( 257, 1, zeros( 65 ) + A1 + zeros( 190 ) + A2 + Ops{ { 0, 0 } } ), 0, 0 ) } );
    v.push_back( { ma_bgzf::ERR_DIST_SET, member( dynamic( 258, 2, zeros( 65 ) + A1 + zeros( 190 ) + A2 + A2 + A2 + A2 ), 0, 0 ) } );
    {
        BitWriter w;
        fixedStart( w );
        xFixed.symbol( w, 286 );
        xFixed.symbol( w, 256 );
        v.push_back( { ma_bgzf::ERR_LITLEN_CODE, member( w.done( ), 0, 0 ) } );
    }
    {
        BitWriter w;
        fixedStart( w );
        xFixed.symbol( w, 'A' );
        xFixed.symbol( w, 257 );
        w.code( 30, 5 );
        xFixed.symbol( w, 256 );
        v.push_back( { ma_bgzf::ERR_DIST_CODE, member( w.done( ), zcrc( "AAAA" ), 4 ) } );
    }
    {
        BitWriter w;
        fixedStart( w );
        xFixed.symbol( w, 'A' );
        xFixed.match( w, 3, 2 );
        xFixed.symbol( w, 256 );
        v.push_back( { ma_bgzf::ERR_DIST_FAR, member( w.done( ), zcrc( "AAAA" ), 4 ) } );
    }
    {
        BitWriter w;
        fixedStart( w );
        xFixed.symbol( w, 'A' ); // (and no end code: five bits of padding are all that is left)
        v.push_back( { ma_bgzf::ERR_INPUT_END, member( w.done( ), zcrc( "A" ), 1 ) } );
    }
    v.push_back( { ma_bgzf::ERR_TRAILING, member( sDeflate + Bytes( 1, '\0' ), uiCrc, uiIsize ) } );
    v.push_back( { ma_bgzf::ERR_LENGTH, member( sDeflate, uiCrc, uiIsize + 1 ) } );
    v.push_back( { ma_bgzf::ERR_CRC, member( sDeflate, uiCrc ^ 1u, uiIsize ) } );
    if( v.size( ) + 1 != ma_bgzf::N_REASONS )
        return fail( "not one stream per reason" );
    for( size_t i = 0; i < v.size( ); i++ )
    {
        if( v[ i ].uiReason != i + 1 )
            return fail( "the reasons are out of order" );
        // a good member in front, one behind (unless the walk cannot get there): member 1, the byte behind the good one
        const bool bHeader = v[ i ].uiReason <= ma_bgzf::ERR_ISIZE;
        const Hosted h = oursStream( sGood + v[ i ].sMember + ( bHeader ? Bytes( ) : sGood ) );
        const std::string sWant =
            "ma_batch_set_reads_bgzf: member 1 (byte " + std::to_string( sGood.size( ) ) + "): " + ma_bgzf::errorText( v[ i ].uiReason );
        if( h.bOk || h.sMessage != sWant )
            return fail( "reason " + std::to_string( i + 1 ) + ": wanted '" + sWant + "', got '" + ( h.bOk ? "accepted" : h.sMessage ) + "'" );
        if( std::string( ma_bgzf::errorText( v[ i ].uiReason ) ) == "no error" )
            return fail( "a reason without a text" );
        if( bPrint ) // (for tests/test_gpu_bgzf.py: the stream in hex, the message)
            for( unsigned char c : sGood + v[ i ].sMember + ( bHeader ? Bytes( ) : sGood ) )
                printf( "%02x", c );
        printf( "%s%s\n", bPrint ? " " : "", h.sMessage.c_str( ) );
    }
    if( bPrint )
        return 0;
    if( std::string( ma_bgzf::errorText( ma_bgzf::ERR_NOT_BGZF ) ).find( "a gzip member without the BGZF size field: single-member gzip stays with GzFileStream" ) ==
        std::string::npos )
        return fail( "the plain-gzip reason does not name GzFileStream" );
    // of several violations the lowest member is named; a bad header wins over any stream (nothing is inflated then)
    {
        const Bytes sBadCrc = member( sDeflate, uiCrc ^ 1u, uiIsize ), sBadLen = member( sDeflate, uiCrc, uiIsize + 1 );
        const Hosted a = oursStream( sGood + sBadLen + sBadCrc ), b = oursStream( sGood + sBadCrc + sBadLen ),
                     c = oursStream( sBadCrc + sGood.substr( 0, 20 ) );
        if( a.bOk || a.xResult.uiMember != 1 || a.xResult.uiReason != ma_bgzf::ERR_LENGTH || b.bOk || b.xResult.uiMember != 1 ||
            b.xResult.uiReason != ma_bgzf::ERR_CRC || c.bOk || c.xResult.uiMember != 1 || c.xResult.uiReason != ma_bgzf::ERR_TRUNCATED ||
            c.xResult.uiByte != sBadCrc.size( ) )
            return fail( "of several violations not the expected one is named" );
    }
    printf( "reasons ok: %zu streams\n", v.size( ) );
    return 0;
}

static int crc( uint64_t uiSeed )
{
    Rng r( uiSeed );
    static const size_t aSizes[] = { 0, 1, 2, 63, 64, 65, 127, 4097, 65535, 65536 };
    for( size_t uiSize : aSizes )
    {
        Bytes s( uiSize, '\0' );
        for( char& c : s )
            c = (char)pick( r, 256 );
        std::unique_ptr<uint8_t[]> p( new uint8_t[ uiSize ] );
        memcpy( p.get( ), s.data( ), uiSize );
        if( ma_bgzf::crcOf( p.get( ), uiSize ) != zcrc( s ) )
            return fail( "crcOf of " + std::to_string( uiSize ) + " bytes" );
        const size_t uiSplit = uiSize ? pick( r, uiSize + 1 ) : 0;
        if( ma_bgzf::crcCombine( zcrc( s.substr( 0, uiSplit ) ), zcrc( s.substr( uiSplit ) ), uiSize - uiSplit ) != zcrc( s ) )
            return fail( "crcCombine at " + std::to_string( uiSplit ) + " of " + std::to_string( uiSize ) + " bytes" );
        // k_bgzf_crc's fold: 64 stretches, six steps
        uint32_t aCrc[ 64 ], aLen[ 64 ];
        const uint32_t uiStretch = (uint32_t)( uiSize + 63 ) / 64;
        for( uint32_t l = 0; l < 64; l++ )
        {
            const uint32_t uiFrom = std::min<uint32_t>( l * uiStretch, (uint32_t)uiSize ), uiTo = std::min<uint32_t>( uiFrom + uiStretch, (uint32_t)uiSize );
            aCrc[ l ] = ma_bgzf::crcOf( p.get( ) + uiFrom, uiTo - uiFrom );
            aLen[ l ] = uiTo - uiFrom;
        }
        for( uint32_t uiStep = 1; uiStep < 64; uiStep <<= 1 )
            for( uint32_t l = 0; l < 64; l += 2 * uiStep )
            {
                aCrc[ l ] = ma_bgzf::crcCombine( aCrc[ l ], aCrc[ l + uiStep ], aLen[ l + uiStep ] );
                aLen[ l ] += aLen[ l + uiStep ];
            }
        if( aCrc[ 0 ] != zcrc( s ) || aLen[ 0 ] != uiSize )
            return fail( "the 64-lane fold of " + std::to_string( uiSize ) + " bytes" );
    }
    printf( "crc ok\n" );
    return 0;
}

// ---- BatchBgzfReader ----------------------------------------------------------------------------------------------------------------
static Bytes bgzfOf( const Bytes& sText, size_t uiMemberText, bool bEmptyInside )
{
    Bytes s;
    for( size_t uiAt = 0, k = 0; uiAt < sText.size( ); uiAt += uiMemberText, k++ )
    {
        s += memberOfText( sText.substr( uiAt, uiMemberText ) );
        if( bEmptyInside && k % 5 == 2 )
            s += endMarker( );
    }
    return s + endMarker( );
}
static int readOne( const std::string& sWhat, const Bytes& sText, const Bytes& sFile, size_t uiChunk )
{
    BatchBgzfReader xReader{ ParameterSetManager( ) };
    xReader.uiBatchBytes = uiChunk;
    auto pStream = std::make_shared<StringStream>( sFile );
    Bytes sAll;
    size_t uiBatches = 0;
    while( auto pBatch = xReader.execute( pStream ) )
    {
        const Bytes sBatch = BatchBgzfReader::textOf( *pBatch );
        if( sBatch.empty( ) || sBatch[ 0 ] != sText[ 0 ] || ( !sAll.empty( ) && sAll.back( ) != '\n' ) )
            return fail( sWhat + ": batch " + std::to_string( uiBatches ) + " does not start at a record" );
        if( sText.compare( sAll.size( ), sBatch.size( ), sBatch ) != 0 )
            return fail( sWhat + ": batch " + std::to_string( uiBatches ) + " is not the file's next text" );
        // a record start: for FASTQ the next-but-one line starts with '+'
        if( sText[ 0 ] == '@' )
        {
            const size_t a = sBatch.find( '\n' ), b = a == Bytes::npos ? a : sBatch.find( '\n', a + 1 );
            if( b == Bytes::npos || b + 1 >= sBatch.size( ) || sBatch[ b + 1 ] != '+' )
                return fail( sWhat + ": batch " + std::to_string( uiBatches ) + " starts at an '@' that is no header" );
        }
        sAll += sBatch;
        uiBatches++;
        if( uiBatches > sText.size( ) )
            return fail( sWhat + ": the reader does not end" );
    }
    if( sAll != sText )
        return fail( sWhat + ": the batches do not concatenate to the file" );
    printf( "%s: %zu batches\n", sWhat.c_str( ), uiBatches );
    return 0;
}
static int reader( size_t uiChunk, const std::string& sFastq )
{
    Rng r( 20261020 );
    const Bytes sText = slurp( sFastq );
    Bytes sFasta; // records longer than a member
    for( int k = 0; k < 9; k++ )
    {
        sFasta += ">long" + std::to_string( k ) + " record\n";
        for( size_t n = 700 + pick( r, 900 ), i = 0; i < n; i += 60 )
            sFasta += Bytes( std::min<size_t>( 60, n - i ), "ACGT"[ pick( r, 4 ) ] ) + "\n";
    }
    static const size_t aMemberText[] = { 1, 7, 300, 65280 };
    for( size_t uiMemberText : aMemberText )
    {
        const std::string sTag = " at " + std::to_string( uiMemberText ) + " bytes per member";
        if( readOne( "fastq" + sTag, sText, bgzfOf( sText, uiMemberText, uiMemberText == 7 ), uiChunk ) ||
            readOne( "fasta" + sTag, sFasta, bgzfOf( sFasta, uiMemberText, uiMemberText == 300 ), uiChunk ) )
            return 1;
    }
    // plain gzip: the reader throws and names the stream that serves it
    {
        Bytes s( "\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff", 10 );
        s += deflateRaw( sText, Z_DEFAULT_COMPRESSION, Z_DEFAULT_STRATEGY );
        le( s, zcrc( sText ), 4 );
        le( s, (uint32_t)sText.size( ), 4 );
        try
        {
            BatchBgzfReader xReader{ ParameterSetManager( ) };
            xReader.uiBatchBytes = uiChunk;
            xReader.execute( std::make_shared<StringStream>( s ) );
            return fail( "a plain gzip stream was read" );
        }
        catch( const std::runtime_error& rE )
        {
            if( std::string( rE.what( ) ).find( "GzFileStream" ) == std::string::npos )
                return fail( std::string( "'" ) + rE.what( ) + "' does not name GzFileStream" );
        }
    }
    // a file that ends inside a member is refused
    try
    {
        const Bytes sFile = bgzfOf( sText, 300, false );
        BatchBgzfReader xReader{ ParameterSetManager( ) };
        xReader.uiBatchBytes = uiChunk;
        auto pStream = std::make_shared<StringStream>( sFile.substr( 0, sFile.size( ) - 31 ) );
        while( xReader.execute( pStream ) )
            ;
        return fail( "a truncated file was read to its end" );
    }
    catch( const std::runtime_error& rE )
    {
        if( std::string( rE.what( ) ).find( "truncated" ) == std::string::npos )
            return fail( std::string( "'" ) + rE.what( ) + "' does not say truncated" );
    }
    printf( "reader ok: chunk %zu\n", uiChunk );
    return 0;
}

int main( int argc, char** argv )
{
    try
    {
        const std::string sMode = argc > 1 ? argv[ 1 ] : "";
        if( sMode == "kinds" && argc > 2 )
            return kinds( strtoull( argv[ 2 ], nullptr, 10 ) );
        if( sMode == "handmade" )
            return handmade( );
        if( sMode == "mutants" && argc > 3 )
            return mutants( strtoull( argv[ 2 ], nullptr, 10 ), (size_t)atol( argv[ 3 ] ) );
        if( sMode == "reasons" )
            return reasons( argc > 2 && std::string( argv[ 2 ] ) == "print" );
        if( sMode == "crc" && argc > 2 )
            return crc( strtoull( argv[ 2 ], nullptr, 10 ) );
        if( sMode == "reader" && argc > 3 )
            return reader( (size_t)atol( argv[ 2 ] ), argv[ 3 ] );
        fprintf( stderr, "usage: bgzf_dev_test kinds <seed> | handmade | mutants <seed> <n> | reasons [print] | crc <seed> | reader <bytes> <fq>\n" );
        return 2;
    }
    catch( const std::exception& rE )
    {
        printf( "EXCEPTION %s\n", rE.what( ) );
        return 3;
    }
}
