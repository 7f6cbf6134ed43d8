// CPU-only checks of the rules of ma_batch_set_mates_bgzf (ma_amd/host/ma_mates_bgzf_dev.h: ma_bgzf::pairBgzfHost, the serial
// statement the kernels are compared with) against zlib, which writes the members here (<zlib.h>: not the code under test),
// ma_text::pairHost on the uncompressed texts, PairedFileReader of ma_amd/host/ma_sam.h over in-memory streams and the
// reference's own reader output (tests/golden/reader/mates.*).
//   mates_bgzf_test golden <dir>        mates_1.fq / mates_2.fq as members of 40 text bytes, rev_comp 0 and 1: mates.rc0.ref / rc1.ref
//   mates_bgzf_test random <seed> <n>   seeded text pairs cut into members anywhere, with heads and drops: pairHost's result
//   mates_bgzf_test reasons [print]     the refusals: wording and precedence (print: hex of both sides' members + message per line)
//   mates_bgzf_test reader <target>     BatchPairedBgzfReader over in-memory BGZF streams, the rests handed back by pairBgzfHost: the
//                                       pairs are PairedFileReader's, the carry stays bounded, an abandoned batch blocks nobody
// Every buffer handed to pairBgzfHost holds exactly its bytes, so that an AddressSanitizer build of this program sees any byte
// touched outside of them.
#include "ma_batch_nodes.h"
#include "ma_mates_bgzf_dev.h"
#include <fstream>
#include <future>
#include <random>
#include <zlib.h>

using namespace libMA;

struct Read
{
    std::string sName;
    std::vector<uint8_t> vCodes, vQual;
    bool operator==( const Read& o ) const
    {
        return sName == o.sName && vCodes == o.vCodes && vQual == o.vQual;
    }
};
typedef std::mt19937_64 Rng;
static size_t pick( Rng& r, size_t n )
{
    return (size_t)( r( ) % n );
}

// ---- BGZF written with zlib -----------------------------------------------------------------------------------------------------
static std::string wrap( const std::string& sStream, uint32_t uiCrc, uint32_t uiIsize )
{
    std::string s( "\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0", 16 );
    const uint32_t uiBsize = (uint32_t)sStream.size( ) + 25;
    s += (char)( uiBsize & 0xff );
    s += (char)( uiBsize >> 8 );
    s += sStream;
    for( uint32_t v : { uiCrc, uiIsize } )
        for( int k = 0; k < 4; k++ )
            s += (char)( ( v >> ( 8 * k ) ) & 0xff );
    return s;
}
static std::string deflated( const std::string& sText, int iKind ) // stored, fixed, dynamic, Huffman only, RLE
{
    static const int aLevel[] = { 0, 6, 6, 6, 6 }, aStrategy[] = { Z_DEFAULT_STRATEGY, Z_FIXED, Z_DEFAULT_STRATEGY, Z_HUFFMAN_ONLY, Z_RLE };
    z_stream z;
    memset( &z, 0, sizeof( z ) );
    if( deflateInit2( &z, aLevel[ iKind % 5 ], Z_DEFLATED, -15, 9, aStrategy[ iKind % 5 ] ) != Z_OK )
        throw std::runtime_error( "deflateInit2" );
    std::string sOut( deflateBound( &z, sText.size( ) ) + 64, '\0' );
    z.next_in = (Bytef*)sText.data( ), z.avail_in = (uInt)sText.size( );
    z.next_out = (Bytef*)&sOut[ 0 ], z.avail_out = (uInt)sOut.size( );
    if( deflate( &z, Z_FINISH ) != Z_STREAM_END )
        throw std::runtime_error( "deflate" );
    sOut.resize( z.total_out );
    deflateEnd( &z );
    return sOut;
}
static std::string member( const std::string& sText, int iKind = 2 )
{
    return wrap( deflated( sText, iKind ), (uint32_t)crc32( crc32( 0, nullptr, 0 ), (const Bytef*)sText.data( ), (uInt)sText.size( ) ), (uint32_t)sText.size( ) );
}
// the members of sText cut at the offsets given (an offset twice: an empty member), every kind in turn
static std::string members( const std::string& sText, std::vector<size_t> vCuts, int iFirstKind = 0 )
{
    std::sort( vCuts.begin( ), vCuts.end( ) );
    vCuts.push_back( sText.size( ) );
    std::string s;
    size_t uiFrom = 0;
    int iKind = iFirstKind;
    for( size_t uiTo : vCuts )
    {
        s += member( sText.substr( uiFrom, uiTo - uiFrom ), iKind++ );
        uiFrom = uiTo;
    }
    return s;
}

// ---- the two statements ---------------------------------------------------------------------------------------------------------
struct Paired
{
    bool bAccepted = false;
    std::string sMessage;
    ma_text::PairResult xResult;
    uint64_t aTextBytes[ 2 ] = { 0, 0 };
    std::string aText[ 2 ]; // pairBgzfHost: T_1, T_2
    std::vector<Read> vReads;
};
static std::unique_ptr<char[]> exactCopy( const std::string& s )
{
    std::unique_ptr<char[]> p( new char[ std::max<size_t>( s.size( ), 1 ) ] );
    memcpy( p.get( ), s.data( ), s.size( ) );
    return p;
}
static void readsOf( Paired& p, const uint64_t* pOff, const uint8_t* pCodes, const uint64_t* pNameOff, const char* pNames, const uint8_t* pQual )
{
    for( uint64_t i = 0; i < 2 * p.xResult.uiPairs; i++ )
    {
        Read x;
        x.sName.assign( pNames + pNameOff[ i ], pNameOff[ i + 1 ] - pNameOff[ i ] );
        x.vCodes.assign( pCodes + pOff[ i ], pCodes + pOff[ i + 1 ] );
        if( p.xResult.iHasQual )
            x.vQual.assign( pQual + pOff[ i ], pQual + pOff[ i + 1 ] );
        p.vReads.push_back( std::move( x ) );
    }
}
struct SideBytes
{
    std::string sHead, sMembers;
    uint64_t uiDrop = 0;
};
static Paired hostBgzf( const SideBytes aIn[ 2 ], bool bRev )
{
    Paired p;
    const auto pH0 = exactCopy( aIn[ 0 ].sHead ), pM0 = exactCopy( aIn[ 0 ].sMembers ), pH1 = exactCopy( aIn[ 1 ].sHead ), pM1 = exactCopy( aIn[ 1 ].sMembers );
    const ma_bgzf::PairSide aSide[ 2 ] = { { pH0.get( ), aIn[ 0 ].sHead.size( ), (const uint8_t*)pM0.get( ), aIn[ 0 ].sMembers.size( ), aIn[ 0 ].uiDrop },
                                           { pH1.get( ), aIn[ 1 ].sHead.size( ), (const uint8_t*)pM1.get( ), aIn[ 1 ].sMembers.size( ), aIn[ 1 ].uiDrop } };
    ma_bgzf::PairBgzfResult r;
    char* apText[ 2 ];
    if( ma_bgzf::pairBgzfHost( aSide, bRev, apText, nullptr, nullptr, nullptr, nullptr, nullptr, &r ) )
    {
        char aMessage[ 320 ];
        ma_bgzf::messagePair( aMessage, sizeof( aMessage ), r );
        p.sMessage = aMessage;
        p.xResult = r.xPair;
        if( apText[ 0 ] || apText[ 1 ] || r.xPair.uiPairs || r.xPair.aConsumed[ 0 ] || r.xPair.aConsumed[ 1 ] || r.aTextBytes[ 0 ] || r.aTextBytes[ 1 ] )
            throw std::runtime_error( "pairBgzfHost: a refusal with texts, pairs, consumed or text bytes" );
        return p;
    }
    free( apText[ 0 ] );
    free( apText[ 1 ] );
    p.xResult = r.xPair;
    const uint64_t n = 2 * r.xPair.uiPairs;
    std::unique_ptr<uint64_t[]> pOff( new uint64_t[ n + 1 ] ), pNameOff( new uint64_t[ n + 1 ] );
    std::unique_ptr<uint8_t[]> pCodes( new uint8_t[ r.xPair.uiBases ] ), pQual( new uint8_t[ r.xPair.iHasQual ? r.xPair.uiBases : 0 ] );
    std::unique_ptr<char[]> pNames( new char[ r.xPair.uiNameBytes ] );
    ma_bgzf::PairBgzfResult xAgain;
    if( ma_bgzf::pairBgzfHost( aSide, bRev, apText, pOff.get( ), pCodes.get( ), pNameOff.get( ), pNames.get( ), r.xPair.iHasQual ? pQual.get( ) : nullptr,
                               &xAgain ) ||
        xAgain.xPair.uiPairs != r.xPair.uiPairs || xAgain.xPair.uiBases != r.xPair.uiBases || xAgain.aTextBytes[ 1 ] != r.aTextBytes[ 1 ] )
        throw std::runtime_error( "pairBgzfHost: the second pass disagrees with the first" );
    for( int i = 0; i < 2; i++ )
    {
        p.aTextBytes[ i ] = r.aTextBytes[ i ];
        p.aText[ i ].assign( apText[ i ], r.aTextBytes[ i ] );
        free( apText[ i ] );
    }
    readsOf( p, pOff.get( ), pCodes.get( ), pNameOff.get( ), pNames.get( ), pQual.get( ) );
    p.bAccepted = true;
    return p;
}
static Paired hostText( const std::string& s1, const std::string& s2, bool bRev )
{
    Paired p;
    const auto p1 = exactCopy( s1 ), p2 = exactCopy( s2 );
    if( ma_text::pairHost( p1.get( ), s1.size( ), p2.get( ), s2.size( ), bRev, nullptr, nullptr, nullptr, nullptr, nullptr, &p.xResult ) )
    {
        char aMessage[ 320 ];
        const ma_text::PairResult& r = p.xResult;
        ma_text::messageMatesOf( aMessage, sizeof( aMessage ), "ma_batch_set_mates_bgzf", r.uiRefusal, r.uiText, r.uiLine, r.uiByte, r.uiReason );
        p.sMessage = aMessage;
        return p;
    }
    const ma_text::PairResult r = p.xResult;
    const uint64_t n = 2 * r.uiPairs;
    std::unique_ptr<uint64_t[]> pOff( new uint64_t[ n + 1 ] ), pNameOff( new uint64_t[ n + 1 ] );
    std::unique_ptr<uint8_t[]> pCodes( new uint8_t[ r.uiBases ] ), pQual( new uint8_t[ r.iHasQual ? r.uiBases : 0 ] );
    std::unique_ptr<char[]> pNames( new char[ r.uiNameBytes ] );
    ma_text::PairResult xAgain;
    ma_text::pairHost( p1.get( ), s1.size( ), p2.get( ), s2.size( ), bRev, pOff.get( ), pCodes.get( ), pNameOff.get( ), pNames.get( ),
                       r.iHasQual ? pQual.get( ) : nullptr, &xAgain );
    readsOf( p, pOff.get( ), pCodes.get( ), pNameOff.get( ), pNames.get( ), pQual.get( ) );
    p.aText[ 0 ] = s1, p.aText[ 1 ] = s2;
    p.bAccepted = true;
    return p;
}
// PairedFileReader of ma_sam.h over two in-memory streams
static std::vector<Read> yardstick( const std::string& s1, const std::string& s2, bool bRev )
{
    ParameterSetManager xParameters;
    xParameters.bRevCompPairedReadMates = bRev;
    PairedFileReader xReader( xParameters );
    auto pStreams = std::make_shared<PairedFileStream>( std::make_shared<StringStream>( s1 ), std::make_shared<StringStream>( s2 ) );
    std::vector<Read> v;
    while( auto pPair = xReader.execute( pStreams ) )
        for( auto& pQ : *pPair )
            v.push_back( Read{ pQ->sName, pQ->xCodes, pQ->xQuality } );
    return v;
}
static std::string slurp( const std::string& sPath )
{
    std::ifstream xIn( sPath, std::ios::binary );
    if( !xIn )
        throw std::runtime_error( "cannot read " + sPath );
    std::stringstream xAll;
    xAll << xIn.rdbuf( );
    return xAll.str( );
}

// ---- golden ---------------------------------------------------------------------------------------------------------------------
static std::vector<Read> refDump( const std::string& sPath )
{
    std::vector<Read> v;
    std::ifstream xIn( sPath );
    std::string sLine;
    while( std::getline( xIn, sLine ) )
    {
        std::istringstream xL( sLine );
        std::string sName, sCodes, sQual;
        size_t n = 0;
        xL >> sName >> n >> sCodes >> sQual;
        Read x;
        x.sName = sName;
        for( char c : sCodes )
            x.vCodes.push_back( (uint8_t)( c - '0' ) );
        x.vQual.assign( sQual.begin( ), sQual.end( ) );
        if( x.vCodes.size( ) != n )
            throw std::runtime_error( "bad line in " + sPath );
        v.push_back( x );
    }
    return v;
}
static std::vector<size_t> every( size_t uiStep, size_t n )
{
    std::vector<size_t> v;
    for( size_t a = uiStep; a < n; a += uiStep )
        v.push_back( a );
    return v;
}
static int golden( const std::string& sDir )
{
    const std::string s1 = slurp( sDir + "/mates_1.fq" ), s2 = slurp( sDir + "/mates_2.fq" );
    SideBytes aIn[ 2 ];
    aIn[ 0 ].sMembers = members( s1, every( 40, s1.size( ) ) ), aIn[ 1 ].sMembers = members( s2, every( 40, s2.size( ) ), 3 );
    size_t uiReads = 0;
    for( int iRev = 0; iRev < 2; iRev++ )
    {
        const Paired h = hostBgzf( aIn, iRev != 0 );
        const std::vector<Read> vRef = refDump( sDir + ( iRev ? "/mates.rc1.ref" : "/mates.rc0.ref" ) );
        if( !h.bAccepted || vRef.empty( ) || h.vReads != vRef )
            return printf( "FAIL rev_comp %d: %s\n", iRev, h.bAccepted ? "differs from the reference's dump" : h.sMessage.c_str( ) ), 1;
        if( h.vReads != yardstick( s1, s2, iRev != 0 ) || h.aText[ 0 ] != s1 || h.aText[ 1 ] != s2 )
            return printf( "FAIL rev_comp %d: differs from PairedFileReader, or the texts are not the files\n", iRev ), 1;
        uiReads += h.vReads.size( );
    }
    printf( "golden ok: %zu reads equal\n", uiReads );
    return 0;
}

// ---- random ---------------------------------------------------------------------------------------------------------------------
static std::string record( Rng& r, bool bFastq, const std::string& sName, size_t n, const std::string& sEnd )
{
    static const char aLetters[] = "ACGTACGTACGTACGTNNRYKMSWBDHVUacgtn";
    std::string sBases, sQual;
    for( size_t i = 0; i < n; i++ )
    {
        sBases += aLetters[ pick( r, pick( r, 4 ) ? 16 : sizeof( aLetters ) - 1 ) ];
        sQual += (char)( 33 + pick( r, 94 ) );
    }
    const std::string sHeader = sName + ( pick( r, 3 ) == 0 ? " some description" : "" );
    if( bFastq )
        return "@" + sHeader + sEnd + sBases + sEnd + "+" + sEnd + sQual + sEnd;
    std::string s = ">" + sHeader + sEnd;
    for( size_t uiAt = 0; uiAt < n; ) // one to three lines
    {
        const size_t m = pick( r, 2 ) ? n - uiAt : 1 + pick( r, n - uiAt );
        s += sBases.substr( uiAt, m ) + sEnd;
        uiAt += m;
    }
    return s;
}
static std::string mateText( Rng& r, bool bFastq, size_t uiRecords, int iMate, const std::string& sEnd, bool bFinalEnd )
{
    std::string s;
    for( size_t k = 0; k < uiRecords; k++ )
        s += record( r, bFastq, "p" + std::to_string( k ) + "/" + std::to_string( iMate ), 1 + pick( r, 70 ), sEnd );
    if( !bFinalEnd && !s.empty( ) )
        s.resize( s.size( ) - sEnd.size( ) );
    return s;
}
// T as a head, members and a drop: the head 0 .. a few records long and cut anywhere (mid-line too); the members cut at random
// offsets, between "\r" and "\n" where there is one, with empty members; the drop 0, inside the last member, or across two
static SideBytes sideOf( Rng& r, const std::string& sText, size_t uiCase )
{
    SideBytes x;
    const size_t uiHead = pick( r, 3 ) == 0 ? 0 : pick( r, std::min<size_t>( sText.size( ), 300 ) + 1 );
    x.sHead = sText.substr( 0, uiHead );
    std::string sBody = sText.substr( uiHead );
    const size_t uiKind = uiCase % 3; // of the drop
    std::string sExtra;
    for( size_t i = 0, n = uiKind == 0 ? 0 : 1 + pick( r, 90 ); i < n; i++ )
        sExtra += "@ACGT\r\n+I>"[ pick( r, 11 ) ];
    const size_t uiBody = sBody.size( );
    sBody += sExtra;
    std::vector<size_t> vCuts;
    for( size_t i = 0, n = pick( r, 9 ); i < n && !sBody.empty( ); i++ )
        vCuts.push_back( pick( r, sBody.size( ) + 1 ) );
    for( size_t i = 0; i + 1 < sBody.size( ) && vCuts.size( ) < 12; i++ )
        if( sBody[ i ] == '\r' && sBody[ i + 1 ] == '\n' && pick( r, 8 ) == 0 )
            vCuts.push_back( i + 1 );
    if( pick( r, 3 ) == 0 && !vCuts.empty( ) )
        vCuts.push_back( vCuts[ 0 ] ); // an empty member
    if( uiKind == 2 && sExtra.size( ) >= 2 )
        vCuts.push_back( uiBody + sExtra.size( ) / 2 ); // the drop spans two members
    if( uiKind == 1 && !sExtra.empty( ) && uiBody > 0 )
        vCuts.erase( std::remove_if( vCuts.begin( ), vCuts.end( ), [ & ]( size_t c ) { return c >= uiBody; } ), vCuts.end( ) ); // inside the last one
    x.sMembers = sBody.empty( ) && pick( r, 2 ) ? std::string( ) : members( sBody, vCuts, (int)pick( r, 5 ) );
    x.uiDrop = sExtra.size( );
    return x;
}
static int randomPairs( uint64_t uiSeed, size_t n )
{
    Rng r( uiSeed );
    size_t uiReads = 0, uiUnequal = 0, uiRests = 0;
    for( size_t t = 0; t < n; t++ )
    {
        const bool bFastq = t % 2 == 0;
        const size_t uiRecords = t % 11 == 0 ? 0 : 1 + pick( r, 12 ), uiMore = t % 5 < 2 ? 0 : 1 + pick( r, 3 ); // 3 of 5 unequal
        const size_t uiRecords1 = uiRecords + ( t % 5 >= 2 && t % 2 == 0 ? uiMore : 0 ), uiRecords2 = uiRecords + ( t % 5 >= 2 && t % 2 == 1 ? uiMore : 0 );
        const std::string sEnd = pick( r, 2 ) ? "\n" : "\r\n";
        const std::string aT[ 2 ] = { mateText( r, bFastq, uiRecords1, 1, sEnd, pick( r, 3 ) != 0 ), mateText( r, bFastq, uiRecords2, 2, sEnd, pick( r, 3 ) != 0 ) };
        const SideBytes aIn[ 2 ] = { sideOf( r, aT[ 0 ], t ), sideOf( r, aT[ 1 ], t / 3 ) };
        for( int iRev = 0; iRev < 2; iRev++ )
        {
            const Paired h = hostBgzf( aIn, iRev != 0 ), w = hostText( aT[ 0 ], aT[ 1 ], iRev != 0 );
            if( !h.bAccepted || !w.bAccepted )
                return printf( "FAIL pair %zu refused: %s\n", t, ( h.bAccepted ? w : h ).sMessage.c_str( ) ), 1;
            const ma_text::PairResult &a = h.xResult, &e = w.xResult;
            if( h.vReads != w.vReads || a.uiPairs != e.uiPairs || a.uiBases != e.uiBases || a.uiNameBytes != e.uiNameBytes || a.uiMaxLen != e.uiMaxLen ||
                a.iHasQual != e.iHasQual || a.aConsumed[ 0 ] != e.aConsumed[ 0 ] || a.aConsumed[ 1 ] != e.aConsumed[ 1 ] )
                return printf( "FAIL pair %zu (rev_comp %d) differs from pairHost on the texts\n", t, iRev ), 1;
            if( h.vReads != yardstick( aT[ 0 ], aT[ 1 ], iRev != 0 ) || h.vReads.size( ) != 2 * std::min( uiRecords1, uiRecords2 ) )
                return printf( "FAIL pair %zu (rev_comp %d) differs from PairedFileReader\n", t, iRev ), 1;
            for( int i = 0; i < 2; i++ ) // the texts, their sizes, and so the rests T_i[ consumed_i .. )
                if( h.aText[ i ] != aT[ i ] || h.aTextBytes[ i ] != aT[ i ].size( ) || a.aConsumed[ i ] > aT[ i ].size( ) )
                    return printf( "FAIL pair %zu: text %d is not head + members - drop\n", t, i + 1 ), 1;
            uiRests += ( a.aConsumed[ 0 ] < aT[ 0 ].size( ) ) + ( a.aConsumed[ 1 ] < aT[ 1 ].size( ) );
            uiReads += h.vReads.size( );
        }
        uiUnequal += uiRecords1 != uiRecords2;
    }
    if( 5 * uiUnequal < 2 * n )
        return printf( "FAIL: only %zu of %zu text pairs have unequal counts\n", uiUnequal, n ), 1;
    printf( "random ok: %zu text pairs, %zu of unequal counts, %zu rests, %zu reads equal\n", n, uiUnequal, uiRests, uiReads );
    return 0;
}

// ---- reasons --------------------------------------------------------------------------------------------------------------------
struct Reason
{
    const char* sWhat;
    SideBytes aIn[ 2 ];
    std::string sWant; // behind "ma_batch_set_mates_bgzf: "
};
static SideBytes plain( const std::string& sMembers, uint64_t uiDrop = 0 )
{
    SideBytes x;
    x.sMembers = sMembers, x.uiDrop = uiDrop;
    return x;
}
static std::string badCrc( const std::string& sText )
{
    std::string s = member( sText );
    s[ s.size( ) - 8 ] ^= 4;
    return s;
}
static std::vector<Reason> reasonTable( )
{
    const std::string sGood = "@r\nACGT\n+\nIIII\n", sShortQual = "@r\nACGT\n+\nIII\n", sNoPlus = "@r\nACGT\nIIII\n@s\n", sFasta = ">r\nACGT\n";
    const std::string sQualLen = ma_text::errorText( ma_text::ERR_FQ_QUAL_LEN ), sPlus = ma_text::errorText( ma_text::ERR_FQ_PLUS );
    const std::string sCrc = ma_bgzf::errorText( ma_bgzf::ERR_CRC ), sNot = ma_bgzf::errorText( ma_bgzf::ERR_NOT_BGZF );
    const std::string sG = member( sGood ), sDrop = "n_drop is larger than the inflated part of the text";
    std::string sBadHeader = sG;
    sBadHeader[ 3 ] = 0; // FLG without FEXTRA
    const std::string s2 = std::to_string( sG.size( ) );
    return {
        // one per row of the refusal table (the null argument and the capacity are the library's)
        { "bad header in text 1", { plain( sG + sBadHeader ), plain( sG ) }, "text 1: member 1 (byte " + s2 + "): " + sNot },
        { "bad header in text 2", { plain( sG ), plain( sG + sG + sBadHeader ) }, "text 2: member 2 (byte " + std::to_string( 2 * sG.size( ) ) + "): " + sNot },
        { "CRC mismatch in text 1", { plain( sG + badCrc( sGood ) ), plain( sG + sG ) }, "text 1: member 1 (byte " + s2 + "): " + sCrc },
        { "CRC mismatch in text 2", { plain( sG ), plain( badCrc( sGood ) ) }, "text 2: member 0 (byte 0): " + sCrc },
        { "drop too large in text 1", { plain( sG, sGood.size( ) + 1 ), plain( sG ) }, "text 1: " + sDrop },
        { "drop too large in text 2", { plain( sG ), plain( sG, sGood.size( ) + 1 ) }, "text 2: " + sDrop },
        { "line violation in text 1", { plain( member( sShortQual ) ), plain( sG ) }, "text 1: line 4 (byte 10): " + sQualLen },
        { "line violation in text 2", { plain( sG ), plain( sG + member( sShortQual ) ) }, "text 2: line 8 (byte 25): " + sQualLen },
        { "text 1 of neither kind", { plain( member( "x" ) ), plain( member( sShortQual ) ) },
          std::string( "text 1: line 1 (byte 0): " ) + ma_text::errorText( ma_text::ERR_KIND ) },
        { "text 2 of neither kind", { plain( sG ), plain( member( "ACGT\n" ) ) }, std::string( "text 2: line 1 (byte 0): " ) + ma_text::errorText( ma_text::ERR_KIND ) },
        { "the kinds differ", { plain( sG ), plain( member( sFasta ) ) }, "the two texts differ in kind" },
        // precedence
        { "a bad header in text 2 wins over a CRC mismatch in text 1", { plain( badCrc( sGood ) ), plain( sG + sBadHeader ) },
          "text 2: member 1 (byte " + s2 + "): " + sNot },
        { "a CRC mismatch in text 2 wins over a line violation in text 1", { plain( member( sShortQual ) ), plain( sG + badCrc( sGood ) ) },
          "text 2: member 1 (byte " + s2 + "): " + sCrc },
        { "a CRC mismatch in text 2 wins over a drop too large in text 1", { plain( sG, 100 ), plain( badCrc( sGood ) ) }, "text 2: member 0 (byte 0): " + sCrc },
        { "a drop too large in text 2 wins over a line violation in text 1", { plain( member( sShortQual ) ), plain( sG, 100 ) }, "text 2: " + sDrop },
        { "bad headers in both: text 1 is named", { plain( sBadHeader ), plain( sBadHeader ) }, "text 1: member 0 (byte 0): " + sNot },
        { "CRC mismatches in both: text 1 is named", { plain( sG + sG + badCrc( sGood ) ), plain( badCrc( sGood ) ) },
          "text 1: member 2 (byte " + std::to_string( 2 * sG.size( ) ) + "): " + sCrc },
        { "line violations in both: text 1 is named", { plain( sG + member( sNoPlus ) ), plain( member( sShortQual ) ) }, "text 1: line 7 (byte 23): " + sPlus },
        { "a violation beyond the pairs", { plain( sG ), plain( sG + sG + sG + member( sNoPlus ) ) }, "text 2: line 15 (byte 53): " + sPlus },
        { "a violation wins over the kinds", { plain( member( sFasta ) ), plain( member( sShortQual ) ) }, "text 2: line 4 (byte 10): " + sQualLen },
    };
}
static int reasons( bool bPrint )
{
    for( const Reason& x : reasonTable( ) )
    {
        const std::string sWant = "ma_batch_set_mates_bgzf: " + x.sWant;
        if( bPrint ) // the table for the GPU test: both sides' members in hex, their drops, then the message
        {
            for( const SideBytes& s : x.aIn )
            {
                for( unsigned char c : s.sMembers )
                    printf( "%02x", c );
                printf( ":%llu ", (unsigned long long)s.uiDrop );
            }
            printf( "%s\n", sWant.c_str( ) );
            continue;
        }
        for( int iRev = 0; iRev < 2; iRev++ )
        {
            const Paired h = hostBgzf( x.aIn, iRev != 0 );
            if( h.bAccepted || h.sMessage != sWant )
                return printf( "FAIL %s: '%s', expected '%s'\n", x.sWhat, h.bAccepted ? "accepted" : h.sMessage.c_str( ), sWant.c_str( ) ), 1;
        }
    }
    ma_bgzf::PairBgzfResult xCapacity;
    memset( &xCapacity, 0, sizeof( xCapacity ) );
    xCapacity.uiRefusal = ma_bgzf::PAIR_TEXT, xCapacity.xPair.uiRefusal = ma_text::MATES_CAPACITY;
    char aCapacity[ 320 ];
    ma_bgzf::messagePair( aCapacity, sizeof( aCapacity ), xCapacity );
    if( std::string( aCapacity ) != "ma_batch_set_mates_bgzf: batch capacity exceeded" )
        return printf( "FAIL wording: %s\n", aCapacity ), 1;
    if( !bPrint )
        printf( "reasons ok: %zu cases\n", reasonTable( ).size( ) );
    return 0;
}

// ---- reader ---------------------------------------------------------------------------------------------------------------------
// uiRecords FASTQ records of uiBases bases each (names of one width: every record of a text is equally long)
static std::string fixedText( Rng& r, size_t uiRecords, size_t uiBases, int iMate )
{
    std::string s;
    char aName[ 32 ];
    for( size_t k = 0; k < uiRecords; k++ )
    {
        snprintf( aName, sizeof( aName ), "p%06zu/%d", k, iMate );
        std::string sBases, sQual;
        for( size_t i = 0; i < uiBases; i++ )
        {
            sBases += "ACGTN"[ pick( r, 50 ) ? pick( r, 4 ) : 4 ];
            sQual += (char)( 33 + pick( r, 94 ) );
        }
        s += "@" + std::string( aName ) + "\n" + sBases + "\n+\n" + sQual + "\n";
    }
    return s;
}
static std::string bgzfFile( const std::string& sText )
{
    std::vector<size_t> vCuts;
    for( size_t a = 700; a < sText.size( ); a += 700 )
        vCuts.push_back( a );
    return ( sText.empty( ) ? std::string( ) : members( sText, vCuts ) ) + member( "" ); // the end-of-file marker behind them
}
// BatchPairedBgzfReader over two in-memory BGZF streams, the rests computed by pairBgzfHost and handed back; *pPeak: the longest
// carried head
static int readerOne( Rng& r, size_t uiTarget, size_t uiPairs, size_t uiBases1, size_t uiBases2, size_t uiMore1, size_t uiMore2, size_t* pPeak )
{
    const std::string s1 = fixedText( r, uiPairs + uiMore1, uiBases1, 1 ), s2 = fixedText( r, uiPairs + uiMore2, uiBases2, 2 );
    const std::string sWhat = std::to_string( uiPairs ) + "+" + std::to_string( uiMore1 ) + "/+" + std::to_string( uiMore2 ) + " pairs of " +
                              std::to_string( uiBases1 ) + "/" + std::to_string( uiBases2 ) + " bases, target " + std::to_string( uiTarget );
    const size_t uiLongest = 2 * std::max( uiBases1, uiBases2 ) + 16, uiBound = uiTarget / 2 + 2 * 700 + uiLongest;
    BatchPairedBgzfReader xReader{ ParameterSetManager( ) };
    xReader.uiBatchBytes = uiTarget;
    auto pStreams = std::make_shared<PairedFileStream>( std::make_shared<StringStream>( bgzfFile( s1 ) ), std::make_shared<StringStream>( bgzfFile( s2 ) ) );
    std::vector<Read> vAll;
    size_t uiBatches = 0;
    while( auto pBatch = xReader.execute( pStreams ) )
    {
        SideBytes aIn[ 2 ];
        for( int i = 0; i < 2; i++ )
        {
            aIn[ i ].sHead = pBatch->asHead[ i ], aIn[ i ].sMembers = pBatch->asMembers[ i ], aIn[ i ].uiDrop = pBatch->auiDrop[ i ];
            if( aIn[ i ].sHead.size( ) > uiBound )
                return printf( "FAIL %s: batch %zu carries %zu bytes of stream %d, more than %zu\n", sWhat.c_str( ), uiBatches, aIn[ i ].sHead.size( ), i + 1, uiBound ), 1;
            *pPeak = std::max( *pPeak, aIn[ i ].sHead.size( ) );
        }
        const Paired h = hostBgzf( aIn, true );
        if( !h.bAccepted )
            return printf( "FAIL %s: batch %zu refused: %s\n", sWhat.c_str( ), uiBatches, h.sMessage.c_str( ) ), 1;
        vAll.insert( vAll.end( ), h.vReads.begin( ), h.vReads.end( ) );
        pBatch->handBack( h.aText[ 0 ].substr( h.xResult.aConsumed[ 0 ] ), h.aText[ 1 ].substr( h.xResult.aConsumed[ 1 ] ) );
        if( ++uiBatches > 100000 )
            return printf( "FAIL %s: the reader does not end\n", sWhat.c_str( ) ), 1;
    }
    if( xReader.execute( pStreams ) != nullptr )
        return printf( "FAIL %s: a batch behind the end\n", sWhat.c_str( ) ), 1;
    // the stream ends where the shorter file ends, and the pairs are PairedFileReader's over the uncompressed texts
    if( vAll.size( ) != 2 * uiPairs || vAll != yardstick( s1, s2, true ) )
        return printf( "FAIL %s: %zu reads in %zu batches differ from PairedFileReader's\n", sWhat.c_str( ), vAll.size( ), uiBatches ), 1;
    return 0;
}
static std::string plainGzip( const std::string& sText )
{
    z_stream z;
    memset( &z, 0, sizeof( z ) );
    if( deflateInit2( &z, 6, Z_DEFLATED, 31, 8, Z_DEFAULT_STRATEGY ) != Z_OK )
        throw std::runtime_error( "deflateInit2" );
    std::string sOut( deflateBound( &z, sText.size( ) ) + 64, '\0' );
    z.next_in = (Bytef*)sText.data( ), z.avail_in = (uInt)sText.size( );
    z.next_out = (Bytef*)&sOut[ 0 ], z.avail_out = (uInt)sOut.size( );
    if( deflate( &z, Z_FINISH ) != Z_STREAM_END )
        throw std::runtime_error( "deflate" );
    sOut.resize( z.total_out );
    deflateEnd( &z );
    return sOut;
}
static int reader( size_t uiTarget )
{
    Rng r( 20261020 );
    size_t uiRuns = 0, aPeak[ 2 ] = { 0, 0 };
    static const size_t aBases[ 3 ][ 2 ] = { { 65, 65 }, { 65, 215 }, { 215, 65 } }; // records of 150 / 150, 150 / 450 and 450 / 150 bytes
    for( size_t uiPairs : { 0, 1, 2, 37, 1000 } )
        for( int iLen = 0; iLen < 3; iLen++ )
            for( int iMore = 0; iMore < 3; iMore++, uiRuns++ ) // equal counts, file 1 three records longer, file 2 three records longer
            {
                size_t uiPeak = 0;
                if( readerOne( r, uiTarget, uiPairs, aBases[ iLen ][ 0 ], aBases[ iLen ][ 1 ], iMore == 1 ? 3 : 0, iMore == 2 ? 3 : 0, &uiPeak ) )
                    return 1;
                if( uiPairs == 1000 && iLen > 0 )
                    aPeak[ iLen - 1 ] = std::max( aPeak[ iLen - 1 ], uiPeak );
            }
    // the carry does not grow with the file: the peak of 1 000 pairs of 150 / 450 is not exceeded with 4 000
    for( int iLen = 1; iLen < 3; iLen++, uiRuns++ )
    {
        size_t uiPeak = 0;
        if( readerOne( r, uiTarget, 4000, aBases[ iLen ][ 0 ], aBases[ iLen ][ 1 ], 0, 0, &uiPeak ) )
            return 1;
        if( uiPeak > aPeak[ iLen - 1 ] )
            return printf( "FAIL: 4000 pairs carry up to %zu bytes, 1000 pairs %zu\n", uiPeak, aPeak[ iLen - 1 ] ), 1;
    }
    // a batch destroyed without hand-back: a second thread that waits in execute( ) is released and throws, and so does the next call
    {
        const std::string s1 = fixedText( r, 37, 65, 1 ), s2 = fixedText( r, 37, 215, 2 );
        auto pReader = std::make_shared<BatchPairedBgzfReader>( ParameterSetManager( ) );
        pReader->uiBatchBytes = uiTarget;
        auto pStreams = std::make_shared<PairedFileStream>( std::make_shared<StringStream>( bgzfFile( s1 ) ), std::make_shared<StringStream>( bgzfFile( s2 ) ) );
        auto pFirst = pReader->execute( pStreams );
        if( pFirst == nullptr )
            return printf( "FAIL: no first batch\n" ), 1;
        const auto xThrows = [ pReader, pStreams ]( ) {
            try
            {
                pReader->execute( pStreams );
            }
            catch( const std::runtime_error& rE )
            {
                return std::string( rE.what( ) );
            }
            return std::string( "no exception" );
        };
        auto xWaiting = std::async( std::launch::async, xThrows );
        pFirst.reset( ); // (whether the thread waits already or not yet: it must come back either way)
        if( xWaiting.wait_for( std::chrono::seconds( 20 ) ) != std::future_status::ready )
        {
            printf( "FAIL: a thread is still blocked in execute( ) after the batch it waits for was destroyed\n" );
            fflush( stdout );
            _Exit( 1 );
        }
        for( const std::string& sGot : { xWaiting.get( ), xThrows( ) } )
            if( sGot.find( "destroyed without handing back" ) == std::string::npos )
                return printf( "FAIL: '%s' after a batch was destroyed without handing back\n", sGot.c_str( ) ), 1;
    }
    // a plain-gzip stream throws BatchBgzfReader's message
    try
    {
        const std::string s = fixedText( r, 3, 65, 1 );
        BatchPairedBgzfReader xReader{ ParameterSetManager( ) };
        xReader.execute( std::make_shared<PairedFileStream>( std::make_shared<StringStream>( bgzfFile( s ) ), std::make_shared<StringStream>( plainGzip( s ) ) ) );
        return printf( "FAIL: a plain gzip stream was read\n" ), 1;
    }
    catch( const std::runtime_error& rE )
    {
        if( std::string( rE.what( ) ).find( "BatchBgzfReader: the stream" ) != 0 || std::string( rE.what( ) ).find( "GzFileStream" ) == std::string::npos )
            return printf( "FAIL: '%s' is not BatchBgzfReader's message\n", rE.what( ) ), 1;
    }
    printf( "reader ok: %zu runs, target %zu bytes\n", uiRuns, uiTarget );
    return 0;
}

int main( int argc, char** argv )
{
    try
    {
        const std::string sMode = argc > 1 ? argv[ 1 ] : "";
        if( sMode == "golden" && argc > 2 )
            return golden( argv[ 2 ] );
        if( sMode == "random" && argc > 3 )
            return randomPairs( strtoull( argv[ 2 ], nullptr, 10 ), (size_t)atol( argv[ 3 ] ) );
        if( sMode == "reasons" )
            return reasons( argc > 2 && std::string( argv[ 2 ] ) == "print" );
        if( sMode == "reader" && argc > 2 )
            return reader( (size_t)atol( argv[ 2 ] ) );
        fprintf( stderr, "usage: mates_bgzf_test golden <dir> | random <seed> <n> | reasons [print] | reader <target bytes>\n" );
        return 2;
    }
    catch( const std::exception& rE )
    {
        printf( "EXCEPTION %s\n", rE.what( ) );
        return 3;
    }
}
