// ma_genome_dev.h -- the rules of ma_genome_append_text / ma_genome_build_index, written ONCE: which FASTA text a genome is read
// from, what becomes of its bytes, what a hole is, how the hole bases are filled, and how a refusal is worded.  Its users:
//   - the kernels of ma_amd/csrc/stage_genome.h call the per-lane functions (holeMasks( )), and ma_text::lineOf / code( ) as the
//     reads' parser does;
//   - libma_amd.so books a parsed chunk into its genome with commit( ) and draws the fill with Rand / packedDraws( );
//   - parseHost( ) below runs the same functions serially: the statement the CPU tests (tests/emul/genome_text_test.cpp) compare
//     with the yardstick -- FileReader + the base loop of buildIndex (ma_modules.h) -- and with the files the reference's
//     Pack::vAppendSequence wrote (pack.h:586-698), and the GPU tests with the kernels.
//
// The text is FASTA in the strict form of ma_text_dev.h (lines, names, bases: ma_text::lineOf and its reasons), with these
// differences: a text that starts with '@' is refused (a genome is FASTA); what follows the name on a header line is dropped; a
// chunk after the first may begin with base lines, which continue the contig that is open.  A file arrives in chunks of whole
// lines; the chunk with end_of_file closes the file, and the next chunk starts another file with a header.
//   codes    A C G T in either case 0 1 2 3; every other kept byte is a HOLE BASE, code 4 (nucSeq.cpp:17-28: R, Y, ... are N)
//   holes    a hole base opens a new hole unless the base before it IN THE SAME CONTIG is a hole base too; a hole is (start on
//            the forward strand, length); every contig carries its number of holes
//   contigs  name, start (sum of the lengths before it), length
//   fill     the k-th hole base in text order becomes rand( ) & 3 of the k-th draw after srand( seed ) of glibc (Rand)
#pragma once
#include "ma_text_dev.h"

#include <string>
#include <vector>

namespace ma_genome_dev
{
static const uint8_t HOLE = 4; // the code of a hole base that is not filled yet
MA_TEXT_HD bool isHole( uint8_t uiCode )
{
    return uiCode >= 4;
}

// ---- holes, 16 bases at a time ------------------------------------------------------------------------------------------------
// uiHole: bit k = base k of the 16 is a hole base (bases outside the chunk: 0); bPrev / bNext: the base before the 16 / behind
// them is a hole base of the chunk; uiFirst: bit k (k = 0..16) = base k is the first base of a contig.  A run starts at a hole
// base whose predecessor is no hole base of the same contig, and ends at one whose successor is none.
struct HoleMasks
{
    uint32_t uiStarts, uiEnds;
};
MA_TEXT_HD HoleMasks holeMasks( uint32_t uiHole, bool bPrev, bool bNext, uint32_t uiFirst )
{
    HoleMasks m;
    m.uiStarts = uiHole & ~( ( ( uiHole << 1 ) | ( bPrev ? 1u : 0u ) ) & ~uiFirst ) & 0xffffu;
    m.uiEnds = uiHole & ~( ( ( uiHole >> 1 ) | ( bNext ? 0x8000u : 0u ) ) & ~( uiFirst >> 1 ) ) & 0xffffu;
    return m;
}

// ---- the generator -----------------------------------------------------------------------------------------------------------
// glibc stdlib/random_r.c, TYPE_3, as srand( seed ) leaves it: r[ i ] = r[ i - 3 ] + r[ i - 31 ], output >> 1 (the state of
// ChainParams::rng_ring, ma_amd/csrc/chain.h).  Its own state: no call touches libc's.
struct Rand
{
    uint32_t aRing[ 31 ];
    int iFront, iRear;
    explicit Rand( uint32_t uiSeed )
    {
        if( uiSeed == 0 )
            uiSeed = 1;
        int32_t iWord = (int32_t)uiSeed;
        aRing[ 0 ] = (uint32_t)iWord;
        for( int i = 1; i < 31; i++ )
        {
            const long iHi = iWord / 127773, iLo = iWord % 127773;
            iWord = (int32_t)( 16807 * iLo - 2836 * iHi );
            if( iWord < 0 )
                iWord += 2147483647;
            aRing[ i ] = (uint32_t)iWord;
        }
        iFront = 3, iRear = 0;
        for( int i = 0; i < 310; i++ )
            next( );
    }
    uint32_t next( ) // rand( )
    {
        aRing[ iFront ] += aRing[ iRear ];
        const uint32_t uiOut = aRing[ iFront ] >> 1;
        iFront = iFront + 1 >= 31 ? 0 : iFront + 1;
        iRear = iRear + 1 >= 31 ? 0 : iRear + 1;
        return uiOut;
    }
};
// draw k of the packed fill: four draws per byte, draw k in bits 2 ( k & 3 ) of byte k / 4
MA_TEXT_HD uint8_t drawOf( const uint8_t* pPacked, uint64_t k )
{
    return (uint8_t)( ( pPacked[ k >> 2 ] >> ( 2 * ( k & 3 ) ) ) & 3u );
}

// the first n draws & 3 after srand( uiSeed ), packed for drawOf( )
inline std::vector<uint8_t> packedDraws( uint32_t uiSeed, uint64_t n )
{
    std::vector<uint8_t> v( ( n + 3 ) / 4 + 1, 0 );
    Rand xRand( uiSeed );
    for( uint64_t k = 0; k < n; k++ )
        v[ k >> 2 ] |= (uint8_t)( ( xRand.next( ) & 3u ) << ( 2 * ( k & 3 ) ) );
    return v;
}

// ---- a genome being read, and one parsed chunk ----------------------------------------------------------------------------------
struct Genome
{
    std::vector<uint64_t> vNameOff = { 0 }; // CSR of sNames
    std::string sNames;
    std::vector<uint64_t> vStarts, vLens, vNumHoles; // per contig
    std::vector<uint64_t> vHoleStart, vHoleLen;
    uint64_t uiBases = 0, uiHoleBases = 0;
    uint64_t uiLines = 0, uiBytes = 0; // consumed so far
    bool bOpen = false; // base lines may continue the last contig (false: the next chunk starts a file)
    uint64_t uiOpenLine = 0, uiOpenByte = 0; // the open contig's header line, counted over everything consumed
    bool bLastHole = false; // the genome's last base is a hole base of the open contig
    bool bBuilt = false; // ma_genome_build_index was called
    std::vector<uint8_t> vCodes; // parseHost only (the library keeps them on the device)
};
// What one chunk adds, as the kernels (or parseHost's serial pass) see the chunk ALONE: holes that touch the chunk's first base
// are not joined with the genome's last hole yet -- commit( ) does that.
struct Chunk
{
    uint64_t uiLines = 0, uiBytes = 0, uiBases = 0, uiHoleBases = 0;
    bool bStartsWithHeader = false, bEndOfFile = false;
    std::vector<uint64_t> vNameOff = { 0 }; // the chunk's new contigs: CSR of sNames,
    std::string sNames;
    std::vector<uint64_t> vStarts; //                                        start in the genome,
    std::vector<uint64_t> vHdrLine, vHdrByte; //                             header line and its byte offset in the chunk
    std::vector<uint64_t> vHoleStart, vHoleLen; // in the genome
};
enum : uint32_t // why a chunk is refused
{
    REFUSE_NONE = 0u,
    REFUSE_LINE = 1u, // a rule violation: line, byte (over everything consumed) and a reason of ma_text
    REFUSE_FASTQ = 2u, // an '@' where a header is due
    REFUSE_CAPACITY = 3u,
    REFUSE_TOO_LARGE = 4u,
    REFUSE_BUILT = 5u,
    REFUSE_COMPRESSED = 6u // BGZF or gzip bytes where a header is due
};
inline std::string refusalText( uint32_t uiRefusal, uint64_t uiLine, uint64_t uiByte, uint32_t uiReason, uint64_t uiBases )
{
    char aMessage[ 320 ];
    if( uiRefusal == REFUSE_LINE )
        ma_text::messageOf( aMessage, sizeof( aMessage ), "ma_genome_append_text", uiLine, uiByte, uiReason );
    else if( uiRefusal == REFUSE_CAPACITY )
        snprintf( aMessage, sizeof( aMessage ), "ma_genome_append_text: genome capacity exceeded (%llu bases)", (unsigned long long)uiBases );
    else
        snprintf( aMessage, sizeof( aMessage ), "ma_genome_append_text: %s",
                  uiRefusal == REFUSE_FASTQ        ? "a genome is FASTA"
                  : uiRefusal == REFUSE_TOO_LARGE  ? "too large"
                  : uiRefusal == REFUSE_COMPRESSED ? "a genome as BGZF or gzip is not served (plain FASTA text only)"
                                                   : "the index was already built" );
    return aMessage;
}
// bytes of a chunk that a call consumes: whole lines only, an unterminated last line with end_of_file
inline uint64_t consumable( const char* pText, uint64_t n, bool bEndOfFile )
{
    if( bEndOfFile )
        return n;
    while( n > 0 && pText[ n - 1 ] != '\n' )
        n--;
    return n;
}
// What the host decides before any line is parsed: REFUSE_NONE and in *pConsumable the bytes the call will consume, or the refusal
// (of the chunk's first line).  The size is the chunk's, n_bytes, and is judged before the chunk is looked at; the first byte is
// judged only when the call consumes something.
inline uint32_t refusalAtStart( const Genome& g, const char* pText, uint64_t uiBytes, bool bEndOfFile, uint64_t* pConsumable, uint32_t* pReason )
{
    *pReason = ma_text::OK;
    *pConsumable = 0;
    if( g.bBuilt )
        return REFUSE_BUILT;
    if( uiBytes > ma_text::MAX_TEXT_BYTES )
        return REFUSE_TOO_LARGE;
    const uint64_t n = consumable( pText, uiBytes, bEndOfFile );
    *pConsumable = n;
    if( n > 0 && !g.bOpen && pText[ 0 ] == '@' )
        return REFUSE_FASTQ;
    if( n > 1 && !g.bOpen && (uint8_t)pText[ 0 ] == 0x1fu && (uint8_t)pText[ 1 ] == 0x8bu ) // the magic of RFC 1952
        return REFUSE_COMPRESSED;
    if( n > 0 && !g.bOpen && pText[ 0 ] != '>' )
    {
        *pReason = ma_text::ERR_KIND;
        return REFUSE_LINE;
    }
    return REFUSE_NONE;
}
// The open contig has no bases yet (the chunk before ended in its header), and this chunk gives it none before its next header or
// the file's end: "a record has bases", at that header's line.  uiFirstBases: the chunk's bases before its first header.
inline bool openStaysEmpty( const Genome& g, uint64_t uiFirstBases, bool bHasHeader, bool bEndOfFile )
{
    return g.bOpen && !g.vLens.empty( ) && g.vLens.back( ) == 0 && uiFirstBases == 0 && ( bHasHeader || bEndOfFile );
}
// books an accepted chunk
inline void commit( Genome& g, const Chunk& c )
{
    const uint64_t uiFrom = g.uiBases, uiTo = g.uiBases + c.uiBases, uiNew = c.vStarts.size( );
    const uint64_t uiFirstNew = g.vStarts.size( );
    // contigs: the open one grows up to the first new start
    if( !g.vLens.empty( ) )
        g.vLens.back( ) += ( uiNew ? c.vStarts[ 0 ] : uiTo ) - uiFrom;
    for( uint64_t i = 0; i < uiNew; i++ )
    {
        g.vStarts.push_back( c.vStarts[ i ] );
        g.vLens.push_back( ( i + 1 < uiNew ? c.vStarts[ i + 1 ] : uiTo ) - c.vStarts[ i ] );
        g.vNumHoles.push_back( 0 );
        g.sNames.append( c.sNames, c.vNameOff[ i ], c.vNameOff[ i + 1 ] - c.vNameOff[ i ] );
        g.vNameOff.push_back( g.sNames.size( ) );
    }
    // holes: one that starts at the chunk's first base continues the genome's last hole if that base belongs to the open contig
    uint64_t uiContig = uiFirstNew ? uiFirstNew - 1 : 0; // the contig of the hole at hand
    for( uint64_t i = 0; i < c.vHoleStart.size( ); i++ )
    {
        const uint64_t uiStart = c.vHoleStart[ i ];
        if( i == 0 && g.bLastHole && uiStart == uiFrom && ( uiNew == 0 || c.vStarts[ 0 ] > uiFrom ) )
        {
            g.vHoleLen.back( ) += c.vHoleLen[ i ];
            continue;
        }
        while( uiContig + 1 < g.vStarts.size( ) && g.vStarts[ uiContig + 1 ] <= uiStart )
            uiContig++;
        g.vHoleStart.push_back( uiStart );
        g.vHoleLen.push_back( c.vHoleLen[ i ] );
        g.vNumHoles[ uiContig ]++;
    }
    if( uiNew && g.vLens.back( ) == 0 )
        g.bLastHole = false; // a fresh contig without bases
    else if( c.uiBases )
        g.bLastHole = !c.vHoleStart.empty( ) && c.vHoleStart.back( ) + c.vHoleLen.back( ) == uiTo;
    if( uiNew )
    {
        g.uiOpenLine = g.uiLines + c.vHdrLine.back( );
        g.uiOpenByte = g.uiBytes + c.vHdrByte.back( );
    }
    g.uiBases = uiTo;
    g.uiHoleBases += c.uiHoleBases;
    g.uiLines += c.uiLines;
    g.uiBytes += c.uiBytes;
    g.bOpen = !c.bEndOfFile;
}

// ---- the serial driver ------------------------------------------------------------------------------------------------------
// ma_genome_append_text on the host: consumes the whole lines of pText (consumable( )), books them into g (codes into g.vCodes,
// hole bases as HOLE) and returns 0 with *pConsumed, or returns 1 with the refusal's words in *pMessage, *pConsumed = 0 and g
// untouched.
inline int parseHost( Genome& g, const char* pText, uint64_t uiBytes, bool bEndOfFile, uint64_t uiMaxBases, uint64_t* pConsumed,
                      std::string* pMessage )
{
    *pConsumed = 0;
    uint64_t n;
    uint32_t uiReason;
    const uint32_t uiAtStart = refusalAtStart( g, pText, uiBytes, bEndOfFile, &n, &uiReason );
    if( uiAtStart != REFUSE_NONE )
    {
        *pMessage = refusalText( uiAtStart, g.uiLines, g.uiBytes, uiReason, 0 );
        return 1;
    }
    Chunk c;
    c.bEndOfFile = bEndOfFile;
    c.uiBytes = n;
    std::vector<uint8_t> vCodes;
    uint64_t uiKey = ma_text::NO_VIOLATION;
    uint64_t uiFirstBases = 0;
    std::vector<uint32_t> vStart( n + 2 );
    if( n > 0 )
    {
        uint64_t uiFeeds = 0, uiLoneCr = n;
        vStart[ 0 ] = 0;
        for( uint64_t p = 0; p < n; p++ )
        {
            if( pText[ p ] == '\n' )
                vStart[ ++uiFeeds ] = (uint32_t)( p + 1 );
            if( uiLoneCr == n && ma_text::loneCr( pText, n, p ) )
                uiLoneCr = p;
        }
        const uint64_t uiLines = ma_text::nLines( uiFeeds, pText[ n - 1 ] );
        vStart[ uiLines ] = (uint32_t)n;
        c.uiLines = uiLines;
        c.bStartsWithHeader = pText[ 0 ] == '>';
        uint64_t uiRecFrom = 0, uiRecLine = 0;
        bool bInRecord = false;
        for( uint64_t i = 0; i <= uiLines; i++ )
        {
            ma_text::Line x;
            x.uiKind = ma_text::LINE_HEADER; // (the end of the chunk closes its last record like a header)
            x.uiBases = x.uiName = x.uiLen = 0;
            if( i < uiLines )
            {
                x = ma_text::lineOf( ma_text::KIND_FASTA, pText, vStart.data( ), i, uiLines, uiLoneCr );
                if( x.uiReason != ma_text::OK && ma_text::key( i, x.uiReason ) < uiKey )
                    uiKey = ma_text::key( i, x.uiReason );
            }
            if( x.uiKind == ma_text::LINE_HEADER )
            {
                if( bInRecord && ( i < uiLines || bEndOfFile ) ) // (a header that ends a chunk waits for the next one)
                {
                    const uint64_t k = ma_text::recordKey( uiRecLine, uiRecFrom, vCodes.size( ) );
                    uiKey = k < uiKey ? k : uiKey;
                }
                if( !bInRecord )
                    uiFirstBases = vCodes.size( );
                if( i < uiLines )
                {
                    bInRecord = true, uiRecFrom = vCodes.size( ), uiRecLine = i;
                    c.vStarts.push_back( g.uiBases + vCodes.size( ) );
                    c.vHdrLine.push_back( i );
                    c.vHdrByte.push_back( vStart[ i ] );
                }
            }
            for( uint32_t k = 0; k < x.uiLen && i < uiLines; k++ )
            {
                uint32_t j;
                const uint32_t t = ma_text::byteTarget( x, k, &j );
                const char b = pText[ vStart[ i ] + k ];
                if( t == ma_text::TO_CODES )
                    vCodes.push_back( ma_text::code( (uint8_t)b ) );
                else if( t == ma_text::TO_NAMES )
                    c.sNames.push_back( b );
            }
            if( i < uiLines && x.uiKind == ma_text::LINE_HEADER )
                c.vNameOff.push_back( c.sNames.size( ) );
        }
    }
    if( openStaysEmpty( g, uiFirstBases, !c.vStarts.empty( ), bEndOfFile ) )
    {
        *pMessage = refusalText( REFUSE_LINE, g.uiOpenLine, g.uiOpenByte, ma_text::ERR_FA_NO_BASES, 0 );
        return 1;
    }
    if( uiKey != ma_text::NO_VIOLATION )
    {
        *pMessage = refusalText( REFUSE_LINE, g.uiLines + ( uiKey >> 8 ), g.uiBytes + vStart[ uiKey >> 8 ], (uint32_t)( uiKey & 0xffu ), 0 );
        return 1;
    }
    c.uiBases = vCodes.size( );
    if( g.uiBases + c.uiBases > uiMaxBases )
    {
        *pMessage = refusalText( REFUSE_CAPACITY, 0, 0, 0, g.uiBases + c.uiBases );
        return 1;
    }
    // the holes of the chunk alone, 16 bases at a time as the kernels find them
    uint64_t uiNext = 0; // the next new contig at or behind the bases at hand
    for( uint64_t a = 0; a < c.uiBases; a += 16 )
    {
        uint32_t uiHole = 0, uiFirst = 0;
        for( uint64_t k = 0; k < 16 && a + k < c.uiBases; k++ )
            uiHole |= ( isHole( vCodes[ a + k ] ) ? 1u : 0u ) << k;
        while( uiNext < c.vStarts.size( ) && c.vStarts[ uiNext ] - g.uiBases < a )
            uiNext++;
        for( uint64_t i = uiNext; i < c.vStarts.size( ) && c.vStarts[ i ] - g.uiBases <= a + 16; i++ )
            uiFirst |= 1u << ( c.vStarts[ i ] - g.uiBases - a );
        const HoleMasks m = holeMasks( uiHole, a > 0 && isHole( vCodes[ a - 1 ] ), a + 16 < c.uiBases && isHole( vCodes[ a + 16 ] ), uiFirst );
        for( uint32_t k = 0; k < 16; k++ )
        {
            if( ( m.uiStarts >> k ) & 1u )
                c.vHoleStart.push_back( g.uiBases + a + k );
            if( ( m.uiEnds >> k ) & 1u )
                c.vHoleLen.push_back( g.uiBases + a + k + 1 ); // (the end for now)
            c.uiHoleBases += ( uiHole >> k ) & 1u;
        }
    }
    for( uint64_t i = 0; i < c.vHoleStart.size( ); i++ )
        c.vHoleLen[ i ] -= c.vHoleStart[ i ];
    commit( g, c );
    g.vCodes.insert( g.vCodes.end( ), vCodes.begin( ), vCodes.end( ) );
    *pConsumed = n;
    return 0;
}
// why ma_genome_build_index refuses (NULL: it does not)
inline const char* buildRefusal( const Genome& g )
{
    if( g.bBuilt )
        return "ma_genome_build_index: the index was already built";
    if( g.vStarts.empty( ) )
        return "ma_genome_build_index: the genome has no contigs";
    if( g.vLens.back( ) == 0 )
        return "ma_genome_build_index: the last contig is still open without bases";
    return NULL;
}
// the fill of ma_genome_build_index on g.vCodes
inline void fillHost( Genome& g, uint32_t uiSeed )
{
    const std::vector<uint8_t> vDraws = packedDraws( uiSeed, g.uiHoleBases );
    uint64_t k = 0;
    for( uint8_t& c : g.vCodes )
        if( isHole( c ) )
            c = drawOf( vDraws.data( ), k++ );
    g.bBuilt = true;
}
} // namespace ma_genome_dev
