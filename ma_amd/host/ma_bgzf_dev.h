// ma_bgzf_dev.h -- the rules of ma_batch_set_reads_bgzf, written ONCE: which compressed bytes the device inflates, what it makes
// of them, and how it words a refusal.  Its users:
//   - the kernels of ma_amd/csrc/stage_bgzf.h call inflate( ) with one member per lane and crcOf( ) / crcCombine( ) with one
//     member per wavefront;
//   - inflateHost( ) below runs the same routine serially: the statement of the rules the CPU tests (tests/emul/bgzf_dev_test.cpp)
//     compare with zlib, and the GPU tests with the kernels; BatchBgzfReader (ma_batch_nodes.h) inflates the last members of a
//     chunk with it to find its cut;
//   - libma_amd.so words a refusal with errorText( ) / message( ), ma_batch_set_mates_bgzf with messageMates( ); that call's
//     own rules -- two such chains, paired -- are in ma_mates_bgzf_dev.h.
// No zlib, no containers, no strings.
//
// BGZF (what bgzip and htslib write) is a chain of independent gzip members of at most 64 KiB of text each, every one with its
// compressed size in its header: the host finds all members without decoding anything, and every member is inflated by a lane
// of its own.  A gzip file that is one member has no such parallelism and is refused by name.
//
// THE STRICT MEMBER FORM (anything else is a refusal, never a guess)
//   bytes 0..3   1f 8b 08 04 (gzip, deflate, FLG = FEXTRA alone); MTIME, XFL and OS may be anything
//   XLEN         >= 6; the extra field is a run of subfields SI1 SI2 SLEN data that fills it exactly; exactly one of them has
//                SI 'B' 'C', and its SLEN is 2: its value BSIZE gives the member's size BSIZE + 1.  Other subfields are skipped.
//   size         BSIZE + 1 >= 12 + XLEN + 8, and the member lies inside the bytes given
//   trailer      CRC32 of the text, then ISIZE, its length: at most 65 536
//   deflate      the raw deflate stream occupies exactly the bytes between the extra field and the trailer: its final block
//                ends inside the last of them (only the padding bits of that byte may remain), it produces exactly ISIZE
//                bytes, and their CRC32 is the trailer's
//   ISIZE 0      such a member may stand anywhere and contributes nothing (the 28-byte end-of-file marker is one); it is checked
//                like every other
// THE DEFLATE STREAM is accepted exactly where zlib's inflate accepts it (inflate.c, inftrees.c of zlib 1.2.11):
//   stored, fixed and dynamic blocks, any number per member; block type 3 is refused;
//   a stored block whose LEN is not the complement of NLEN is refused;
//   a dynamic block with HLIT > 286 or HDIST > 30 is refused; an over-subscribed or incomplete code-length set is refused; a
//   repeat code 16 with no length before it, and a repeat that runs past HLIT + HDIST, are refused; no code for symbol 256 is
//   refused; an over-subscribed literal/length or distance set is refused; an incomplete one is refused unless it is the ONE
//   code of length 1 (zlib's "max != 1"; for literal/length sets that leaves the block that is its end-of-block code alone);
//   a distance set without any code is accepted;
//   a bit pattern that is no code of its set, the length symbols 286 / 287 and the distance symbols 30 / 31 are refused when met;
//   a back-reference may not reach before the first byte of its own member (members are independent).
// inflate( ) cannot run away: every input read is bounded by the member's deflate bytes (the source returns zeros beyond them
// and the bits consumed are compared with the bits there are at every step), every output write by ISIZE, and every loop
// iteration consumes at least one bit or ends.
//
// A refusal names the lowest-numbered offending member (0-based), the offset of its first byte in the data given, and one
// reason: taking the minimum of key( member, reason ) over all violations gives that -- on the device with atomicMin.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#if defined( __HIPCC__ )
#define MA_BGZF_HD __host__ __device__ __forceinline__
#else
#define MA_BGZF_HD inline
#endif

namespace ma_bgzf
{
enum : uint32_t // the header's checks first, then the stream's in the order it is read, then the two of the trailer
{
    OK = 0u,
    ERR_NOT_BGZF = 1u, // not 1f 8b 08 04, or an extra field without exactly one well-formed BC subfield, or a BSIZE too small
    ERR_TRUNCATED = 2u, // the header, or the size it states, reaches beyond the bytes given
    ERR_ISIZE = 3u, // ISIZE > 65 536
    ERR_BTYPE = 4u,
    ERR_STORED_LEN = 5u,
    ERR_SYMBOL_COUNT = 6u, // HLIT > 286 or HDIST > 30
    ERR_CODELEN_SET = 7u,
    ERR_REPEAT_FIRST = 8u,
    ERR_REPEAT_OVER = 9u,
    ERR_NO_EOB = 10u,
    ERR_LITLEN_SET = 11u,
    ERR_DIST_SET = 12u,
    ERR_LITLEN_CODE = 13u,
    ERR_DIST_CODE = 14u,
    ERR_DIST_FAR = 15u,
    ERR_INPUT_END = 16u, // the stream wants more bits than the member has
    ERR_TRAILING = 17u, // the final block ends before the last deflate byte
    ERR_LENGTH = 18u, // more or fewer bytes than ISIZE
    ERR_CRC = 19u,
    N_REASONS = 20u
};
static const uint64_t NO_VIOLATION = ~(uint64_t)0;
static const uint32_t MAX_ISIZE = 65536u;
static const uint32_t HEADER_BYTES = 12u, TRAILER_BYTES = 8u, MIN_PROBE_BYTES = 18u;

MA_BGZF_HD const char* errorText( uint32_t uiReason )
{
    switch( uiReason )
    {
        case ERR_NOT_BGZF:
            return "a gzip member without the BGZF size field: single-member gzip stays with GzFileStream (or no gzip member at all)";
        case ERR_TRUNCATED:
            return "a truncated member: its header or the size it states reaches beyond the data";
        case ERR_ISIZE:
            return "ISIZE is larger than 65536";
        case ERR_BTYPE:
            return "deflate: block type 3";
        case ERR_STORED_LEN:
            return "deflate: a stored block whose LEN is not the complement of NLEN";
        case ERR_SYMBOL_COUNT:
            return "deflate: more than 286 literal/length or more than 30 distance symbols";
        case ERR_CODELEN_SET:
            return "deflate: an over-subscribed or incomplete code-length set";
        case ERR_REPEAT_FIRST:
            return "deflate: a length repeat with no length before it";
        case ERR_REPEAT_OVER:
            return "deflate: a length repeat that runs past the symbols of the block";
        case ERR_NO_EOB:
            return "deflate: no code for the end-of-block symbol";
        case ERR_LITLEN_SET:
            return "deflate: an over-subscribed or incomplete literal/length set";
        case ERR_DIST_SET:
            return "deflate: an over-subscribed or incomplete distance set";
        case ERR_LITLEN_CODE:
            return "deflate: an invalid literal/length code";
        case ERR_DIST_CODE:
            return "deflate: an invalid distance code";
        case ERR_DIST_FAR:
            return "deflate: a back-reference that reaches before the start of its member";
        case ERR_INPUT_END:
            return "deflate: the stream does not end inside its member";
        case ERR_TRAILING:
            return "deflate: the final block ends before the member's last deflate byte";
        case ERR_LENGTH:
            return "length mismatch: the member does not inflate to ISIZE bytes";
        case ERR_CRC:
            return "CRC mismatch";
        default:
            return "no error";
    }
}
// "ma_batch_set_reads_bgzf: member <k> (byte <X>): <reason>" into pOut (at least 256 bytes)
inline void message( char* pOut, size_t uiCap, uint64_t uiMember, uint64_t uiByte, uint32_t uiReason )
{
    snprintf( pOut, uiCap, "ma_batch_set_reads_bgzf: member %llu (byte %llu): %s", (unsigned long long)uiMember, (unsigned long long)uiByte,
              errorText( uiReason ) );
}
// "ma_batch_set_mates_bgzf: text <1|2>: member <k> (byte <X>): <reason>": k and X count within that text's members
inline void messageMates( char* pOut, size_t uiCap, uint32_t uiText, uint64_t uiMember, uint64_t uiByte, uint32_t uiReason )
{
    snprintf( pOut, uiCap, "ma_batch_set_mates_bgzf: text %u: member %llu (byte %llu): %s", (unsigned)uiText, (unsigned long long)uiMember,
              (unsigned long long)uiByte, errorText( uiReason ) );
}
// violations are ordered by member, then by reason
MA_BGZF_HD uint64_t key( uint64_t uiMember, uint32_t uiReason )
{
    return ( uiMember << 8 ) | uiReason;
}

// ---- the member header ----------------------------------------------------------------------------------------------------------
// One member as the host's walk finds it (the device's member table is an array of these)
struct Member
{
    uint64_t uiIn; // offset of the member's first byte in the data
    uint64_t uiDeflate; // offset of its first deflate byte in the data
    uint64_t uiOut; // offset of its first text byte in the inflated text (the running sum of ISIZE)
    uint32_t uiDeflateBytes, uiIsize, uiCrc, uiBytes; // uiBytes: BSIZE + 1
};
MA_BGZF_HD uint32_t le16( const uint8_t* p )
{
    return (uint32_t)p[ 0 ] | ( (uint32_t)p[ 1 ] << 8 );
}
MA_BGZF_HD uint32_t le32( const uint8_t* p )
{
    return le16( p ) | ( le16( p + 2 ) << 16 );
}
// the member that starts at pData[ uiAt ] of n bytes: OK and *pM (uiOut is left alone), or the reason
inline uint32_t header( const uint8_t* pData, uint64_t n, uint64_t uiAt, Member* pM )
{
    static const uint8_t aMagic[ 4 ] = { 0x1f, 0x8b, 0x08, 0x04 };
    const uint64_t uiLeft = n - uiAt;
    const uint8_t* const p = pData + uiAt;
    for( uint64_t i = 0; i < 4 && i < uiLeft; i++ )
        if( p[ i ] != aMagic[ i ] )
            return ERR_NOT_BGZF;
    if( uiLeft < HEADER_BYTES )
        return ERR_TRUNCATED;
    const uint32_t uiXlen = le16( p + 10 );
    if( uiXlen < 6 )
        return ERR_NOT_BGZF;
    if( uiLeft < HEADER_BYTES + uiXlen )
        return ERR_TRUNCATED;
    uint32_t uiFound = 0, uiBsize = 0, uiOff = 0;
    while( uiOff + 4 <= uiXlen )
    {
        const uint8_t* const f = p + HEADER_BYTES + uiOff;
        const uint32_t uiSlen = le16( f + 2 );
        if( uiOff + 4 + uiSlen > uiXlen )
            return ERR_NOT_BGZF;
        if( f[ 0 ] == 'B' && f[ 1 ] == 'C' )
        {
            if( uiSlen != 2 )
                return ERR_NOT_BGZF;
            uiBsize = le16( f + 4 );
            uiFound++;
        }
        uiOff += 4 + uiSlen;
    }
    if( uiOff != uiXlen || uiFound != 1 )
        return ERR_NOT_BGZF;
    const uint32_t uiBytes = uiBsize + 1;
    if( uiBytes < HEADER_BYTES + uiXlen + TRAILER_BYTES )
        return ERR_NOT_BGZF;
    if( uiLeft < uiBytes )
        return ERR_TRUNCATED;
    pM->uiIn = uiAt;
    pM->uiDeflate = uiAt + HEADER_BYTES + uiXlen;
    pM->uiDeflateBytes = uiBytes - HEADER_BYTES - uiXlen - TRAILER_BYTES;
    pM->uiBytes = uiBytes;
    pM->uiCrc = le32( p + uiBytes - 8 );
    pM->uiIsize = le32( p + uiBytes - 4 );
    return pM->uiIsize > MAX_ISIZE ? (uint32_t)ERR_ISIZE : (uint32_t)OK;
}

// ---- CRC32 (the gzip polynomial, reflected) -------------------------------------------------------------------------------------
// Bit by bit: no table to place anywhere.  The device computes a member's CRC with 64 lanes, one stretch of the text each, and
// folds the lanes' values with crcCombine( ): crc( A B ) = crc( A ) * x^( 8 |B| ) + crc( B ) in GF(2)[x] mod the polynomial.
static const uint32_t CRC_POLY = 0xedb88320u;
MA_BGZF_HD uint32_t crcByte( uint32_t uiCrc, uint32_t uiByte ) // on the raw register (all ones at the start, complemented at the end)
{
    uiCrc ^= uiByte;
    for( int k = 0; k < 8; k++ )
        uiCrc = ( uiCrc >> 1 ) ^ ( CRC_POLY & ( 0u - ( uiCrc & 1u ) ) );
    return uiCrc;
}
MA_BGZF_HD uint32_t crcOf( const uint8_t* p, uint64_t n )
{
    uint32_t c = 0xffffffffu;
    for( uint64_t i = 0; i < n; i++ )
        c = crcByte( c, p[ i ] );
    return ~c;
}
MA_BGZF_HD uint32_t crcMul( uint32_t a, uint32_t b ) // a * b mod the polynomial; bit 31 is x^0
{
    uint32_t p = 0;
    for( uint32_t m = 0x80000000u; m != 0; m >>= 1 )
    {
        if( a & m )
            p ^= b;
        b = ( b >> 1 ) ^ ( CRC_POLY & ( 0u - ( b & 1u ) ) );
    }
    return p;
}
MA_BGZF_HD uint32_t crcCombine( uint32_t uiCrcA, uint32_t uiCrcB, uint64_t uiBytesB )
{
    uint32_t r = 0x80000000u, q = 0x00800000u; // 1 and x^8
    for( uint64_t k = uiBytesB; k != 0; k >>= 1 )
    {
        if( k & 1 )
            r = crcMul( r, q );
        q = crcMul( q, q );
    }
    return crcMul( r, uiCrcA ) ^ uiCrcB;
}

// ---- inflate ----------------------------------------------------------------------------------------------------------------------
// The decode tables of ONE stream, as 16-bit words behind get( ) / set( ): the host keeps them in an array, a lane of the kernel
// in LDS.  Canonical decoding from the number of codes of every length and the symbols in code order (as puff.c of zlib's
// contrib decodes): 700 bytes for both sets, against 2 KiB and more for a first-level lookup table.
enum : uint32_t
{
    T_LEN_COUNT = 0u, // 16: literal/length (and, while a dynamic header is read, code-length) codes of every length
    T_LEN_SYMBOL = 16u, // 288
    T_DIST_COUNT = 304u, // 16
    T_DIST_SYMBOL = 320u, // 30 (32)
    T_OFFSET = 352u, // 16: construct( )'s first index of every length
    T_LENGTHS = 368u, // 80: the code lengths of a header, four to a word
    T_WORDS = 448u
};
struct HostTables
{
    uint16_t a[ T_WORDS ];
    uint32_t get( uint32_t i ) const
    {
        return a[ i ];
    }
    void set( uint32_t i, uint32_t v )
    {
        a[ i ] = (uint16_t)v;
    }
};
// n bytes behind a pointer as a source (reads beyond them give zeros) and as a sink
struct ByteSource
{
    const uint8_t* p;
    uint32_t n;
    MA_BGZF_HD uint32_t size( ) const
    {
        return n;
    }
    MA_BGZF_HD uint32_t word( uint32_t uiPos ) const // bytes uiPos .. uiPos + 3, the first one lowest
    {
        if( uiPos + 4 <= n )
        {
            uint32_t w;
            memcpy( &w, p + uiPos, 4 );
            return w;
        }
        uint32_t w = 0;
        for( uint32_t k = 0; k < 4; k++ )
            if( uiPos + k < n )
                w |= (uint32_t)p[ uiPos + k ] << ( 8 * k );
        return w;
    }
};
struct ByteSink
{
    uint8_t* p;
    MA_BGZF_HD void put( uint32_t i, uint32_t v )
    {
        p[ i ] = (uint8_t)v;
    }
    MA_BGZF_HD uint32_t get( uint32_t i ) const
    {
        return p[ i ];
    }
};

// the bit stream: 64 bits in registers, refilled a word at a time; uiUsed counts the bits consumed, zeros beyond the source
template <typename SRC> struct Bits
{
    const SRC& rSrc;
    uint64_t uiBuf;
    uint32_t uiCnt, uiPos, uiUsed, uiTotal;
    MA_BGZF_HD Bits( const SRC& r ) : rSrc( r ), uiBuf( 0 ), uiCnt( 0 ), uiPos( 0 ), uiUsed( 0 ), uiTotal( 8u * r.size( ) )
    {}
    MA_BGZF_HD void refill( ) // afterwards at least 33 bits are there
    {
        if( uiCnt <= 32 )
        {
            uiBuf |= (uint64_t)rSrc.word( uiPos ) << uiCnt;
            uiPos += 4;
            uiCnt += 32;
        }
    }
    MA_BGZF_HD uint32_t peek( uint32_t k ) const // k <= 16
    {
        return (uint32_t)uiBuf & ( ( 1u << k ) - 1u );
    }
    MA_BGZF_HD void drop( uint32_t k )
    {
        uiBuf >>= k;
        uiCnt -= k;
        uiUsed += k;
    }
    MA_BGZF_HD uint32_t take( uint32_t k )
    {
        const uint32_t v = peek( k );
        drop( k );
        return v;
    }
    MA_BGZF_HD bool over( ) const
    {
        return uiUsed > uiTotal;
    }
};
static const uint32_t NO_SYMBOL = 0xffffffffu;

template <typename TAB> MA_BGZF_HD uint32_t lengthOf( const TAB& T, uint32_t uiSym )
{
    return ( T.get( T_LENGTHS + ( uiSym >> 2 ) ) >> ( 4 * ( uiSym & 3u ) ) ) & 15u;
}
template <typename TAB> MA_BGZF_HD void setLength( TAB& T, uint32_t uiSym, uint32_t uiLen )
{
    const uint32_t w = T.get( T_LENGTHS + ( uiSym >> 2 ) ), s = 4 * ( uiSym & 3u );
    T.set( T_LENGTHS + ( uiSym >> 2 ), ( w & ~( 15u << s ) ) | ( uiLen << s ) );
}
// The code set of the lengths [ uiFrom, uiFrom + n ) into the counts at uiCount and the symbols at uiSymbol.  Returns what is
// left of the code space: 0 complete, negative over-subscribed, positive incomplete; *pCodes: the symbols that have a code.
template <typename TAB> MA_BGZF_HD int32_t construct( TAB& T, uint32_t uiCount, uint32_t uiSymbol, uint32_t uiFrom, uint32_t n, uint32_t* pCodes )
{
    for( uint32_t l = 0; l < 16; l++ )
        T.set( uiCount + l, 0 );
    for( uint32_t s = 0; s < n; s++ )
    {
        const uint32_t l = lengthOf( T, uiFrom + s );
        T.set( uiCount + l, T.get( uiCount + l ) + 1 );
    }
    *pCodes = n - T.get( uiCount );
    int32_t iLeft = 1;
    uint32_t uiAt = 0;
    for( uint32_t l = 1; l < 16; l++ )
    {
        iLeft = 2 * iLeft - (int32_t)T.get( uiCount + l );
        if( iLeft < 0 )
            return iLeft;
        T.set( T_OFFSET + l, uiAt );
        uiAt += T.get( uiCount + l );
    }
    for( uint32_t s = 0; s < n; s++ )
    {
        const uint32_t l = lengthOf( T, uiFrom + s );
        if( l != 0 )
        {
            const uint32_t o = T.get( T_OFFSET + l );
            T.set( uiSymbol + o, s );
            T.set( T_OFFSET + l, o + 1 );
        }
    }
    return iLeft;
}
// the next symbol of the set at uiCount / uiSymbol (its bits are consumed), or NO_SYMBOL when the next 15 bits are no code
template <typename SRC, typename TAB> MA_BGZF_HD uint32_t decode( Bits<SRC>& B, const TAB& T, uint32_t uiCount, uint32_t uiSymbol )
{
    const uint32_t uiBits = B.peek( 15 );
    uint32_t uiCode = 0, uiFirst = 0, uiIndex = 0;
    for( uint32_t l = 1; l < 16; l++ )
    {
        uiCode |= ( uiBits >> ( l - 1 ) ) & 1u;
        const uint32_t c = T.get( uiCount + l );
        if( uiCode - uiFirst < c )
        {
            B.drop( l );
            return T.get( uiSymbol + uiIndex + ( uiCode - uiFirst ) );
        }
        uiIndex += c;
        uiFirst = ( uiFirst + c ) << 1;
        uiCode <<= 1;
    }
    B.drop( 15 );
    return NO_SYMBOL;
}
// the order in which a dynamic header gives the lengths of the code-length codes: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
MA_BGZF_HD uint32_t codeLengthOrder( uint32_t i )
{
    const uint64_t a = 16ull | ( 17ull << 5 ) | ( 18ull << 10 ) | ( 0ull << 15 ) | ( 8ull << 20 ) | ( 7ull << 25 ) | ( 9ull << 30 ) | ( 6ull << 35 ) |
                       ( 10ull << 40 ) | ( 5ull << 45 ) | ( 11ull << 50 ) | ( 4ull << 55 );
    const uint64_t b = 12ull | ( 3ull << 5 ) | ( 13ull << 10 ) | ( 2ull << 15 ) | ( 14ull << 20 ) | ( 1ull << 25 ) | ( 15ull << 30 );
    return (uint32_t)( ( i < 12 ? a >> ( 5 * i ) : b >> ( 5 * ( i - 12 ) ) ) & 31u );
}
// zlib's tolerance (inftrees.c, "max != 1"): an incomplete set passes when it is one code of length 1
template <typename TAB> MA_BGZF_HD bool oneShortCode( const TAB& T, uint32_t uiCount, uint32_t uiCodes )
{
    return uiCodes == 1 && T.get( uiCount + 1 ) == 1;
}
template <typename TAB> MA_BGZF_HD void fixedTables( TAB& T )
{
    uint32_t uiCodes;
    for( uint32_t s = 0; s < 288; s++ )
        setLength( T, s, s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u );
    construct( T, T_LEN_COUNT, T_LEN_SYMBOL, 0, 288, &uiCodes );
    for( uint32_t s = 0; s < 30; s++ )
        setLength( T, s, 5 );
    construct( T, T_DIST_COUNT, T_DIST_SYMBOL, 0, 30, &uiCodes );
}
// the header of a dynamic block: both code sets, or the reason
template <typename SRC, typename TAB> MA_BGZF_HD uint32_t dynamicTables( Bits<SRC>& B, TAB& T )
{
    uint32_t uiSetCodes;
    B.refill( );
    const uint32_t uiLit = B.take( 5 ) + 257, uiDist = B.take( 5 ) + 1, uiCodes = B.take( 4 ) + 4;
    if( B.over( ) )
        return ERR_INPUT_END;
    if( uiLit > 286 || uiDist > 30 )
        return ERR_SYMBOL_COUNT;
    for( uint32_t i = 0; i < 19; i++ )
    {
        uint32_t l = 0;
        if( i < uiCodes )
        {
            B.refill( );
            l = B.take( 3 );
        }
        setLength( T, codeLengthOrder( i ), l );
    }
    if( B.over( ) )
        return ERR_INPUT_END;
    if( construct( T, T_LEN_COUNT, T_LEN_SYMBOL, 0, 19, &uiSetCodes ) != 0 )
        return ERR_CODELEN_SET;
    uint32_t uiHave = 0;
    while( uiHave < uiLit + uiDist )
    {
        B.refill( );
        const uint32_t s = decode( B, T, T_LEN_COUNT, T_LEN_SYMBOL );
        if( s == NO_SYMBOL ) // (before the end of the input is looked at: a pattern that is no code takes 15 bits)
            return ERR_CODELEN_SET;
        if( B.over( ) )
            return ERR_INPUT_END;
        if( s < 16 )
        {
            setLength( T, uiHave++, s );
            continue;
        }
        uint32_t uiLen = 0, uiRepeat;
        if( s == 16 )
        {
            if( uiHave == 0 )
                return ERR_REPEAT_FIRST;
            uiLen = lengthOf( T, uiHave - 1 );
            uiRepeat = 3 + B.take( 2 );
        }
        else if( s == 17 )
            uiRepeat = 3 + B.take( 3 );
        else
            uiRepeat = 11 + B.take( 7 );
        if( B.over( ) )
            return ERR_INPUT_END;
        if( uiHave + uiRepeat > uiLit + uiDist )
            return ERR_REPEAT_OVER;
        while( uiRepeat-- )
            setLength( T, uiHave++, uiLen );
    }
    if( lengthOf( T, 256 ) == 0 )
        return ERR_NO_EOB;
    int32_t iLeft = construct( T, T_LEN_COUNT, T_LEN_SYMBOL, 0, uiLit, &uiSetCodes );
    if( iLeft < 0 || ( iLeft > 0 && !oneShortCode( T, T_LEN_COUNT, uiSetCodes ) ) )
        return ERR_LITLEN_SET;
    iLeft = construct( T, T_DIST_COUNT, T_DIST_SYMBOL, uiLit, uiDist, &uiSetCodes );
    if( iLeft < 0 || ( iLeft > 0 && uiSetCodes != 0 && !oneShortCode( T, T_DIST_COUNT, uiSetCodes ) ) )
        return ERR_DIST_SET;
    return OK;
}

// Inflates the raw deflate stream of rSrc into rSink, which holds uiIsize bytes: OK when the stream is the strict form's -- it
// ends inside the source's last byte and produces exactly uiIsize bytes -- or the reason.  (The CRC is the caller's.)
template <typename SRC, typename SINK, typename TAB> MA_BGZF_HD uint32_t inflate( const SRC& rSrc, SINK& rSink, TAB& T, uint32_t uiIsize )
{
    Bits<SRC> B( rSrc );
    uint32_t uiOut = 0;
    bool bFixed = false; // the tables are the fixed ones
    for( ;; )
    {
        B.refill( );
        const uint32_t uiLast = B.take( 1 ), uiType = B.take( 2 );
        if( B.over( ) )
            return ERR_INPUT_END;
        if( uiType == 3 )
            return ERR_BTYPE;
        if( uiType == 0 )
        {
            B.drop( ( 8u - ( B.uiUsed & 7u ) ) & 7u );
            B.refill( );
            const uint32_t uiLen = B.take( 16 ), uiNlen = B.take( 16 );
            if( B.over( ) )
                return ERR_INPUT_END;
            if( uiLen != ( ~uiNlen & 0xffffu ) )
                return ERR_STORED_LEN;
            if( B.uiUsed + 8u * uiLen > B.uiTotal )
                return ERR_INPUT_END;
            if( uiOut + uiLen > uiIsize )
                return ERR_LENGTH;
            for( uint32_t i = 0; i < uiLen; i++ )
            {
                B.refill( );
                rSink.put( uiOut++, B.take( 8 ) );
            }
        }
        else
        {
            if( uiType == 1 )
            {
                if( !bFixed )
                    fixedTables( T );
                bFixed = true;
            }
            else
            {
                bFixed = false;
                const uint32_t uiReason = dynamicTables( B, T );
                if( uiReason != OK )
                    return uiReason;
            }
            for( ;; ) // (every turn consumes a code: at least one bit)
            {
                B.refill( );
                const uint32_t s = decode( B, T, T_LEN_COUNT, T_LEN_SYMBOL );
                if( s == NO_SYMBOL )
                    return ERR_LITLEN_CODE;
                if( B.over( ) )
                    return ERR_INPUT_END;
                if( s < 256 )
                {
                    if( uiOut >= uiIsize )
                        return ERR_LENGTH;
                    rSink.put( uiOut++, s );
                    continue;
                }
                if( s == 256 )
                    break;
                if( s >= 286 )
                    return ERR_LITLEN_CODE;
                // length 3 .. 258: symbols 257 .. 264 one each, then four symbols per number of extra bits, 285 is 258
                const uint32_t i = s - 257, le = i < 8 || i == 28 ? 0u : ( i >> 2 ) - 1u;
                const uint32_t uiLen = ( i < 8 ? 3u + i : i == 28 ? 258u : 3u + ( ( 4u + ( i & 3u ) ) << le ) ) + B.take( le );
                B.refill( );
                const uint32_t d = decode( B, T, T_DIST_COUNT, T_DIST_SYMBOL );
                if( d == NO_SYMBOL )
                    return ERR_DIST_CODE;
                if( B.over( ) )
                    return ERR_INPUT_END;
                if( d >= 30 )
                    return ERR_DIST_CODE;
                // distance 1 .. 32 768: symbols 0 .. 3 one each, then two symbols per number of extra bits
                const uint32_t de = d < 4 ? 0u : ( d >> 1 ) - 1u;
                const uint32_t uiDist = ( d < 4 ? 1u + d : 1u + ( ( 2u + ( d & 1u ) ) << de ) ) + B.take( de );
                if( B.over( ) )
                    return ERR_INPUT_END;
                if( uiDist > uiOut )
                    return ERR_DIST_FAR;
                if( uiOut + uiLen > uiIsize )
                    return ERR_LENGTH;
                for( uint32_t k = 0; k < uiLen; k++, uiOut++ ) // (byte by byte: a copy may overlap itself)
                    rSink.put( uiOut, rSink.get( uiOut - uiDist ) );
            }
        }
        if( uiLast )
            break;
    }
    if( ( B.uiUsed + 7u ) / 8u != rSrc.size( ) )
        return ERR_TRAILING;
    return uiOut != uiIsize ? (uint32_t)ERR_LENGTH : (uint32_t)OK;
}

// ---- the serial driver ----------------------------------------------------------------------------------------------------------
struct Result
{
    uint64_t uiMembers, uiBytes; // members walked, bytes of text (the sum of ISIZE)
    uint32_t uiReason; // OK, or the refusal:
    uint64_t uiMember, uiByte; // 0-based member, offset of its first byte
};
// one member with its trailer's checks: pOut holds rM.uiIsize bytes
inline uint32_t inflateMember( const uint8_t* pData, const Member& rM, uint8_t* pOut )
{
    HostTables xTables;
    memset( xTables.a, 0, sizeof( xTables.a ) );
    const ByteSource xSrc = { pData + rM.uiDeflate, rM.uiDeflateBytes };
    ByteSink xSink = { pOut };
    const uint32_t uiReason = inflate( xSrc, xSink, xTables, rM.uiIsize );
    if( uiReason != OK )
        return uiReason;
    return crcOf( pOut, rM.uiIsize ) != rM.uiCrc ? (uint32_t)ERR_CRC : (uint32_t)OK;
}
// Walks the members of n bytes and, with pOut, inflates them in order as the kernels do.  Returns 0 and fills *pResult, or
// returns 1 with the refusal in *pResult (message( ) words it): the first bad header if there is one (no member behind it can
// be found, and ma_batch_set_reads_bgzf launches nothing then), else the lowest member whose stream or trailer is refused.
// Call with pOut == NULL first for the size (headers only).
inline int inflateHost( const uint8_t* pData, uint64_t n, uint8_t* pOut, Result* pResult )
{
    Result r = { 0, 0, OK, 0, 0 };
    uint64_t uiKey = NO_VIOLATION, uiKeyByte = 0;
    for( uint64_t uiAt = 0, k = 0; pOut != NULL && uiAt < n; k++ )
    {
        Member m;
        const uint32_t uiReason = header( pData, n, uiAt, &m );
        if( uiReason != OK )
        {
            r.uiReason = uiReason, r.uiMember = k, r.uiByte = uiAt;
            *pResult = r;
            return 1;
        }
        uiAt += m.uiBytes;
    }
    for( uint64_t uiAt = 0; uiAt < n; )
    {
        Member m;
        const uint32_t uiReason = header( pData, n, uiAt, &m );
        if( uiReason != OK )
        {
            uiKey = key( r.uiMembers, uiReason ), uiKeyByte = uiAt;
            break;
        }
        if( pOut )
        {
            const uint32_t uiStream = inflateMember( pData, m, pOut + r.uiBytes );
            if( uiStream != OK && key( r.uiMembers, uiStream ) < uiKey )
                uiKey = key( r.uiMembers, uiStream ), uiKeyByte = uiAt;
        }
        r.uiMembers++;
        r.uiBytes += m.uiIsize;
        uiAt += m.uiBytes;
    }
    if( uiKey != NO_VIOLATION )
    {
        r.uiReason = (uint32_t)( uiKey & 0xffu );
        r.uiMember = uiKey >> 8;
        r.uiByte = uiKeyByte;
        *pResult = r;
        return 1;
    }
    *pResult = r;
    return 0;
}
} // namespace ma_bgzf
