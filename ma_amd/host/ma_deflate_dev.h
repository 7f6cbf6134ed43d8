// ma_deflate_dev.h -- the rules of ma_sam_bgzf_batch and ma_bgzf_deflate, written ONCE: how a text is cut into BGZF members, which
// LZ77 parse a member gets, which Huffman codes, and which bytes that makes.  Its users:
//   - the kernels of ma_amd/csrc/stage_deflate.h call its routines, one wavefront per member;
//   - deflateHost( ) below runs the same routines serially: the statement the CPU tests (tests/emul/sam_bgzf_test.cpp) compare with
//     zlib's inflate and the GPU tests with the kernels, byte for byte; the host writers (ma_sam.h) compress with it what they
//     format themselves.
// No zlib, no containers, no strings.  The inflate side, the member form and the CRC32 are ma_bgzf_dev.h's.
//
// THE CUTS  A text of n bytes is cut at fixed offsets: member k holds text[ 65280 k .. min( 65280 ( k + 1 ), n ) ), so there are
//   ceil( n / 65280 ) members and none for n == 0.  65 280 is htslib's block size: the stored form (31 bytes of frame) always
//   fits the 16-bit BSIZE.  Records may straddle members; the members of consecutive texts concatenate to a legal file.
// THE MEMBER  18 header bytes (1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 02 00, BSIZE = size - 1), one raw deflate
//   stream, the CRC32 of the text, ISIZE: what htslib writes and what the strict form of ma_bgzf_dev.h accepts.
// THE STREAM  ONE dynamic-Huffman block over the parse below, or ONE stored block whenever the dynamic form would not be smaller.
//   The size of the dynamic form follows from the symbol histogram and the code lengths (planBits( )) before a bit is written, so the
//   choice and every member's size are known before emission, and no member exceeds its text + 31 bytes.
// THE PARSE is a function of the text alone (the serial statement and the wavefront give the same tokens):
//   positions are taken in strips of 64.  A position p with 4 bytes behind it has a hash of them; the table holds, per hash, the
//   latest position of the COMPLETED strips (it is updated after a strip, the highest position wins).  p has at most two
//   candidates: the table's entry for its hash if it is at most 32 768 back, and p - 1 (runs).  The length of a candidate is the
//   common prefix, capped at 258 and at the member's end; it counts from 4 bytes on, and a 4-byte match further back than 4 096
//   does not count (its distance bits cost more than the literals).  The longer candidate wins, p - 1 on a tie.  The walk is
//   greedy, left to right: a counting match at p is taken and the walk goes on behind it, else text[ p ] is a literal.
// THE CODES  Huffman lengths from the histogram of the tokens (two-queue construction over the symbols ranked by ( count, symbol )),
//   limited to 15 -- 7 for the code-length code -- the way zlib's gen_bitlen limits them, then handed out by rank; canonical
//   codes.  An alphabet with fewer than two used symbols gets what zlib's deflate gives it: a second (or two) symbols of count 1,
//   so a block without matches has two distance codes of length 1.  The code lengths are written as ONE sequence of
//   HLIT + HDIST lengths, runs coded greedily (18 for 11..138 zeros, 17 for 3..10, 16 for 3..6 repeats of a length).
#pragma once

#include "ma_bgzf_dev.h"

namespace ma_bgzf
{
static const uint32_t DEFLATE_CHUNK = 65280u; // text bytes per member
static const uint32_t MEMBER_FRAME = 26u, STORED_FRAME = 31u, MEMBER_HEAD = 18u, EOF_BYTES = 28u;
static const uint32_t HASH_BITS = 13u, HASH_SIZE = 1u << HASH_BITS, NO_POS = 0xffffu;
static const uint32_t STRIP = 64u, MIN_MATCH = 4u, MAX_MATCH = 258u, MAX_DIST = 32768u, FAR_DIST = 4096u;
static const uint32_t N_LITLEN = 286u, N_DIST = 30u, N_CODELEN = 19u, END_OF_BLOCK = 256u;
// the three alphabets side by side in the arrays of DeflateWork
static const uint32_t A_LITLEN = 0u, A_DIST = N_LITLEN, A_CODELEN = N_LITLEN + N_DIST, A_ALL = N_LITLEN + N_DIST + N_CODELEN;

// the end-of-file marker: an empty member
MA_BGZF_HD uint8_t eofByte( uint32_t i )
{
    return i == 0 ? 0x1f : i == 1 ? 0x8b : i == 2 ? 0x08 : i == 3 ? 0x04 : i == 9 ? 0xff : i == 10 ? 0x06 : i == 12 ? 0x42 : i == 13 ? 0x43 :
           i == 14 ? 0x02 : i == 16 ? 0x1b : i == 18 ? 0x03 : 0x00;
}
MA_BGZF_HD uint64_t deflateMembers( uint64_t n )
{
    return ( n + DEFLATE_CHUNK - 1 ) / DEFLATE_CHUNK;
}
MA_BGZF_HD uint32_t memberText( uint64_t n, uint64_t k ) // the text bytes of member k
{
    const uint64_t uiLeft = n - k * DEFLATE_CHUNK;
    return uiLeft < DEFLATE_CHUNK ? (uint32_t)uiLeft : DEFLATE_CHUNK;
}

// ---- the parse ------------------------------------------------------------------------------------------------------------------
MA_BGZF_HD uint32_t hashOf( const uint8_t* p ) // of p[ 0 .. 3 ]
{
    const uint32_t w = (uint32_t)p[ 0 ] | ( (uint32_t)p[ 1 ] << 8 ) | ( (uint32_t)p[ 2 ] << 16 ) | ( (uint32_t)p[ 3 ] << 24 );
    return ( w * 2654435761u ) >> ( 32u - HASH_BITS );
}
MA_BGZF_HD uint32_t commonPrefix( const uint8_t* a, const uint8_t* b, uint32_t uiCap )
{
    uint32_t l = 0;
    while( l < uiCap && a[ l ] == b[ l ] )
        l++;
    return l;
}
// the match at position p of the member T of n bytes (p < n); uiCand: the table's entry for p's hash, or NO_POS.  *pLen is 0
// when nothing counts.
MA_BGZF_HD void findMatch( const uint8_t* T, uint32_t n, uint32_t p, uint32_t uiCand, uint32_t* pLen, uint32_t* pDist )
{
    const uint32_t uiCap = n - p < MAX_MATCH ? n - p : MAX_MATCH;
    uint32_t uiBest = 0, uiDist = 0;
    if( uiCap >= MIN_MATCH )
    {
        if( p >= 1 )
        {
            const uint32_t l = commonPrefix( T + p - 1, T + p, uiCap );
            if( l >= MIN_MATCH )
                uiBest = l, uiDist = 1;
        }
        if( uiCand != NO_POS && uiCand < p && p - uiCand <= MAX_DIST )
        {
            const uint32_t l = commonPrefix( T + uiCand, T + p, uiCap );
            if( l > uiBest && l >= MIN_MATCH && !( l == MIN_MATCH && p - uiCand > FAR_DIST ) )
                uiBest = l, uiDist = p - uiCand;
        }
    }
    *pLen = uiBest;
    *pDist = uiDist;
}
// a token: a literal is its byte; a match is length << 16 | distance - 1
MA_BGZF_HD uint32_t matchToken( uint32_t uiLen, uint32_t uiDist )
{
    return ( uiLen << 16 ) | ( uiDist - 1u );
}
MA_BGZF_HD uint32_t log2Of( uint32_t v ) // v > 0
{
    return 31u - (uint32_t)__builtin_clz( v );
}
// length 3 .. 258 -> symbol 257 .. 285, its extra bits and their value
MA_BGZF_HD uint32_t lengthSymbol( uint32_t uiLen, uint32_t* pExtra, uint32_t* pValue )
{
    const uint32_t l = uiLen - 3u;
    if( l < 8u || uiLen == MAX_MATCH )
    {
        *pExtra = 0, *pValue = 0;
        return uiLen == MAX_MATCH ? 285u : 257u + l;
    }
    const uint32_t e = log2Of( l ) - 2u;
    *pExtra = e, *pValue = l & ( ( 1u << e ) - 1u );
    return 261u + 4u * e + ( ( l >> e ) & 3u );
}
// distance 1 .. 32 768 -> symbol 0 .. 29
MA_BGZF_HD uint32_t distSymbol( uint32_t uiDist, uint32_t* pExtra, uint32_t* pValue )
{
    const uint32_t d = uiDist - 1u;
    if( d < 4u )
    {
        *pExtra = 0, *pValue = 0;
        return d;
    }
    const uint32_t e = log2Of( d ) - 1u;
    *pExtra = e, *pValue = d & ( ( 1u << e ) - 1u );
    return 2u * e + 2u + ( ( d >> e ) & 1u );
}
MA_BGZF_HD uint32_t lengthExtraOf( uint32_t uiSym ) // of a literal/length symbol
{
    return uiSym < 265u || uiSym == 285u ? 0u : ( uiSym - 261u ) >> 2;
}
MA_BGZF_HD uint32_t distExtraOf( uint32_t uiSym )
{
    return uiSym < 4u ? 0u : ( uiSym >> 1 ) - 1u;
}

// ---- the codes ------------------------------------------------------------------------------------------------------------------
// Everything one member's code construction needs: the host keeps it on the stack, a wavefront in LDS (6.3 KiB)
struct DeflateWork
{
    uint32_t aCount[ A_ALL ]; // the histogram of the tokens (and of the header's code-length symbols)
    uint32_t aNode[ 2 * N_LITLEN ]; // the tree: counts of the leaves (in rank order), then of the inner nodes
    uint16_t aCode[ A_ALL ]; // the codes, bit-reversed: as they go into the stream
    uint16_t aOrder[ N_LITLEN ]; // the used symbols of an alphabet by ( count, symbol )
    uint16_t aParent[ 2 * N_LITLEN ]; // per node its parent, then its depth
    uint16_t aPerLength[ 16 ], aNext[ 16 ];
    uint8_t aLength[ A_ALL ];
    uint32_t uiLit, uiDist, uiCodeLens; // HLIT + 257, HDIST + 1, HCLEN + 4
};
// the place of symbol s among the used symbols of the alphabet at uiBase, by ( count, symbol ): one symbol per call, so that the
// lanes of a wavefront share the work
MA_BGZF_HD uint32_t rankOf( const DeflateWork& W, uint32_t uiBase, uint32_t n, uint32_t s )
{
    const uint32_t c = W.aCount[ uiBase + s ];
    uint32_t r = 0;
    for( uint32_t t = 0; t < n; t++ )
    {
        const uint32_t ct = W.aCount[ uiBase + t ];
        r += ( ct != 0 && ( ct < c || ( ct == c && t < s ) ) ) ? 1u : 0u;
    }
    return r;
}
// zlib's padding (trees.c, build_tree): an alphabet with fewer than two used symbols gets symbols of count 1 until it has two
MA_BGZF_HD void padAlphabet( DeflateWork& W, uint32_t uiBase, uint32_t n )
{
    uint32_t uiUsed = 0;
    int32_t iMax = -1;
    for( uint32_t s = 0; s < n; s++ )
        if( W.aCount[ uiBase + s ] != 0 )
            uiUsed++, iMax = (int32_t)s;
    while( uiUsed < 2 )
    {
        const uint32_t s = iMax < 2 ? (uint32_t)++iMax : 0u;
        W.aCount[ uiBase + s ] = 1;
        uiUsed++;
    }
}
// the code lengths of the alphabet at uiBase from its counts; aOrder holds its m >= 2 used symbols by rank (rankOf)
MA_BGZF_HD void lengthsOf( DeflateWork& W, uint32_t uiBase, uint32_t n, uint32_t m, uint32_t uiMaxLength )
{
    for( uint32_t s = 0; s < n; s++ )
        W.aLength[ uiBase + s ] = 0;
    for( uint32_t i = 0; i < m; i++ )
        W.aNode[ i ] = W.aCount[ uiBase + W.aOrder[ i ] ];
    // two queues: the leaves by rank, the inner nodes in the order they are made (their counts never decrease); a leaf wins a tie
    uint32_t uiLeaf = 0, uiInner = m;
    for( uint32_t k = m; k < 2 * m - 1; k++ )
    {
        uint32_t uiSum = 0;
        for( uint32_t j = 0; j < 2; j++ )
        {
            uint32_t uiPick;
            if( uiLeaf < m && ( uiInner >= k || W.aNode[ uiLeaf ] <= W.aNode[ uiInner ] ) )
                uiPick = uiLeaf++;
            else
                uiPick = uiInner++;
            uiSum += W.aNode[ uiPick ];
            W.aParent[ uiPick ] = (uint16_t)k;
        }
        W.aNode[ k ] = uiSum;
    }
    // depths from the root down, cut at the limit (gen_bitlen of zlib's trees.c counts the nodes it cuts, leaves and inner ones)
    for( uint32_t l = 0; l < 16; l++ )
        W.aPerLength[ l ] = 0;
    int32_t iOverflow = 0;
    W.aParent[ 2 * m - 2 ] = 0;
    for( uint32_t i = 2 * m - 2; i-- > 0; )
    {
        uint32_t d = (uint32_t)W.aParent[ W.aParent[ i ] ] + 1u;
        if( d > uiMaxLength )
            d = uiMaxLength, iOverflow++;
        W.aParent[ i ] = (uint16_t)d;
        if( i < m )
            W.aPerLength[ d ]++;
    }
    while( iOverflow > 0 )
    {
        uint32_t l = uiMaxLength - 1;
        while( l > 0 && W.aPerLength[ l ] == 0 )
            l--;
        if( l == 0 ) // (cannot be: a cut node has a leaf above the limit's level beside its ancestors)
            break;
        W.aPerLength[ l ]--; // one leaf moves down and takes a cut leaf as its brother
        W.aPerLength[ l + 1 ] += 2;
        W.aPerLength[ uiMaxLength ]--;
        iOverflow -= 2;
    }
    // the rarest symbols get the longest codes
    uint32_t i = 0;
    for( uint32_t l = uiMaxLength; l >= 1; l-- )
        for( uint32_t c = W.aPerLength[ l ]; c != 0; c-- )
            W.aLength[ uiBase + W.aOrder[ i++ ] ] = (uint8_t)l;
}
// canonical codes from the lengths, bit-reversed
MA_BGZF_HD void codesOf( DeflateWork& W, uint32_t uiBase, uint32_t n )
{
    for( uint32_t l = 0; l < 16; l++ )
        W.aPerLength[ l ] = 0;
    for( uint32_t s = 0; s < n; s++ )
        W.aPerLength[ W.aLength[ uiBase + s ] ]++;
    uint32_t uiCode = 0;
    W.aPerLength[ 0 ] = 0;
    for( uint32_t l = 1; l < 16; l++ )
    {
        uiCode = ( uiCode + W.aPerLength[ l - 1 ] ) << 1;
        W.aNext[ l ] = (uint16_t)uiCode;
    }
    for( uint32_t s = 0; s < n; s++ )
    {
        const uint32_t l = W.aLength[ uiBase + s ];
        uint32_t c = 0;
        if( l != 0 )
        {
            const uint32_t v = W.aNext[ l ]++;
            for( uint32_t k = 0; k < l; k++ )
                c |= ( ( v >> k ) & 1u ) << ( l - 1 - k );
        }
        W.aCode[ uiBase + s ] = (uint16_t)c;
    }
}
// one alphabet, serially: padding, ranks, lengths, codes.  (The kernel spreads rankOf over its lanes and calls the rest.)
MA_BGZF_HD uint32_t rankAll( DeflateWork& W, uint32_t uiBase, uint32_t n )
{
    uint32_t m = 0;
    for( uint32_t s = 0; s < n; s++ )
        if( W.aCount[ uiBase + s ] != 0 )
        {
            W.aOrder[ rankOf( W, uiBase, n, s ) ] = (uint16_t)s;
            m++;
        }
    return m;
}
MA_BGZF_HD uint32_t usedOf( const DeflateWork& W, uint32_t uiBase, uint32_t n )
{
    uint32_t m = 0;
    for( uint32_t s = 0; s < n; s++ )
        m += W.aCount[ uiBase + s ] != 0 ? 1u : 0u;
    return m;
}

// the header's code lengths as code-length symbols: f( symbol, extra bits, value ) for each, runs coded greedily
template <typename F> MA_BGZF_HD void codeLengthRuns( const DeflateWork& W, F&& f )
{
    const uint32_t uiTotal = W.uiLit + W.uiDist;
    uint32_t i = 0;
    while( i < uiTotal )
    {
        const uint32_t l = W.aLength[ i < W.uiLit ? i : A_DIST + ( i - W.uiLit ) ];
        uint32_t uiRun = 1;
        while( i + uiRun < uiTotal )
        {
            const uint32_t j = i + uiRun;
            if( W.aLength[ j < W.uiLit ? j : A_DIST + ( j - W.uiLit ) ] != l )
                break;
            uiRun++;
        }
        i += uiRun;
        if( l == 0 )
        {
            while( uiRun >= 11 )
            {
                const uint32_t r = uiRun < 138 ? uiRun : 138;
                f( 18u, 7u, r - 11 );
                uiRun -= r;
            }
            if( uiRun >= 3 )
            {
                f( 17u, 3u, uiRun - 3 );
                uiRun = 0;
            }
        }
        else
        {
            f( l, 0u, 0u );
            uiRun--;
            while( uiRun >= 3 )
            {
                const uint32_t r = uiRun < 6 ? uiRun : 6;
                f( 16u, 2u, r - 3 );
                uiRun -= r;
            }
        }
        for( ; uiRun != 0; uiRun-- )
            f( l, 0u, 0u );
    }
}
struct CountRuns
{
    DeflateWork& W;
    MA_BGZF_HD void operator( )( uint32_t s, uint32_t, uint32_t )
    {
        W.aCount[ A_CODELEN + s ]++;
    }
};

// After the literal/length and distance lengths: HLIT, HDIST, and the histogram of the code-length symbols
MA_BGZF_HD void planHeader( DeflateWork& W )
{
    uint32_t uiLit = N_LITLEN, uiDist = N_DIST;
    while( uiLit > 257 && W.aLength[ A_LITLEN + uiLit - 1 ] == 0 )
        uiLit--;
    while( uiDist > 1 && W.aLength[ A_DIST + uiDist - 1 ] == 0 )
        uiDist--;
    W.uiLit = uiLit, W.uiDist = uiDist;
    for( uint32_t s = 0; s < N_CODELEN; s++ )
        W.aCount[ A_CODELEN + s ] = 0;
    CountRuns xCount = { W };
    codeLengthRuns( W, xCount );
}
// After the code-length code: HCLEN, and the bits of the whole dynamic block.  The counts of the literal/length and distance
// alphabets must be the tokens' again (the padding taken back) with the end-of-block symbol counted once.
MA_BGZF_HD uint64_t planBits( DeflateWork& W )
{
    uint32_t uiCodeLens = N_CODELEN;
    while( uiCodeLens > 4 && W.aLength[ A_CODELEN + codeLengthOrder( uiCodeLens - 1 ) ] == 0 )
        uiCodeLens--;
    W.uiCodeLens = uiCodeLens;
    uint64_t uiBits = 3 + 5 + 5 + 4 + 3 * uiCodeLens;
    for( uint32_t s = 0; s < N_CODELEN; s++ )
        uiBits += (uint64_t)W.aCount[ A_CODELEN + s ] * ( W.aLength[ A_CODELEN + s ] + ( s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u ) );
    for( uint32_t s = 0; s < N_LITLEN; s++ )
        uiBits += (uint64_t)W.aCount[ A_LITLEN + s ] * ( W.aLength[ A_LITLEN + s ] + lengthExtraOf( s ) );
    for( uint32_t s = 0; s < N_DIST; s++ )
        uiBits += (uint64_t)W.aCount[ A_DIST + s ] * ( W.aLength[ A_DIST + s ] + distExtraOf( s ) );
    return uiBits;
}
// the deflate bytes of a member of n text bytes whose dynamic form has uiBits bits: that form if it is smaller than the stored one
MA_BGZF_HD uint32_t deflateBytesOf( uint32_t n, uint64_t uiBits, bool* pStored )
{
    const uint64_t uiDynamic = ( uiBits + 7 ) / 8;
    *pStored = uiDynamic >= (uint64_t)n + 5u;
    return *pStored ? n + 5u : (uint32_t)uiDynamic;
}

// Serially, all of the above for one member whose counts of literal/length (with the end of block) and distance symbols are in W
MA_BGZF_HD uint64_t planSerial( DeflateWork& W )
{
    uint32_t aTrue[ 3 ] = { W.aCount[ A_DIST ], W.aCount[ A_DIST + 1 ], W.aCount[ A_DIST + 2 ] };
    lengthsOf( W, A_LITLEN, N_LITLEN, rankAll( W, A_LITLEN, N_LITLEN ), 15 ); // (a member has a literal and the end of block)
    codesOf( W, A_LITLEN, N_LITLEN );
    padAlphabet( W, A_DIST, N_DIST );
    lengthsOf( W, A_DIST, N_DIST, rankAll( W, A_DIST, N_DIST ), 15 );
    codesOf( W, A_DIST, N_DIST );
    for( uint32_t s = 0; s < 3; s++ ) // (padding touches symbols 0 .. 2 only)
        W.aCount[ A_DIST + s ] = aTrue[ s ];
    planHeader( W );
    padAlphabet( W, A_CODELEN, N_CODELEN );
    lengthsOf( W, A_CODELEN, N_CODELEN, rankAll( W, A_CODELEN, N_CODELEN ), 7 );
    codesOf( W, A_CODELEN, N_CODELEN );
    // (a padded code-length symbol is never written: its count goes back to 0 for the sum)
    planHeader( W );
    return planBits( W );
}

// ---- the bits -------------------------------------------------------------------------------------------------------------------
// bits into at most uiCap bytes behind p (uiBytes goes on counting beyond them)
struct BitWriter
{
    uint8_t* p;
    uint32_t uiCap, uiBytes;
    uint64_t uiAcc;
    uint32_t uiCnt; // < 8 between calls
    MA_BGZF_HD void put( uint64_t v, uint32_t n ) // n <= 48
    {
        uiAcc |= v << uiCnt;
        uiCnt += n;
        while( uiCnt >= 8 )
        {
            if( uiBytes < uiCap )
                p[ uiBytes ] = (uint8_t)uiAcc;
            uiBytes++;
            uiAcc >>= 8;
            uiCnt -= 8;
        }
    }
    MA_BGZF_HD void finish( )
    {
        if( uiCnt != 0 )
            put( 0, 8 - uiCnt );
    }
};
struct WriteRuns
{
    const DeflateWork& W;
    BitWriter& B;
    MA_BGZF_HD void operator( )( uint32_t s, uint32_t uiExtra, uint32_t uiValue )
    {
        B.put( (uint64_t)W.aCode[ A_CODELEN + s ] | ( (uint64_t)uiValue << W.aLength[ A_CODELEN + s ] ), W.aLength[ A_CODELEN + s ] + uiExtra );
    }
};
// the block header of the dynamic form: BFINAL 1, BTYPE 2, the three counts, the code-length code, the code lengths
MA_BGZF_HD void writeHeader( const DeflateWork& W, BitWriter& B )
{
    B.put( 1u | ( 2u << 1 ), 3 );
    B.put( W.uiLit - 257u, 5 );
    B.put( W.uiDist - 1u, 5 );
    B.put( W.uiCodeLens - 4u, 4 );
    for( uint32_t i = 0; i < W.uiCodeLens; i++ )
        B.put( W.aLength[ A_CODELEN + codeLengthOrder( i ) ], 3 );
    WriteRuns xWrite = { W, B };
    codeLengthRuns( W, xWrite );
}
// a token's bits (at most 48) and their number
MA_BGZF_HD uint64_t tokenBits( const DeflateWork& W, uint32_t uiToken, uint32_t* pBits )
{
    if( uiToken < 256u )
    {
        *pBits = W.aLength[ uiToken ];
        return W.aCode[ uiToken ];
    }
    uint32_t le, lv, de, dv;
    const uint32_t ls = lengthSymbol( uiToken >> 16, &le, &lv ), ds = A_DIST + distSymbol( ( uiToken & 0xffffu ) + 1u, &de, &dv );
    uint64_t v = W.aCode[ ls ];
    uint32_t n = W.aLength[ ls ];
    v |= (uint64_t)lv << n;
    n += le;
    v |= (uint64_t)W.aCode[ ds ] << n;
    n += W.aLength[ ds ];
    v |= (uint64_t)dv << n;
    n += de;
    *pBits = n;
    return v;
}
MA_BGZF_HD void countToken( DeflateWork& W, uint32_t uiToken )
{
    if( uiToken < 256u )
    {
        W.aCount[ uiToken ]++;
        return;
    }
    uint32_t e, v;
    W.aCount[ lengthSymbol( uiToken >> 16, &e, &v ) ]++;
    W.aCount[ A_DIST + distSymbol( ( uiToken & 0xffffu ) + 1u, &e, &v ) ]++;
}

// the 18 bytes in front of the deflate stream and the 8 behind it
MA_BGZF_HD void writeMemberHead( uint8_t* p, uint32_t uiMemberBytes )
{
    for( uint32_t i = 0; i < 16; i++ )
        p[ i ] = eofByte( i );
    p[ 16 ] = (uint8_t)( ( uiMemberBytes - 1u ) & 0xffu );
    p[ 17 ] = (uint8_t)( ( uiMemberBytes - 1u ) >> 8 );
}
MA_BGZF_HD void writeMemberTail( uint8_t* p, uint32_t uiCrc, uint32_t uiIsize )
{
    for( uint32_t i = 0; i < 4; i++ )
    {
        p[ i ] = (uint8_t)( uiCrc >> ( 8 * i ) );
        p[ 4 + i ] = (uint8_t)( uiIsize >> ( 8 * i ) );
    }
}
MA_BGZF_HD void writeStoredHead( uint8_t* p, uint32_t n ) // 5 bytes; the text follows
{
    p[ 0 ] = 1;
    p[ 1 ] = (uint8_t)( n & 0xffu ), p[ 2 ] = (uint8_t)( n >> 8 );
    p[ 3 ] = (uint8_t)( ~n & 0xffu ), p[ 4 ] = (uint8_t)( ( ~n >> 8 ) & 0xffu );
}

// ---- the serial statement -------------------------------------------------------------------------------------------------------
// The tokens of the member T of n bytes (1 <= n <= DEFLATE_CHUNK) into pTokens (n entries) with their counts in W; returns their
// number.  pHash: HASH_SIZE entries.
inline uint32_t parseSerial( const uint8_t* T, uint32_t n, uint16_t* pHash, uint32_t* pTokens, DeflateWork& W )
{
    for( uint32_t h = 0; h < HASH_SIZE; h++ )
        pHash[ h ] = (uint16_t)NO_POS;
    for( uint32_t s = 0; s < A_ALL; s++ )
        W.aCount[ s ] = 0;
    uint32_t uiTokens = 0, uiPos = 0;
    for( uint32_t uiBase = 0; uiBase < n; uiBase += STRIP )
    {
        const uint32_t uiEnd = uiBase + STRIP < n ? uiBase + STRIP : n;
        while( uiPos < uiEnd )
        {
            uint32_t uiLen, uiDist;
            findMatch( T, n, uiPos, uiPos + 4 <= n ? pHash[ hashOf( T + uiPos ) ] : NO_POS, &uiLen, &uiDist );
            const uint32_t uiToken = uiLen >= MIN_MATCH ? matchToken( uiLen, uiDist ) : T[ uiPos ];
            countToken( W, uiToken );
            pTokens[ uiTokens++ ] = uiToken;
            uiPos += uiLen >= MIN_MATCH ? uiLen : 1u;
        }
        for( uint32_t p = uiBase; p < uiEnd && p + 4 <= n; p++ )
            pHash[ hashOf( T + p ) ] = (uint16_t)p;
    }
    W.aCount[ END_OF_BLOCK ] = 1;
    return uiTokens;
}
struct DeflateScratch // deflateHost's, so that a caller with many texts allocates once
{
    uint16_t aHash[ HASH_SIZE ];
    uint32_t aTokens[ DEFLATE_CHUNK ];
    DeflateWork xWork;
};
// One member: its bytes into pOut (room for n + STORED_FRAME), returns their number
inline uint32_t deflateMember( const uint8_t* T, uint32_t n, uint8_t* pOut, DeflateScratch& S )
{
    DeflateWork& W = S.xWork;
    const uint32_t uiTokens = parseSerial( T, n, S.aHash, S.aTokens, W );
    bool bStored;
    const uint32_t uiDeflate = deflateBytesOf( n, planSerial( W ), &bStored );
    const uint32_t uiMember = MEMBER_FRAME + uiDeflate;
    writeMemberHead( pOut, uiMember );
    uint8_t* const pStream = pOut + MEMBER_HEAD;
    if( bStored )
    {
        writeStoredHead( pStream, n );
        memcpy( pStream + 5, T, n );
    }
    else
    {
        BitWriter B = { pStream, uiDeflate, 0, 0, 0 };
        writeHeader( W, B );
        for( uint32_t i = 0; i < uiTokens; i++ )
        {
            uint32_t uiBits;
            const uint64_t v = tokenBits( W, S.aTokens[ i ], &uiBits );
            B.put( v, uiBits );
        }
        B.put( W.aCode[ END_OF_BLOCK ], W.aLength[ END_OF_BLOCK ] );
        B.finish( );
    }
    writeMemberTail( pStream + uiDeflate, crcOf( T, n ), n );
    return uiMember;
}
// The members of a text of n bytes, packed back to back into pOut (room for n + STORED_FRAME * deflateMembers( n ) bytes);
// pMemberOff, if given, gets deflateMembers( n ) + 1 offsets.  Returns the bytes written.
inline uint64_t deflateHost( const uint8_t* pText, uint64_t n, uint8_t* pOut, uint64_t* pMemberOff )
{
    DeflateScratch* const pS = new DeflateScratch;
    uint64_t uiOut = 0;
    const uint64_t uiMembers = deflateMembers( n );
    for( uint64_t k = 0; k < uiMembers; k++ )
    {
        if( pMemberOff )
            pMemberOff[ k ] = uiOut;
        uiOut += deflateMember( pText + k * DEFLATE_CHUNK, memberText( n, k ), pOut + uiOut, *pS );
    }
    if( pMemberOff )
        pMemberOff[ uiMembers ] = uiOut;
    delete pS;
    return uiOut;
}
MA_BGZF_HD uint64_t deflateBound( uint64_t n )
{
    return n + STORED_FRAME * deflateMembers( n );
}
inline void writeEof( uint8_t* p )
{
    for( uint32_t i = 0; i < EOF_BYTES; i++ )
        p[ i ] = eofByte( i );
}
} // namespace ma_bgzf
