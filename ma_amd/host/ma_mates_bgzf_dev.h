// ma_mates_bgzf_dev.h -- the rules of ma_batch_set_mates_bgzf, written ONCE: the two BGZF-compressed read files of a paired-end
// run.  Nothing new is decided here: ma_bgzf::inflateHost (ma_bgzf_dev.h) per side, head and drop, ma_text::pairHost
// (ma_text_dev.h) on the two texts, and the order in which the refusals of the two win over each other.  Its users:
//   - pairBgzfHost( ) is the serial statement the GPU tests compare the kernels with; tests/emul/mates_bgzf_test.cpp pins it to
//     zlib and to pairHost;
//   - libma_amd.so words a refusal with message( ) and the functions it calls.
// No zlib, no containers, no strings.
//
// For each side i, T_i = head_i followed by what members_i inflate to, minus its last drop_i bytes (ma_batch_set_reads_bgzf's
// definition, the same strict member form).  The call then is ma_batch_set_mates_text( T_1, T_2 ).  THE ORDER OF THE REFUSALS:
//   1  a bad member header: text 1's first, else text 2's first (nothing is inflated then); otherwise the lowest member of text
//      1 whose stream or trailer is refused, else the lowest of text 2
//   2  a drop larger than the inflated part of the text: text 1, else text 2
//   3  the refusals of ma_batch_set_mates_text on ( T_1, T_2 ), in its order: a line of text 1, a line of text 2, the kinds, the
//      capacity (the library's check; pairBgzfHost knows no batch)
// so a member that does not inflate wins over every rule of the text: a text that did not inflate is not parsed.  One exception:
// a T_i of 2 GiB or more (known from the headers alone) is refused BEFORE anything is inflated, behind a bad header and before
// everything else -- text 1, else text 2, with ma_text::ERR_TOO_LARGE at line 1.
#pragma once
#include "ma_bgzf_dev.h"
#include "ma_text_dev.h"

namespace ma_bgzf
{
enum : uint32_t // why a paired call is refused
{
    PAIR_OK = 0u,
    PAIR_MEMBER = 1u, // uiText, uiMember, uiByte, uiReason (ma_bgzf::ERR_*)
    PAIR_DROP = 2u, // uiText
    PAIR_TEXT = 3u // xPair holds the refusal of ma_text::pairHost (or MATES_LINE / ERR_TOO_LARGE)
};
struct PairSide
{
    const char* pHead;
    uint64_t uiHead;
    const uint8_t* pMembers;
    uint64_t uiBytes, uiDrop;
};
struct PairBgzfResult
{
    uint32_t uiRefusal; // PAIR_*
    uint32_t uiText, uiReason; // PAIR_MEMBER, PAIR_DROP: 1 or 2; PAIR_MEMBER: the reason
    uint64_t uiMember, uiByte; // PAIR_MEMBER: 0-based member of that text, offset of its first byte in that text's members
    uint64_t aTextBytes[ 2 ]; // |T_i| (0 after a refusal)
    ma_text::PairResult xPair; // the pairs (all zero after a refusal that is not PAIR_TEXT)
};
// "ma_batch_set_mates_bgzf: text <1|2>: n_drop is larger than the inflated part of the text"
inline void messageMatesDrop( char* pOut, size_t uiCap, uint32_t uiText )
{
    snprintf( pOut, uiCap, "ma_batch_set_mates_bgzf: text %u: n_drop is larger than the inflated part of the text", (unsigned)uiText );
}
// the words of a refusal of pairBgzfHost into pOut (at least 320 bytes): what ma_last_error( ) says after ma_batch_set_mates_bgzf
inline void messagePair( char* pOut, size_t uiCap, const PairBgzfResult& r )
{
    if( r.uiRefusal == PAIR_MEMBER )
        messageMates( pOut, uiCap, r.uiText, r.uiMember, r.uiByte, r.uiReason );
    else if( r.uiRefusal == PAIR_DROP )
        messageMatesDrop( pOut, uiCap, r.uiText );
    else
        ma_text::messageMatesOf( pOut, uiCap, "ma_batch_set_mates_bgzf", r.xPair.uiRefusal, r.xPair.uiText, r.xPair.uiLine, r.xPair.uiByte,
                                 r.xPair.uiReason );
}
// The serial statement of ma_batch_set_mates_bgzf.  Returns 0 and fills *pResult, apText (T_1 and T_2, malloc'ed: the caller
// frees them; a streaming caller's rest is apText[ i ] + xPair.aConsumed[ i ]) and the arrays that are not NULL as pairHost does
// (call with NULLs first for the sizes), or returns 1 with the refusal in *pResult (messagePair( ) words it), apText NULL and
// the arrays untouched.
inline int pairBgzfHost( const PairSide aSide[ 2 ], int32_t iRevComp, char* apText[ 2 ], uint64_t* pOffsets, uint8_t* pCodes, uint64_t* pNameOff,
                         char* pNames, uint8_t* pQual, PairBgzfResult* pResult )
{
    PairBgzfResult r;
    memset( &r, 0, sizeof( r ) );
    apText[ 0 ] = apText[ 1 ] = NULL;
    *pResult = r;
    Result aWalk[ 2 ];
    for( int i = 0; i < 2 && r.uiRefusal == PAIR_OK; i++ ) // the headers: nothing is decoded
        if( inflateHost( aSide[ i ].pMembers, aSide[ i ].uiBytes, NULL, &aWalk[ i ] ) )
        {
            r.uiRefusal = PAIR_MEMBER, r.uiText = (uint32_t)i + 1;
            r.uiReason = aWalk[ i ].uiReason, r.uiMember = aWalk[ i ].uiMember, r.uiByte = aWalk[ i ].uiByte;
        }
    for( int i = 0; i < 2 && r.uiRefusal == PAIR_OK; i++ )
        if( aSide[ i ].uiDrop <= aWalk[ i ].uiBytes && aSide[ i ].uiHead + aWalk[ i ].uiBytes - aSide[ i ].uiDrop > ma_text::MAX_TEXT_BYTES )
        {
            r.uiRefusal = PAIR_TEXT;
            r.xPair.uiRefusal = ma_text::MATES_LINE, r.xPair.uiText = (uint32_t)i + 1, r.xPair.uiReason = ma_text::ERR_TOO_LARGE;
        }
    uint8_t* apWhole[ 2 ] = { NULL, NULL }; // head + everything the members inflate to
    for( int i = 0; i < 2 && r.uiRefusal == PAIR_OK; i++ )
        apWhole[ i ] = (uint8_t*)malloc( aSide[ i ].uiHead + aWalk[ i ].uiBytes + 1 );
    for( int i = 0; i < 2 && r.uiRefusal == PAIR_OK; i++ )
    {
        if( aSide[ i ].uiHead )
            memcpy( apWhole[ i ], aSide[ i ].pHead, aSide[ i ].uiHead );
        Result xInflated;
        if( inflateHost( aSide[ i ].pMembers, aSide[ i ].uiBytes, apWhole[ i ] + aSide[ i ].uiHead, &xInflated ) )
        {
            r.uiRefusal = PAIR_MEMBER, r.uiText = (uint32_t)i + 1;
            r.uiReason = xInflated.uiReason, r.uiMember = xInflated.uiMember, r.uiByte = xInflated.uiByte;
        }
    }
    for( int i = 0; i < 2 && r.uiRefusal == PAIR_OK; i++ )
        if( aSide[ i ].uiDrop > aWalk[ i ].uiBytes )
            r.uiRefusal = PAIR_DROP, r.uiText = (uint32_t)i + 1;
    if( r.uiRefusal == PAIR_OK )
    {
        const uint64_t aN[ 2 ] = { aSide[ 0 ].uiHead + aWalk[ 0 ].uiBytes - aSide[ 0 ].uiDrop, aSide[ 1 ].uiHead + aWalk[ 1 ].uiBytes - aSide[ 1 ].uiDrop };
        if( ma_text::pairHost( (const char*)apWhole[ 0 ], aN[ 0 ], (const char*)apWhole[ 1 ], aN[ 1 ], iRevComp, pOffsets, pCodes, pNameOff, pNames, pQual,
                               &r.xPair ) )
            r.uiRefusal = PAIR_TEXT;
        else
            r.aTextBytes[ 0 ] = aN[ 0 ], r.aTextBytes[ 1 ] = aN[ 1 ];
    }
    if( r.uiRefusal != PAIR_OK )
    {
        free( apWhole[ 0 ] );
        free( apWhole[ 1 ] );
        *pResult = r;
        return 1;
    }
    apText[ 0 ] = (char*)apWhole[ 0 ], apText[ 1 ] = (char*)apWhole[ 1 ];
    *pResult = r;
    return 0;
}
} // namespace ma_bgzf
