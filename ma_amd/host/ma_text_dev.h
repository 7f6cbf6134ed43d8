// ma_text_dev.h -- the rules of ma_batch_set_reads_text, written ONCE: which FASTQ / FASTA texts the device parses, what it makes
// of them, and how it words a refusal.  Its users:
//   - the kernels of ma_amd/csrc/stage_text.h call the per-line functions, one lane per line, and code( ) per byte;
//   - parseHost( ) below runs the same functions serially: the statement of the rules the CPU tests (tests/emul/text_dev_test.cpp)
//     compare with the yardstick, FileReader::parseRecord of ma_sam.h (fileReader.cpp:37-203), and the GPU tests with the kernels;
//   - libma_amd.so words a refusal with errorText( ) / message( ).
// The rules of ma_batch_set_mates_text -- two such texts interleaved into mate pairs -- follow at the end: pairHost( ), the serial
// statement the k_text_mates_* kernels are compared with (tests/emul/mates_text_test.cpp compares it with PairedFileReader of
// ma_sam.h), and messageMates( ).
// No reference headers, no containers, no strings: include/ma_amd.h only.
//
// The reference's record grammar is a serial state machine; the device serves the two plain shapes real read files have (the
// STRICT form) and refuses every other text, naming a line.  It never guesses.  A text that passes is consumed line by line as
// the reference consumes it, so the names, codes and qualities are the reference's.
//   lines    end with "\n" or "\r\n", the last one may lack its end; a "\r" anywhere else is refused (the reference ends a line
//            at a lone "\r" too: nothing the strict form needs)
//   kind     the first byte of the text: '@' FASTQ, '>' FASTA
//   FASTQ    four lines per record: '@' header; bases; '+' line (anything may follow the '+'); qualities of exactly as many
//            bytes as there are bases, whatever they start with.  The bases line is not empty, does not start with '+', a blank
//            or '@' (the reference would take the first two for the end of the sequence; the third keeps the host's cut at
//            "an '@' line whose next-but-one line starts with '+'" exact) and holds an IUPAC letter.
//   FASTA    '>' header lines; every other line is not empty and does not start with a blank or '@' (the reference ends the
//            sequence at a blank-led line and skips empty ones); every record has a base
//   bases    the bytes of a sequence line up to and including its LAST IUPAC letter (ACGTUNRYKMSWBDHV, either case): trailing
//            junk is dropped, junk in between is kept (sic) and becomes code 4
//   name     the header's bytes from index 1 up to the first ' ' (a tab belongs to the name), or to the line's end
//   codes    A/a 0, C/c 1, G/g 2, T/t 3, every other kept byte 4 (nucSeq.cpp:17-28)
//
// A refusal names the lowest-numbered offending line (1-based), the byte offset of that line's first byte, and one reason: the
// smallest reason code that applies to the line (the enum's order is the order of the checks).  A wrong FASTQ line count is
// attributed to the last line, a FASTA record without bases to its header line; a lower-numbered violation wins over either,
// which is what taking the minimum of key( line, reason ) over all violations gives -- on the device with atomicMin.
#pragma once
#if !defined( MA_AMD_H ) // (libma_amd.so includes it by its own path)
#include "ma_amd.h"
#endif

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#if defined( __HIPCC__ )
#define MA_TEXT_HD __host__ __device__ __forceinline__
#else
#define MA_TEXT_HD inline
#endif

namespace ma_text
{
enum : uint32_t
{
    KIND_FASTQ = 0u,
    KIND_FASTA = 1u
};
enum : uint32_t // the order of the checks of one line
{
    OK = 0u,
    ERR_KIND = 1u, // the text starts with neither '@' nor '>'
    ERR_LONE_CR = 2u, // a '\r' that is not directly followed by '\n'
    ERR_FQ_HEADER = 3u, // FASTQ line 4k does not start with '@'
    ERR_SEQ_EMPTY = 4u, // an empty line where bases are expected (FASTQ line 4k+1, any FASTA line)
    ERR_SEQ_START = 5u, // a sequence line that starts with a blank or '@' (FASTQ: or '+')
    ERR_SEQ_NO_BASES = 6u, // FASTQ line 4k+1 without any IUPAC letter
    ERR_FQ_PLUS = 7u, // FASTQ line 4k+2 does not start with '+'
    ERR_FQ_QUAL_LEN = 8u, // FASTQ line 4k+3 is not as long as the bases
    ERR_FQ_COUNT = 9u, // the number of FASTQ lines is no multiple of four (attributed to the last line)
    ERR_FA_NO_BASES = 10u, // a FASTA record without bases (attributed to its header line)
    ERR_TOO_LARGE = 11u, // the text has 2 GiB or more: line starts and sums are 32-bit words, the scans count with int
    N_REASONS = 12u
};
static const uint64_t NO_VIOLATION = ~(uint64_t)0;
static const uint64_t MAX_TEXT_BYTES = 0x7ffffff0ull;

MA_TEXT_HD const char* errorText( uint32_t uiReason )
{
    switch( uiReason )
    {
        case ERR_KIND:
            return "the text starts with neither '@' (FASTQ) nor '>' (FASTA)";
        case ERR_LONE_CR:
            return "a carriage return that is not followed by a line feed";
        case ERR_FQ_HEADER:
            return "a FASTQ record must start with '@' (four lines per record; multi-line FASTQ is not served)";
        case ERR_SEQ_EMPTY:
            return "an empty line where bases are expected";
        case ERR_SEQ_START:
            return "a sequence line must not start with a blank or '@' (FASTQ: nor with '+')";
        case ERR_SEQ_NO_BASES:
            return "a sequence line without any nucleotide letter";
        case ERR_FQ_PLUS:
            return "the third line of a FASTQ record must start with '+' (multi-line FASTQ is not served)";
        case ERR_FQ_QUAL_LEN:
            return "the quality line is not as long as the bases";
        case ERR_FQ_COUNT:
            return "the number of FASTQ lines is no multiple of four";
        case ERR_FA_NO_BASES:
            return "a FASTA record without bases";
        case ERR_TOO_LARGE:
            return "texts of 2 GiB and more are not served";
        default:
            return "no error";
    }
}

// "<who>: line <L> (byte <X>): <reason>" into pOut (at least 192 bytes); uiLine is 0-based here.  (ma_batch_set_reads_bgzf words
// a violation in its inflated text with it.)
inline void messageOf( char* pOut, size_t uiCap, const char* pWho, uint64_t uiLine, uint64_t uiByte, uint32_t uiReason )
{
    snprintf( pOut, uiCap, "%s: line %llu (byte %llu): %s", pWho, (unsigned long long)( uiLine + 1 ), (unsigned long long)uiByte, errorText( uiReason ) );
}
// "ma_batch_set_reads_text: line <L> (byte <X>): <reason>"
inline void message( char* pOut, size_t uiCap, uint64_t uiLine, uint64_t uiByte, uint32_t uiReason )
{
    messageOf( pOut, uiCap, "ma_batch_set_reads_text", uiLine, uiByte, uiReason );
}

// ---- character classes ------------------------------------------------------------------------------------------------
MA_TEXT_HD bool isIupac( uint8_t c )
{
    const uint32_t f = ( c | 0x20u ) - 'a'; // case-fold; letters a..z -> 0..25
    // a b c d g h k m n r s t u v w y
    const uint32_t uiSet = ( 1u << 0 ) | ( 1u << 1 ) | ( 1u << 2 ) | ( 1u << 3 ) | ( 1u << 6 ) | ( 1u << 7 ) | ( 1u << 10 ) | ( 1u << 12 ) | ( 1u << 13 ) |
                           ( 1u << 17 ) | ( 1u << 18 ) | ( 1u << 19 ) | ( 1u << 20 ) | ( 1u << 21 ) | ( 1u << 22 ) | ( 1u << 24 );
    return ( c & 0xc0u ) == 0x40u && f < 26u && ( ( uiSet >> f ) & 1u ) != 0; // (0x40..0x7f: the fold maps nothing else onto a letter)
}
MA_TEXT_HD uint8_t code( uint8_t c ) // nucSeq.cpp:17-28
{
    const uint8_t f = (uint8_t)( c | 0x20u );
    if( ( c & 0xc0u ) != 0x40u )
        return 4;
    return f == 'a' ? 0 : f == 'c' ? 1 : f == 'g' ? 2 : f == 't' ? 3 : 4;
}
// position p holds a '\r' that no '\n' follows
MA_TEXT_HD bool loneCr( const char* pText, uint64_t n, uint64_t p )
{
    return pText[ p ] == '\r' && ( p + 1 >= n || pText[ p + 1 ] != '\n' );
}

// ---- lines --------------------------------------------------------------------------------------------------------------
// A text of n > 0 bytes has nLines( ) lines; line i is [ start[ i ], start[ i + 1 ] ) WITH its line end, start[ 0 ] = 0, every
// '\n' at p gives a start p + 1, start[ nLines ] = n.  (The kernels and parseHost fill the same array.)
MA_TEXT_HD uint64_t nLines( uint64_t uiLineFeeds, char cLast )
{
    return uiLineFeeds + ( cLast != '\n' ? 1 : 0 );
}
// the length of a line without its end ("\n" or "\r\n")
MA_TEXT_HD uint32_t content( const char* pText, uint64_t uiFrom, uint64_t uiTo )
{
    uint64_t e = uiTo;
    if( e > uiFrom && pText[ e - 1 ] == '\n' )
    {
        e--;
        if( e > uiFrom && pText[ e - 1 ] == '\r' )
            e--;
    }
    return (uint32_t)( e - uiFrom );
}
// kind of a line
enum : uint32_t
{
    LINE_HEADER = 0u,
    LINE_BASES = 1u,
    LINE_PLUS = 2u,
    LINE_QUAL = 3u
};
MA_TEXT_HD uint32_t lineKind( uint32_t uiKind, uint64_t uiLine, const char* pLine, uint32_t uiLen )
{
    if( uiKind == KIND_FASTQ )
        return (uint32_t)( uiLine & 3u );
    return uiLen > 0 && pLine[ 0 ] == '>' ? LINE_HEADER : LINE_BASES;
}
// bytes of a sequence line up to and including its last IUPAC letter.  (One lane walks back over the trailing junk: none in
// real files.)
MA_TEXT_HD uint32_t trimmed( const char* pLine, uint32_t uiLen )
{
    while( uiLen > 0 && !isIupac( (uint8_t)pLine[ uiLen - 1 ] ) )
        uiLen--;
    return uiLen;
}
// bytes of a header's name: from index 1 to the first ' ' or the line's end
MA_TEXT_HD uint32_t nameLength( const char* pLine, uint32_t uiLen )
{
    uint32_t e = 1;
    while( e < uiLen && pLine[ e ] != ' ' )
        e++;
    return uiLen > 0 ? e - 1 : 0;
}

// What one line contributes
struct Line
{
    uint32_t uiKind; // LINE_*
    uint32_t uiLen; // bytes without the line end
    uint32_t uiBases; // LINE_BASES: bases it contributes
    uint32_t uiName; // LINE_HEADER: bytes of the name
    uint32_t uiReason; // OK or its first violation
};
// Everything about line uiLine of a text of uiLines lines with the line starts pStart[ 0 .. uiLines ].  uiLoneCr: position of the
// text's FIRST lone '\r' (n if there is none): the lowest line that has one is all a refusal needs.
MA_TEXT_HD Line lineOf( uint32_t uiKind, const char* pText, const uint32_t* pStart, uint64_t uiLine, uint64_t uiLines, uint64_t uiLoneCr )
{
    const uint64_t uiFrom = pStart[ uiLine ], uiTo = pStart[ uiLine + 1 ];
    const char* const p = pText + uiFrom;
    const uint32_t n = content( pText, uiFrom, uiTo );
    Line x;
    x.uiKind = lineKind( uiKind, uiLine, p, n );
    x.uiLen = n;
    x.uiBases = x.uiName = 0;
    uint32_t uiReason = OK;
    const char c0 = n > 0 ? p[ 0 ] : '\0';
    if( x.uiKind == LINE_HEADER )
    {
        if( uiKind == KIND_FASTQ && c0 != '@' )
            uiReason = ERR_FQ_HEADER;
        else
            x.uiName = nameLength( p, n );
    }
    else if( x.uiKind == LINE_BASES )
    {
        if( n == 0 )
            uiReason = ERR_SEQ_EMPTY;
        else if( c0 == ' ' || c0 == '@' || ( uiKind == KIND_FASTQ && c0 == '+' ) )
            uiReason = ERR_SEQ_START;
        else if( ( x.uiBases = trimmed( p, n ) ) == 0 && uiKind == KIND_FASTQ )
            uiReason = ERR_SEQ_NO_BASES;
    }
    else if( x.uiKind == LINE_PLUS )
    {
        if( c0 != '+' )
            uiReason = ERR_FQ_PLUS;
    }
    else // LINE_QUAL: as long as the bases two lines up (if that line is refused itself, it is the lower one and wins)
    {
        const uint64_t uiSeqFrom = pStart[ uiLine - 2 ];
        if( n != trimmed( pText + uiSeqFrom, content( pText, uiSeqFrom, pStart[ uiLine - 1 ] ) ) )
            uiReason = ERR_FQ_QUAL_LEN;
    }
    if( uiFrom <= uiLoneCr && uiLoneCr < uiTo )
        uiReason = ERR_LONE_CR; // (the first check of a line)
    if( uiReason == OK && uiKind == KIND_FASTQ && uiLine + 1 == uiLines && ( uiLines & 3u ) != 0 )
        uiReason = ERR_FQ_COUNT;
    x.uiReason = uiReason;
    return x;
}
// violations are ordered by line, then by reason
MA_TEXT_HD uint64_t key( uint64_t uiLine, uint32_t uiReason )
{
    return ( uiLine << 8 ) | uiReason;
}
// the per-record FASTA rule: a record whose bases end where they begin is refused at its header line
MA_TEXT_HD uint64_t recordKey( uint64_t uiHeaderLine, uint64_t uiBasesFrom, uint64_t uiBasesTo )
{
    return uiBasesTo == uiBasesFrom ? key( uiHeaderLine, ERR_FA_NO_BASES ) : NO_VIOLATION;
}
// where byte uiAt of line x goes: 0 nowhere, 1 codes[ bases sum + *pIndex ], 2 qual[ bases sum two lines up + *pIndex ],
// 3 names[ name sum + *pIndex ]
enum : uint32_t
{
    TO_NONE = 0u,
    TO_CODES = 1u,
    TO_QUAL = 2u,
    TO_NAMES = 3u
};
MA_TEXT_HD uint32_t byteTarget( const Line& x, uint32_t uiAt, uint32_t* pIndex )
{
    *pIndex = uiAt;
    if( x.uiKind == LINE_BASES )
        return uiAt < x.uiBases ? TO_CODES : TO_NONE;
    if( x.uiKind == LINE_QUAL )
        return uiAt < x.uiLen ? TO_QUAL : TO_NONE;
    if( x.uiKind == LINE_HEADER && uiAt >= 1 && uiAt - 1 < x.uiName )
    {
        *pIndex = uiAt - 1;
        return TO_NAMES;
    }
    return TO_NONE;
}

// ---- the serial driver ------------------------------------------------------------------------------------------------------
struct Result
{
    uint64_t uiReads, uiBases, uiNameBytes, uiMaxLen;
    int32_t iHasQual; // 1: FASTQ
    uint32_t uiReason; // OK, or the refusal:
    uint64_t uiLine, uiByte; // 0-based line, offset of its first byte
};
// Parses a text as the kernels do.  Returns 0 and fills *pResult and the arrays that are not NULL (pOffsets / pNameOff: reads + 1
// entries, pCodes / pQual: bases, pNames: name bytes; call with NULLs first for the sizes), or returns 1 with the refusal in
// *pResult (message( ) words it) and the arrays untouched.  pStart: scratch of n + 2 words.
inline int parseHost( const char* pText, uint64_t n, uint32_t* pStart, uint64_t* pOffsets, uint8_t* pCodes, uint64_t* pNameOff, char* pNames,
                      uint8_t* pQual, Result* pResult )
{
    Result r = { 0, 0, 0, 0, 0, OK, 0, 0 };
    *pResult = r;
    if( n == 0 )
    {
        if( pOffsets )
            pOffsets[ 0 ] = 0;
        if( pNameOff )
            pNameOff[ 0 ] = 0;
        return 0;
    }
    uint64_t uiKey = NO_VIOLATION;
    if( n > MAX_TEXT_BYTES )
        uiKey = key( 0, ERR_TOO_LARGE );
    else if( pText[ 0 ] != '@' && pText[ 0 ] != '>' )
        uiKey = key( 0, ERR_KIND );
    if( uiKey != NO_VIOLATION )
    {
        r.uiReason = (uint32_t)( uiKey & 0xffu );
        *pResult = r;
        return 1;
    }
    const uint32_t uiKind = pText[ 0 ] == '@' ? KIND_FASTQ : KIND_FASTA;
    r.iHasQual = uiKind == KIND_FASTQ;
    uint64_t uiFeeds = 0, uiLoneCr = n;
    pStart[ 0 ] = 0;
    for( uint64_t p = 0; p < n; p++ )
    {
        if( pText[ p ] == '\n' )
            pStart[ ++uiFeeds ] = (uint32_t)( p + 1 );
        if( uiLoneCr == n && loneCr( pText, n, p ) )
            uiLoneCr = p;
    }
    const uint64_t uiLines = nLines( uiFeeds, pText[ n - 1 ] );
    pStart[ uiLines ] = (uint32_t)n;
    // pass 1: the violations and the sums
    uint64_t uiReads = 0, uiBases = 0, uiNames = 0, uiRecFrom = 0, uiRecLine = 0, uiMaxLen = 0;
    for( uint64_t i = 0; i <= uiLines; i++ )
    {
        Line x;
        x.uiKind = LINE_HEADER; // (the end of the text closes the last record like a header)
        x.uiBases = x.uiName = 0;
        if( i < uiLines )
        {
            x = lineOf( uiKind, pText, pStart, i, uiLines, uiLoneCr );
            if( x.uiReason != OK && key( i, x.uiReason ) < uiKey )
                uiKey = key( i, x.uiReason );
        }
        if( x.uiKind == LINE_HEADER )
        {
            if( uiReads > 0 || i == uiLines )
            {
                const uint64_t k = recordKey( uiRecLine, uiRecFrom, uiBases );
                if( uiKind == KIND_FASTA && k < uiKey )
                    uiKey = k;
                if( uiBases - uiRecFrom > uiMaxLen )
                    uiMaxLen = uiBases - uiRecFrom;
            }
            if( i < uiLines )
                uiReads++, uiRecFrom = uiBases, uiRecLine = i;
        }
        uiBases += x.uiBases;
        uiNames += x.uiName;
    }
    if( uiKey != NO_VIOLATION )
    {
        r.uiReason = (uint32_t)( uiKey & 0xffu );
        r.uiLine = uiKey >> 8;
        r.uiByte = pStart[ r.uiLine ];
        *pResult = r;
        return 1;
    }
    r.uiReads = uiReads, r.uiBases = uiBases, r.uiNameBytes = uiNames, r.uiMaxLen = uiMaxLen;
    *pResult = r;
    // pass 2: the bytes
    uint64_t uiRead = 0, uiBase = 0, uiName = 0, uiQualAt = 0;
    for( uint64_t i = 0; i < uiLines; i++ )
    {
        const Line x = lineOf( uiKind, pText, pStart, i, uiLines, uiLoneCr );
        if( x.uiKind == LINE_HEADER )
        {
            if( pOffsets )
                pOffsets[ uiRead ] = uiBase;
            if( pNameOff )
                pNameOff[ uiRead ] = uiName;
            uiRead++;
            uiQualAt = uiBase; // FASTQ: the one bases line of the record starts here
        }
        for( uint32_t k = 0; k < x.uiLen; k++ )
        {
            uint32_t j;
            const uint32_t t = byteTarget( x, k, &j );
            const char c = pText[ pStart[ i ] + k ];
            if( t == TO_CODES && pCodes )
                pCodes[ uiBase + j ] = code( (uint8_t)c );
            else if( t == TO_QUAL && pQual )
                pQual[ uiQualAt + j ] = (uint8_t)c;
            else if( t == TO_NAMES && pNames )
                pNames[ uiName + j ] = c;
        }
        uiBase += x.uiBases;
        uiName += x.uiName;
    }
    if( pOffsets )
        pOffsets[ uiRead ] = uiBase;
    if( pNameOff )
        pNameOff[ uiRead ] = uiName;
    return 0;
}

// ---- mate pairs out of two texts (ma_batch_set_mates_text) -----------------------------------------------------------------------
// PairedFileReader::execute (fileReader.h:568-617) over two texts in the strict form: record k of text 1 becomes read 2k, record
// k of text 2 read 2k + 1; the shorter text ends the stream (R = min( R1, R2 ) pairs), the surplus records of the longer one are
// validated and dropped.  With iRevComp every read 2k + 1 is reversed with its qualities (NucSeq::vReverse, nucSeq.h:373-381)
// and complemented (vSwitchAllBasePairsToComplement, nucSeq.h:537-543: a code below 4 becomes 3 - c, every other code 5 (sic)).
MA_TEXT_HD uint8_t mateCode( uint8_t c ) // the complement of a code
{
    return c < 4 ? (uint8_t)( 3 - c ) : (uint8_t)5;
}
enum : uint32_t // why a call is refused, in the order of precedence
{
    MATES_OK = 0u,
    MATES_LINE = 1u, // a rule violation in text uiText (text 1 wins over text 2; within a text as parseHost)
    MATES_KIND = 2u, // one FASTQ and one FASTA text
    MATES_CAPACITY = 3u // more pairs or bases than the batch holds (the library's check; pairHost knows no batch)
};
struct PairResult
{
    uint64_t uiPairs, uiBases, uiNameBytes, uiMaxLen; // over the paired records only
    uint64_t aConsumed[ 2 ]; // offset of the first byte of record R of each text (its size when it has exactly R records)
    int32_t iHasQual;
    uint32_t uiRefusal; // MATES_*
    uint32_t uiText, uiReason; // MATES_LINE: 1 or 2, and the reason
    uint64_t uiLine, uiByte; // MATES_LINE: 0-based line, offset of its first byte
};
// "<who>: text <1|2>: line <L> (byte <X>): <reason>" and the two other refusals; uiLine is 0-based here.  (ma_batch_set_mates_bgzf
// words a refusal of its inflated texts with it.)
inline void messageMatesOf( char* pOut, size_t uiCap, const char* pWho, uint32_t uiRefusal, uint32_t uiText, uint64_t uiLine, uint64_t uiByte,
                            uint32_t uiReason )
{
    if( uiRefusal == MATES_LINE )
        snprintf( pOut, uiCap, "%s: text %u: line %llu (byte %llu): %s", pWho, (unsigned)uiText, (unsigned long long)( uiLine + 1 ),
                  (unsigned long long)uiByte, errorText( uiReason ) );
    else
        snprintf( pOut, uiCap, "%s: %s", pWho,
                  uiRefusal == MATES_KIND ? "the two texts differ in kind" : uiRefusal == MATES_CAPACITY ? "batch capacity exceeded" : "no error" );
}
// "ma_batch_set_mates_text: text <1|2>: line <L> (byte <X>): <reason>" ...
inline void messageMates( char* pOut, size_t uiCap, uint32_t uiRefusal, uint32_t uiText, uint64_t uiLine, uint64_t uiByte, uint32_t uiReason )
{
    messageMatesOf( pOut, uiCap, "ma_batch_set_mates_text", uiRefusal, uiText, uiLine, uiByte, uiReason );
}
// offset of the first byte of record uiRecord of an ACCEPTED text with the line starts parseHost left in pStart (n if the text
// has no such record)
inline uint64_t recordStartHost( const char* pText, uint64_t n, const uint32_t* pStart, uint64_t uiRecord )
{
    if( n == 0 )
        return 0;
    const uint32_t uiKind = pText[ 0 ] == '@' ? KIND_FASTQ : KIND_FASTA;
    uint64_t uiFeeds = 0;
    for( uint64_t p = 0; p < n; p++ )
        uiFeeds += pText[ p ] == '\n' ? 1 : 0;
    const uint64_t uiLines = nLines( uiFeeds, pText[ n - 1 ] );
    uint64_t uiSeen = 0;
    for( uint64_t i = 0; i < uiLines; i++ )
        if( lineKind( uiKind, i, pText + pStart[ i ], content( pText, pStart[ i ], pStart[ i + 1 ] ) ) == LINE_HEADER && uiSeen++ == uiRecord )
            return pStart[ i ];
    return n;
}
// The serial statement of ma_batch_set_mates_text: parseHost on each text, interleave, reverse complement.  Returns 0 and fills
// *pResult and the arrays that are not NULL (pOffsets / pNameOff: 2 R + 1 entries, pCodes / pQual: bases, pNames: name bytes;
// call with NULLs first for the sizes), or returns 1 with the refusal in *pResult (messageMates( ) words it) and the arrays
// untouched.  An empty text is a text of no records: 0 pairs, the other text is validated all the same.
inline int pairHost( const char* pText1, uint64_t n1, const char* pText2, uint64_t n2, int32_t iRevComp, uint64_t* pOffsets, uint8_t* pCodes,
                     uint64_t* pNameOff, char* pNames, uint8_t* pQual, PairResult* pResult )
{
    PairResult r = { 0, 0, 0, 0, { 0, 0 }, 0, MATES_OK, 0, OK, 0, 0 };
    *pResult = r;
    const char* const apText[ 2 ] = { pText1, pText2 };
    const uint64_t aN[ 2 ] = { n1, n2 };
    uint32_t* apStart[ 2 ] = { NULL, NULL };
    uint64_t *apOff[ 2 ] = { NULL, NULL }, *apNameOff[ 2 ] = { NULL, NULL };
    uint8_t *apCodes[ 2 ] = { NULL, NULL }, *apQual[ 2 ] = { NULL, NULL };
    char* apNames[ 2 ] = { NULL, NULL };
    Result aParsed[ 2 ];
    int iRet = 0;
    for( int t = 0; t < 2; t++ )
    {
        apStart[ t ] = (uint32_t*)malloc( ( aN[ t ] + 2 ) * sizeof( uint32_t ) );
        if( parseHost( apText[ t ], aN[ t ], apStart[ t ], NULL, NULL, NULL, NULL, NULL, &aParsed[ t ] ) && iRet == 0 )
        {
            r.uiRefusal = MATES_LINE;
            r.uiText = (uint32_t)t + 1;
            r.uiReason = aParsed[ t ].uiReason, r.uiLine = aParsed[ t ].uiLine, r.uiByte = aParsed[ t ].uiByte;
            iRet = 1;
        }
    }
    if( iRet == 0 && n1 > 0 && n2 > 0 && aParsed[ 0 ].iHasQual != aParsed[ 1 ].iHasQual )
    {
        r.uiRefusal = MATES_KIND;
        iRet = 1;
    }
    if( iRet == 0 )
    {
        const uint64_t R = aParsed[ 0 ].uiReads < aParsed[ 1 ].uiReads ? aParsed[ 0 ].uiReads : aParsed[ 1 ].uiReads;
        r.uiPairs = R;
        r.iHasQual = n1 > 0 && n2 > 0 ? aParsed[ 0 ].iHasQual : 0; // (an empty text has no kind: no reads, no qualities)
        for( int t = 0; t < 2; t++ )
        {
            const Result& p = aParsed[ t ];
            apOff[ t ] = (uint64_t*)malloc( ( p.uiReads + 1 ) * sizeof( uint64_t ) );
            apNameOff[ t ] = (uint64_t*)malloc( ( p.uiReads + 1 ) * sizeof( uint64_t ) );
            apCodes[ t ] = (uint8_t*)malloc( p.uiBases + 1 );
            apQual[ t ] = (uint8_t*)malloc( p.uiBases + 1 );
            apNames[ t ] = (char*)malloc( p.uiNameBytes + 1 );
            Result xAgain;
            parseHost( apText[ t ], aN[ t ], apStart[ t ], apOff[ t ], apCodes[ t ], apNameOff[ t ], apNames[ t ], p.iHasQual ? apQual[ t ] : NULL, &xAgain );
            r.aConsumed[ t ] = R < p.uiReads ? recordStartHost( apText[ t ], aN[ t ], apStart[ t ], R ) : aN[ t ];
        }
        uint64_t uiBase = 0, uiName = 0;
        for( uint64_t k = 0; k < 2 * R; k++ )
        {
            const int t = (int)( k & 1 );
            const uint64_t uiRec = k >> 1, uiFrom = apOff[ t ][ uiRec ], uiLen = apOff[ t ][ uiRec + 1 ] - uiFrom;
            const uint64_t uiNameFrom = apNameOff[ t ][ uiRec ], uiNameLen = apNameOff[ t ][ uiRec + 1 ] - uiNameFrom;
            const bool bRev = t == 1 && iRevComp != 0;
            if( pOffsets )
                pOffsets[ k ] = uiBase;
            if( pNameOff )
                pNameOff[ k ] = uiName;
            for( uint64_t j = 0; j < uiLen; j++ )
            {
                const uint64_t uiSrc = uiFrom + ( bRev ? uiLen - 1 - j : j );
                if( pCodes )
                    pCodes[ uiBase + j ] = bRev ? mateCode( apCodes[ t ][ uiSrc ] ) : apCodes[ t ][ uiSrc ];
                if( pQual && r.iHasQual )
                    pQual[ uiBase + j ] = apQual[ t ][ uiSrc ];
            }
            if( pNames )
                memcpy( pNames + uiName, apNames[ t ] + uiNameFrom, uiNameLen );
            uiBase += uiLen;
            uiName += uiNameLen;
            if( uiLen > r.uiMaxLen )
                r.uiMaxLen = uiLen;
        }
        if( pOffsets )
            pOffsets[ 2 * R ] = uiBase;
        if( pNameOff )
            pNameOff[ 2 * R ] = uiName;
        r.uiBases = uiBase, r.uiNameBytes = uiName;
    }
    for( int t = 0; t < 2; t++ )
    {
        free( apStart[ t ] );
        free( apOff[ t ] );
        free( apNameOff[ t ] );
        free( apCodes[ t ] );
        free( apQual[ t ] );
        free( apNames[ t ] );
    }
    *pResult = r;
    return iRet;
}
} // namespace ma_text
