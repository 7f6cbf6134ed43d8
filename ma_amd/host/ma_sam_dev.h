// ma_sam_dev.h -- the SAM record formatter over FLAT records (the arrays of ma_batch_get_mapq_alignments / ma_batch_get_pairs),
// written ONCE over a templated sink: formatRead prints the bytes of the reference's FileWriter::execute
// (libs/ma/src/module/fileWriter.cpp:11-158), formatPair those of PairedFileWriter::execute (:158-383), both with
// Alignment::cigarString / getSamFlag / getSamPosition / getQuerySequence (libs/ma/inc/ma/container/alignment.h:367-467, 576-623)
// and Pack's position arithmetic (pack.h:900-997, 1063-1067).  Its users:
//   - the device stages (ma_amd/csrc/stage_sam.h, stage_pair_sam.h) run formatRead( ) / formatPair( ) inside their two kernels:
//     with the counting sink to size every read's (pair's) text, with a writing sink to store it;
//   - the host's flat writers (ma_flat_sam.h: flat::formatRead / flat::formatPair, an adapter that runs the same functions over
//     a sink on its byte arena) for BatchFileWriter / BatchPairedFileWriter of ma_batch_nodes.h;
//   - libma_amd.so words the error of a bad record with errorText( ).
// The yardstick is the independent implementation on Alignment containers, FileWriter / PairedFileWriter of ma_sam.h, which
// tests/test_sam_writer.py and tests/test_pairs_host.py pin to the SAM goldens the compiled reference wrote: the CPU tests
// (tests/emul/sam_dev_test.cpp, sam_pair_dev_test.cpp, sam_tags_dev_test.cpp) run the functions of this file on the host and
// compare them with it byte for byte, and the GPU tests compare the kernels' text with it.
// With NGMLR_TAGS (single-end only) a record also carries the tags of the reference's "Emulate NGMLR's tag output"
// (TagGenerator::computeTag, fileWriter.h:120-326): MD SV AS NM XI XE XR CV SA QS QE, byte for byte what ma_amd::FileWriter
// (ma_sam.h: sam::ngmlrTags, FileWriter::execute) prints.  They need the reference's bases and its runs of N: a Ref (below),
// handed to formatRead( sink, options, contigs, read, list, ref ).
// No reference headers, no containers, no strings: include/ma_amd.h only.  The reference's oddities are listed HERE and nowhere
// else; they are kept as they are:
//   position one further on the reverse strand (alignment.h:596-603), the contig that of the begin (pack.h:1063-1067);
//   MAPQ = (int)ceil( mapq * 254 ), 255 for NaN, capped at 255 by the paired writer only (fileWriter.cpp:262); the cigar walked
//   backwards on the reverse strand, seed / match / mismatch merged into M (or printed as = / X), H or S clips with the
//   left-over clip taken against the read length -- of the FIRST mate in a pair (alignment.h:367-467, fileWriter.cpp:191-193);
//   SEQ reverse-complemented on the reverse strand, QUAL the aligned part and never reversed (alignment.h:611-614,
//   nucSeq.h:697-709), "*" without qualities; "<len>S" + the CG:B:I tag from 0x10000 ops on (fileWriter.h:327-357); alignments of
//   op length 0 skipped; secondary / supplementary records dropped on request; the unmapped record with MAPQ text 255 for an
//   empty list and 0 when every alignment was skipped (fileWriter.cpp:126-140); a pair's TLEN is never output (:317), RNEXT is
//   "=" on a contig of the same NAME, an unaligned mate stands at record 0 of the list, printed or not (:348-366).
//
// A sink is anything with
//   put( c ), bytes( p, n ), number( x ), size( )          plain columns
//   seq( read, from, to, reverse, k )                       SEQ of record k of the list (k = UNMAPPED: of the unmapped record;
//                                                           UNMAPPED_FIRST / UNMAPPED_SECOND: of a pair's unaligned mate)
//   qual( read, from, to, k )                               QUAL (only called when the read has qualities)
//   error( kind, value, k )                                 record k cannot be printed (see ERR_*)
// The kernels' writing sink leaves SEQ and QUAL out (it only notes where they go): the wavefront copies them together.
#pragma once
#if !defined( MA_AMD_H ) // (libma_amd.so includes it by its own path)
#include "ma_amd.h"
#endif

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined( __HIPCC__ )
#define MA_SAM_HD __host__ __device__ __forceinline__
#else
#define MA_SAM_HD inline
#endif

namespace ma_sam
{
enum : uint32_t // == MA_SAM_* of include/ma_amd.h
{
    SOFT_CLIP = 1u, // S instead of H clips, SEQ = the whole read
    EQX_CIGAR = 2u, // = and X instead of M
    NO_SECONDARY = 4u,
    NO_SUPPLEMENTARY = 8u,
    NO_CG_TAG = 16u, // over-long cigars are printed as they are
    NGMLR_TAGS = 32u, // the NGMLR tag emulation (single-end records only); the CIGAR column is M-style then
    PAIR_OPTIONS = 31u, // what formatPair serves
    ALL_OPTIONS = 63u
};
enum : uint32_t
{
    ERR_QUERY_LENGTH = 1u, // "Query length is off by <value>." (forward strand, end_q beyond the read; fileWriter.cpp:106)
    ERR_COMP_CHAR_AT = 2u, // "Index out of range (compCharAt)" (reverse strand, the same)
    // with NGMLR_TAGS only:
    ERR_BRIDGING = 3u, // [begin_ref, end_ref) lies on both strands or ends beyond the doubled text (pack.h:1238-1330)
    ERR_OPS_COVERAGE = 4u // the ops do not cover exactly [begin_ref, end_ref) and [begin_q, end_q): the host formatter would read
                          // outside its buffer, the library refuses the record
};
enum : uint32_t
{
    UNMAPPED = 0xffffffffu, // the one unmapped record of a read (formatRead)
    UNMAPPED_FIRST = 0xfffffffeu, // the record of an unaligned first / second mate (formatPair): a pair can have both
    UNMAPPED_SECOND = 0xfffffffdu
};

// contig table of the pack (forward strand); names[ name_off[ i ] .. name_off[ i + 1 ] ) is contig i's RNAME
struct Contigs
{
    const char* names;
    const uint64_t* name_off;
    const uint64_t* starts;
    const uint64_t* lengths;
    uint32_t n; // >= 1
    MA_SAM_HD uint64_t forwardSize( ) const
    {
        return starts[ n - 1 ] + lengths[ n - 1 ];
    }
    // Pack::uiSequenceIdForPosition (pack.h:933-990) of a position on the forward strand
    MA_SAM_HD uint32_t idOfForward( uint64_t uiPos ) const
    {
        uint32_t lo = 0, hi = n;
        while( hi - lo > 1 )
        {
            const uint32_t mid = lo + ( hi - lo ) / 2;
            if( uiPos >= starts[ mid ] )
                lo = mid;
            else
                hi = mid;
        }
        return lo;
    }
};
struct Read
{
    const char* name;
    uint64_t name_len;
    const uint8_t* codes; // A0 C1 G2 T3, else N
    const uint8_t* qual; // FASTQ quality characters or null
    uint64_t length;
};
// what a record reads of an alignment
struct Rec
{
    uint64_t begin_ref, end_ref, begin_q, end_q;
    uint32_t n_ops, secondary, supplementary;
    double mapq;
    int64_t score = 0; // (read by the tags only)
};
// Reference bases and runs of N for the tags.  pac: the forward strand, 2 bits per base, first base in the top bits (Pack's
// packed text, the index's pac); holes: Pack::vHoles, (start, length) on the forward strand, sorted and not overlapping.
struct Ref
{
    const uint8_t* pac;
    const uint64_t* hole_start;
    const uint64_t* hole_len;
    uint64_t n_holes;
    uint64_t forward; // size of the forward strand
    // base of position p of the doubled text (referenceCodes of ma_sam.h without hole marking: the random base that replaced an N)
    MA_SAM_HD uint8_t code( uint64_t p ) const
    {
        const bool bRev = p >= forward;
        const uint64_t a = bRev ? 2 * forward - 1 - p : p;
        const uint8_t b = (uint8_t)( ( pac[ a >> 2 ] >> ( ( ~a & 3 ) << 1 ) ) & 3 );
        return bRev ? (uint8_t)( 3 - b ) : b;
    }
    // bases of the raw interval [a, b) that lie inside holes: a binary search for the first hole that ends behind a, then
    // the holes that start before b (0 for a > b)
    MA_SAM_HD uint64_t holeBases( uint64_t a, uint64_t b ) const
    {
        if( a >= b )
            return 0;
        uint64_t lo = 0, hi = n_holes;
        while( lo < hi )
        {
            const uint64_t mid = lo + ( hi - lo ) / 2;
            if( hole_start[ mid ] + hole_len[ mid ] > a )
                hi = mid;
            else
                lo = mid + 1;
        }
        uint64_t uiSum = 0;
        for( ; lo < n_holes && hole_start[ lo ] < b; lo++ )
        {
            const uint64_t s = hole_start[ lo ] > a ? hole_start[ lo ] : a, e = hole_start[ lo ] + hole_len[ lo ];
            uiSum += ( e < b ? e : b ) - s;
        }
        return uiSum;
    }
    // the same for [p, p + n) of the doubled text, which lies on one strand
    MA_SAM_HD uint64_t holeBasesDoubled( uint64_t p, uint64_t n ) const
    {
        return p >= forward ? holeBases( 2 * forward - ( p + n ), 2 * forward - p ) : holeBases( p, p + n );
    }
};
struct NoRef
{};
// what a record of a pair has beyond a single read's; the defaults are a single read's
struct RecordExtras
{
    uint32_t extra_flags = 0;
    bool cap_mapq = false; // the paired writer caps MAPQ at 255 (fileWriter.cpp:262)
    bool has_partner = false; // RNEXT / PNEXT of partner, else "*" and 0
    uint64_t clip_length = 0; // query length the cigar is clipped against
    uint64_t partner_begin_ref = 0, partner_end_ref = 0;
};
// A list is anything with size( ), rec( k ), opType( k, j ), opLen( k, j ).  This one is over the arrays of
// ma_batch_get_mapq_alignments (ops_off counts (type, length) pairs).
struct FlatList
{
    const ma_alignment* alns;
    uint32_t n;
    const uint64_t* ops;
    MA_SAM_HD uint32_t size( ) const
    {
        return n;
    }
    MA_SAM_HD Rec rec( uint32_t k ) const
    {
        const ma_alignment& a = alns[ k ];
        return Rec{ (uint64_t)a.begin_ref, (uint64_t)a.end_ref, (uint64_t)a.begin_q, (uint64_t)a.end_q, a.n_ops, a.secondary, a.supplementary, a.mapq,
                    a.score };
    }
    MA_SAM_HD uint64_t opType( uint32_t k, uint32_t j ) const
    {
        return ops[ 2 * ( alns[ k ].ops_off + j ) ];
    }
    MA_SAM_HD uint64_t opLen( uint32_t k, uint32_t j ) const
    {
        return ops[ 2 * ( alns[ k ].ops_off + j ) + 1 ];
    }
};
// A pair list is a list that yields the records of ONE pair in the order of ma_batch_get_pairs and also has mate( k ) (!= 0:
// record of the first mate) and other( k ) (index of the partner's record in the pair or -1).  This one is over the arrays
// of ma_batch_get_pairs.
struct FlatPairList : FlatList
{
    const int32_t* mates;
    const int32_t* others;
    MA_SAM_HD int32_t mate( uint32_t k ) const
    {
        return mates[ k ];
    }
    MA_SAM_HD int32_t other( uint32_t k ) const
    {
        return others[ k ];
    }
};

// ---- characters ----------------------------------------------------------------------------------------------------------
MA_SAM_HD char baseChar( uint8_t c ) // "ACGTN"[ c < 4 ? c : 4 ] without a table
{
    return (char)( ( 0x4E54474341ull >> ( 8 * ( c < 4 ? c : 4 ) ) ) & 0xff );
}
MA_SAM_HD char complementChar( uint8_t c )
{
    return baseChar( c < 4 ? (uint8_t)( 3 - c ) : (uint8_t)4 );
}
MA_SAM_HD uint32_t digits( uint64_t x ) // decimal digits of x
{
    uint32_t d = 1;
    uint64_t p = 10;
    while( d < 20 && x >= p )
    {
        d++;
        p *= 10; // (wraps only after d reached 20)
    }
    return d;
}

// ---- the two sinks -------------------------------------------------------------------------------------------------------
struct CountSink
{
    uint64_t n = 0;
    uint32_t nErrors = 0, firstKind = 0, firstRecord = 0;
    int64_t firstValue = 0;
    MA_SAM_HD uint64_t size( ) const
    {
        return n;
    }
    MA_SAM_HD void put( char )
    {
        n++;
    }
    MA_SAM_HD void bytes( const char*, uint64_t k )
    {
        n += k;
    }
    MA_SAM_HD void number( uint64_t x )
    {
        n += digits( x );
    }
    MA_SAM_HD void seq( const Read&, uint64_t uiFrom, uint64_t uiTo, bool, uint32_t )
    {
        n += uiTo - uiFrom;
    }
    MA_SAM_HD void qual( const Read&, uint64_t uiFrom, uint64_t uiTo, uint32_t )
    {
        n += uiTo - uiFrom;
    }
    MA_SAM_HD void error( uint32_t uiKind, int64_t iValue, uint32_t k )
    {
        if( nErrors++ == 0 )
            firstKind = uiKind, firstValue = iValue, firstRecord = k;
    }
};
struct WriteSink
{
    char* p;
    uint64_t n = 0;
    MA_SAM_HD uint64_t size( ) const
    {
        return n;
    }
    MA_SAM_HD void put( char c )
    {
        p[ n++ ] = c;
    }
    MA_SAM_HD void bytes( const char* s, uint64_t k )
    {
        for( uint64_t i = 0; i < k; i++ )
            p[ n + i ] = s[ i ];
        n += k;
    }
    MA_SAM_HD void number( uint64_t x ) // by digit count: the last digit first, each where it belongs
    {
        const uint32_t d = digits( x );
        for( uint32_t i = d; i > 0; i-- )
        {
            p[ n + i - 1 ] = (char)( '0' + x % 10 );
            x /= 10;
        }
        n += d;
    }
    MA_SAM_HD void seq( const Read& rQ, uint64_t uiFrom, uint64_t uiTo, bool bRev, uint32_t )
    {
        for( uint64_t i = 0; i < uiTo - uiFrom; i++ )
            p[ n + i ] = bRev ? complementChar( rQ.codes[ uiTo - 1 - i ] ) : baseChar( rQ.codes[ uiFrom + i ] );
        n += uiTo - uiFrom;
    }
    MA_SAM_HD void qual( const Read& rQ, uint64_t uiFrom, uint64_t uiTo, uint32_t )
    {
        bytes( (const char*)rQ.qual + uiFrom, uiTo - uiFrom );
    }
    MA_SAM_HD void error( uint32_t, int64_t, uint32_t )
    {}
};

namespace detail
{
template <class Sink, size_t N> MA_SAM_HD void lit( Sink& rOut, const char ( &s )[ N ] )
{
    for( size_t i = 0; i + 1 < N; i++ )
        rOut.put( s[ i ] );
}
template <class Sink> MA_SAM_HD void numberAnd( Sink& rOut, uint64_t x, char c )
{
    rOut.number( x );
    rOut.put( c );
}
// QUAL of [uiFrom, uiTo): clamped to the read (nucSeq.h:697-709), never reversed
template <class Sink> MA_SAM_HD void putQuality( Sink& rOut, const Read& rQ, uint64_t uiFrom, uint64_t uiTo, uint32_t k )
{
    if( rQ.qual == nullptr )
    {
        rOut.put( '*' );
        return;
    }
    if( uiTo > rQ.length )
        uiTo = rQ.length;
    if( uiFrom < uiTo )
        rOut.qual( rQ, uiFrom, uiTo, k );
}
template <class Sink> MA_SAM_HD void putUnmapped( Sink& rOut, const Read& rQ, bool bEmptyList ) // fileWriter.cpp:126-140
{
    rOut.bytes( rQ.name, rQ.name_len );
    lit( rOut, "\t4\t*\t0\t" );
    if( bEmptyList )
        lit( rOut, "255" );
    else
        rOut.put( '0' );
    lit( rOut, "\t*\t*\t0\t0\t" );
    if( rQ.length > 0 )
        rOut.seq( rQ, 0, rQ.length, false, UNMAPPED );
    rOut.put( '\t' );
    putQuality( rOut, rQ, 0, rQ.length, UNMAPPED );
    rOut.put( '\n' );
}
// contig of the begin (pack.h:1063-1067)
MA_SAM_HD uint32_t contigOf( const Contigs& rContigs, uint64_t uiBeginRef )
{
    const uint64_t uiFwd = rContigs.forwardSize( );
    return rContigs.idOfForward( uiBeginRef >= uiFwd ? 2 * uiFwd - ( uiBeginRef + 1 ) : uiBeginRef );
}
// Alignment::getSamPosition (alignment.h:596-603), see putRecord
MA_SAM_HD uint64_t samPosition( const Contigs& rContigs, uint64_t uiBeginRef, uint64_t uiEndRef )
{
    const uint64_t uiFwd = rContigs.forwardSize( );
    const uint64_t uiAbs = uiEndRef >= uiFwd ? 2 * uiFwd - ( uiEndRef + 1 ) : uiBeginRef;
    return uiAbs - rContigs.starts[ rContigs.idOfForward( uiAbs ) ] + ( uiBeginRef >= uiFwd ? 1 : 0 ) + 1;
}
MA_SAM_HD bool sameName( const Contigs& rContigs, uint32_t a, uint32_t b ) // by bytes: two contigs may share a name
{
    const uint64_t oa = rContigs.name_off[ a ], ob = rContigs.name_off[ b ], n = rContigs.name_off[ a + 1 ] - oa;
    if( rContigs.name_off[ b + 1 ] - ob != n )
        return false;
    for( uint64_t i = 0; i < n; i++ )
        if( rContigs.names[ oa + i ] != rContigs.names[ ob + i ] )
            return false;
    return true;
}
// ---- the NGMLR tag emulation -----------------------------------------------------------------------------------------------
// The ops of record k as FileWriter::execute leaves them behind Alignment::invertSuccessiveInserionAndDeletion
// (alignment.h:328-345; ma_sam.h): an insertion directly followed by a deletion, or the other way round, swap places, greedily
// from the left and without overlap (I D I -> D I I, I D I D -> D I D I).  The host mutates the alignment; this is a view, the
// pool stays as it is.  forward( j ) / backward( j ) give the index of the op that stands at place j, for j running up from 0 /
// down from n - 1 in steps of one; both are O( n ) over a whole walk (a run of alternating insertions and deletions is
// measured once, when the backward walk enters it at its end).
template <class List> struct SwappedOps
{
    const List& l;
    uint32_t k, n;
    bool swap;
    bool second = false; // forward: the place at hand is the second of a swapped pair (it shows the pair's first op)
    bool odd = false; // backward: place j is at an odd distance from its run's start
    MA_SAM_HD bool pairable( uint32_t i ) const // ops i - 1 and i: an insertion and a deletion, in either order
    {
        const uint64_t a = l.opType( k, i - 1 ), b = l.opType( k, i );
        return ( a == 3 && b == 4 ) || ( a == 4 && b == 3 );
    }
    MA_SAM_HD uint32_t forward( uint32_t j )
    {
        if( !swap )
            return j;
        if( second )
        {
            second = false;
            return j - 1;
        }
        if( j + 1 < n && pairable( j + 1 ) )
        {
            second = true;
            return j + 1;
        }
        return j;
    }
    MA_SAM_HD uint32_t backward( uint32_t j )
    {
        if( !swap )
            return j;
        const bool bNext = j + 1 < n && pairable( j + 1 ); // place j + 1 belongs to the same run
        if( bNext )
            odd = !odd;
        else
        {
            uint32_t r0 = j;
            while( r0 > 0 && pairable( r0 ) )
                r0--;
            odd = ( ( j - r0 ) & 1 ) != 0;
        }
        return odd ? j - 1 : bNext ? j + 1 : j;
    }
};
// Alignment::cigarString (alignment.h:367-467) with M for seed / match / missmatch, of record k as the tags print it: the
// CIGAR column of a record with tags and the cigars of the SA tag; bSwap: the record's ops were swapped before
template <class Sink, class List>
MA_SAM_HD void putCigarM( Sink& rOut, const List& rList, uint32_t k, const Rec& rA, bool bRev, bool bSwap, bool bSoftClip, uint64_t uiClipLength )
{
    const uint64_t uiLeftOver = rA.end_q < uiClipLength ? uiClipLength - rA.end_q : 0;
    const uint64_t uiHead = bRev ? uiLeftOver : rA.begin_q, uiTail = bRev ? rA.begin_q : uiLeftOver;
    const char cClip = bSoftClip ? 'S' : 'H';
    if( uiHead > 0 )
        numberAnd( rOut, uiHead, cClip );
    SwappedOps<List> xOps{ rList, k, rA.n_ops, bSwap && bRev };
    uint64_t uiRunM = 0;
    for( uint32_t j = 0; j < rA.n_ops; j++ )
    {
        const uint32_t jj = bRev ? xOps.backward( rA.n_ops - 1 - j ) : j;
        const uint64_t uiType = rList.opType( k, jj ), uiLen = rList.opLen( k, jj );
        if( uiType <= 2 )
            uiRunM += uiLen;
        else
        {
            if( uiRunM > 0 )
                numberAnd( rOut, uiRunM, 'M' );
            uiRunM = 0;
            numberAnd( rOut, uiLen, uiType == 3 ? 'I' : 'D' );
        }
    }
    if( uiRunM > 0 )
        numberAnd( rOut, uiRunM, 'M' );
    if( uiTail > 0 )
        numberAnd( rOut, uiTail, cClip );
}
template <class Sink> MA_SAM_HD void putSigned( Sink& rOut, int64_t x )
{
    if( x < 0 )
    {
        rOut.put( '-' );
        rOut.number( (uint64_t)0 - (uint64_t)x );
    }
    else
        rOut.number( (uint64_t)x );
}
// ---- XI:f and CV:f: std::to_string( float ), i.e. "%f" of the float promoted to double, without printf -----------------------
// single-precision operations, each rounded to nearest even whatever the flags of the translation unit
MA_SAM_HD float floatOf( uint64_t x )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    return __ull2float_rn( x );
#else
    return (float)x;
#endif
}
MA_SAM_HD float floatDiv( float a, float b )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    return __fdiv_rn( a, b );
#else
    return a / b;
#endif
}
MA_SAM_HD float floatMul( float a, float b )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    return __fmul_rn( a, b );
#else
    return a * b;
#endif
}
template <class Sink> MA_SAM_HD void putPadded18( Sink& rOut, uint64_t x ) // 18 digits
{
    for( uint32_t d = digits( x ); d < 18; d++ )
        rOut.put( '0' );
    rOut.number( x );
}
// "%f" of a float: it is m * 2^e with m < 2^24.  The integer part is exact; the six fraction digits are
// m_frac * 10^6 / 2^k (k = -e) rounded half to even on the exact value, as glibc does.  m_frac * 10^6 < 2^44: u64 suffices;
// for k >= 64 the digits are 0.
template <class Sink> MA_SAM_HD void putFloat( Sink& rOut, float f )
{
    uint32_t uiBits;
    __builtin_memcpy( &uiBits, &f, 4 );
    const uint32_t uiExp = ( uiBits >> 23 ) & 0xff, uiMant = uiBits & 0x7fffff;
    if( uiBits >> 31 )
        rOut.put( '-' );
    if( uiExp == 0xff )
    {
        if( uiMant )
            lit( rOut, "nan" );
        else
            lit( rOut, "inf" );
        return;
    }
    const uint64_t m = uiExp ? ( uiMant | 0x800000u ) : uiMant;
    const int e = uiExp ? (int)uiExp - 150 : -149;
    if( e >= 0 )
    {
        if( e <= 40 )
            rOut.number( m << e );
        else // up to 2^128: three limbs of 18 decimal digits, doubled e times
        {
            const uint64_t P = 1000000000000000000ull;
            uint64_t a = 0, b = 0, c = m;
            for( int i = 0; i < e; i++ )
            {
                c *= 2; // (c < 10^18: no wrap)
                const uint64_t cc = c >= P ? 1 : 0;
                c -= cc ? P : 0;
                b = 2 * b + cc;
                const uint64_t cb = b >= P ? 1 : 0;
                b -= cb ? P : 0;
                a = 2 * a + cb;
            }
            if( a )
            {
                rOut.number( a );
                putPadded18( rOut, b );
            }
            else
                rOut.number( b );
            putPadded18( rOut, c );
        }
        lit( rOut, ".000000" );
        return;
    }
    const uint32_t k = (uint32_t)-e; // 1 .. 149
    uint64_t uiInt = k < 64 ? m >> k : 0, uiFrac = 0;
    if( k < 64 )
    {
        const uint64_t uiProduct = ( m & ( ( 1ull << k ) - 1 ) ) * 1000000u, uiHalf = 1ull << ( k - 1 );
        const uint64_t uiRest = uiProduct & ( ( 1ull << k ) - 1 );
        uiFrac = uiProduct >> k;
        if( uiRest > uiHalf || ( uiRest == uiHalf && ( uiFrac & 1 ) ) )
            uiFrac++;
        if( uiFrac == 1000000u )
            uiFrac = 0, uiInt++;
    }
    numberAnd( rOut, uiInt, '.' );
    for( uint32_t d = digits( uiFrac ); d < 6; d++ )
        rOut.put( '0' );
    rOut.number( uiFrac );
}
// num / den as the host computes and prints XI ( (float)matches / (float)min( spans ) ) and CV ( 100.0f * (float)span /
// (float)length ).  A denominator of 0 is taken here, on the integers: 0 / 0 is the NaN the host's division makes, which its
// printf shows as "-nan"; x / 0 is "inf".
template <class Sink> MA_SAM_HD void putRatio( Sink& rOut, bool bTimes100, uint64_t uiNum, uint64_t uiDen )
{
    if( uiDen == 0 )
    {
        if( uiNum == 0 )
            lit( rOut, "-nan" );
        else
            lit( rOut, "inf" );
        return;
    }
    const float fNum = bTimes100 ? floatMul( 100.0f, floatOf( uiNum ) ) : floatOf( uiNum );
    putFloat( rOut, floatDiv( fNum, floatOf( uiDen ) ) );
}
// Alignment::length( ) != 0 and not dropped by the options: the record is printed
template <class List> MA_SAM_HD bool isPrinted( uint32_t uiOptions, const List& rList, uint32_t k, const Rec& rA )
{
    if( ( ( uiOptions & NO_SECONDARY ) && rA.secondary ) || ( ( uiOptions & NO_SUPPLEMENTARY ) && rA.supplementary ) )
        return false;
    for( uint32_t j = 0; j < rA.n_ops; j++ )
        if( rList.opLen( k, j ) != 0 )
            return true;
    return false;
}
// The tags of record k (sam::ngmlrTags of ma_sam.h), in NGMLR's order.  The host code is the contract, oddities included:
//   MD   over the swapped ops; no "0" for an empty count, but one before every mismatching base after the first of its section
//        and before the first directly behind a deletion; bases without hole marking
//   SV   +1: more than 0.8 of the 100 positions before begin_ref or behind end_ref lie in holes -- on RAW positions of the
//        doubled text, begin_ref - 100 wrapping around below 100 (sic, pack.h:551-566); +2: the record spans 95 % of the read,
//        or soft clipping
//   AS = XE = the score; NM = mismatches + inserted + deleted bases + hole bases under seeds and matches; XR = QE - QS
//   SA   every other alignment of the list that is not secondary, printed or not, with the NM of THIS record (sic); a sister
//        that stands before this record, is on the reverse strand and was printed shows its swapped ops (the host swapped them
//        when it printed her)
// A record that cannot be printed reports ERR_BRIDGING or ERR_OPS_COVERAGE and has no tags; nothing outside
// [begin_ref, end_ref) of pac is ever read.
template <class Sink, class List, class RefT>
MA_SAM_HD void putNgmlrTags( Sink& rOut, uint32_t uiOptions, const Contigs& rContigs, const Read& rQ, const Rec& rA, const List& rList, uint32_t k,
                             const RefT& rRef )
{
    const uint64_t uiFwd = rContigs.forwardSize( );
    const bool bSoftClip = ( uiOptions & SOFT_CLIP ) != 0, bRev = rA.begin_ref >= uiFwd;
    if( rA.end_ref > rA.begin_ref && ( rA.end_ref > 2 * uiFwd || bRev != ( rA.end_ref - 1 >= uiFwd ) ) )
    {
        rOut.error( ERR_BRIDGING, 0, k );
        return;
    }
    const uint64_t uiSpanR = rA.end_ref - rA.begin_ref, uiSpanQ = rA.end_q - rA.begin_q;
    uint64_t uiMatches = 0, uiNm = 0;
    {
        uint64_t uiLeftR = uiSpanR, uiLeftQ = uiSpanQ; // (counted down: no sum can wrap)
        bool bBad = rA.end_ref < rA.begin_ref || rA.end_q < rA.begin_q;
        for( uint32_t j = 0; j < rA.n_ops && !bBad; j++ )
        {
            const uint64_t uiType = rList.opType( k, j ), uiLen = rList.opLen( k, j );
            if( uiType > 4 || ( uiType != 3 && uiLen > uiLeftR ) || ( uiType != 4 && uiLen > uiLeftQ ) )
                bBad = true;
            else
            {
                uiLeftR -= uiType != 3 ? uiLen : 0;
                uiLeftQ -= uiType != 4 ? uiLen : 0;
                if( uiType <= 1 )
                    uiMatches += uiLen;
                else
                    uiNm += uiLen;
            }
        }
        if( bBad || uiLeftR != 0 || uiLeftQ != 0 )
        {
            rOut.error( ERR_OPS_COVERAGE, 0, k );
            return;
        }
    }
    lit( rOut, "\tMD:Z:" );
    {
        SwappedOps<List> xOps{ rList, k, rA.n_ops, bRev };
        uint64_t uiAt = rA.begin_ref, uiPending = 0;
        bool bAfterDeletion = false;
        for( uint32_t j = 0; j < rA.n_ops; j++ )
        {
            const uint32_t jj = xOps.forward( j );
            const uint64_t uiType = rList.opType( k, jj ), uiLen = rList.opLen( k, jj );
            if( uiType == 3 )
            {
                bAfterDeletion = false;
                continue;
            }
            if( uiType <= 1 )
            {
                uiPending += uiLen;
                uiNm += rRef.holeBasesDoubled( uiAt, uiLen );
            }
            else
            {
                if( uiPending > 0 )
                    rOut.number( uiPending );
                uiPending = 0;
                if( uiType == 4 )
                    rOut.put( '^' );
                for( uint64_t i = 0; i < uiLen; i++ )
                {
                    if( uiType == 2 && ( i > 0 || bAfterDeletion ) )
                        rOut.put( '0' );
                    rOut.put( baseChar( rRef.code( uiAt + i ) ) );
                }
            }
            uiAt += uiLen;
            bAfterDeletion = uiType == 4;
        }
        if( uiPending > 0 )
            rOut.number( uiPending );
    }
    {
        // covered / 100.0 > .8 of the host: 80 / 100.0 is the double 0.8 itself, so it is "more than 80 positions"
        uint32_t uiSv = 0;
        if( rRef.holeBases( rA.begin_ref - 100, rA.begin_ref ) > 80 || rRef.holeBases( rA.end_ref, rA.end_ref + 100 ) > 80 )
            uiSv += 1;
        if( (double)uiSpanQ >= (double)rQ.length * 0.95 || bSoftClip )
            uiSv += 2;
        lit( rOut, "\tSV:i:" );
        rOut.number( uiSv );
    }
    lit( rOut, "\tAS:i:" );
    putSigned( rOut, rA.score );
    lit( rOut, "\tNM:i:" );
    rOut.number( uiNm );
    lit( rOut, "\tXI:f:" );
    putRatio( rOut, false, uiMatches, uiSpanQ < uiSpanR ? uiSpanQ : uiSpanR );
    lit( rOut, "\tXE:i:" ); // (sic) NGMLR puts the score here
    putSigned( rOut, rA.score );
    lit( rOut, "\tXR:i:" );
    rOut.number( uiSpanQ );
    lit( rOut, "\tCV:f:" );
    putRatio( rOut, true, uiSpanQ, rQ.length );
    const uint32_t uiAlns = rList.size( );
    bool bTagOpen = false;
    for( uint32_t s = 0; s < uiAlns && uiAlns > 1; s++ )
    {
        if( s == k )
            continue;
        const Rec xS = rList.rec( s );
        if( xS.secondary )
            continue;
        if( !bTagOpen )
            lit( rOut, "\tSA:Z:" );
        bTagOpen = true;
        const bool bSisterRev = xS.begin_ref >= uiFwd;
        const uint32_t uiContig = contigOf( rContigs, xS.begin_ref );
        rOut.bytes( rContigs.names + rContigs.name_off[ uiContig ], rContigs.name_off[ uiContig + 1 ] - rContigs.name_off[ uiContig ] );
        rOut.put( ',' );
        rOut.number( samPosition( rContigs, xS.begin_ref, xS.end_ref ) );
        rOut.put( ',' );
        rOut.put( bSisterRev ? '-' : '+' );
        rOut.put( ',' );
        putCigarM( rOut, rList, s, xS, bSisterRev, s < k && bSisterRev && isPrinted( uiOptions, rList, s, xS ), bSoftClip, rQ.length );
        rOut.put( ',' );
        if( xS.mapq != xS.mapq )
            lit( rOut, "255" );
        else
            putSigned( rOut, (int64_t)(int)ceil( xS.mapq * 254 ) );
        rOut.put( ',' );
        numberAnd( rOut, uiNm, ';' );
    }
    lit( rOut, "\tQS:i:" );
    rOut.number( rA.begin_q );
    lit( rOut, "\tQE:i:" );
    rOut.number( rA.end_q );
}
// One record of an aligned read: the eleven columns and the CG tag.  rX: what a mate's record has beyond a single read's
// (its clip_length is the read's length for a single read).  Tags: with the NGMLR tags of a single read's record (rRef: a
// Ref) -- the ops of a reverse-strand record are swapped before anything of it is printed, the CIGAR column is M-style
// whatever EQX_CIGAR says (ma_sam.h: FileWriter::execute), the tags stand behind QUAL and before the CG tag.
template <bool Tags = false, class RefT = NoRef, class Sink, class List>
MA_SAM_HD void putRecord( Sink& rOut, uint32_t uiOptions, const Contigs& rContigs, const Read& rQ, const Rec& rA, const List& rList, uint32_t k,
                          const RecordExtras& rX, const RefT& rRef = RefT( ) )
{
    const bool bSoftClip = ( uiOptions & SOFT_CLIP ) != 0, bMCigar = ( uiOptions & EQX_CIGAR ) == 0;
    const uint64_t uiFwd = rContigs.forwardSize( );
    const uint64_t uiBeginRef = rA.begin_ref, uiEndRef = rA.end_ref, uiBeginQ = rA.begin_q, uiEndQ = rA.end_q;
    const bool bRev = uiBeginRef >= uiFwd;
    const bool bLong = ( uiOptions & NO_CG_TAG ) == 0 && rA.n_ops >= 0x10000;
    // QNAME FLAG RNAME POS MAPQ
    rOut.bytes( rQ.name, rQ.name_len );
    rOut.put( '\t' );
    numberAnd( rOut, ( bRev ? 0x10u : 0u ) | ( rA.secondary ? 0x100u : 0u ) | ( rA.supplementary ? 0x800u : 0u ) | rX.extra_flags, '\t' );
    // contig of the begin (pack.h:1063-1067); position of the alignment's forward-strand start, 1-based, (sic) one further for
    // reverse-strand alignments (alignment.h:596-603)
    const uint32_t uiContig = rContigs.idOfForward( bRev ? 2 * uiFwd - ( uiBeginRef + 1 ) : uiBeginRef );
    rOut.bytes( rContigs.names + rContigs.name_off[ uiContig ], rContigs.name_off[ uiContig + 1 ] - rContigs.name_off[ uiContig ] );
    rOut.put( '\t' );
    const uint64_t uiAbs = uiEndRef >= uiFwd ? 2 * uiFwd - ( uiEndRef + 1 ) : uiBeginRef;
    numberAnd( rOut, uiAbs - rContigs.starts[ rContigs.idOfForward( uiAbs ) ] + ( bRev ? 1 : 0 ) + 1, '\t' );
    if( rA.mapq != rA.mapq ) // NaN
        lit( rOut, "255" );
    else
    {
        const int iMapQ = (int)ceil( rA.mapq * 254 );
        if( iMapQ < 0 )
        {
            rOut.put( '-' );
            rOut.number( (uint64_t)( -(int64_t)iMapQ ) );
        }
        else
            rOut.number( (uint64_t)( rX.cap_mapq && iMapQ > 255 ? 255 : iMapQ ) );
    }
    rOut.put( '\t' );
    // CIGAR (alignment.h:367-467): clip, the sections in forward-strand direction, clip
    if( bLong )
        numberAnd( rOut, uiEndQ - uiBeginQ, 'S' );
    else if constexpr( Tags )
        putCigarM( rOut, rList, k, rA, bRev, true, bSoftClip, rX.clip_length );
    else
    {
        const uint64_t uiLeftOver = uiEndQ < rX.clip_length ? rX.clip_length - uiEndQ : 0;
        const uint64_t uiHead = bRev ? uiLeftOver : uiBeginQ, uiTail = bRev ? uiBeginQ : uiLeftOver;
        const char cClip = bSoftClip ? 'S' : 'H';
        if( uiHead > 0 )
            numberAnd( rOut, uiHead, cClip );
        uint64_t uiRunM = 0;
        for( uint32_t j = 0; j < rA.n_ops; j++ )
        {
            const uint32_t jj = bRev ? rA.n_ops - 1 - j : j;
            const uint64_t uiType = rList.opType( k, jj ), uiLen = rList.opLen( k, jj );
            if( uiType <= 2 ) // seed, match, missmatch
            {
                if( bMCigar )
                    uiRunM += uiLen;
                else
                    numberAnd( rOut, uiLen, uiType == 2 ? 'X' : '=' );
            }
            else
            {
                if( bMCigar && uiRunM > 0 )
                {
                    numberAnd( rOut, uiRunM, 'M' );
                    uiRunM = 0;
                }
                numberAnd( rOut, uiLen, uiType == 3 ? 'I' : 'D' );
            }
        }
        if( bMCigar && uiRunM > 0 )
            numberAnd( rOut, uiRunM, 'M' );
        if( uiTail > 0 )
            numberAnd( rOut, uiTail, cClip );
    }
    if( !rX.has_partner )
        lit( rOut, "\t*\t0\t0\t" );
    else // RNEXT ("=" on a contig of the same name) PNEXT, TLEN is not output by the reference (fileWriter.cpp:317)
    {
        const uint32_t uiNext = contigOf( rContigs, rX.partner_begin_ref );
        rOut.put( '\t' );
        if( sameName( rContigs, uiNext, uiContig ) )
            rOut.put( '=' );
        else
            rOut.bytes( rContigs.names + rContigs.name_off[ uiNext ], rContigs.name_off[ uiNext + 1 ] - rContigs.name_off[ uiNext ] );
        rOut.put( '\t' );
        rOut.number( samPosition( rContigs, rX.partner_begin_ref, rX.partner_end_ref ) );
        lit( rOut, "\t0\t" );
    }
    // SEQ: the whole read when soft clipping, else the aligned part; reverse-complemented on the reverse strand.  A record that
    // ends beyond the read is an error (the host formatter throws); nothing beyond the read is ever touched.
    const uint64_t uiFrom = bSoftClip ? 0 : uiBeginQ;
    uint64_t uiTo = bSoftClip ? rQ.length : uiEndQ;
    if( uiTo > rQ.length )
    {
        if( bRev )
            rOut.error( ERR_COMP_CHAR_AT, 0, k );
        else
            rOut.error( ERR_QUERY_LENGTH, (int64_t)rQ.length - (int64_t)uiTo, k );
        uiTo = rQ.length;
    }
    if( uiFrom < uiTo )
        rOut.seq( rQ, uiFrom, uiTo, bRev, k );
    rOut.put( '\t' );
    putQuality( rOut, rQ, uiBeginQ, uiEndQ, k ); // (sic) the aligned part, not reversed (alignment.h:611-614)
    if constexpr( Tags )
        putNgmlrTags( rOut, uiOptions, rContigs, rQ, rA, rList, k, rRef );
    if( bLong ) // TagGenerator::computeTag (fileWriter.h:327-357): the real cigar as CG:B:I
    {
        lit( rOut, "\tCG:B:I" );
        if constexpr( Tags )
        {
            SwappedOps<List> xOps{ rList, k, rA.n_ops, bRev };
            for( uint32_t j = 0; j < rA.n_ops; j++ )
            {
                const uint32_t jj = xOps.forward( j );
                const uint64_t uiType = rList.opType( k, jj );
                rOut.put( ',' );
                rOut.number( (uint32_t)( rList.opLen( k, jj ) << 4 ) | (uint32_t)( ( 0x21877u >> ( 4 * ( uiType < 5 ? uiType : 0 ) ) ) & 0xf ) );
            }
        }
        else
            for( uint32_t j = 0; j < rA.n_ops; j++ )
            {
                const uint64_t uiType = rList.opType( k, j );
                rOut.put( ',' );
                // op codes 7 7 8 1 2 of seed, match, missmatch, insertion, deletion
                rOut.number( (uint32_t)( rList.opLen( k, j ) << 4 ) | (uint32_t)( ( 0x21877u >> ( 4 * ( uiType < 5 ? uiType : 0 ) ) ) & 0xf ) );
            }
    }
    rOut.put( '\n' );
}
} // namespace detail

// The SAM records of ONE read: the alignments of rList in MappingQuality order.
template <class Sink, class List>
MA_SAM_HD void formatRead( Sink& rOut, uint32_t uiOptions, const Contigs& rContigs, const Read& rQ, const List& rList )
{
    const uint32_t uiAlns = rList.size( );
    bool bAny = false;
    for( uint32_t k = 0; k < uiAlns; k++ )
    {
        const Rec xA = rList.rec( k );
        bool bNonZero = false; // Alignment::length( ) != 0
        for( uint32_t j = 0; j < xA.n_ops && !bNonZero; j++ )
            bNonZero = rList.opLen( k, j ) != 0;
        if( !bNonZero )
            continue;
        if( ( ( uiOptions & NO_SECONDARY ) && xA.secondary ) || ( ( uiOptions & NO_SUPPLEMENTARY ) && xA.supplementary ) )
            continue;
        RecordExtras xExtras;
        xExtras.clip_length = rQ.length;
        detail::putRecord( rOut, uiOptions, rContigs, rQ, xA, rList, k, xExtras );
        bAny = true;
    }
    if( uiAlns == 0 )
        detail::putUnmapped( rOut, rQ, true );
    else if( !bAny )
        detail::putUnmapped( rOut, rQ, false );
}
// The same with reference bases and holes at hand: with NGMLR_TAGS among the options every record carries the tags, without
// the bit this is formatRead above.
template <class Sink, class List, class RefT>
MA_SAM_HD void formatRead( Sink& rOut, uint32_t uiOptions, const Contigs& rContigs, const Read& rQ, const List& rList, const RefT& rRef )
{
    if( ( uiOptions & NGMLR_TAGS ) == 0 )
    {
        formatRead( rOut, uiOptions, rContigs, rQ, rList );
        return;
    }
    const uint32_t uiAlns = rList.size( );
    bool bAny = false;
    for( uint32_t k = 0; k < uiAlns; k++ )
    {
        const Rec xA = rList.rec( k );
        if( !detail::isPrinted( uiOptions, rList, k, xA ) )
            continue;
        RecordExtras xExtras;
        xExtras.clip_length = rQ.length;
        detail::putRecord<true>( rOut, uiOptions, rContigs, rQ, xA, rList, k, xExtras, rRef );
        bAny = true;
    }
    if( uiAlns == 0 )
        detail::putUnmapped( rOut, rQ, true );
    else if( !bAny )
        detail::putUnmapped( rOut, rQ, false );
}

namespace detail
{
// The record of an unaligned mate (fileWriter.cpp:320-366): without an anchor the pair has no record at all (QUAL printed), with
// one the mate is placed at the anchor's position (RNEXT "=", QUAL "*")
template <class Sink>
MA_SAM_HD void putUnalignedMate( Sink& rOut, const Contigs& rContigs, const Read& rQ, bool bFirst, uint32_t uiExtraFlags, bool bAnchor,
                                 uint64_t uiAnchorBeginRef, uint64_t uiAnchorEndRef )
{
    const uint32_t k = bFirst ? UNMAPPED_FIRST : UNMAPPED_SECOND;
    rOut.bytes( rQ.name, rQ.name_len );
    rOut.put( '\t' );
    numberAnd( rOut, 0x4u | 0x1u | ( bFirst ? 0x40u : 0x80u ) | uiExtraFlags, '\t' );
    if( !bAnchor )
        lit( rOut, "*\t0\t0\t*\t*\t0\t0\t" );
    else
    {
        const uint32_t uiContig = contigOf( rContigs, uiAnchorBeginRef );
        const uint64_t uiPos = samPosition( rContigs, uiAnchorBeginRef, uiAnchorEndRef );
        rOut.bytes( rContigs.names + rContigs.name_off[ uiContig ], rContigs.name_off[ uiContig + 1 ] - rContigs.name_off[ uiContig ] );
        rOut.put( '\t' );
        rOut.number( uiPos );
        lit( rOut, "\t0\t*\t=\t" );
        rOut.number( uiPos );
        lit( rOut, "\t0\t" );
    }
    if( rQ.length > 0 )
        rOut.seq( rQ, 0, rQ.length, false, k );
    rOut.put( '\t' );
    if( !bAnchor )
        putQuality( rOut, rQ, 0, rQ.length, k );
    else
        rOut.put( '*' );
    rOut.put( '\n' );
}
} // namespace detail

// The SAM records of ONE mate pair: the bytes of PairedFileWriter::execute (fileWriter.cpp:158-383; ma_sam.h) from a pair
// list, in its three record shapes, oddities included:
//   aligned mate          FLAG = strand | secondary | supplementary | 0x1 | 0x2 (always) | 0x40 / 0x80 | 0x20 (partner on the
//                         reverse strand), RNEXT / PNEXT = the partner ("=" on a contig of the same name), TLEN 0, MAPQ capped
//                         at 255, CIGAR clipped against the length of the FIRST mate (sic, :191-193)
//   pair without any      FLAG = 0x4 | 0x1 | 0x40 / 0x80 | 0x8, everything else empty, QUAL printed
//   one mate unaligned    placed at record 0 of the list, printed or not (:348-366), RNEXT "=", QUAL "*"
// error( kind, value, k ) names record k of the pair list.
template <class Sink, class PairList>
MA_SAM_HD void formatPair( Sink& rOut, uint32_t uiOptions, const Contigs& rContigs, const Read& rQ1, const Read& rQ2, const PairList& rList )
{
    const uint32_t uiAlns = rList.size( );
    const uint64_t uiFwd = rContigs.forwardSize( );
    bool bHasFirst = false, bHasSecond = false;
    for( uint32_t k = 0; k < uiAlns; k++ )
    {
        const Rec xA = rList.rec( k );
        bool bNonZero = false; // Alignment::length( ) != 0
        for( uint32_t j = 0; j < xA.n_ops && !bNonZero; j++ )
            bNonZero = rList.opLen( k, j ) != 0;
        if( !bNonZero || ( ( uiOptions & NO_SECONDARY ) && xA.secondary ) || ( ( uiOptions & NO_SUPPLEMENTARY ) && xA.supplementary ) )
            continue;
        const bool bFirst = rList.mate( k ) != 0;
        if( bFirst )
            bHasFirst = true;
        else
            bHasSecond = true;
        RecordExtras xExtras;
        xExtras.extra_flags = 0x1u | 0x2u | ( bFirst ? 0x40u : 0x80u );
        xExtras.cap_mapq = true;
        xExtras.clip_length = rQ1.length;
        const int32_t iOther = rList.other( k );
        if( iOther >= 0 )
        {
            xExtras.has_partner = true;
            const Rec xOther = rList.rec( (uint32_t)iOther );
            xExtras.partner_begin_ref = xOther.begin_ref, xExtras.partner_end_ref = xOther.end_ref;
            if( xOther.begin_ref >= uiFwd )
                xExtras.extra_flags |= 0x20u;
        }
        const Read xQ = bFirst ? rQ1 : rQ2; // (a copy: a reference would pin both reads in memory on the device)
        detail::putRecord( rOut, uiOptions, rContigs, xQ, xA, rList, k, xExtras );
    }
    if( !bHasFirst && !bHasSecond )
    {
        detail::putUnalignedMate( rOut, rContigs, rQ1, true, 0x8u, false, 0, 0 );
        detail::putUnalignedMate( rOut, rContigs, rQ2, false, 0x8u, false, 0, 0 );
    }
    else if( bHasFirst != bHasSecond )
    {
        const Read xQ = bHasFirst ? rQ2 : rQ1;
        const Rec xAnchor = rList.rec( 0 );
        detail::putUnalignedMate( rOut, rContigs, xQ, !bHasFirst, 0, true, xAnchor.begin_ref, xAnchor.end_ref );
    }
}

// The text of the host formatter's exception for an error a sink was told of; returns its length (the text is
// 0-terminated; 64 bytes hold the two kinds of a record beyond its read, 96 bytes every kind).
inline size_t errorText( char* buf, uint32_t uiKind, int64_t iValue )
{
    WriteSink xOut{ buf };
    if( uiKind == ERR_QUERY_LENGTH )
    {
        detail::lit( xOut, "Query length is off by " );
        if( iValue < 0 )
        {
            xOut.put( '-' );
            xOut.number( (uint64_t)( -iValue ) );
        }
        else
            xOut.number( (uint64_t)iValue );
        xOut.put( '.' );
    }
    else if( uiKind == ERR_BRIDGING )
        detail::lit( xOut, "(vExtractSubsection) Try to extract bridging sequence. This is impossible." );
    else if( uiKind == ERR_OPS_COVERAGE ) // (the library's own: the caller names the record)
        detail::lit( xOut, "the ops do not cover the record's reference and query intervals" );
    else
        detail::lit( xOut, "Index out of range (compCharAt)" );
    xOut.put( '\0' );
    return (size_t)xOut.size( ) - 1;
}
} // namespace ma_sam
