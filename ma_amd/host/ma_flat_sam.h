// ma_flat_sam.h -- SAM text straight from the FLAT result of a device batch (ma_engine.h: BatchResult -- one header array +
// one ops array per batch, as ma_batch_get_mapq_alignments downloads them), without building an Alignment object per
// alignment.  Reference-free (C ABI records + plain views of the reads and of the contig table), so the mirror modules
// (ma_modules.h / ma_sam.h) and the binding on the reference's real types (ma_ref_binding.h) share it.
//
// The bytes are those of the reference's FileWriter::execute (libs/ma/src/module/fileWriter.cpp:11-158) with
// Alignment::cigarString / getSamFlag / getSamPosition / getQuerySequence (libs/ma/inc/ma/container/alignment.h:367-467,
// 576-623) and Pack's position arithmetic (pack.h:900-997,1063-1067) for the options a flat view can serve: soft / hard
// clipping, M or =/X cigars, the CG tag of over-long cigars, omitting secondary / supplementary records.  "Emulate NGMLR's
// tag output" needs reference bases and Alignment objects: callers fall back to the per-read writer for it.
// formatPair is the same for PairedFileWriter::execute (fileWriter.cpp:158-383) on the records ma_batch_get_pairs returns.
// Pinned by tests/test_sam_writer.py and tests/test_pairs_host.py against the SAM goldens the compiled reference wrote.
#pragma once
#include "ma_amd.h"
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace ma_amd
{
namespace flat
{
struct SamFormat
{
    bool bNoSecondary = false, bNoSupplementary = false, bOutputMCigar = true, bCGTag = true, bSoftClip = false;
};
// contig table of the pack (forward strand): names, start offsets, lengths
struct Contigs
{
    std::vector<std::string> vNames;
    std::vector<uint64_t> vStarts, vLengths;
    uint64_t forwardSize( ) const
    {
        return vStarts.empty( ) ? 0 : vStarts.back( ) + vLengths.back( );
    }
    // Pack::uiSequenceIdForPosition (pack.h:933-990) of a position on the forward strand
    size_t idOfForward( uint64_t uiPos ) const
    {
        size_t lo = 0, hi = vStarts.size( );
        while( hi - lo > 1 )
        {
            const size_t mid = ( lo + hi ) / 2;
            if( uiPos >= vStarts[ mid ] )
                lo = mid;
            else
                hi = mid;
        }
        return lo;
    }
};
struct ReadView
{
    const char* sName = nullptr;
    size_t uiNameLen = 0;
    const uint8_t* pCodes = nullptr; // A0 C1 G2 T3, else N
    const uint8_t* pQuality = nullptr; // FASTQ quality characters or null
    size_t uiLength = 0;
};

// An append-only byte arena: one per formatting thread and batch, written to the stream with one call.
class Arena
{
    std::vector<char> v;
    size_t n = 0;

  public:
    void clear( )
    {
        n = 0;
    }
    size_t size( ) const
    {
        return n;
    }
    const char* data( ) const
    {
        return v.data( );
    }
    char* grow( size_t k ) // k more bytes, returns where they start
    {
        if( n + k > v.size( ) )
            v.resize( ( n + k ) * 2 + 4096 );
        char* p = v.data( ) + n;
        n += k;
        return p;
    }
    void put( char c )
    {
        *grow( 1 ) = c;
    }
    void put( const char* s, size_t k )
    {
        memcpy( grow( k ), s, k );
    }
    void lit( const char* s )
    {
        put( s, strlen( s ) );
    }
    void number( uint64_t x )
    {
        char a[ 24 ];
        int k = 0;
        do
        {
            a[ k++ ] = (char)( '0' + x % 10 );
            x /= 10;
        } while( x != 0 );
        char* p = grow( (size_t)k );
        while( k > 0 )
            *p++ = a[ --k ];
    }
    void numberSigned( int64_t x )
    {
        if( x < 0 )
        {
            put( '-' );
            number( (uint64_t)( -x ) );
        }
        else
            number( (uint64_t)x );
    }
};

namespace detail
{
inline const char* baseChars( )
{
    return "ACGTN";
}
inline void putBases( Arena& rOut, const ReadView& rQ, uint64_t uiFrom, uint64_t uiTo )
{
    if( uiTo > rQ.uiLength )
        uiTo = rQ.uiLength;
    if( uiFrom >= uiTo )
        return;
    char* p = rOut.grow( uiTo - uiFrom );
    for( uint64_t i = uiFrom; i < uiTo; i++ )
        *p++ = baseChars( )[ rQ.pCodes[ i ] < 4 ? rQ.pCodes[ i ] : 4 ];
}
inline void putBasesReverseComplement( Arena& rOut, const ReadView& rQ, uint64_t uiFrom, uint64_t uiTo )
{
    if( uiTo > rQ.uiLength )
        throw std::runtime_error( "Index out of range (compCharAt)" );
    if( uiFrom >= uiTo )
        return;
    char* p = rOut.grow( uiTo - uiFrom );
    for( uint64_t i = uiTo; i > uiFrom; i-- )
    {
        const uint8_t c = rQ.pCodes[ i - 1 ];
        *p++ = baseChars( )[ c < 4 ? 3 - c : 4 ];
    }
}
inline void putQuality( Arena& rOut, const ReadView& rQ, uint64_t uiFrom, uint64_t uiTo ) // nucSeq.h:697-709; never reversed
{
    if( rQ.pQuality == nullptr )
    {
        rOut.put( '*' );
        return;
    }
    if( uiTo > rQ.uiLength )
        uiTo = rQ.uiLength;
    if( uiFrom < uiTo )
        rOut.put( (const char*)rQ.pQuality + uiFrom, uiTo - uiFrom );
}
inline void putUnmapped( Arena& rOut, const ReadView& rQ, const char* sMapQ ) // fileWriter.cpp:126-140
{
    rOut.put( rQ.sName, rQ.uiNameLen );
    rOut.lit( "\t4\t*\t0\t" );
    rOut.lit( sMapQ );
    rOut.lit( "\t*\t*\t0\t0\t" );
    putBases( rOut, rQ, 0, rQ.uiLength );
    rOut.put( '\t' );
    putQuality( rOut, rQ, 0, rQ.uiLength );
    rOut.put( '\n' );
}
} // namespace detail

namespace detail
{
// contig of the begin (pack.h:1063-1067)
inline size_t contigOf( const Contigs& rContigs, const ma_alignment& rA )
{
    const uint64_t uiFwd = rContigs.forwardSize( ), uiBeginRef = (uint64_t)rA.begin_ref;
    return rContigs.idOfForward( uiBeginRef >= uiFwd ? 2 * uiFwd - ( uiBeginRef + 1 ) : uiBeginRef );
}
// Alignment::getSamPosition: position of the alignment's forward-strand start, 1-based, (sic) one further for reverse-strand
// alignments (alignment.h:596-603)
inline uint64_t samPosition( const Contigs& rContigs, const ma_alignment& rA )
{
    const uint64_t uiFwd = rContigs.forwardSize( ), uiBeginRef = (uint64_t)rA.begin_ref, uiEndRef = (uint64_t)rA.end_ref;
    const uint64_t uiAbs = uiEndRef >= uiFwd ? 2 * uiFwd - ( uiEndRef + 1 ) : uiBeginRef;
    return uiAbs - rContigs.vStarts[ rContigs.idOfForward( uiAbs ) ] + ( uiBeginRef >= uiFwd ? 1 : 0 ) + 1;
}
// what a record of a pair has beyond a single read's (all neutral for FileWriter's records)
struct RecordExtras
{
    uint32_t uiExtraFlags = 0;
    bool bCapMapQ = false; // the paired writer caps MAPQ at 255 (fileWriter.cpp:262)
    uint64_t uiClipLength = 0; // query length the cigar is clipped against
    const ma_alignment* pPartner = nullptr; // RNEXT / PNEXT
};
// One record of an aligned read: the eleven columns and the CG tag
inline void putRecord( Arena& rOut, const SamFormat& rF, const Contigs& rContigs, const ReadView& rQ, const ma_alignment& rA,
                       const uint64_t* pPairs, const RecordExtras& rX )
{
    const uint64_t uiFwd = rContigs.forwardSize( );
    const uint64_t uiBeginRef = (uint64_t)rA.begin_ref;
    const uint64_t uiBeginQ = (uint64_t)rA.begin_q, uiEndQ = (uint64_t)rA.end_q;
    const bool bRev = uiBeginRef >= uiFwd;
    const bool bLong = rF.bCGTag && rA.n_ops >= 0x10000;
    // QNAME FLAG RNAME POS MAPQ
    rOut.put( rQ.sName, rQ.uiNameLen );
    rOut.put( '\t' );
    rOut.number( ( bRev ? 0x10u : 0u ) | ( rA.secondary ? 0x100u : 0u ) | ( rA.supplementary ? 0x800u : 0u ) | rX.uiExtraFlags );
    rOut.put( '\t' );
    // contig of the begin (pack.h:1063-1067); position of the alignment's forward-strand start, 1-based, (sic) one further
    // for reverse-strand alignments (alignment.h:596-603)
    const std::string& rName = rContigs.vNames[ contigOf( rContigs, rA ) ];
    rOut.put( rName.data( ), rName.size( ) );
    rOut.put( '\t' );
    rOut.number( samPosition( rContigs, rA ) );
    rOut.put( '\t' );
    if( std::isnan( rA.mapq ) )
        rOut.lit( "255" );
    else
    {
        const int iMapQ = static_cast<int>( std::ceil( rA.mapq * 254 ) );
        rOut.numberSigned( (int64_t)( rX.bCapMapQ && iMapQ > 255 ? 255 : iMapQ ) );
    }
    rOut.put( '\t' );
    // CIGAR (alignment.h:367-467): clip, the sections in forward-strand direction, clip
    if( bLong )
    {
        rOut.number( uiEndQ - uiBeginQ );
        rOut.put( 'S' );
    }
    else
    {
        const uint64_t uiLeftOver = uiEndQ < rX.uiClipLength ? rX.uiClipLength - uiEndQ : 0;
        const uint64_t uiHead = bRev ? uiLeftOver : uiBeginQ, uiTail = bRev ? uiBeginQ : uiLeftOver;
        const char cClip = rF.bSoftClip ? 'S' : 'H';
        if( uiHead > 0 )
        {
            rOut.number( uiHead );
            rOut.put( cClip );
        }
        uint64_t uiRunM = 0;
        for( uint32_t j = 0; j < rA.n_ops; j++ )
        {
            const uint64_t* pPair = pPairs + 2 * ( bRev ? rA.n_ops - 1 - j : j );
            const uint64_t uiType = pPair[ 0 ], uiLen = pPair[ 1 ];
            if( uiType <= 2 ) // seed, match, missmatch
            {
                if( rF.bOutputMCigar )
                    uiRunM += uiLen;
                else
                {
                    rOut.number( uiLen );
                    rOut.put( uiType == 2 ? 'X' : '=' );
                }
            }
            else
            {
                if( rF.bOutputMCigar && uiRunM > 0 )
                {
                    rOut.number( uiRunM );
                    rOut.put( 'M' );
                    uiRunM = 0;
                }
                rOut.number( uiLen );
                rOut.put( uiType == 3 ? 'I' : 'D' );
            }
        }
        if( rF.bOutputMCigar && uiRunM > 0 )
        {
            rOut.number( uiRunM );
            rOut.put( 'M' );
        }
        if( uiTail > 0 )
        {
            rOut.number( uiTail );
            rOut.put( cClip );
        }
    }
    if( rX.pPartner == nullptr )
        rOut.lit( "\t*\t0\t0\t" );
    else // RNEXT ("=" on a contig of the same name) PNEXT, TLEN is not output by the reference (fileWriter.cpp:317)
    {
        const std::string& rNext = rContigs.vNames[ contigOf( rContigs, *rX.pPartner ) ];
        rOut.put( '\t' );
        if( rNext == rName )
            rOut.put( '=' );
        else
            rOut.put( rNext.data( ), rNext.size( ) );
        rOut.put( '\t' );
        rOut.number( samPosition( rContigs, *rX.pPartner ) );
        rOut.lit( "\t0\t" );
    }
    // SEQ: the whole read when soft clipping, else the aligned part; reverse-complemented on the reverse strand
    const uint64_t uiFrom = rF.bSoftClip ? 0 : uiBeginQ, uiTo = rF.bSoftClip ? rQ.uiLength : uiEndQ;
    if( !rF.bSoftClip && uiTo > rQ.uiLength && !bRev )
        throw std::runtime_error( "Query length is off by " + std::to_string( (int64_t)rQ.uiLength - (int64_t)uiTo ) + "." );
    if( bRev )
        detail::putBasesReverseComplement( rOut, rQ, uiFrom, uiTo );
    else
        detail::putBases( rOut, rQ, uiFrom, uiTo );
    rOut.put( '\t' );
    detail::putQuality( rOut, rQ, uiBeginQ, uiEndQ ); // (sic) the aligned part, not reversed (alignment.h:611-614)
    if( bLong ) // TagGenerator::computeTag (fileWriter.h:327-357): the real cigar as CG:B:I
    {
        rOut.lit( "\tCG:B:I" );
        for( uint32_t j = 0; j < rA.n_ops; j++ )
        {
            static const uint32_t aOp[ 5 ] = { 7, 7, 8, 1, 2 };
            rOut.put( ',' );
            rOut.number( (uint32_t)( pPairs[ 2 * j + 1 ] << 4 ) | aOp[ pPairs[ 2 * j ] < 5 ? pPairs[ 2 * j ] : 0 ] );
        }
    }
    rOut.put( '\n' );
}
} // namespace detail

// The SAM records of ONE read: its alignments pAlns[0 .. uiAlns) (MappingQuality order) with their (type, length) pairs in
// pOps (pAlns[k].ops_off counts pairs).
inline void formatRead( Arena& rOut, const SamFormat& rF, const Contigs& rContigs, const ReadView& rQ, const ma_alignment* pAlns, size_t uiAlns,
                        const uint64_t* pOps )
{
    const size_t uiStart = rOut.size( );
    for( size_t k = 0; k < uiAlns; k++ )
    {
        const ma_alignment& rA = pAlns[ k ];
        const uint64_t* pPairs = pOps + 2 * rA.ops_off;
        uint64_t uiLength = 0;
        for( uint32_t j = 0; j < rA.n_ops; j++ )
            uiLength += pPairs[ 2 * j + 1 ];
        if( uiLength == 0 )
            continue;
        if( ( rF.bNoSecondary && rA.secondary ) || ( rF.bNoSupplementary && rA.supplementary ) )
            continue;
        detail::RecordExtras xExtras;
        xExtras.uiClipLength = rQ.uiLength;
        detail::putRecord( rOut, rF, rContigs, rQ, rA, pPairs, xExtras );
    }
    if( uiAlns == 0 )
        detail::putUnmapped( rOut, rQ, "255" );
    else if( rOut.size( ) == uiStart )
        detail::putUnmapped( rOut, rQ, "0" );
}

// The SAM records of ONE mate pair: the records PairedReads left (ma_batch_get_pairs: pAlns[0 .. uiAlns), pMate[k] != 0 =
// record of the first mate, pOther[k] = index of the partner's record or -1).  The bytes are those of
// PairedFileWriter::execute (fileWriter.cpp:158-383) in its three record shapes, oddities included:
//   aligned mate          FLAG = strand | secondary | supplementary | 0x1 | 0x2 (always) | 0x40 / 0x80 | 0x20 (partner on the
//                         reverse strand), RNEXT / PNEXT = the partner ("=" on a contig of the same name), TLEN 0, MAPQ capped
//                         at 255, CIGAR clipped against the length of the FIRST mate (sic, :191-193)
//   pair without any      FLAG = 0x4 | 0x1 | 0x40 / 0x80 | 0x8, everything else empty, QUAL printed
//   one mate unaligned    placed at the first record of the list (:348-366), RNEXT "=", QUAL "*"
inline void formatPair( Arena& rOut, const SamFormat& rF, const Contigs& rContigs, const ReadView& rQ1, const ReadView& rQ2,
                        const ma_alignment* pAlns, size_t uiAlns, const uint64_t* pOps, const int32_t* pMate, const int32_t* pOther )
{
    const ReadView* const apMate[ 2 ] = { &rQ1, &rQ2 };
    const uint32_t aMateFlag[ 2 ] = { 0x40u, 0x80u };
    const uint64_t uiFwd = rContigs.forwardSize( );
    bool aHasRecord[ 2 ] = { false, false };
    for( size_t k = 0; k < uiAlns; k++ )
    {
        const ma_alignment& rA = pAlns[ k ];
        const uint64_t* pPairs = pOps + 2 * rA.ops_off;
        uint64_t uiLength = 0;
        for( uint32_t j = 0; j < rA.n_ops; j++ )
            uiLength += pPairs[ 2 * j + 1 ];
        if( uiLength == 0 || ( rF.bNoSecondary && rA.secondary ) || ( rF.bNoSupplementary && rA.supplementary ) )
            continue;
        const int iMate = pMate[ k ] != 0 ? 0 : 1;
        aHasRecord[ iMate ] = true;
        detail::RecordExtras xExtras;
        xExtras.uiExtraFlags = 0x1u | 0x2u | aMateFlag[ iMate ];
        xExtras.bCapMapQ = true;
        xExtras.uiClipLength = rQ1.uiLength;
        if( pOther[ k ] >= 0 )
        {
            xExtras.pPartner = pAlns + pOther[ k ];
            if( (uint64_t)xExtras.pPartner->begin_ref >= uiFwd )
                xExtras.uiExtraFlags |= 0x20u;
        }
        detail::putRecord( rOut, rF, rContigs, *apMate[ iMate ], rA, pPairs, xExtras );
    }
    auto unaligned = [ & ]( int iMate, uint32_t uiExtraFlags, const ma_alignment* pAnchor, bool bWithQuality ) {
        const ReadView& rQ = *apMate[ iMate ];
        rOut.put( rQ.sName, rQ.uiNameLen );
        rOut.put( '\t' );
        rOut.number( 0x4u | 0x1u | aMateFlag[ iMate ] | uiExtraFlags );
        rOut.put( '\t' );
        if( pAnchor == nullptr )
            rOut.lit( "*\t0\t0\t*\t*\t0\t0\t" );
        else
        {
            const std::string& rName = rContigs.vNames[ detail::contigOf( rContigs, *pAnchor ) ];
            const uint64_t uiPos = detail::samPosition( rContigs, *pAnchor );
            rOut.put( rName.data( ), rName.size( ) );
            rOut.put( '\t' );
            rOut.number( uiPos );
            rOut.lit( "\t0\t*\t=\t" );
            rOut.number( uiPos );
            rOut.lit( "\t0\t" );
        }
        detail::putBases( rOut, rQ, 0, rQ.uiLength );
        rOut.put( '\t' );
        if( bWithQuality )
            detail::putQuality( rOut, rQ, 0, rQ.uiLength );
        else
            rOut.put( '*' );
        rOut.put( '\n' );
    };
    if( !aHasRecord[ 0 ] && !aHasRecord[ 1 ] )
        for( int iMate = 0; iMate < 2; iMate++ )
            unaligned( iMate, 0x8u, nullptr, true );
    else if( aHasRecord[ 0 ] != aHasRecord[ 1 ] )
        unaligned( aHasRecord[ 0 ] ? 1 : 0, 0, pAlns, false );
}
} // namespace flat
} // namespace ma_amd
