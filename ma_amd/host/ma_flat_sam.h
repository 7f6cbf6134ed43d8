// ma_flat_sam.h -- SAM text straight from the FLAT result of a device batch (ma_engine.h: BatchResult -- one header array +
// one ops array per batch, as ma_batch_get_mapq_alignments downloads them), without building an Alignment object per
// alignment.  Reference-free (C ABI records + plain views of the reads and of the contig table), so the mirror modules
// (ma_modules.h / ma_sam.h) and the binding on the reference's real types (ma_ref_binding.h) share it.
//
// An ADAPTER: the record layout -- the bytes of the reference's FileWriter::execute and PairedFileWriter::execute, every
// oddity included -- is ma_sam::formatRead / ma_sam::formatPair of ma_sam_dev.h, the formatter the device stage runs.  This
// file only gives it a sink on a byte arena, the contig table in the form it reads and the options as MA_SAM_* bits.  It
// serves the options a flat view can serve: soft / hard clipping, M or =/X cigars, the CG tag of over-long cigars, omitting
// secondary / supplementary records.  "Emulate NGMLR's tag output" needs reference bases: callers fall back to the per-read
// writer for it.  tests/emul/sam_dev_test.cpp and sam_pair_dev_test.cpp pin formatRead / formatPair, byte for byte and
// exception for exception, to the independent writers on containers (ma_sam.h), tests/test_pairs_host.py to the paired golden.
#pragma once
#include "ma_amd.h"
#include "ma_sam_dev.h"
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
    uint32_t options( ) const // the MA_SAM_* bits
    {
        return ( bSoftClip ? ma_sam::SOFT_CLIP : 0u ) | ( bOutputMCigar ? 0u : ma_sam::EQX_CIGAR ) | ( bNoSecondary ? ma_sam::NO_SECONDARY : 0u ) |
               ( bNoSupplementary ? ma_sam::NO_SUPPLEMENTARY : 0u ) | ( bCGTag ? 0u : ma_sam::NO_CG_TAG );
    }
};
// contig table of the pack (forward strand) in the form the formatter reads: the names as one byte array plus offsets, start
// offsets, lengths.  Built ONCE per writer with set( ) and read-only from then on: view( ) hands it to any number of
// formatting threads.  A pack without contigs can only yield unmapped records, which never look at the table; view( ) shows
// it as one nameless contig of length 0, so that nothing ever indexes an empty array.
class ContigTable
{
    std::vector<char> vNames;
    std::vector<uint64_t> vNameOff, vStarts, vLengths;

  public:
    void set( const std::vector<std::string>& rNames, const std::vector<uint64_t>& rStarts, const std::vector<uint64_t>& rLengths )
    {
        if( rNames.size( ) != rStarts.size( ) || rNames.size( ) != rLengths.size( ) )
            throw std::runtime_error( "flat::ContigTable: names, starts and lengths of different counts" );
        vStarts = rStarts, vLengths = rLengths;
        vNames.clear( );
        vNameOff.assign( 1, 0 );
        for( const std::string& s : rNames )
        {
            vNames.insert( vNames.end( ), s.begin( ), s.end( ) );
            vNameOff.push_back( vNames.size( ) );
        }
    }
    ma_sam::Contigs view( ) const
    {
        static const uint64_t aNone[ 2 ] = { 0, 0 };
        if( vStarts.empty( ) )
            return ma_sam::Contigs{ "", aNone, aNone, aNone, 1 };
        return ma_sam::Contigs{ vNames.data( ), vNameOff.data( ), vStarts.data( ), vLengths.data( ), (uint32_t)vStarts.size( ) };
    }
};
// The contig table as three plain vectors: the earlier interface of this file, kept so that code written against it still
// compiles and prints the same bytes.  It holds nothing else -- no flat form that could go stale --, so the overloads of
// formatRead / formatPair that take it build a ContigTable PER CALL and are marked deprecated.
struct Contigs
{
    std::vector<std::string> vNames;
    std::vector<uint64_t> vStarts, vLengths;
    uint64_t forwardSize( ) const
    {
        return vStarts.empty( ) ? 0 : vStarts.back( ) + vLengths.back( );
    }
};
struct ReadView
{
    const char* sName = nullptr;
    size_t uiNameLen = 0;
    const uint8_t* pCodes = nullptr; // A0 C1 G2 T3, else N
    const uint8_t* pQuality = nullptr; // FASTQ quality characters or null
    size_t uiLength = 0;
    ma_sam::Read read( ) const
    {
        return ma_sam::Read{ sName, uiNameLen, pCodes, pQuality, uiLength };
    }
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
};

// The sink of ma_sam_dev.h over an arena (host only).  SEQ and QUAL go in with one grow( ) each; a record that cannot be
// printed throws the text of the reference's exception, "Query length is off by <n>." or "Index out of range (compCharAt)"
// (what the arena holds by then is of no use to anybody).
struct ArenaSink
{
    Arena& rOut;
    uint64_t size( ) const
    {
        return rOut.size( );
    }
    void put( char c )
    {
        rOut.put( c );
    }
    void bytes( const char* s, uint64_t k )
    {
        rOut.put( s, (size_t)k );
    }
    void number( uint64_t x )
    {
        rOut.number( x );
    }
    void seq( const ma_sam::Read& rQ, uint64_t uiFrom, uint64_t uiTo, bool bRev, uint32_t )
    {
        char* p = rOut.grow( (size_t)( uiTo - uiFrom ) );
        if( bRev )
            for( uint64_t i = uiTo; i > uiFrom; i-- )
                *p++ = ma_sam::complementChar( rQ.codes[ i - 1 ] );
        else
            for( uint64_t i = uiFrom; i < uiTo; i++ )
                *p++ = ma_sam::baseChar( rQ.codes[ i ] );
    }
    void qual( const ma_sam::Read& rQ, uint64_t uiFrom, uint64_t uiTo, uint32_t )
    {
        rOut.put( (const char*)rQ.qual + uiFrom, (size_t)( uiTo - uiFrom ) );
    }
    [[noreturn]] void error( uint32_t uiKind, int64_t iValue, uint32_t )
    {
        char aText[ 96 ];
        ma_sam::errorText( aText, uiKind, iValue );
        throw std::runtime_error( aText );
    }
};

// The SAM records of ONE read: its alignments pAlns[0 .. uiAlns) (MappingQuality order) with their (type, length) pairs in
// pOps (pAlns[k].ops_off counts pairs).
inline void formatRead( Arena& rOut, const SamFormat& rF, const ContigTable& rContigs, const ReadView& rQ, const ma_alignment* pAlns, size_t uiAlns,
                        const uint64_t* pOps )
{
    ArenaSink xSink{ rOut };
    ma_sam::formatRead( xSink, rF.options( ), rContigs.view( ), rQ.read( ), ma_sam::FlatList{ pAlns, (uint32_t)uiAlns, pOps } );
}

// The SAM records of ONE mate pair: the records PairedReads left (ma_batch_get_pairs: pAlns[0 .. uiAlns), pMate[k] != 0 =
// record of the first mate, pOther[k] = index of the partner's record or -1).
inline void formatPair( Arena& rOut, const SamFormat& rF, const ContigTable& rContigs, const ReadView& rQ1, const ReadView& rQ2,
                        const ma_alignment* pAlns, size_t uiAlns, const uint64_t* pOps, const int32_t* pMate, const int32_t* pOther )
{
    ArenaSink xSink{ rOut };
    ma_sam::formatPair( xSink, rF.options( ), rContigs.view( ), rQ1.read( ), rQ2.read( ),
                        ma_sam::FlatPairList{ { pAlns, (uint32_t)uiAlns, pOps }, pMate, pOther } );
}

// the same on the plain vectors (see Contigs)
[[deprecated( "builds the contig table per call: hold a flat::ContigTable" )]] inline void
formatRead( Arena& rOut, const SamFormat& rF, const Contigs& rContigs, const ReadView& rQ, const ma_alignment* pAlns, size_t uiAlns, const uint64_t* pOps )
{
    ContigTable xTable;
    xTable.set( rContigs.vNames, rContigs.vStarts, rContigs.vLengths );
    formatRead( rOut, rF, xTable, rQ, pAlns, uiAlns, pOps );
}
[[deprecated( "builds the contig table per call: hold a flat::ContigTable" )]] inline void
formatPair( Arena& rOut, const SamFormat& rF, const Contigs& rContigs, const ReadView& rQ1, const ReadView& rQ2, const ma_alignment* pAlns, size_t uiAlns,
            const uint64_t* pOps, const int32_t* pMate, const int32_t* pOther )
{
    ContigTable xTable;
    xTable.set( rContigs.vNames, rContigs.vStarts, rContigs.vLengths );
    formatPair( rOut, rF, xTable, rQ1, rQ2, pAlns, uiAlns, pOps, pMate, pOther );
}
} // namespace flat
} // namespace ma_amd
