// ma_genome.h -- genome FASTA -> index with the text read on the device: buildIndexFromFastaText, the counterpart of
// buildIndexFromFasta (ma_sam.h) that does not walk the file on the host.  The file goes up in chunks of page-locked memory
// (ma_genome_append_text parses them: contigs, codes, holes), ma_genome_build_index fills the hole bases with the draws of
// srand( uiSeed ) and sorts; the Pack is filled the way buildIndex fills it.  For the same file and seed storeIndex writes the same
// files as after srand( uiSeed ) + buildIndexFromFasta.  A header of its own: ma_engine.h stays as it is.
// Not served, refused by name: a genome as BGZF or gzip (by its first bytes); FASTQ genomes (the library's "a genome is FASTA").
#pragma once
#include "ma_modules.h"
#include <cstdio>

namespace libMA
{
// a genome object of the library, destroyed with its last owner
struct GenomeText
{
    ma_genome* p = nullptr;
    GenomeText( ) = default;
    GenomeText( const GenomeText& ) = delete;
    GenomeText& operator=( const GenomeText& ) = delete;
    ~GenomeText( )
    {
        if( p )
            ma_genome_destroy( p );
    }
};

// The text step: the file to codes on the device, contig table and holes (no index yet).
inline std::shared_ptr<GenomeText> readFastaText( const std::string& sFastaFilePath, uint64_t uiChunkBytes = 256ull << 20 )
{
    struct File
    {
        FILE* p;
        ~File( )
        {
            if( p )
                fclose( p );
        }
    } xFile{ fopen( sFastaFilePath.c_str( ), "rb" ) };
    if( !xFile.p )
        throw std::runtime_error( "File open error." );
    if( fseek( xFile.p, 0, SEEK_END ) != 0 )
        throw std::runtime_error( "buildIndexFromFastaText: " + sFastaFilePath + " is not a file that can be sized" );
    const uint64_t uiFileBytes = (uint64_t)ftell( xFile.p );
    rewind( xFile.p );
    if( uiChunkBytes < 2 )
        uiChunkBytes = 2;
    struct Pinned
    {
        void* p = nullptr;
        ~Pinned( )
        {
            if( p )
                ma_host_free( p );
        }
    } xBuffer;
    auto pGenome = std::make_shared<GenomeText>( );
    GenomeText& xGenome = *pGenome;
    uint64_t uiCap = std::min<uint64_t>( uiChunkBytes, std::max<uint64_t>( uiFileBytes, 2 ) );
    maCheck( ma_host_alloc( uiCap, &xBuffer.p ) );
    maCheck( ma_genome_create( -1, std::max<uint64_t>( uiFileBytes, 1 ), &xGenome.p ) ); // (never more bases than bytes)
    uint64_t uiHeld = 0; // bytes at the front of the buffer that the call before did not consume
    bool bFirst = true;
    for( bool bEnd = false; !bEnd; )
    {
        if( uiHeld == uiCap ) // one line longer than the buffer: a larger one
        {
            Pinned xLarger;
            maCheck( ma_host_alloc( 2 * uiCap, &xLarger.p ) );
            memcpy( xLarger.p, xBuffer.p, uiHeld );
            std::swap( xLarger.p, xBuffer.p );
            uiCap *= 2;
        }
        char* const pText = (char*)xBuffer.p;
        const size_t uiRead = fread( pText + uiHeld, 1, uiCap - uiHeld, xFile.p );
        if( ferror( xFile.p ) )
            throw std::runtime_error( "buildIndexFromFastaText: reading " + sFastaFilePath + " failed" );
        const uint64_t n = uiHeld + uiRead;
        bEnd = uiRead < uiCap - uiHeld;
        if( bFirst && n >= 2 && (uint8_t)pText[ 0 ] == 0x1f && (uint8_t)pText[ 1 ] == 0x8b )
            throw std::runtime_error( "buildIndexFromFastaText: " + sFastaFilePath +
                                      " is compressed (BGZF or gzip); the device reads a genome as plain FASTA text (buildIndexFromFasta)" );
        bFirst = false;
        uint64_t uiConsumed = 0;
        maCheck( ma_genome_append_text( xGenome.p, pText, n, bEnd ? 1 : 0, &uiConsumed ) );
        uiHeld = n - uiConsumed;
        memmove( pText, pText + uiConsumed, uiHeld );
    }
    return pGenome;
}

// The rest: the fill with the draws of srand( uiSeed ), the suffix sort, and the Pack as buildIndex fills it.
inline void buildIndexFromGenomeText( const std::shared_ptr<GenomeText>& pGenome, std::shared_ptr<Pack>& pPack, std::shared_ptr<FMIndex>& pFM,
                                      uint32_t uiSeed = 1 )
{
    GenomeText& xGenome = *pGenome;
    auto pDev = std::make_shared<DeviceIndex>( );
    maCheck( ma_genome_build_index( xGenome.p, uiSeed, &pDev->p ) );
    uint64_t uiContigs = 0, uiBases = 0, uiNameBytes = 0, uiHoles = 0, uiHoleBases = 0;
    maCheck( ma_genome_counts( xGenome.p, &uiContigs, &uiBases, &uiNameBytes, &uiHoles, &uiHoleBases ) );
    std::vector<uint64_t> vNameOff( uiContigs + 1 ), vHoleStart( uiHoles ), vHoleLen( uiHoles );
    std::string sNames( uiNameBytes, '\0' );
    pPack = std::make_shared<Pack>( );
    pPack->vStarts.resize( uiContigs );
    pPack->vLengths.resize( uiContigs );
    pPack->vNumHoles.resize( uiContigs );
    maCheck( ma_genome_get_contigs( xGenome.p, vNameOff.data( ), uiNameBytes ? &sNames[ 0 ] : nullptr, pPack->vStarts.data( ), pPack->vLengths.data( ),
                                    pPack->vNumHoles.data( ) ) );
    maCheck( ma_genome_get_holes( xGenome.p, vHoleStart.data( ), vHoleLen.data( ) ) );
    for( uint64_t i = 0; i < uiContigs; i++ )
        pPack->vNames.push_back( sNames.substr( vNameOff[ i ], vNameOff[ i + 1 ] - vNameOff[ i ] ) );
    for( uint64_t i = 0; i < uiHoles; i++ )
        pPack->vHoles.emplace_back( vHoleStart[ i ], vHoleLen[ i ] );
    pPack->pDev = pDev;
    pFM = std::make_shared<FMIndex>( );
    pFM->pDev = pDev;
}

inline void buildIndexFromFastaText( const std::string& sFastaFilePath, std::shared_ptr<Pack>& pPack, std::shared_ptr<FMIndex>& pFM,
                                     uint32_t uiSeed = 1, uint64_t uiChunkBytes = 256ull << 20 )
{
    buildIndexFromGenomeText( readFastaText( sFastaFilePath, uiChunkBytes ), pPack, pFM, uiSeed );
}
} // namespace libMA
