// GPU check of the SAM mode of the host layer with "Emulate NGMLR's tag output": the same reads through
//   host   BatchAligner::execute + FileWriter (Alignment containers, the tags formatted on the host)             -> <out>.host.sam
//   dev    BatchAligner::executeFlatSam + BatchFileWriter::write (text with tags formatted on the device)        -> <out>.dev.sam
//   multi  MultiDeviceAligner::executeFlatSam over <shards> replicas on device 0, run twice                      -> <out>.multi.sam
// in device batches of <batch> reads, two in flight.  The caller compares the files.  The pack gets the holes given (start,
// length pairs on the forward strand), which BatchAligner pushes to the index and its replicas.  Every batch has to come back as
// device text made with the tag bit; a writer without the option has to refuse it.
//
//   sam_tags_graph_test <genome.fa> <reads.fa|fq> <out prefix> <preset> <batch> <shards> <sam options: bits of ma_sam_batch> [hole start, length]...
#include "ma_batch_nodes.h"
#include <cstdio>

using namespace libMA;

int main( int argc, char** argv )
{
    if( argc < 8 )
    {
        fprintf( stderr, "usage: sam_tags_graph_test <genome.fa> <reads> <out prefix> <preset> <batch> <shards> <sam options> [holes]\n" );
        return 2;
    }
    try
    {
        ParameterSetManager xParams;
        xParams.setSelected( argv[ 4 ] );
        const uint32_t uiBits = (uint32_t)atoi( argv[ 7 ] );
        xParams.xSam.bSoftClip = ( uiBits & MA_SAM_SOFT_CLIP ) != 0, xParams.xSam.bOutputMCigar = ( uiBits & MA_SAM_EQX_CIGAR ) == 0;
        xParams.xSam.bNoSecondary = ( uiBits & MA_SAM_NO_SECONDARY ) != 0, xParams.xSam.bNoSupplementary = ( uiBits & MA_SAM_NO_SUPPLEMENTARY ) != 0;
        xParams.xSam.bCGTag = ( uiBits & MA_SAM_NO_CG_TAG ) == 0, xParams.xSam.bEmulateNgmlrTags = ( uiBits & MA_SAM_NGMLR_TAGS ) != 0;
        if( BatchAligner::samOptionBits( xParams.xSam ) != uiBits || !xParams.xSam.bEmulateNgmlrTags )
            throw std::runtime_error( "samOptionBits does not give the bits back, or the tag bit is not among them" );
        std::shared_ptr<Pack> pPack;
        std::shared_ptr<FMIndex> pFM;
        srand( 1 );
        buildIndexFromFasta( argv[ 1 ], pPack, pFM );
        for( int i = 8; i + 1 < argc; i += 2 )
            pPack->vHoles.emplace_back( strtoull( argv[ i ], nullptr, 10 ), strtoull( argv[ i + 1 ], nullptr, 10 ) );
        FileReader xReader( xParams );
        auto pIn = fileStreamFromPath( argv[ 2 ] );
        auto pReads = std::make_shared<ReadVector>( );
        while( auto pQ = xReader.execute( pIn ) )
            pReads->push_back( pQ );
        const std::string sOut = argv[ 3 ];
        const size_t uiBatch = (size_t)atoi( argv[ 5 ] );
        size_t uiText = 0, uiRecords = 0;
        auto writeAll = [ & ]( const std::string& sFile, BatchAligner::TP_FLAT& rFlat ) {
            BatchFileWriter xWriter( xParams, std::make_shared<FileWriter>( xParams, sFile, pPack ), pPack );
            size_t uiAt = 0;
            for( const auto& pB : rFlat )
            {
                if( pB == nullptr || pB->uiFirst != uiAt )
                    throw std::runtime_error( "the batches are not in input order" );
                xWriter.write( *pB, pPack );
                uiAt += pB->size( );
                ( pB->hasSamText( ) && ( pB->samOptions( ) & MA_SAM_NGMLR_TAGS ) ? uiText : uiRecords )++;
            }
            if( uiAt != pReads->size( ) || xWriter.uiReads != pReads->size( ) )
                throw std::runtime_error( "the batches do not cover the reads" );
        };
        {
            BatchAligner xAligner( xParams );
            xAligner.uiBatchReads = uiBatch, xAligner.uiInflight = 2;
            if( !xAligner.servesSam( ) || xAligner.servesPairSam( ) )
                throw std::runtime_error( "servesSam( ) / servesPairSam( ) under the tag emulation" );
            {
                auto pRes = xAligner.execute( pFM, pReads );
                FileWriter xWriter( xParams, sOut + ".host.sam", pPack );
                for( size_t i = 0; i < pReads->size( ); i++ )
                    xWriter.execute( ( *pReads )[ i ], ( *pRes )[ i ], pPack );
            }
            auto pDev = xAligner.executeFlatSam( pFM, pReads, pPack );
            writeAll( sOut + ".dev.sam", *pDev );
            // a writer whose options do not ask for the tags refuses the text that carries them
            ParameterSetManager xPlain = xParams;
            xPlain.xSam.bEmulateNgmlrTags = false;
            BatchFileWriter xRefuses( xPlain, std::static_pointer_cast<OutStream>( std::make_shared<StringOutStream>( ) ), pPack );
            bool bRefused = false;
            try
            {
                xRefuses.write( *pDev->front( ), pPack );
            }
            catch( const std::runtime_error& )
            {
                bRefused = true;
            }
            if( !bRefused )
                throw std::runtime_error( "a writer without the option wrote text with tags" );
        }
        const int iShards = atoi( argv[ 6 ] );
        auto vReplicas = MultiDeviceAligner::replicate( pFM, std::vector<int>( (size_t)iShards, 0 ), 0 );
        MultiDeviceAligner xMulti( xParams, vReplicas );
        xMulti.uiBatchReads = uiBatch, xMulti.uiInflight = 2;
        xMulti.executeFlatSam( pReads, pPack );
        auto pMulti = xMulti.executeFlatSam( pReads, pPack );
        writeAll( sOut + ".multi.sam", *pMulti );
        size_t uiShardsUsed = 0;
        for( const auto& rT : xMulti.vLast )
            uiShardsUsed += rT.uiBatches != 0;
        printf( "{\"reads\": %zu, \"text_batches\": %zu, \"record_batches\": %zu, \"shards_used\": %zu}\n", pReads->size( ), uiText, uiRecords,
                uiShardsUsed );
    }
    catch( const std::exception& e )
    {
        fprintf( stderr, "error: %s\n", e.what( ) );
        return 1;
    }
    return 0;
}
