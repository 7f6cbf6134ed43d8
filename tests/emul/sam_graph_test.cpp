// GPU check of the SAM mode of the host layer: the same reads through
//   flat   BatchAligner::executeFlat + BatchFileWriter (records downloaded, formatted on the host)        -> <out>.flat.sam
//   dev    BatchAligner::executeFlatSam + BatchFileWriter::write (text formatted on the device)          -> <out>.dev.sam
//   multi  MultiDeviceAligner::executeFlatSam over <shards> replicas on device 0, run twice              -> <out>.multi.sam
// in device batches of <batch> reads, two in flight.  The caller compares the files.  Prints how many batches came back as
// device text and how many as records (a batch whose reads only partly have qualities is not served by the device).
//
//   sam_graph_test <genome.fa> <reads.fa|fq> <out prefix> <preset> <batch> <shards> <sam options: bits of ma_sam_batch> [mix]
// mix: the qualities of reads 0 .. 49 are dropped, so that one batch holds reads with and reads without qualities
#include "ma_batch_nodes.h"
#include <cstdio>

using namespace libMA;

int main( int argc, char** argv )
{
    if( argc < 8 )
    {
        fprintf( stderr, "usage: sam_graph_test <genome.fa> <reads> <out prefix> <preset> <batch> <shards> <sam options>\n" );
        return 2;
    }
    try
    {
        ParameterSetManager xParams;
        xParams.setSelected( argv[ 4 ] );
        const uint32_t uiBits = (uint32_t)atoi( argv[ 7 ] );
        xParams.xSam.bSoftClip = ( uiBits & MA_SAM_SOFT_CLIP ) != 0, xParams.xSam.bOutputMCigar = ( uiBits & MA_SAM_EQX_CIGAR ) == 0;
        xParams.xSam.bNoSecondary = ( uiBits & MA_SAM_NO_SECONDARY ) != 0, xParams.xSam.bNoSupplementary = ( uiBits & MA_SAM_NO_SUPPLEMENTARY ) != 0;
        xParams.xSam.bCGTag = ( uiBits & MA_SAM_NO_CG_TAG ) == 0;
        if( BatchAligner::samOptionBits( xParams.xSam ) != uiBits )
            throw std::runtime_error( "samOptionBits does not give the bits back" );
        std::shared_ptr<Pack> pPack;
        std::shared_ptr<FMIndex> pFM;
        srand( 1 );
        buildIndexFromFasta( argv[ 1 ], pPack, pFM );
        FileReader xReader( xParams );
        auto pIn = fileStreamFromPath( argv[ 2 ] );
        auto pReads = std::make_shared<ReadVector>( );
        while( auto pQ = xReader.execute( pIn ) )
            pReads->push_back( pQ );
        if( argc >= 9 && std::string( argv[ 8 ] ) == "mix" )
            for( size_t i = 0; i < pReads->size( ) && i < 50; i++ )
                ( *pReads )[ i ]->xQuality.clear( );
        const std::string sOut = argv[ 3 ];
        const size_t uiBatch = (size_t)atoi( argv[ 5 ] );
        size_t uiText = 0, uiRecords = 0;
        auto writeAll = [ & ]( const std::string& sFile, BatchAligner::TP_FLAT& rFlat, bool bCount ) {
            BatchFileWriter xWriter( xParams, std::make_shared<FileWriter>( xParams, sFile, pPack ), pPack );
            size_t uiAt = 0;
            for( const auto& pB : rFlat )
            {
                if( pB == nullptr || pB->uiFirst != uiAt )
                    throw std::runtime_error( "the batches are not in input order" );
                xWriter.write( *pB, pPack );
                uiAt += pB->size( );
                if( bCount )
                    ( pB->hasSamText( ) ? uiText : uiRecords )++;
            }
            if( uiAt != pReads->size( ) || xWriter.uiReads != pReads->size( ) )
                throw std::runtime_error( "the batches do not cover the reads" );
        };
        {
            BatchAligner xAligner( xParams );
            xAligner.uiBatchReads = uiBatch, xAligner.uiInflight = 2;
            auto pFlat = xAligner.executeFlat( pFM, pReads );
            writeAll( sOut + ".flat.sam", *pFlat, false );
            auto pDev = xAligner.executeFlatSam( pFM, pReads, pPack );
            writeAll( sOut + ".dev.sam", *pDev, true );
            // the records of a later executeFlat are not touched by the SAM mode the engines ran in before
            auto pAgain = xAligner.executeFlat( pFM, pReads );
            writeAll( sOut + ".again.sam", *pAgain, false );
        }
        const int iShards = atoi( argv[ 6 ] );
        auto vReplicas = MultiDeviceAligner::replicate( pFM, std::vector<int>( (size_t)iShards, 0 ), 0 );
        MultiDeviceAligner xMulti( xParams, vReplicas );
        xMulti.uiBatchReads = uiBatch, xMulti.uiInflight = 2;
        xMulti.executeFlatSam( pReads, pPack );
        auto pMulti = xMulti.executeFlatSam( pReads, pPack );
        writeAll( sOut + ".multi.sam", *pMulti, false );
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
