// GPU check of the pairs-and-SAM mode of the host layer: the same mates through
//   flat   BatchAligner::executePairedFlat + BatchPairedFileWriter (pair records downloaded, formatted on the host)   -> <out>.flat.sam
//   dev    BatchAligner::executePairedFlatSam + BatchPairedFileWriter (text formatted on the device)                  -> <out>.dev.sam
//   multi  MultiDeviceAligner::executePairedFlatSam over two replicas on device 0, run twice                         -> <out>.multi.sam
// The caller compares the files.  Prints how many batches came back as device text and how many as pair records (a batch
// whose reads only partly have qualities is not served by the device).
//
//   pair_sam_graph_test <case> <pairs> <reads per batch> <batches in flight> <out prefix> <preset> <sam options> [quals | mix]
// <pairs>: the first that many pairs of the case (0: all).  quals: every read gets a quality string; mix: all but reads
// 0 .. 49, so that one batch holds reads with and reads without qualities.
#include "../../oracle/dump_format.h"
#include "ma_batch_nodes.h"

#include <cstdio>

using namespace libMA;
using namespace libMS;

int main( int argc, char** argv )
{
    if( argc < 8 )
    {
        fprintf( stderr, "usage: pair_sam_graph_test <case> <pairs> <batch> <in flight> <out prefix> <preset> <sam options> [quals | mix]\n" );
        return 2;
    }
    try
    {
        CaseFile c = readCase( argv[ 1 ] );
        const size_t uiPairs = (size_t)atol( argv[ 2 ] ), uiBatch = (size_t)atol( argv[ 3 ] ), uiInflight = (size_t)atol( argv[ 4 ] );
        const std::string sOut = argv[ 5 ], sQual = argc >= 9 ? argv[ 8 ] : "";
        ParameterSetManager xParams;
        xParams.setSelected( argv[ 6 ] );
        const uint32_t uiBits = (uint32_t)atoi( argv[ 7 ] );
        xParams.xSam.bSoftClip = ( uiBits & MA_SAM_SOFT_CLIP ) != 0, xParams.xSam.bOutputMCigar = ( uiBits & MA_SAM_EQX_CIGAR ) == 0;
        xParams.xSam.bNoSecondary = ( uiBits & MA_SAM_NO_SECONDARY ) != 0, xParams.xSam.bNoSupplementary = ( uiBits & MA_SAM_NO_SUPPLEMENTARY ) != 0;
        xParams.xSam.bCGTag = ( uiBits & MA_SAM_NO_CG_TAG ) == 0;
        std::vector<std::shared_ptr<NucSeq>> vContigs;
        for( size_t i = 0; i < c.contigs.size( ); i++ )
        {
            auto p = std::make_shared<NucSeq>( );
            p->xCodes = c.contigs[ i ];
            p->sName = c.names[ i ];
            vContigs.push_back( p );
        }
        std::shared_ptr<Pack> pPack;
        std::shared_ptr<FMIndex> pFM;
        buildIndex( vContigs, pPack, pFM );
        auto pAll = std::make_shared<ReadVector>( );
        const size_t uiReads = uiPairs ? std::min( 2 * uiPairs, c.reads.size( ) / 2 * 2 ) : c.reads.size( ) / 2 * 2;
        for( size_t i = 0; i < uiReads; i++ )
        {
            auto p = std::make_shared<NucSeq>( );
            p->xCodes = c.reads[ i ];
            p->sName = "r" + std::to_string( i );
            if( sQual == "quals" || ( sQual == "mix" && i >= 50 ) )
                for( size_t k = 0; k < p->xCodes.size( ); k++ )
                    p->xQuality.push_back( (uint8_t)( '#' + ( i * 7 + k * 13 + k / 5 ) % 60 ) );
            pAll->push_back( p );
        }
        size_t uiText = 0, uiRecords = 0;
        auto writeAll = [ & ]( const std::string& sFile, BatchAligner::TP_FLAT& rFlat, bool bCount ) {
            // (on a stream, as the golden was written: PairedFileWriter's header differs between its file and its stream form)
            auto pStream = std::make_shared<StringOutStream>( );
            BatchPairedFileWriter xWriter( xParams, std::static_pointer_cast<OutStream>( pStream ), pPack );
            size_t uiAt = 0;
            for( const auto& pB : rFlat )
            {
                if( pB == nullptr || pB->uiFirst != uiAt )
                    throw std::runtime_error( "the batches are not in input order" );
                if( pB->size( ) % 2 || !pB->paired( ) )
                    throw std::runtime_error( "a batch boundary splits a pair" );
                xWriter.execute( *pB );
                uiAt += pB->size( );
                if( bCount )
                    ( pB->hasSamText( ) ? uiText : uiRecords )++;
            }
            if( uiAt != pAll->size( ) || xWriter.uiReads != pAll->size( ) )
                throw std::runtime_error( "the batches do not cover the reads" );
            FILE* f = fopen( sFile.c_str( ), "w" );
            if( f == nullptr || fwrite( pStream->sText.data( ), 1, pStream->sText.size( ), f ) != pStream->sText.size( ) || fclose( f ) )
                throw std::runtime_error( "cannot write " + sFile );
        };
        {
            BatchAligner xAligner( xParams );
            xAligner.uiBatchReads = uiBatch, xAligner.uiInflight = uiInflight;
            auto pFlat = xAligner.executePairedFlat( pFM, pAll );
            writeAll( sOut + ".flat.sam", *pFlat, false );
            auto pDev = xAligner.executePairedFlatSam( pFM, pAll, pPack );
            writeAll( sOut + ".dev.sam", *pDev, true );
        }
        auto vReplicas = MultiDeviceAligner::replicate( pFM, std::vector<int>( 2, 0 ), 0 );
        MultiDeviceAligner xMulti( xParams, vReplicas );
        xMulti.uiBatchReads = uiBatch, xMulti.uiInflight = uiInflight;
        xMulti.executePairedFlatSam( pAll, pPack );
        auto pMulti = xMulti.executePairedFlatSam( pAll, pPack );
        writeAll( sOut + ".multi.sam", *pMulti, false );
        size_t uiShardsUsed = 0;
        for( const auto& rT : xMulti.vLast )
            uiShardsUsed += rT.uiBatches != 0;
        printf( "{\"pairs\": %zu, \"text_batches\": %zu, \"record_batches\": %zu, \"shards_used\": %zu}\n", pAll->size( ) / 2, uiText, uiRecords,
                uiShardsUsed );
    }
    catch( const std::exception& e )
    {
        fprintf( stderr, "error: %s\n", e.what( ) );
        return 1;
    }
    return 0;
}
