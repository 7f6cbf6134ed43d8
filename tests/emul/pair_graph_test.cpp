// GPU check of the flat paired path of the host layer: BatchAligner::executePairedFlat (mates paired on the device by
// ma_pair_batch, results left flat) + BatchPairedFileWriter (ma_flat_sam.h formatPair) against BatchAligner::executePaired
// (containers, PairedReads on the host) + PairedFileWriter on the same mates.
// usage: pair_graph_test <case> <preset> <inversions 0|1> <sam options> <reads per batch> <batches in flight> <flat.sam> <container.sam> [shards]
// with <shards> > 0 the flat run goes through MultiDeviceAligner::executePairedFlat over that many replicas on device 0.
// Prints "batches <n> host_pairs <m>" of the flat run.
#include "../../oracle/dump_format.h"
#include "ma_batch_nodes.h"

#include <cstdio>

using namespace libMA;
using namespace libMS;

int main( int argc, char** argv )
{
    if( argc < 9 )
        return 2;
    try
    {
        CaseFile c = readCase( argv[ 1 ] );
        const int iOptions = atoi( argv[ 4 ] );
        const int iShards = argc >= 10 ? atoi( argv[ 9 ] ) : 0;
        ParameterSetManager xParams;
        xParams.setSelected( argv[ 2 ] );
        xParams.getSelected( )->search_inversions = atoi( argv[ 3 ] );
        xParams.xSam.bSoftClip = ( iOptions & 1 ) != 0;
        xParams.xSam.bOutputMCigar = ( iOptions & 2 ) == 0;
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
        auto pAll = std::make_shared<ContainerVector<std::shared_ptr<NucSeq>>>( );
        for( size_t i = 0; i < c.reads.size( ); i++ )
        {
            auto p = std::make_shared<NucSeq>( );
            p->xCodes = c.reads[ i ];
            p->sName = "r" + std::to_string( i );
            pAll->push_back( p );
        }
        if( pAll->size( ) % 2 )
            pAll->pop_back( );
        auto write = []( const char* sPath, const std::string& sText ) {
            FILE* f = fopen( sPath, "w" );
            fwrite( sText.data( ), 1, sText.size( ), f );
            fclose( f );
        };
        {
            auto pStream = std::make_shared<StringOutStream>( );
            BatchPairedFileWriter xWriter( xParams, std::static_pointer_cast<OutStream>( pStream ), pPack );
            std::shared_ptr<BatchAligner::TP_FLAT> pFlat;
            BatchAligner xAligner( xParams );
            std::unique_ptr<MultiDeviceAligner> pMulti;
            if( iShards > 0 )
            {
                pMulti.reset( new MultiDeviceAligner( xParams, MultiDeviceAligner::replicate( pFM, std::vector<int>( (size_t)iShards, 0 ) ) ) );
                pMulti->uiBatchReads = (size_t)atol( argv[ 5 ] ), pMulti->uiInflight = (size_t)atol( argv[ 6 ] );
                pFlat = pMulti->executePairedFlat( pAll );
            }
            else
            {
                xAligner.uiBatchReads = (size_t)atol( argv[ 5 ] ), xAligner.uiInflight = (size_t)atol( argv[ 6 ] );
                pFlat = xAligner.executePairedFlat( pFM, pAll );
            }
            uint64_t uiHost = 0, uiReads = 0;
            for( auto& pB : *pFlat )
            {
                if( pB->size( ) % 2 )
                    throw std::runtime_error( "a batch boundary splits a pair" );
                xWriter.execute( *pB );
                uiHost += pB->pResult->uiPairsOnHost, uiReads += pB->size( );
            }
            if( uiReads != pAll->size( ) )
                throw std::runtime_error( "the batches do not cover the reads" );
            printf( "batches %zu host_pairs %llu\n", pFlat->size( ), (unsigned long long)uiHost );
            write( argv[ 7 ], pStream->sText );
        }
        {
            auto pStream = std::make_shared<StringOutStream>( );
            BatchAligner xAligner( xParams );
            xAligner.uiBatchReads = (size_t)atol( argv[ 5 ] ), xAligner.uiInflight = (size_t)atol( argv[ 6 ] );
            auto pRes = xAligner.executePaired( pFM, pAll );
            PairedFileWriter xWriter( xParams, std::static_pointer_cast<OutStream>( pStream ), pPack );
            for( size_t k = 0; k < pRes->size( ); k++ )
                xWriter.execute( ( *pAll )[ 2 * k ], ( *pAll )[ 2 * k + 1 ], ( *pRes )[ k ], pPack );
            write( argv[ 8 ], pStream->sText );
        }
    }
    catch( const std::exception& e )
    {
        fprintf( stderr, "error: %s\n", e.what( ) );
        return 1;
    }
    return 0;
}
