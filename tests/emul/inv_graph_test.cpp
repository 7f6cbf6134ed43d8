// GPU checks of "Detect Small Inversions" in the host layer.
//   layer <case> <Z Drop Inversions> <sam options> <paired 0|1> <reads per batch> <out prefix>
//     the reads of the case under ("default", search_inversions) through the container path -- BatchAligner::execute +
//     FileWriter, or executePaired + PairedFileWriter (the host module SmallInversions, the yardstick) -> <out>.cont.sam --
//     and through the flat paths, which find the inversions on the device (ma_inversions_batch): executeFlat +
//     BatchFileWriter / executePairedFlat + BatchPairedFileWriter -> <out>.flat.sam, executeFlatSam / executePairedFlatSam
//     -> <out>.dev.sam, and the same two through MultiDeviceAligner over two replicas on device 0 -> <out>.multi.flat.sam,
//     <out>.multi.dev.sam.  The caller compares the files.
//   lists <case> <lists: R / FIN / f lines of an f4 dump> <Z Drop Inversions> <disable heuristics 0|1> <out>
//     SmallInversions::executeBatch of the host module on given MappingQuality lists; the lists it returns -> <out>, as the
//     'f' lines of an f4 dump.
#include "inv_common.h"
#include "ma_batch_nodes.h"

using namespace libMS;

static void buildFromCase( const CaseFile& c, std::shared_ptr<Pack>& pPack, std::shared_ptr<FMIndex>& pFM )
{
    std::vector<std::shared_ptr<NucSeq>> vContigs;
    for( size_t i = 0; i < c.contigs.size( ); i++ )
    {
        auto p = std::make_shared<NucSeq>( );
        p->xCodes = c.contigs[ i ];
        p->sName = c.names[ i ];
        vContigs.push_back( p );
    }
    buildIndex( vContigs, pPack, pFM );
}
static void writeFile( const std::string& sPath, const std::string& sText )
{
    FILE* f = fopen( sPath.c_str( ), "w" );
    if( !f || fwrite( sText.data( ), 1, sText.size( ), f ) != sText.size( ) || fclose( f ) != 0 )
        throw std::runtime_error( "cannot write " + sPath );
}

static int layer( char** argv )
{
    CaseFile c = readCase( argv[ 2 ] );
    const uint32_t uiBits = (uint32_t)atoi( argv[ 4 ] );
    const bool bPaired = atoi( argv[ 5 ] ) != 0;
    const size_t uiBatch = (size_t)atol( argv[ 6 ] );
    const std::string sOut = argv[ 7 ];
    ParameterSetManager xParams;
    xParams.setSelected( "default" );
    xParams.getSelected( )->search_inversions = 1;
    xParams.getSelected( )->zdrop_inversion = atoi( argv[ 3 ] );
    xParams.xSam = optionsOf( uiBits );
    std::shared_ptr<Pack> pPack;
    std::shared_ptr<FMIndex> pFM;
    buildFromCase( c, pPack, pFM );
    auto pAll = std::make_shared<ReadVector>( );
    for( size_t i = 0; i < c.reads.size( ); i++ )
    {
        auto p = std::make_shared<NucSeq>( );
        p->xCodes = c.reads[ i ];
        p->sName = "r" + std::to_string( i );
        pAll->push_back( p );
    }
    BatchAligner xAligner( xParams );
    xAligner.uiBatchReads = uiBatch, xAligner.uiInflight = 2;
    if( !xAligner.servesSam( ) || !xAligner.servesPairSam( ) )
        throw std::runtime_error( "servesSam( ) / servesPairSam( ) with 'Detect Small Inversions'" );
    MultiDeviceAligner xMulti( xParams, MultiDeviceAligner::replicate( pFM, std::vector<int>( 2, 0 ), 0 ) );
    xMulti.uiBatchReads = uiBatch, xMulti.uiInflight = 2;
    // the flat batches of a run through the flat writer; bText: every batch must have come back as device text
    auto flatText = [ & ]( BatchAligner::TP_FLAT& rFlat, bool bText ) {
        auto pStream = std::make_shared<StringOutStream>( );
        size_t uiAt = 0;
        auto each = [ & ]( auto& rWriter, auto write ) {
            for( const auto& pB : rFlat )
            {
                if( pB == nullptr || pB->uiFirst != uiAt || pB->hasSamText( ) != bText || pB->paired( ) != bPaired )
                    throw std::runtime_error( "the batches are not in input order, or not of the kind asked for" );
                write( rWriter, *pB );
                uiAt += pB->size( );
            }
        };
        if( bPaired )
        {
            BatchPairedFileWriter xWriter( xParams, std::static_pointer_cast<OutStream>( pStream ), pPack );
            each( xWriter, []( BatchPairedFileWriter& rW, const AlignedBatch& rB ) { rW.execute( rB ); } );
        }
        else
        {
            BatchFileWriter xWriter( xParams, std::make_shared<FileWriter>( xParams, std::static_pointer_cast<OutStream>( pStream ), pPack ), pPack );
            each( xWriter, [ & ]( BatchFileWriter& rW, const AlignedBatch& rB ) { rW.write( rB, pPack ); } );
        }
        if( uiAt != pAll->size( ) )
            throw std::runtime_error( "the batches do not cover the reads" );
        return pStream->sText;
    };
    if( bPaired )
    {
        {
            auto pStream = std::make_shared<StringOutStream>( );
            auto pRes = xAligner.executePaired( pFM, pAll );
            PairedFileWriter xWriter( xParams, std::static_pointer_cast<OutStream>( pStream ), pPack );
            for( size_t k = 0; k < pRes->size( ); k++ )
                xWriter.execute( ( *pAll )[ 2 * k ], ( *pAll )[ 2 * k + 1 ], ( *pRes )[ k ], pPack );
            xWriter.flush( );
            writeFile( sOut + ".cont.sam", pStream->sText );
        }
        writeFile( sOut + ".flat.sam", flatText( *xAligner.executePairedFlat( pFM, pAll ), false ) );
        writeFile( sOut + ".dev.sam", flatText( *xAligner.executePairedFlatSam( pFM, pAll, pPack ), true ) );
        writeFile( sOut + ".multi.flat.sam", flatText( *xMulti.executePairedFlat( pAll ), false ) );
        writeFile( sOut + ".multi.dev.sam", flatText( *xMulti.executePairedFlatSam( pAll, pPack ), true ) );
    }
    else
    {
        {
            auto pStream = std::make_shared<StringOutStream>( );
            auto pRes = xAligner.execute( pFM, pAll );
            FileWriter xWriter( xParams, std::static_pointer_cast<OutStream>( pStream ), pPack );
            for( size_t r = 0; r < pRes->size( ); r++ )
                xWriter.execute( ( *pAll )[ r ], ( *pRes )[ r ], pPack );
            xWriter.flush( );
            writeFile( sOut + ".cont.sam", pStream->sText );
        }
        writeFile( sOut + ".flat.sam", flatText( *xAligner.executeFlat( pFM, pAll ), false ) );
        writeFile( sOut + ".dev.sam", flatText( *xAligner.executeFlatSam( pFM, pAll, pPack ), true ) );
        writeFile( sOut + ".multi.flat.sam", flatText( *xMulti.executeFlat( pAll ), false ) );
        writeFile( sOut + ".multi.dev.sam", flatText( *xMulti.executeFlatSam( pAll, pPack ), true ) );
    }
    printf( "layer ok\n" );
    return 0;
}

static int lists( char** argv )
{
    CaseFile c = readCase( argv[ 2 ] );
    const Input in = fromF4Dump( argv[ 2 ], argv[ 3 ], false );
    ParameterSetManager xParams;
    xParams.setSelected( "default" );
    xParams.getSelected( )->zdrop_inversion = atoi( argv[ 4 ] );
    xParams.getSelected( )->disable_heuristics = atoi( argv[ 5 ] );
    std::shared_ptr<Pack> pPack;
    std::shared_ptr<FMIndex> pFM;
    buildFromCase( c, pPack, pFM );
    std::vector<std::shared_ptr<SmallInversions::TP_ALIGNMENTS>> vIn;
    std::vector<std::shared_ptr<NucSeq>> vQ;
    for( size_t r = 0; r < in.vReads.size( ); r++ )
    {
        auto pV = in.containers( r );
        for( size_t k = 0; k < pV->size( ); k++ )
            ( *pV )[ k ]->index_of_strip = in.vAlns[ in.vOff[ r ] + k ].soc_index;
        vIn.push_back( pV );
        vQ.push_back( in.vReads[ r ].container( ) );
    }
    auto vOut = SmallInversions( xParams ).executeBatch( vIn, vQ, pPack );
    std::string sText;
    char buf[ 256 ];
    for( size_t r = 0; r < vOut.size( ); r++ )
    {
        snprintf( buf, sizeof( buf ), "R %zu %zu\nFIN 0 %zu\n", r, in.vReads[ r ].vCodes.size( ), vOut[ r ]->size( ) );
        sText += buf;
        for( auto& pA : *vOut[ r ] )
        {
            snprintf( buf, sizeof( buf ), "f 0 -1 %llu %llu %llu %llu %lld %u %d %d %.17g %zu", (unsigned long long)pA->uiBeginOnRef,
                      (unsigned long long)pA->uiEndOnRef, (unsigned long long)pA->uiBeginOnQuery, (unsigned long long)pA->uiEndOnQuery,
                      (long long)pA->iScore, pA->index_of_strip, pA->bSecondary ? 1 : 0, pA->bSupplementary ? 1 : 0, pA->fMappingQuality, pA->data.size( ) );
            sText += buf;
            for( auto& rD : pA->data )
                sText += " " + std::to_string( (int)rD.first ) + ":" + std::to_string( rD.second );
            sText += "\n";
        }
    }
    writeFile( argv[ 6 ], sText );
    printf( "lists ok\n" );
    return 0;
}

int main( int argc, char** argv )
{
    try
    {
        if( argc == 8 && !strcmp( argv[ 1 ], "layer" ) )
            return layer( argv );
        if( argc == 7 && !strcmp( argv[ 1 ], "lists" ) )
            return lists( argv );
        fprintf( stderr, "usage: inv_graph_test layer <case> <zd> <sam options> <paired> <batch> <out prefix> | lists <case> <lists> <zd> <disable heuristics> <out>\n" );
        return 2;
    }
    catch( const std::exception& e )
    {
        fprintf( stderr, "error: %s\n", e.what( ) );
        return 1;
    }
}
