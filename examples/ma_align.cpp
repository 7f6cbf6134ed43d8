// examples/ma_align.cpp -- reads in, SAM out, on the GPU, with the drop-in host layer (ma_amd/host): what a user of
// `maCMD -x <genome> -i <reads> [-m <mates>] -o <out.sam> -p <preset>` needs from the hot path.  Not a re-implementation
// of cmdMa.cpp: no option parsing beyond the four arguments, no thread pool (the batches are the parallelism).
//
//   ma_align [--host-sam] [--ngmlr-tags] [--text-input] [--bgzf-output] [--genome-text] <genome.fa | index prefix> <reads.fa|fq[.gz]> <out.sam[.gz]|stdout> [preset] [mates.fa|fq[.gz]]
//
// Single-end input is printed on the device (BatchAligner::executeFlatSam: the SAM text is what comes down) whenever the
// options are ones the device serves -- with --ngmlr-tags ("Emulate NGMLR's tag output") and with "Detect Small Inversions"
// (found on the device, ma_inversions_batch) too; with --host-sam the records come down and FileWriter prints them.  Paired input likewise: mates are paired and their
// records printed on the device (BatchAligner::executePairedFlatSam), or the pair records come down and
// BatchPairedFileWriter formats them (the paired writers refuse the tag emulation).  The bytes are the same.
// With --text-input the input is not parsed on the host at all: BatchTextReader cuts the file into runs of whole records
// and the device parses them (BatchAligner::executeTextSam, ma_batch_set_reads_text); with a mates file BatchPairedTextReader cuts
// both files into runs of equally many records and the device parses, interleaves and reverse-complements them
// (BatchAligner::executePairedTextSam, ma_batch_set_mates_text).  A single-end reads file that bgzip wrote (BGZF, told by its first
// bytes) goes up compressed: BatchBgzfReader cuts it at member borders and the device inflates it in front of its parser
// (BatchAligner::executeBgzfSam, ma_batch_set_reads_bgzf); two BGZF files of a pair likewise (BatchPairedBgzfReader,
// BatchAligner::executePairedBgzfSam, ma_batch_set_mates_bgzf); one BGZF file beside one that is not, and plain gzip, are not served with the flag.  The device serves four-line FASTQ and plain FASTA only; any other file ends the program with the library's message, which names the line -- there is no silent fallback.
// With --bgzf-output, or an output name that ends in .gz, the output is BGZF (SamOptions::bBgzf; what bgzip writes: samtools, zcat
// and gzip read it): on the device paths every batch's text is deflated where it was printed (ma_sam_bgzf_batch) and only its
// members come down; the header, and with --host-sam every byte, goes through the host statement of the same rules
// (ma_bgzf::deflateHost).  The file inflates to the bytes of the run without the option.
// With --genome-text a FASTA genome is not walked on the host either: buildIndexFromFastaText (ma_genome.h) sends the file up in
// chunks, the device parses contigs, codes and holes (ma_genome_append_text) and fills the hole bases with the draws of srand( 1 ),
// the seed the program gives libc without the flag.  The output is the same bytes.  With an index prefix in place of a FASTA file
// the flag has no effect (the index files are loaded) and the program says so on stderr.
//
// build: g++ -std=c++17 -O2 [-DMA_WITH_ZLIB] -Iinclude -Ima_amd/host examples/ma_align.cpp -Lma_amd -lma_amd [-lz] -lpthread
#include "ma_batch_nodes.h"
#include "ma_genome.h"
#include <cstdio>

using namespace libMA;
typedef libMS::ContainerVector<std::shared_ptr<NucSeq>> ReadVec;

int main( int argc, char** argv )
{
    bool bHostSam = false, bNgmlrTags = false, bTextInput = false, bBgzfOutput = false, bGenomeText = false;
    for( int i = 1; i < argc; i++ )
        if( std::string( argv[ i ] ) == "--host-sam" || std::string( argv[ i ] ) == "--ngmlr-tags" || std::string( argv[ i ] ) == "--text-input" ||
            std::string( argv[ i ] ) == "--bgzf-output" || std::string( argv[ i ] ) == "--genome-text" )
        {
            ( std::string( argv[ i ] ) == "--host-sam"      ? bHostSam
              : std::string( argv[ i ] ) == "--ngmlr-tags"  ? bNgmlrTags
              : std::string( argv[ i ] ) == "--text-input"  ? bTextInput
              : std::string( argv[ i ] ) == "--genome-text" ? bGenomeText
                                                            : bBgzfOutput ) = true;
            for( int j = i; j + 1 < argc; j++ )
                argv[ j ] = argv[ j + 1 ];
            argc--, i--;
        }
    if( argc < 4 )
    {
        fprintf( stderr, "usage: ma_align [--host-sam] [--ngmlr-tags] [--text-input] [--bgzf-output] [--genome-text] <genome.fa | index prefix> <reads> <out.sam[.gz]|stdout> [preset] [mates]\n" );
        return 2;
    }
    try
    {
        ParameterSetManager xParams;
        xParams.setSelected( argc >= 5 ? argv[ 4 ] : ( argc >= 6 ? "illuminapaired" : "default" ) );
        xParams.xSam.bEmulateNgmlrTags = bNgmlrTags;
        const std::string sOutName = argv[ 3 ];
        xParams.xSam.bBgzf = bBgzfOutput || ( sOutName.size( ) >= 3 && sOutName.compare( sOutName.size( ) - 3, 3, ".gz" ) == 0 );
        const bool bPaired = argc >= 6;
        if( bTextInput && bHostSam )
            throw std::runtime_error( "--text-input serves input printed on the device (not with --host-sam: the host's writers need the reads)" );
        // a single-end reads file that starts with a BGZF member (what bgzip writes; told by its first 18 bytes, not by its name)
        // is inflated on the device; any other compressed file is not served with the flag
        // with a mates file both files must be BGZF for that
        const auto startsWithBgzf = []( const char* pPath ) {
            uint8_t aFirst[ ma_bgzf::MIN_PROBE_BYTES ];
            std::ifstream xProbe( pPath, std::ios::binary );
            xProbe.read( (char*)aFirst, sizeof( aFirst ) );
            ma_bgzf::Member xMember;
            const uint32_t uiReason = xProbe.gcount( ) == (std::streamsize)sizeof( aFirst ) ? ma_bgzf::header( aFirst, sizeof( aFirst ), 0, &xMember )
                                                                                             : (uint32_t)ma_bgzf::ERR_NOT_BGZF;
            return uiReason == ma_bgzf::OK || uiReason == ma_bgzf::ERR_TRUNCATED; // (truncated: the member goes on behind the 18 bytes)
        };
        const bool bBgzfReads = bTextInput && startsWithBgzf( argv[ 2 ] ), bBgzfMates = bTextInput && bPaired && startsWithBgzf( argv[ 5 ] );
        const bool bBgzf = bPaired ? bBgzfReads && bBgzfMates : bBgzfReads;
        if( bTextInput && bPaired && bBgzfReads != bBgzfMates )
            throw std::runtime_error( std::string( "--text-input: " ) + argv[ bBgzfReads ? 2 : 5 ] + " is compressed (BGZF) and " +
                                      argv[ bBgzfReads ? 5 : 2 ] +
                                      " is not; the device inflates a pair of read files only when bgzip wrote both (run without the flag)" );
        for( int iFile : { 2, 5 } )
        {
            const std::string sReads = iFile < argc ? argv[ iFile ] : "";
            if( bTextInput && !bBgzf && sReads.size( ) >= 3 && sReads.compare( sReads.size( ) - 3, 3, ".gz" ) == 0 )
                throw std::runtime_error( "--text-input: " + sReads +
                                          " is compressed; the device parses plain text, and inflates reads that bgzip wrote (BGZF; of a pair, "
                                          "both files), but no plain gzip (run without the flag)" );
        }
        std::shared_ptr<Pack> pPack;
        std::shared_ptr<FMIndex> pFM;
        const std::string sGenome = argv[ 1 ];
        if( std::ifstream( sGenome + ".bwt" ).good( ) )
        {
            if( bGenomeText )
                fprintf( stderr, "ma_align: --genome-text has no effect: %s is an index prefix, its files are loaded\n", sGenome.c_str( ) );
            loadIndex( sGenome, pPack, pFM ); // the reference's own index files (or storeIndex output)
        }
        else
        {
            srand( 1 );
            if( bGenomeText )
                buildIndexFromFastaText( sGenome, pPack, pFM, 1 ); // the FASTA text read on the device, the draws of srand( 1 )
            else
                buildIndexFromFasta( sGenome, pPack, pFM ); // suffix sort on the GPU
        }
        BatchAligner xAligner( xParams );
        FileReader xReader( xParams );
        std::shared_ptr<FileStream> pIn = bBgzf ? std::make_shared<StdFileStream>( argv[ 2 ] ) : fileStreamFromPath( argv[ 2 ] ); // (BGZF: its bytes as they are)
        const size_t uiBatch = 1000000; // reads per device batch
        if( bBgzf && bPaired )
        {
            // the compressed paired path: the members of both files go to the device, which inflates both chains in one launch,
            // parses, pairs and prints; what it leaves over of either text is the front of the reader's next batch
            BatchPairedFileWriter xWriter( xParams, std::make_shared<PairedFileWriter>( xParams, std::string( argv[ 3 ] ), pPack ), pPack );
            BatchPairedBgzfReader xBgzfReader( xParams );
            auto pStreams = std::make_shared<PairedFileStream>( pIn, std::make_shared<StdFileStream>( argv[ 5 ] ) );
            while( auto pMembers = xBgzfReader.execute( pStreams ) )
                xWriter.execute( *xAligner.executePairedBgzfSam( pFM, pMembers, pPack ) );
        }
        else if( bTextInput && bPaired )
        {
            // the paired text path: the bytes of both files go to the device, which parses, reverse-complements the mates as the
            // parameter set says (bRevCompPairedReadMates), aligns, pairs and prints; one write per batch
            BatchPairedFileWriter xWriter( xParams, std::make_shared<PairedFileWriter>( xParams, std::string( argv[ 3 ] ), pPack ), pPack );
            BatchPairedTextReader xTextReader( xParams );
            auto pStreams = std::make_shared<PairedFileStream>( pIn, fileStreamFromPath( argv[ 5 ] ) );
            while( auto pTexts = xTextReader.execute( pStreams ) )
                xWriter.execute( *xAligner.executePairedTextSam( pFM, pTexts, pPack ) );
        }
        else if( bBgzf )
        {
            // the compressed text path: the members go to the device, which inflates, parses, aligns and prints
            BatchFileWriter xWriter( xParams, std::make_shared<FileWriter>( xParams, std::string( argv[ 3 ] ), pPack ), pPack );
            BatchBgzfReader xBgzfReader( xParams );
            while( auto pMembers = xBgzfReader.execute( pIn ) )
                xWriter.write( *xAligner.executeBgzfSam( pFM, pMembers, pPack ), pPack );
        }
        else if( bTextInput )
        {
            // the text path: the bytes of the file go to the device, which parses, aligns and prints; one write per batch
            BatchFileWriter xWriter( xParams, std::make_shared<FileWriter>( xParams, std::string( argv[ 3 ] ), pPack ), pPack );
            BatchTextReader xTextReader( xParams );
            while( auto pText = xTextReader.execute( pIn ) )
                xWriter.write( *xAligner.executeTextSam( pFM, pText, pPack ), pPack );
        }
        else if( !bPaired && xAligner.servesSam( ) && !bHostSam )
        {
            // the device path: records formatted by ma_sam_batch, one write per device batch behind FileWriter's header
            BatchFileWriter xWriter( xParams, std::make_shared<FileWriter>( xParams, std::string( argv[ 3 ] ), pPack ), pPack );
            while( true )
            {
                auto pReads = std::make_shared<ReadVec>( );
                while( pReads->size( ) < uiBatch )
                {
                    auto pQ = xReader.execute( pIn );
                    if( pQ == nullptr )
                        break;
                    pReads->push_back( pQ );
                }
                if( pReads->empty( ) )
                    break;
                auto pFlat = xAligner.executeFlatSam( pFM, pReads, pPack );
                for( auto& pBatch : *pFlat )
                    xWriter.write( *pBatch, pPack );
            }
        }
        else if( !bPaired )
        {
            FileWriter xWriter( xParams, std::string( argv[ 3 ] ), pPack );
            while( true )
            {
                auto pReads = std::make_shared<ReadVec>( );
                while( pReads->size( ) < uiBatch )
                {
                    auto pQ = xReader.execute( pIn );
                    if( pQ == nullptr )
                        break;
                    pReads->push_back( pQ );
                }
                if( pReads->empty( ) )
                    break;
                auto pRes = xAligner.execute( pFM, pReads );
                for( size_t i = 0; i < pReads->size( ); i++ )
                    xWriter.execute( ( *pReads )[ i ], ( *pRes )[ i ], pPack );
            }
        }
        else
        {
            PairedFileReader xPairedReader( xParams );
            auto pStreams = std::make_shared<PairedFileStream>( pIn, fileStreamFromPath( argv[ 5 ] ) );
            // the flat paired path: mates paired on the device, and -- where the device serves the options -- printed there
            // (ma_pair_sam_batch), one write per device batch; else SAM text straight from the pair records (with "Detect Small
            // Inversions" executePairedFlat itself goes through containers); the bytes are PairedFileWriter's
            const bool bDeviceSam = xAligner.servesPairSam( ) && !bHostSam;
            BatchPairedFileWriter xWriter( xParams, std::make_shared<PairedFileWriter>( xParams, std::string( argv[ 3 ] ), pPack ), pPack );
            while( true )
            {
                auto pMates = std::make_shared<ReadVec>( );
                while( pMates->size( ) < uiBatch )
                {
                    auto pPair = xPairedReader.execute( pStreams );
                    if( pPair == nullptr )
                        break;
                    pMates->push_back( ( *pPair )[ 0 ] );
                    pMates->push_back( ( *pPair )[ 1 ] );
                }
                if( pMates->empty( ) )
                    break;
                auto pFlat = bDeviceSam ? xAligner.executePairedFlatSam( pFM, pMates, pPack ) : xAligner.executePairedFlat( pFM, pMates );
                for( auto& pBatch : *pFlat )
                    xWriter.execute( *pBatch );
            }
        }
    }
    catch( const std::runtime_error& e )
    {
        fprintf( stderr, "error: %s\n", e.what( ) );
        return 1;
    }
    return 0;
}
