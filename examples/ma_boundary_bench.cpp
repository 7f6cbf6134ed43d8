// examples/ma_boundary_bench.cpp -- host-fed end-to-end throughput through the drop-in boundary (what
// ExecutionContext::doAlign, libs/ma/inc/ma/util/execution-context.h:291-406, does with the reference's modules):
// reads in HOST memory -> H2D -> all stages on the GPU -> D2H -> Alignment containers -> SAM text.
// Three legs over the same synthetic 150 bp reads of the indexed genome:
//   batch_aligner   BatchAligner::execute, device batches of 256 k reads, 1 and 2 in flight; wall + the time of each phase
//   sam             FileWriter::execute for every read on T host threads into a counting sink
//   graph           the UNCHANGED per-read graph of setUpCompGraph (export.cpp:99-126), T graph threads over one shared
//                   reader, per-read execute() calls funnelled into device batches by the DeviceBatcher
// Prints one JSON line.  bench.py runs it after its timed regions and reports it as config.boundary (never as `value`).
//
//   ma_boundary_bench <index prefix> <reads> <read length> <preset> <device> [graph threads]
// (further legs, one per run: paired, pairtext, pairbgzf, sam, sam-tags, sam-bgzf, text, bgzf, inversions -- see the comments at their blocks in main)
//
// build: g++ -std=c++17 -O2 [-DMA_WITH_ZLIB] -Iinclude -Ima_amd/host examples/ma_boundary_bench.cpp -Lma_amd -lma_amd [-lz] -lpthread
#include "ma_batch_nodes.h"
#include "ma_genome.h"
#include <atomic>
#include <random>
#include <unistd.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

using namespace libMA;
using namespace libMS;
typedef ContainerVector<std::shared_ptr<NucSeq>> ReadVec;

static double now( )
{
    return std::chrono::duration<double>( std::chrono::steady_clock::now( ).time_since_epoch( ) ).count( );
}

struct CountingSink : public OutStream
{
    std::atomic<uint64_t> uiBytes{ 0 };
    void put( const char*, size_t n ) override
    {
        uiBytes += n;
    }
    void write( const char*, size_t n ) override
    {
        uiBytes += n;
    }
};

class VecReader : public Module<NucSeq, true>
{
  public:
    const ReadVec& r;
    std::atomic<size_t> i{ 0 };
    VecReader( const ReadVec& r ) : r( r )
    {}
    std::shared_ptr<NucSeq> execute( ) override
    {
        const size_t k = i++;
        return k < r.size( ) ? r[ k ] : nullptr;
    }
};

// volatile source that hands out a NEW NucSeq per call, as a file reader does (FileReader::execute, fileReader.cpp:37-203)
class FreshReader : public Module<NucSeq, true>
{
  public:
    const ReadVec& r;
    std::atomic<size_t> i{ 0 };
    FreshReader( const ReadVec& r ) : r( r )
    {}
    std::shared_ptr<NucSeq> execute( ) override
    {
        const size_t k = i++;
        return k < r.size( ) ? std::make_shared<NucSeq>( *r[ k ] ) : nullptr;
    }
};

// execute( ) of a module, timed (thread time summed over all graph threads): where the host side of the per-read graph goes
template <class TP_MODULE> struct Timed : public TP_MODULE
{
    std::atomic<uint64_t> uiNs{ 0 }, uiCalls{ 0 };
    template <typename... A> Timed( A&&... a ) : TP_MODULE( std::forward<A>( a )... )
    {}
    template <typename F> auto timed( F&& f ) -> decltype( f( ) )
    {
        const auto t0 = std::chrono::steady_clock::now( );
        auto r = f( );
        uiNs += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>( std::chrono::steady_clock::now( ) - t0 ).count( );
        uiCalls++;
        return r;
    }
    double usPerCall( ) const
    {
        return uiCalls ? uiNs / 1e3 / uiCalls : 0.0;
    }
};
struct TReader : public Timed<PrefetchReader<>>
{
    using Timed<PrefetchReader<>>::Timed;
    std::shared_ptr<NucSeq> execute( ) override
    {
        return timed( [ & ]( ) { return PrefetchReader<>::execute( ); } );
    }
};
struct TSeeding : public Timed<BinarySeeding>
{
    using Timed<BinarySeeding>::Timed;
    std::shared_ptr<SegmentVector> execute( std::shared_ptr<SuffixArrayInterface> a, std::shared_ptr<NucSeq> b ) override
    {
        return timed( [ & ]( ) { return BinarySeeding::execute( a, b ); } );
    }
};
struct TSoc : public Timed<StripOfConsideration>
{
    using Timed<StripOfConsideration>::Timed;
    std::shared_ptr<SoCPriorityQueue> execute( std::shared_ptr<SegmentVector> a, std::shared_ptr<NucSeq> b, std::shared_ptr<Pack> c,
                                               std::shared_ptr<FMIndex> d ) override
    {
        return timed( [ & ]( ) { return StripOfConsideration::execute( a, b, c, d ); } );
    }
};
struct THarm : public Timed<Harmonization>
{
    using Timed<Harmonization>::Timed;
    std::shared_ptr<SeedsSetVector> execute( std::shared_ptr<SoCPriorityQueue> a, std::shared_ptr<NucSeq> b, std::shared_ptr<FMIndex> c ) override
    {
        return timed( [ & ]( ) { return Harmonization::execute( a, b, c ); } );
    }
};
typedef libMS::ContainerVector<std::shared_ptr<Alignment>> AlnVec;
struct TDp : public Timed<NeedlemanWunsch>
{
    using Timed<NeedlemanWunsch>::Timed;
    std::shared_ptr<AlnVec> execute( std::shared_ptr<SeedsSetVector> a, std::shared_ptr<NucSeq> b, std::shared_ptr<Pack> c ) override
    {
        return timed( [ & ]( ) { return NeedlemanWunsch::execute( a, b, c ); } );
    }
};
struct TMq : public Timed<MappingQuality>
{
    using Timed<MappingQuality>::Timed;
    std::shared_ptr<AlnVec> execute( std::shared_ptr<NucSeq> a, std::shared_ptr<AlnVec> b ) override
    {
        return timed( [ & ]( ) { return MappingQuality::execute( a, b ); } );
    }
};
struct TWriter : public Timed<FileWriter>
{
    using Timed<FileWriter>::Timed;
    std::shared_ptr<libMS::Container> execute( std::shared_ptr<NucSeq> a, std::shared_ptr<AlnVec> b, std::shared_ptr<Pack> c ) override
    {
        return timed( [ & ]( ) { return FileWriter::execute( a, b, c ); } );
    }
};

// ---- leg 4: the per-read graph of export.cpp:99-126 with the reader node wrapped into a PrefetchReader: reads are pulled ahead
// a device batch at a time and every graph thread gets reads that are already aligned -- a few dozen graph threads
static std::string prefetchLeg( const ParameterSetManager& xParams, std::shared_ptr<ReadVec> pReads, std::shared_ptr<FMIndex> pFM,
                                std::shared_ptr<Pack> pPack, uint64_t uiExpectedSamBytes, double& fPrefetchBest, int& iPrefetchBestThreads )
{
    const size_t n = pReads->size( );
    auto now = []( ) { return std::chrono::duration<double>( std::chrono::steady_clock::now( ).time_since_epoch( ) ).count( ); };
    // Every graph copy gets its own handles of the shared constants (Pack, FMIndex): same objects, but behind a control block
    // of the copy's own.  A constant pledge hands out a shared_ptr copy per get( ) -- six per read -- and with ONE control block
    // for all threads those reference counts bounce a cache line between the cores (measured: ~15 us of thread time per read).
    auto own = []( auto p ) {
        typedef typename decltype( p )::element_type T;
        return std::shared_ptr<T>( p.get( ), [ p ]( T* ) {} );
    };
    double t0 = 0;
    std::string sPrefetch;
    for( int iT : { 8, 16, 32 } )
    {
        detail::PrefetchOptions xPO;
        xPO.uiBatchReads = 1u << 16;
        xPO.uiDepth = 2;
        // (MA_BOUNDARY_SHARED_READS=1: the source hands out the caller's own objects, which PrefetchReader then has to copy)
        std::shared_ptr<Module<NucSeq, true>> pSource;
        if( getenv( "MA_BOUNDARY_SHARED_READS" ) )
            pSource = std::make_shared<VecReader>( *pReads );
        else
            pSource = std::make_shared<FreshReader>( *pReads );
        if( getenv( "MA_PREFETCH_BATCH" ) )
            xPO.uiBatchReads = (size_t)atoi( getenv( "MA_PREFETCH_BATCH" ) );
        if( getenv( "MA_PREFETCH_DEPTH" ) )
            xPO.uiDepth = (size_t)atoi( getenv( "MA_PREFETCH_DEPTH" ) );
        auto pAhead = std::make_shared<TReader>( xParams, pSource, pFM, xPO );
        auto pSeeding4 = std::make_shared<TSeeding>( xParams );
        auto pSoc4 = std::make_shared<TSoc>( xParams );
        auto pHarm4 = std::make_shared<THarm>( xParams );
        auto pDp4 = std::make_shared<TDp>( xParams );
        auto pMq4 = std::make_shared<TMq>( xParams );
        auto pSink4 = std::make_shared<CountingSink>( );
        auto pWriter4 = std::make_shared<TWriter>( xParams, std::static_pointer_cast<OutStream>( pSink4 ), pPack );
        if( !getenv( "MA_BOUNDARY_WRITER_UNBUFFERED" ) )
            pWriter4->uiBufferBytes = 1u << 16; // per-thread buffers: the writer's lock once per 64 KB instead of once per read
        std::vector<std::shared_ptr<BasePledge>> vSinks4;
        for( int t = 0; t < iT; t++ )
        {
            auto pPackP = std::make_shared<Pledge<Pack>>( );
            pPackP->set( own( pPack ) );
            auto pFmP = std::make_shared<Pledge<FMIndex>>( );
            pFmP->set( own( pFM ) );
            auto pSai = std::make_shared<Pledge<SuffixArrayInterface>>( );
            pSai->set( own( std::static_pointer_cast<SuffixArrayInterface>( pFM ) ) );
            auto pQuery = promiseMe( std::make_shared<Lock<NucSeq>>( ), promiseMe( std::static_pointer_cast<PrefetchReader<>>( pAhead ) ) );
            auto pSeeds = promiseMe( std::static_pointer_cast<BinarySeeding>( pSeeding4 ), pSai, pQuery );
            auto pSOCs = promiseMe( std::static_pointer_cast<StripOfConsideration>( pSoc4 ), pSeeds, pQuery, pPackP, pFmP );
            auto pHarmonized = promiseMe( std::static_pointer_cast<Harmonization>( pHarm4 ), pSOCs, pQuery, pFmP );
            auto pAlignments = promiseMe( std::static_pointer_cast<NeedlemanWunsch>( pDp4 ), pHarmonized, pQuery, pPackP );
            auto pWithQuality = promiseMe( std::static_pointer_cast<MappingQuality>( pMq4 ), pQuery, pAlignments );
            auto pWritten = promiseMe( std::static_pointer_cast<FileWriter>( pWriter4 ), pQuery, pWithQuality, pPackP );
            vSinks4.push_back( promiseMe( std::make_shared<UnLock<Container>>( pQuery ), pWritten ) );
        }
        t0 = now( );
        BasePledge::simultaneousGet( vSinks4 );
        pWriter4->flush( );
        const double f4 = now( ) - t0;
        uint64_t uiB = 0, uiR = 0;
        double fRun4 = 0, fPull4 = 0;
        pAhead->stats( uiB, uiR, fRun4, fPull4 );
        if( pSeeding4->batcher( ) != nullptr )
            throw std::runtime_error( "prefetch leg: a read went through the per-read funnel" );
        char buf[ 640 ];
        snprintf( buf, sizeof( buf ), "%s\"graph_threads_%d\": {\"reads_per_s\": %.1f, \"wall_s\": %.4f, \"device_batches\": %llu, "
                                      "\"device_batch_s\": %.4f, \"pull_s\": %.4f, \"sam_bytes\": %llu, \"us_per_read\": {\"thread_time\": %.2f, "
                                      "\"reader\": %.2f, \"seeding\": %.2f, \"soc\": %.2f, \"harmonization\": %.2f, \"dp\": %.2f, \"mapping_quality\": %.2f, "
                                      "\"writer\": %.2f}}",
                  sPrefetch.empty( ) ? "" : ", ", iT, n / f4, f4, (unsigned long long)uiB, fRun4, fPull4, (unsigned long long)pSink4->uiBytes.load( ),
                  f4 * iT * 1e6 / n, pAhead->usPerCall( ), pSeeding4->usPerCall( ), pSoc4->usPerCall( ), pHarm4->usPerCall( ), pDp4->usPerCall( ),
                  pMq4->usPerCall( ), pWriter4->usPerCall( ) );
        sPrefetch += buf;
        if( uiExpectedSamBytes != 0 && pSink4->uiBytes.load( ) != uiExpectedSamBytes )
            throw std::runtime_error( "prefetch leg: SAM bytes differ from the funnel leg's" );
        if( n / f4 > fPrefetchBest )
            fPrefetchBest = n / f4, iPrefetchBestThreads = iT;
    }
    return sPrefetch;
}

#ifdef MA_WITH_ZLIB
// a text as BGZF through zlib at the default level, 65 280 bytes of text per member as bgzip cuts them, the end-of-file marker behind
static std::string bgzfOf( const std::string& sFastq )
{
    std::string sBgzf;
    for( size_t uiAt = 0; uiAt <= sFastq.size( ); uiAt += 65280 ) // (the last turn writes the rest or the end-of-file marker)
    {
        const size_t uiText = std::min<size_t>( 65280, sFastq.size( ) - uiAt );
        z_stream z;
        memset( &z, 0, sizeof( z ) );
        if( deflateInit2( &z, Z_DEFAULT_COMPRESSION, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY ) != Z_OK )
            throw std::runtime_error( "deflateInit2" );
        std::string sOut( deflateBound( &z, (uLong)uiText ) + 64, '\0' );
        z.next_in = (Bytef*)( sFastq.data( ) + uiAt ), z.avail_in = (uInt)uiText;
        z.next_out = (Bytef*)&sOut[ 0 ], z.avail_out = (uInt)sOut.size( );
        if( deflate( &z, Z_FINISH ) != Z_STREAM_END )
            throw std::runtime_error( "deflate" );
        sOut.resize( z.total_out );
        deflateEnd( &z );
        const uint32_t uiCrc = (uint32_t)crc32( crc32( 0L, Z_NULL, 0 ), (const Bytef*)( sFastq.data( ) + uiAt ), (uInt)uiText );
        auto le = [ & ]( uint32_t v, int nBytes ) {
            for( int i = 0; i < nBytes; i++ )
                sBgzf += (char)( ( v >> ( 8 * i ) ) & 0xff );
        };
        sBgzf += std::string( "\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0", 16 );
        le( (uint32_t)sOut.size( ) + 25, 2 );
        sBgzf += sOut;
        le( uiCrc, 4 ), le( (uint32_t)uiText, 4 );
        if( uiText == 0 )
            break;
    }
    return sBgzf;
}
#endif

// ma_boundary_bench genome <bases> [device] [repeats] [chunk MiB]: the wall time from a FASTA file to a usable index, host path
// (buildIndexFromFasta: FileReader + the base loop of buildIndex, then upload + suffix sort) against device text path
// (buildIndexFromFastaText: ma_genome_append_text per chunk, then fill + suffix sort) on one synthetic multi-contig genome with N
// runs, written from a seed to <TMPDIR or /tmp>/ma_boundary_bench.genome.<pid>.fa and removed afterwards.  The two steps of each
// path are timed apart; the repeats alternate between the paths.
static int genomeLeg( int argc, char** argv )
{
    const uint64_t uiBases = strtoull( argv[ 2 ], NULL, 10 );
    const int iDevice = argc >= 4 ? atoi( argv[ 3 ] ) : 0, iRepeats = argc >= 5 ? atoi( argv[ 4 ] ) : 3;
    const uint64_t uiChunk = ( argc >= 6 ? strtoull( argv[ 5 ], NULL, 10 ) : 256 ) << 20;
    maCheck( ma_set_device( iDevice ) );
    maCheck( ma_host_bind_thread( iDevice, 0, nullptr ) );
    const char* pTmp = getenv( "TMPDIR" );
    const std::string sPath = std::string( pTmp ? pTmp : "/tmp" ) + "/ma_boundary_bench.genome." + std::to_string( getpid( ) ) + ".fa";
    uint64_t uiFileBytes = 0, uiHoleBases = 0;
    {
        // 24 contigs of falling size, lines of 60, an N run of 10 - 50 000 every ~2 Mnt and at both ends of every contig
        std::mt19937_64 rng( 20261021 );
        FILE* f = fopen( sPath.c_str( ), "wb" );
        if( !f )
            throw std::runtime_error( "cannot write " + sPath );
        std::string sLine;
        const int nContigs = 24;
        uint64_t uiLeft = uiBases;
        for( int c = 0; c < nContigs && uiLeft; c++ )
        {
            const uint64_t uiLen = c + 1 == nContigs ? uiLeft : std::max<uint64_t>( 1, std::min<uint64_t>( uiLeft, uiBases / 12 * ( nContigs - c ) / nContigs ) );
            uiLeft -= uiLen;
            fprintf( f, ">chr%d synthetic contig of %llu bases\n", c + 1, (unsigned long long)uiLen );
            uint64_t uiHole = std::min<uint64_t>( uiLen / 4, 10000 ); // hole bases to go; the contig starts in a run
            uint64_t uiNext = rng( ) % 2000000;
            for( uint64_t at = 0; at < uiLen; at += 60 )
            {
                const size_t uiLine = (size_t)std::min<uint64_t>( 60, uiLen - at );
                sLine.resize( uiLine );
                uint64_t r = 0;
                for( size_t k = 0; k < uiLine; k++ )
                {
                    if( ( k & 31 ) == 0 )
                        r = rng( );
                    if( at + k + 10000 >= uiLen && uiLen > 40000 )
                        uiHole = std::max<uint64_t>( uiHole, 1 ); // ... and ends in one
                    if( uiHole == 0 && uiNext == 0 )
                        uiHole = 10 + rng( ) % 50000, uiNext = 1 + rng( ) % 4000000;
                    if( uiHole )
                        sLine[ k ] = 'N', uiHole--, uiHoleBases++;
                    else
                        sLine[ k ] = "ACGT"[ ( r >> ( 2 * ( k & 31 ) ) ) & 3 ], uiNext--;
                }
                fwrite( sLine.data( ), 1, uiLine, f );
                fputc( '\n', f );
            }
        }
        uiFileBytes = (uint64_t)ftell( f );
        fclose( f );
    }
    std::vector<double> vHostText, vHostSort, vDevText, vDevSort;
    size_t uiHoles = 0, uiContigs = 0;
    for( int r = 0; r < iRepeats; r++ )
    {
        {
            std::shared_ptr<Pack> pPack = std::make_shared<Pack>( );
            std::shared_ptr<FMIndex> pFM;
            srand( 1 );
            double t0 = now( );
            // the two halves of buildIndexFromFasta + buildIndex, timed apart
            ParameterSetManager xParameters;
            FileReader xReader( xParameters );
            auto pStream = fileStreamFromPath( sPath );
            std::vector<std::shared_ptr<NucSeq>> vContigs;
            while( auto pContig = xReader.execute( pStream ) )
                vContigs.push_back( pContig );
            std::vector<uint64_t> vLens;
            std::vector<uint8_t> vCat;
            packContigs( vContigs, pPack, vLens, vCat );
            vHostText.push_back( now( ) - t0 );
            t0 = now( );
            auto pDev = std::make_shared<DeviceIndex>( );
            maCheck( ma_index_build( (int32_t)vLens.size( ), vLens.data( ), vCat.data( ), &pDev->p ) );
            vHostSort.push_back( now( ) - t0 );
            uiHoles = pPack->vHoles.size( ), uiContigs = vLens.size( );
        }
        {
            std::shared_ptr<Pack> pPack;
            std::shared_ptr<FMIndex> pFM;
            double t0 = now( );
            auto pGenome = readFastaText( sPath, uiChunk );
            vDevText.push_back( now( ) - t0 );
            t0 = now( );
            buildIndexFromGenomeText( pGenome, pPack, pFM, 1 );
            vDevSort.push_back( now( ) - t0 );
            if( pPack->vHoles.size( ) != uiHoles || pPack->vNames.size( ) != uiContigs )
                throw std::runtime_error( "the two paths disagree on the contigs or holes" );
        }
    }
    remove( sPath.c_str( ) );
    auto list = []( const std::vector<double>& v ) {
        std::string s = "[";
        for( size_t i = 0; i < v.size( ); i++ )
            s += ( i ? ", " : "" ) + std::to_string( v[ i ] );
        return s + "]";
    };
    auto sums = []( std::vector<double> a, const std::vector<double>& b ) { // file to index, per repetition
        for( size_t i = 0; i < a.size( ); i++ )
            a[ i ] += b[ i ];
        return a;
    };
    auto median = []( std::vector<double> v ) {
        std::sort( v.begin( ), v.end( ) );
        return v[ v.size( ) / 2 ];
    };
    printf( "{\"leg\": \"genome\", \"bases\": %llu, \"file_bytes\": %llu, \"contigs\": %zu, \"holes\": %zu, \"hole_bases\": %llu, \"chunk_bytes\": %llu, "
            "\"host_text_s\": %s, \"host_upload_sort_s\": %s, \"device_text_s\": %s, \"device_fill_sort_s\": %s, "
            "\"host_text_bytes_per_s\": %.0f, \"device_text_bytes_per_s\": %.0f, \"host_total_median_s\": %.3f, \"device_total_median_s\": %.3f}\n",
            (unsigned long long)uiBases, (unsigned long long)uiFileBytes, uiContigs, uiHoles, (unsigned long long)uiHoleBases, (unsigned long long)uiChunk,
            list( vHostText ).c_str( ), list( vHostSort ).c_str( ), list( vDevText ).c_str( ), list( vDevSort ).c_str( ),
            (double)uiFileBytes / median( vHostText ), (double)uiFileBytes / median( vDevText ), median( sums( vHostText, vHostSort ) ),
            median( sums( vDevText, vDevSort ) ) );
    return 0;
}

int main( int argc, char** argv )
{
    if( argc >= 3 && !strcmp( argv[ 1 ], "genome" ) )
    {
        try
        {
            return genomeLeg( argc, argv );
        }
        catch( const std::exception& rE )
        {
            fprintf( stderr, "ma_boundary_bench genome: %s\n", rE.what( ) );
            return 1;
        }
    }
    if( argc < 6 )
    {
        fprintf( stderr, "usage: ma_boundary_bench <index prefix> <reads> <read length> <preset> <device> [graph threads | paired [repeats] | pairtext [repeats] | pairbgzf [repeats] | sam [repeats] | sam-tags [repeats] | sam-bgzf [repeats] | text [repeats] | bgzf [repeats] | inversions [repeats] [inverted reads per mille]]\n       ma_boundary_bench genome <bases> [device] [repeats] [chunk MiB]\n" );
        return 2;
    }
    try
    {
        const size_t n = (size_t)atoll( argv[ 2 ] ), uiLen = (size_t)atoll( argv[ 3 ] );
        ParameterSetManager xParams;
        xParams.setSelected( argv[ 4 ] );
        maCheck( ma_set_device( atoi( argv[ 5 ] ) ) );
        maCheck( ma_host_bind_thread( atoi( argv[ 5 ] ), 0, nullptr ) ); // this thread and all it starts: the CPUs next to the GPU
        const unsigned uiHw = std::max( 1u, std::thread::hardware_concurrency( ) );
        const int iGraphThreads = argc >= 7 && strcmp( argv[ 6 ], "paired" ) && strcmp( argv[ 6 ], "pairtext" ) && strcmp( argv[ 6 ], "pairbgzf" ) && strcmp( argv[ 6 ], "sam" ) && strcmp( argv[ 6 ], "sam-tags" ) && strcmp( argv[ 6 ], "sam-bgzf" ) && strcmp( argv[ 6 ], "text" ) && strcmp( argv[ 6 ], "bgzf" ) && strcmp( argv[ 6 ], "inversions" ) ? atoi( argv[ 6 ] ) : (int)std::min( 2048u, 8 * uiHw );
        std::shared_ptr<Pack> pPack;
        std::shared_ptr<FMIndex> pFM;
        double t0 = now( );
        loadIndex( argv[ 1 ], pPack, pFM );
        const double fLoad = now( ) - t0;
        // ---- reads: sampled on the host from the packed forward strand, 0.5 % substitutions, every second one reverse
        uint64_t uiN = 0;
        maCheck( ma_index_sizes( pFM->pDev->p, nullptr, nullptr, &uiN, nullptr ) );
        const uint64_t uiF = uiN / 2;
        std::vector<uint8_t> vPac( ( uiF + 3 ) / 4 + 1 );
        maCheck( ma_index_download( pFM->pDev->p, nullptr, nullptr, nullptr, nullptr, vPac.data( ), nullptr, nullptr ) );
        auto pReads = std::make_shared<ReadVec>( );
        uint64_t uiState = 0x9E3779B97F4A7C15ull;
        auto rnd = [ & ]( ) {
            uiState ^= uiState << 13, uiState ^= uiState >> 7, uiState ^= uiState << 17;
            return uiState;
        };
        // the synthetic mates of the paired legs: n / 2 pairs, outer distance 340 .. 460, every second pair seen from the other strand
        auto makeMates = [ & ]( ) {
            auto pMates = std::make_shared<ReadVec>( );
            auto window = [ & ]( uint64_t uiPos, bool bRev, size_t uiName ) {
                auto pQ = std::make_shared<NucSeq>( );
                pQ->sName = "r" + std::to_string( uiName );
                pQ->xCodes.resize( uiLen );
                for( size_t j = 0; j < uiLen; j++ )
                {
                    const uint64_t p = uiPos + j;
                    uint8_t b = ( vPac[ p >> 2 ] >> ( ( ~p & 3 ) << 1 ) ) & 3;
                    if( rnd( ) % 200 == 0 )
                        b = ( b + 1 + rnd( ) % 3 ) & 3;
                    pQ->xCodes[ j ] = b;
                }
                if( bRev )
                {
                    std::reverse( pQ->xCodes.begin( ), pQ->xCodes.end( ) );
                    for( auto& b : pQ->xCodes )
                        b = 3 - b;
                }
                return pQ;
            };
            for( size_t k = 0; 2 * k + 1 < n; k++ )
            {
                const uint64_t uiDist = std::max<uint64_t>( uiLen + 1, 340 + rnd( ) % 121 );
                const uint64_t uiPos = rnd( ) % ( uiF - uiDist - 1 );
                if( k & 1 )
                {
                    pMates->push_back( window( uiPos + uiDist - uiLen, true, 2 * k ) );
                    pMates->push_back( window( uiPos, false, 2 * k + 1 ) );
                }
                else
                {
                    pMates->push_back( window( uiPos, false, 2 * k ) );
                    pMates->push_back( window( uiPos + uiDist - uiLen, true, 2 * k + 1 ) );
                }
            }
            return pMates;
        };
        const bool bPairBgzfLeg = argc >= 7 && !strcmp( argv[ 6 ], "pairbgzf" );
        if( argc >= 7 && ( !strcmp( argv[ 6 ], "pairtext" ) || bPairBgzfLeg ) )
        {
            // (pairbgzf: the same two texts written once as BGZF; see below, behind the lambdas both legs use)
            // ---- the paired text leg: the mates of the paired leg as TWO FASTQ texts in memory, as a sequencer writes them (R2 on
            // the other strand; seeded qualities 35 .. 126), files to SAM text through (a) BatchPairedTextReader ->
            // executePairedTextSam -- blocks of both texts cut into equally many records, parsed, interleaved and reverse-complemented
            // on the device -- and (b) PairedFileReader -> executePairedFlatSam -- one NucSeq per mate, the host's reverse
            // complement, gathered and uploaded as arrays; what examples/ma_align runs with and without --text-input.  (a) with
            // three workers (own aligner each, one device batch of ~256 k mates at a time) that pull their batches from the one pair
            // stream, (b) on an aligner of its own with executePairedFlatSam's three batches in flight.  One warm-up of each keeps its text -- (a)'s
            // batches put into input order by their first QNAME -- and the two files must be the same bytes; then alternating,
            // <repeats> times each, with the texts only counted and every count checked against the file's.
            const int iRepeats = argc >= 8 ? std::max( 1, atoi( argv[ 7 ] ) ) : 5;
            auto pMates = makeMates( );
            std::vector<uint8_t>( ).swap( vPac );
            const size_t uiMates = pMates->size( ), uiWorkers = 3, uiBatchReads = std::min<size_t>( std::max<size_t>( uiMates, 2 ), 1u << 18 );
            std::string asFastq[ 2 ];
            for( size_t i = 0; i < uiMates; i++ )
            {
                std::string& rText = asFastq[ i & 1 ];
                const NucSeq& rQ = *( *pMates )[ i ];
                rText += "@" + rQ.sName + "\n";
                if( i & 1 ) // the file holds the other strand: PairedFileReader and the device turn it back
                    for( size_t j = rQ.xCodes.size( ); j > 0; j-- )
                        rText += "TGCA"[ rQ.xCodes[ j - 1 ] ];
                else
                    for( uint8_t b : rQ.xCodes )
                        rText += "ACGT"[ b ];
                rText += "\n+\n";
                for( size_t j = 0; j < rQ.xCodes.size( ); j++ )
                    rText += (char)( 35 + rnd( ) % 92 );
                rText += "\n";
            }
            pMates->clear( );
            xParams.bRevCompPairedReadMates = true;
            BatchAligner::nameContigs( *pFM->pDev, *pPack );
            std::vector<std::unique_ptr<BatchAligner>> vAligners;
            for( size_t w = 0; w <= uiWorkers; w++ ) // (the last one runs leg (b): engines of its own, so each warm-up warms its leg's)
            {
                vAligners.emplace_back( new BatchAligner( xParams ) );
                vAligners.back( )->uiBatchReads = uiBatchReads;
                vAligners.back( )->uiInflight = w == uiWorkers ? 3 : 1;
            }
            uint64_t uiBytesHost = 0, uiBytesText = 0;
            std::string asGzPath[ 2 ]; // pairbgzf: (b) reads the two .gz files through GzFileStream
            auto host = [ & ]( std::string* pFile ) {
                auto pStreams = asGzPath[ 0 ].empty( )
                                    ? std::make_shared<PairedFileStream>( std::make_shared<StringStream>( asFastq[ 0 ] ), std::make_shared<StringStream>( asFastq[ 1 ] ) )
                                    : std::make_shared<PairedFileStream>( fileStreamFromPath( asGzPath[ 0 ] ), fileStreamFromPath( asGzPath[ 1 ] ) );
                PairedFileReader xReader( xParams );
                const double t = now( );
                uiBytesHost = 0;
                if( pFile != nullptr )
                    pFile->clear( );
                while( true )
                {
                    auto pBatch = std::make_shared<ReadVec>( );
                    while( pBatch->size( ) < 1000000 ) // (ma_align's batch)
                    {
                        auto pPair = xReader.execute( pStreams );
                        if( pPair == nullptr )
                            break;
                        pBatch->push_back( ( *pPair )[ 0 ] );
                        pBatch->push_back( ( *pPair )[ 1 ] );
                    }
                    if( pBatch->empty( ) )
                        break;
                    std::vector<AlignerTiming> vPer;
                    auto pFlat = vAligners[ uiWorkers ]->executePairedFlatSamOn( pFM->pDev->all( ), pBatch, &vPer );
                    for( auto& pB : *pFlat )
                    {
                        uiBytesHost += pB->samBytes( );
                        if( pFile != nullptr )
                            pFile->append( pB->samText( ), pB->samBytes( ) );
                    }
                }
                return now( ) - t;
            };
            auto text = [ & ]( std::string* pFile ) {
                auto pStreams = std::make_shared<PairedFileStream>( std::make_shared<StringStream>( asFastq[ 0 ] ), std::make_shared<StringStream>( asFastq[ 1 ] ) );
                BatchPairedTextReader xReader( xParams );
                xReader.uiBatchBytes = std::max<size_t>( 2, ( asFastq[ 0 ].size( ) + asFastq[ 1 ].size( ) ) / std::max<size_t>( uiMates, 1 ) * uiBatchReads );
                std::vector<std::pair<uint64_t, std::string>> vParts;
                std::mutex xParts;
                std::string sFailure;
                std::atomic<uint64_t> uiBytes{ 0 };
                const double t = now( );
                std::vector<std::thread> vT;
                for( size_t w = 0; w < uiWorkers; w++ )
                    vT.emplace_back( [ &, w ]( ) {
                        try
                        {
                            while( auto pTexts = xReader.execute( pStreams ) )
                            {
                                auto pB = vAligners[ w ]->executePairedTextSamOn( pFM->pDev->p, pTexts );
                                uiBytes += pB->samBytes( );
                                if( pFile != nullptr )
                                {
                                    const uint64_t uiFirst = pB->samBytes( ) > 1 ? strtoull( pB->samText( ) + 1, nullptr, 10 ) : 0; // "r<i>\t..."
                                    std::lock_guard<std::mutex> xGuard( xParts );
                                    vParts.emplace_back( uiFirst, std::string( pB->samText( ), pB->samBytes( ) ) );
                                }
                            }
                        }
                        catch( const std::exception& rE )
                        {
                            std::lock_guard<std::mutex> xGuard( xParts );
                            sFailure = rE.what( );
                        }
                    } );
                for( auto& rT : vT )
                    rT.join( );
                const double f = now( ) - t;
                if( !sFailure.empty( ) )
                    throw std::runtime_error( sFailure );
                uiBytesText = uiBytes.load( );
                if( pFile != nullptr )
                {
                    std::sort( vParts.begin( ), vParts.end( ), []( const auto& a, const auto& b ) { return a.first < b.first; } );
                    pFile->clear( );
                    for( const auto& rPart : vParts )
                        *pFile += rPart.second;
                }
                return f;
            };
            auto list = []( std::vector<double> v ) {
                std::string sAll;
                for( double f : v )
                    sAll += ( sAll.empty( ) ? "" : ", " ) + std::to_string( f );
                std::sort( v.begin( ), v.end( ) );
                return "{\"median\": " + std::to_string( v[ v.size( ) / 2 ] ) + ", \"min\": " + std::to_string( v.front( ) ) +
                       ", \"max\": " + std::to_string( v.back( ) ) + ", \"all\": [" + sAll + "]}";
            };
            if( bPairBgzfLeg )
            {
                // ---- the compressed paired leg: the two texts written once as BGZF (the bgzf leg's setup), files to SAM text through
                // (a) BatchPairedBgzfReader -> executePairedBgzfSam -- both chains inflated by one launch, the rests handed back to
                // the reader, so the set calls of consecutive batches are serial and everything behind them overlaps across the
                // three workers --, (b) the two .gz files through GzFileStream -> PairedFileReader -> executePairedFlatSam -- what a
                // compressed pair gets without it: gzread a byte at a time, one NucSeq per mate -- and (c) the pairtext leg's (a)
                // on the uncompressed texts, the ceiling.  A warm-up of each keeps its text; the three must be the same bytes.  Then
                // alternating, <repeats> times each; then (a) at other uiBatchBytes.  (Needs -DMA_WITH_ZLIB -lz.)
#ifdef MA_WITH_ZLIB
                const std::string asBgzf[ 2 ] = { bgzfOf( asFastq[ 0 ] ), bgzfOf( asFastq[ 1 ] ) };
                for( int i = 0; i < 2; i++ )
                {
                    asGzPath[ i ] = std::string( argv[ 1 ] ) + ".boundary_bench_" + std::to_string( i + 1 ) + ".fq.gz";
                    std::ofstream xOut( asGzPath[ i ], std::ios::binary );
                    xOut.write( asBgzf[ i ].data( ), (std::streamsize)asBgzf[ i ].size( ) );
                    if( !xOut )
                        throw std::runtime_error( "cannot write " + asGzPath[ i ] );
                }
                uint64_t uiBytesBgzf = 0;
                const size_t uiTextPerBatch = std::max<size_t>( 2, ( asFastq[ 0 ].size( ) + asFastq[ 1 ].size( ) ) / std::max<size_t>( uiMates, 1 ) * uiBatchReads );
                auto bgzf = [ & ]( std::string* pFile, size_t uiBatchBytes ) {
                    auto pStreams = std::make_shared<PairedFileStream>( std::make_shared<StringStream>( asBgzf[ 0 ] ), std::make_shared<StringStream>( asBgzf[ 1 ] ) );
                    BatchPairedBgzfReader xReader( xParams );
                    xReader.uiBatchBytes = uiBatchBytes;
                    std::vector<std::pair<uint64_t, std::string>> vParts;
                    std::mutex xParts;
                    std::string sFailure;
                    std::atomic<uint64_t> uiBytes{ 0 };
                    const double t = now( );
                    std::vector<std::thread> vT;
                    for( size_t w = 0; w < uiWorkers; w++ )
                        vT.emplace_back( [ &, w ]( ) {
                            try
                            {
                                while( auto pMembers = xReader.execute( pStreams ) )
                                {
                                    auto pB = vAligners[ w ]->executePairedBgzfSamOn( pFM->pDev->p, pMembers );
                                    uiBytes += pB->samBytes( );
                                    if( pFile != nullptr )
                                    {
                                        const uint64_t uiFirst = pB->samBytes( ) > 1 ? strtoull( pB->samText( ) + 1, nullptr, 10 ) : 0; // "r<i>\t..."
                                        std::lock_guard<std::mutex> xGuard( xParts );
                                        vParts.emplace_back( uiFirst, std::string( pB->samText( ), pB->samBytes( ) ) );
                                    }
                                }
                            }
                            catch( const std::exception& rE )
                            {
                                std::lock_guard<std::mutex> xGuard( xParts );
                                sFailure = rE.what( );
                            }
                        } );
                    for( auto& rT : vT )
                        rT.join( );
                    const double f = now( ) - t;
                    if( !sFailure.empty( ) )
                        throw std::runtime_error( sFailure );
                    uiBytesBgzf = uiBytes.load( );
                    if( pFile != nullptr )
                    {
                        std::sort( vParts.begin( ), vParts.end( ), []( const auto& a, const auto& b ) { return a.first < b.first; } );
                        pFile->clear( );
                        for( const auto& rPart : vParts )
                            *pFile += rPart.second;
                    }
                    return f;
                };
                std::string sFileBgzf, sFileGz, sFileText;
                bgzf( &sFileBgzf, uiTextPerBatch ), host( &sFileGz ), text( &sFileText );
                bool bEqual = sFileBgzf == sFileGz && sFileBgzf == sFileText && !sFileBgzf.empty( );
                const uint64_t uiFileBytes = sFileText.size( );
                std::string( ).swap( sFileBgzf ), std::string( ).swap( sFileGz ), std::string( ).swap( sFileText );
                std::vector<double> vA, vB, vC;
                for( int r = 0; r < iRepeats; r++ )
                {
                    vA.push_back( uiMates / bgzf( nullptr, uiTextPerBatch ) ), vB.push_back( uiMates / host( nullptr ) ), vC.push_back( uiMates / text( nullptr ) );
                    bEqual = bEqual && uiBytesBgzf == uiFileBytes && uiBytesHost == uiFileBytes && uiBytesText == uiFileBytes;
                }
                // (a) at other sizes of the reader's batch: the set calls are serial, so a larger batch makes that section cheaper per read
                std::string sSweep;
                for( size_t uiDiv : { 8, 2, 1 } )
                {
                    std::vector<double> v;
                    for( int r = 0; r < 3; r++ )
                        v.push_back( uiMates / bgzf( nullptr, std::max<size_t>( 2, 2 * uiTextPerBatch / uiDiv ) ) );
                    bEqual = bEqual && uiBytesBgzf == uiFileBytes;
                    sSweep += ( sSweep.empty( ) ? "" : ", " ) + std::string( "{\"batch_bytes\": " ) + std::to_string( 2 * uiTextPerBatch / uiDiv ) +
                              ", \"reads_per_s\": " + list( v ) + "}";
                }
                const bool bFaster = *std::min_element( vA.begin( ), vA.end( ) ) > *std::max_element( vB.begin( ), vB.end( ) );
                printf( "{\"pairbgzf\": {\"mates\": %zu, \"read_len\": %zu, \"repeats\": %d, \"batch_bytes\": %zu, \"workers\": %zu, "
                        "\"paired_bgzf_reader_paired_bgzf_sam_reads_per_s\": %s, \"gz_paired_file_reader_paired_flat_sam_reads_per_s\": %s, "
                        "\"paired_text_reader_paired_text_sam_reads_per_s\": %s, \"other_batch_bytes\": [%s], \"fastq_bytes\": %zu, \"bgzf_bytes\": %zu, "
                        "\"sam_bytes\": %zu, \"equal\": %s, \"slowest_device_above_fastest_gz\": %s}}\n",
                        uiMates, uiLen, iRepeats, uiTextPerBatch, uiWorkers, list( vA ).c_str( ), list( vB ).c_str( ), list( vC ).c_str( ), sSweep.c_str( ),
                        asFastq[ 0 ].size( ) + asFastq[ 1 ].size( ), asBgzf[ 0 ].size( ) + asBgzf[ 1 ].size( ), (size_t)uiFileBytes, bEqual ? "true" : "false",
                        bFaster ? "true" : "false" );
                remove( asGzPath[ 0 ].c_str( ) ), remove( asGzPath[ 1 ].c_str( ) );
                return bEqual && bFaster ? 0 : 1;
#else
                throw std::runtime_error( "the pairbgzf leg writes its files through zlib: build with -DMA_WITH_ZLIB -lz" );
#endif
            }
            // warm-up of both: these two runs keep their files, which must be the same bytes; the timed runs count theirs
            std::string sFileHost, sFileText;
            host( &sFileHost ), text( &sFileText );
            bool bEqual = sFileHost == sFileText && !sFileHost.empty( );
            const uint64_t uiFileBytes = sFileText.size( );
            std::string( ).swap( sFileHost ), std::string( ).swap( sFileText );
            std::vector<double> vH, vD;
            for( int r = 0; r < iRepeats; r++ )
            {
                vD.push_back( uiMates / text( nullptr ) ), vH.push_back( uiMates / host( nullptr ) );
                bEqual = bEqual && uiBytesHost == uiFileBytes && uiBytesText == uiFileBytes;
            }
            printf( "{\"pairtext\": {\"mates\": %zu, \"read_len\": %zu, \"repeats\": %d, \"batch_reads\": %zu, \"workers\": %zu, "
                    "\"paired_text_reader_paired_text_sam_reads_per_s\": %s, \"paired_file_reader_paired_flat_sam_reads_per_s\": %s, "
                    "\"fastq_bytes\": %zu, \"sam_bytes\": %zu, \"equal\": %s}}\n",
                    uiMates, uiLen, iRepeats, uiBatchReads, uiWorkers, list( vD ).c_str( ), list( vH ).c_str( ), asFastq[ 0 ].size( ) + asFastq[ 1 ].size( ),
                    (size_t)uiFileBytes, bEqual ? "true" : "false" );
            return bEqual ? 0 : 1;
        }
        if( argc >= 7 && !strcmp( argv[ 6 ], "paired" ) )
        {
            // ---- the paired leg: n mates (n / 2 pairs, outer distance 340 .. 460, every second pair seen from the other strand)
            // host to host INCLUDING SAM text through (a) BatchAligner::executePaired + PairedFileWriter -- Alignment
            // containers, PairedReads on one host thread -- and (b) executePairedFlat + BatchPairedFileWriter -- paired on the
            // device, text from the flat pair records -- and (c) executePairedFlatSam + BatchPairedFileWriter -- paired AND
            // printed on the device, the text is what comes down; alternating, <repeats> times each after one warm-up of each
            const int iRepeats = argc >= 8 ? std::max( 1, atoi( argv[ 7 ] ) ) : 5;
            auto pMates = makeMates( );
            std::vector<uint8_t>( ).swap( vPac );
            BatchAligner xAligner( xParams );
            xAligner.uiBatchReads = std::min<size_t>( pMates->size( ), 1u << 18 );
            xAligner.uiInflight = 3;
            xAligner.warmUp( pFM, pMates );
            uint64_t uiBytesContainer = 0, uiBytesFlat = 0, uiHostPairs = 0;
            auto container = [ & ]( ) {
                auto pSink = std::make_shared<CountingSink>( );
                PairedFileWriter xWriter( xParams, std::static_pointer_cast<OutStream>( pSink ), pPack );
                const double t = now( );
                auto pPairs = xAligner.executePaired( pFM, pMates );
                for( size_t k = 0; k < pPairs->size( ); k++ )
                    xWriter.execute( ( *pMates )[ 2 * k ], ( *pMates )[ 2 * k + 1 ], ( *pPairs )[ k ], pPack );
                const double f = now( ) - t;
                uiBytesContainer = pSink->uiBytes.load( );
                return f;
            };
            auto flat = [ & ]( ) {
                auto pSink = std::make_shared<CountingSink>( );
                BatchPairedFileWriter xWriter( xParams, std::static_pointer_cast<OutStream>( pSink ), pPack );
                xWriter.uiFormatThreads = std::min( 16u, uiHw );
                const double t = now( );
                uiHostPairs = 0;
                auto pFlat = xAligner.executePairedFlat( pFM, pMates );
                for( auto& pB : *pFlat )
                {
                    xWriter.execute( *pB );
                    uiHostPairs += pB->pResult->uiPairsOnHost;
                }
                const double f = now( ) - t;
                uiBytesFlat = pSink->uiBytes.load( );
                return f;
            };
            uint64_t uiBytesDevice = 0, uiTextBatches = 0;
            auto device = [ & ]( ) {
                auto pSink = std::make_shared<CountingSink>( );
                BatchPairedFileWriter xWriter( xParams, std::static_pointer_cast<OutStream>( pSink ), pPack );
                const double t = now( );
                uiTextBatches = 0;
                auto pFlat = xAligner.executePairedFlatSam( pFM, pMates, pPack );
                for( auto& pB : *pFlat )
                {
                    xWriter.execute( *pB );
                    uiTextBatches += pB->hasSamText( );
                }
                const double f = now( ) - t;
                uiBytesDevice = pSink->uiBytes.load( );
                return f;
            };
            container( ), flat( ), device( ); // warm-up of all three
            std::vector<double> vC, vF, vD;
            for( int r = 0; r < iRepeats; r++ )
                vC.push_back( pMates->size( ) / container( ) ), vF.push_back( pMates->size( ) / flat( ) ), vD.push_back( pMates->size( ) / device( ) );
            auto list = []( std::vector<double> v ) {
                std::sort( v.begin( ), v.end( ) );
                std::string s = "{\"median\": " + std::to_string( v[ v.size( ) / 2 ] ) + ", \"min\": " + std::to_string( v.front( ) ) +
                                ", \"max\": " + std::to_string( v.back( ) ) + "}";
                return s;
            };
            printf( "{\"paired_device_sam\": {\"mates\": %zu, \"repeats\": %d, \"execute_paired_flat_sam_reads_per_s\": %s, \"sam_bytes_device\": %llu, "
                    "\"text_batches\": %llu}}\n",
                    pMates->size( ), iRepeats, list( vD ).c_str( ), (unsigned long long)uiBytesDevice, (unsigned long long)uiTextBatches );
            printf( "{\"paired\": {\"mates\": %zu, \"read_len\": %zu, \"repeats\": %d, \"batch_reads\": %zu, \"in_flight\": 3, "
                    "\"execute_paired_reads_per_s\": %s, \"execute_paired_flat_reads_per_s\": %s, \"sam_bytes_container\": %llu, "
                    "\"sam_bytes_flat\": %llu, \"pairs_finished_on_host\": %llu}}\n",
                    pMates->size( ), uiLen, iRepeats, xAligner.uiBatchReads, list( vC ).c_str( ), list( vF ).c_str( ),
                    (unsigned long long)uiBytesContainer, (unsigned long long)uiBytesFlat, (unsigned long long)uiHostPairs );
            return uiBytesContainer == uiBytesFlat && uiBytesFlat == uiBytesDevice ? 0 : 1;
        }
        for( size_t i = 0; i < n; i++ )
        {
            auto pQ = std::make_shared<NucSeq>( );
            pQ->sName = "r" + std::to_string( i );
            pQ->xCodes.resize( uiLen );
            const uint64_t uiPos = rnd( ) % ( uiF - uiLen );
            for( size_t j = 0; j < uiLen; j++ )
            {
                const uint64_t p = uiPos + j;
                uint8_t b = ( vPac[ p >> 2 ] >> ( ( ~p & 3 ) << 1 ) ) & 3;
                if( rnd( ) % 200 == 0 )
                    b = ( b + 1 + rnd( ) % 3 ) & 3;
                pQ->xCodes[ j ] = b;
            }
            if( i & 1 )
            {
                std::reverse( pQ->xCodes.begin( ), pQ->xCodes.end( ) );
                for( auto& b : pQ->xCodes )
                    b = 3 - b;
            }
            pReads->push_back( pQ );
        }
        const bool bSamTags = argc >= 7 && !strcmp( argv[ 6 ], "sam-tags" );
        if( bSamTags ) // "Emulate NGMLR's tag output": the host writer reads the reference's bases from a host copy of the pack
        {
            xParams.xSam.bEmulateNgmlrTags = true;
            pPack->vPacHost.assign( vPac.begin( ), vPac.end( ) );
        }
        std::vector<uint8_t>( ).swap( vPac );
        if( argc >= 7 && !strcmp( argv[ 6 ], "inversions" ) )
        {
            // ---- the inversions leg: n single-end reads, <share> per mille of them with their middle third (40 .. 300 bases)
            // reverse-complemented in place, host to host INCLUDING SAM text with "Detect Small Inversions" through (a)
            // BatchAligner::execute + FileWriter -- Alignment containers, the host module SmallInversions -- and (b) executeFlatSam
            // -- ma_inversions_batch and ma_sam_batch on the device, the text is what comes down -- and (c) executeFlatSam with
            // the option OFF: against (b) at share 0 the price of the stage when it finds nothing.  (a) <repeats> times after one
            // warm-up, then (c) and (b) alternating, 2 x <repeats> times each after one warm-up of each.
            const int iRepeats = argc >= 8 ? std::max( 1, atoi( argv[ 7 ] ) ) : 3;
            const uint64_t uiShare = argc >= 9 ? (uint64_t)atoll( argv[ 8 ] ) : 50;
            const size_t uiInv = std::min<size_t>( 300, std::max<size_t>( 40, uiLen / 3 ) );
            size_t uiInverted = 0;
            for( auto& pQ : *pReads )
                if( uiLen >= 3 * uiInv && rnd( ) % 1000 < uiShare )
                {
                    auto b = pQ->xCodes.begin( ) + ( uiLen - uiInv ) / 2;
                    std::reverse( b, b + uiInv );
                    for( auto it = b; it != b + uiInv; ++it )
                        *it = 3 - *it;
                    uiInverted++;
                }
            ParameterSetManager xOn = xParams, xOff = xParams;
            xOn.getSelected( )->search_inversions = 1;
            xOff.getSelected( )->search_inversions = 0;
            BatchAligner xAlignerOn( xOn ), xAlignerOff( xOff );
            for( BatchAligner* pA : { &xAlignerOn, &xAlignerOff } )
            {
                pA->uiBatchReads = std::min<size_t>( pReads->size( ), 1u << 18 );
                pA->uiInflight = 3;
                pA->warmUp( pFM, pReads );
            }
            uint64_t uiBytesContainer = 0, uiBytesOn = 0, uiBytesOff = 0;
            AlignerTiming xTimeOn, xTimeOff;
            auto container = [ & ]( ) {
                auto pSink = std::make_shared<CountingSink>( );
                FileWriter xWriter( xOn, std::static_pointer_cast<OutStream>( pSink ), pPack );
                const double t = now( );
                auto pRes = xAlignerOn.execute( pFM, pReads );
                for( size_t r = 0; r < pRes->size( ); r++ )
                    xWriter.execute( ( *pReads )[ r ], ( *pRes )[ r ], pPack );
                xWriter.flush( );
                const double f = now( ) - t;
                uiBytesContainer = pSink->uiBytes.load( );
                return f;
            };
            auto device = [ & ]( BatchAligner& rAligner, const ParameterSetManager& rP, uint64_t& rBytes, AlignerTiming& rTime ) {
                auto pSink = std::make_shared<CountingSink>( );
                BatchFileWriter xWriter( rP, std::static_pointer_cast<OutStream>( pSink ), pPack );
                const double t = now( );
                auto pFlat = rAligner.executeFlatSam( pFM, pReads, pPack );
                for( auto& pB : *pFlat )
                    xWriter.write( *pB, pPack );
                const double f = now( ) - t;
                rTime = rAligner.xLast;
                rBytes = pSink->uiBytes.load( );
                return f;
            };
            // (the container runs first and apart: the millions of containers a run frees leave the allocator busy under whatever
            // runs next, which is not what (b) against (c) is to show)
            std::vector<double> vC, vOn, vOff;
            container( );
            for( int r = 0; r < iRepeats; r++ )
                vC.push_back( n / container( ) );
            device( xAlignerOn, xOn, uiBytesOn, xTimeOn ), device( xAlignerOff, xOff, uiBytesOff, xTimeOff ); // warm-up of both
            for( int r = 0; r < 2 * iRepeats; r++ )
            {
                vOff.push_back( n / device( xAlignerOff, xOff, uiBytesOff, xTimeOff ) );
                vOn.push_back( n / device( xAlignerOn, xOn, uiBytesOn, xTimeOn ) );
            }
            auto list = []( std::vector<double> v ) {
                std::sort( v.begin( ), v.end( ) );
                return "{\"median\": " + std::to_string( v[ v.size( ) / 2 ] ) + ", \"min\": " + std::to_string( v.front( ) ) +
                       ", \"max\": " + std::to_string( v.back( ) ) + "}";
            };
            printf( "{\"inversions\": {\"reads\": %zu, \"read_len\": %zu, \"inverted_reads\": %zu, \"inverted_bases\": %zu, \"repeats\": %d, "
                    "\"batch_reads\": %zu, \"in_flight\": 3, \"execute_plus_file_writer_reads_per_s\": %s, \"execute_flat_sam_reads_per_s\": %s, "
                    "\"execute_flat_sam_option_off_reads_per_s\": %s, \"sam_bytes_container\": %llu, \"sam_bytes_device\": %llu, "
                    "\"sam_bytes_option_off\": %llu, \"stages_s_option_on\": %.4f, \"stages_s_option_off\": %.4f, \"batches\": %llu}}\n",
                    n, uiLen, uiInverted, uiInv, iRepeats, xAlignerOn.uiBatchReads, list( vC ).c_str( ), list( vOn ).c_str( ), list( vOff ).c_str( ),
                    (unsigned long long)uiBytesContainer, (unsigned long long)uiBytesOn, (unsigned long long)uiBytesOff, xTimeOn.fKernels,
                    xTimeOff.fKernels, (unsigned long long)xTimeOn.uiBatches );
            return uiBytesContainer == uiBytesOn ? 0 : 1;
        }
        const bool bBgzfLeg = argc >= 7 && !strcmp( argv[ 6 ], "bgzf" );
        if( argc >= 7 && ( !strcmp( argv[ 6 ], "text" ) || bBgzfLeg ) )
        {
            // ---- the bgzf leg (the workload, workers and checks of the text leg, described below): the FASTQ text written once as
            // BGZF through zlib at the default level, 65 280 bytes of text per member as bgzip cuts them, to a file next to the
            // index; file to SAM text through (a) BatchBgzfReader -> executeBgzfSam -- the compressed bytes cut at member borders,
            // inflated and parsed on the device --, (b) GzFileStream -> BatchFileReader -> executeFlatSam -- what a compressed file
            // gets without it: zlib's gzread a byte at a time, then one NucSeq per read -- and (c) the text leg's (b) on the
            // uncompressed text, the ceiling.  All three must write the same bytes.  (Needs -DMA_WITH_ZLIB -lz.)
            // ---- the text leg: the n reads as ONE FASTQ text in memory (names r<i>, seeded qualities 35 .. 126), file to SAM text
            // through (a) StringStream -> BatchFileReader -> executeFlatSam -- records cut and parsed on the host, one NucSeq per
            // read, gathered and uploaded as arrays -- and (b) BatchTextReader -> executeTextSam -- blocks of text cut at record
            // starts, parsed on the device.  Both with three workers (own aligner each, one device batch of ~256 k reads at a
            // time) that pull their batches from the ONE stream.  One warm-up of each keeps its text -- the batches put into input
            // order by their first QNAME -- and the two files must be the same bytes; then alternating, <repeats> times each, with
            // the texts only counted (as the sam leg's sink does) and every count checked against the file's.
            const int iRepeats = argc >= 8 ? std::max( 1, atoi( argv[ 7 ] ) ) : 5;
            const size_t uiWorkers = 3, uiBatchReads = std::min<size_t>( std::max<size_t>( n, 1 ), 1u << 18 );
            std::string sFastq;
            sFastq.reserve( n * ( 2 * uiLen + 16 ) );
            for( size_t i = 0; i < n; i++ )
            {
                const NucSeq& rQ = *( *pReads )[ i ];
                sFastq += "@" + rQ.sName + "\n";
                for( uint8_t b : rQ.xCodes )
                    sFastq += "ACGTN"[ b ];
                sFastq += "\n+\n";
                for( size_t j = 0; j < rQ.xCodes.size( ); j++ )
                    sFastq += (char)( 35 + rnd( ) % 92 );
                sFastq += "\n";
            }
            pReads->clear( );
            BatchAligner::nameContigs( *pFM->pDev, *pPack );
            std::vector<std::unique_ptr<BatchAligner>> vAligners;
            for( size_t w = 0; w < uiWorkers; w++ )
            {
                vAligners.emplace_back( new BatchAligner( xParams ) );
                vAligners.back( )->uiBatchReads = uiBatchReads;
                vAligners.back( )->uiInflight = 1;
            }
            // runs `work( worker, keep, bytes ) -> false at the end` on the workers: every call handles the worker's next batch and adds
            // the bytes of its SAM text; pFile (the warm-up runs): the text is kept as well and put into input order
            typedef std::function<bool( size_t, std::string*, uint64_t& )> Work;
            auto run = [ & ]( const Work& work, std::string* pFile, uint64_t& ruiBytes ) {
                std::vector<std::pair<uint64_t, std::string>> vParts;
                std::mutex xParts;
                std::string sFailure;
                std::atomic<uint64_t> uiBytes{ 0 };
                const double t = now( );
                std::vector<std::thread> vT;
                for( size_t w = 0; w < uiWorkers; w++ )
                    vT.emplace_back( [ &, w ]( ) {
                        try
                        {
                            std::string sText;
                            uint64_t uiMine = 0;
                            while( work( w, pFile != nullptr ? &sText : nullptr, uiMine ) )
                                if( pFile != nullptr )
                                {
                                    const uint64_t uiFirst = sText.size( ) > 1 ? strtoull( sText.c_str( ) + 1, nullptr, 10 ) : 0; // "r<i>\t..."
                                    std::lock_guard<std::mutex> xGuard( xParts );
                                    vParts.emplace_back( uiFirst, std::move( sText ) );
                                    sText.clear( );
                                }
                            uiBytes += uiMine;
                        }
                        catch( const std::exception& rE )
                        {
                            std::lock_guard<std::mutex> xGuard( xParts );
                            sFailure = rE.what( );
                        }
                    } );
                for( auto& rT : vT )
                    rT.join( );
                const double f = now( ) - t;
                if( !sFailure.empty( ) )
                    throw std::runtime_error( sFailure );
                ruiBytes = uiBytes.load( );
                if( pFile != nullptr )
                {
                    std::sort( vParts.begin( ), vParts.end( ), []( const auto& a, const auto& b ) { return a.first < b.first; } );
                    pFile->clear( );
                    for( const auto& rPart : vParts )
                        *pFile += rPart.second;
                }
                return f;
            };
            uint64_t uiBytesHost = 0, uiBytesText = 0;
            auto host = [ & ]( std::string* pFile ) {
                auto pStream = std::make_shared<StringStream>( sFastq );
                BatchFileReader xReader( xParams );
                xReader.uiBatchReads = uiBatchReads;
                return run(
                    [ & ]( size_t w, std::string* pKeep, uint64_t& ruiBytes ) {
                        auto pBatch = xReader.execute( pStream );
                        if( pBatch == nullptr )
                            return false;
                        std::vector<AlignerTiming> vPer;
                        auto pFlat = vAligners[ w ]->executeFlatSamOn( pFM->pDev->all( ), pBatch, &vPer );
                        if( pKeep != nullptr )
                            pKeep->clear( );
                        for( auto& pB : *pFlat )
                        {
                            ruiBytes += pB->samBytes( );
                            if( pKeep != nullptr )
                                pKeep->append( pB->samText( ), pB->samBytes( ) );
                        }
                        return true;
                    },
                    pFile, uiBytesHost );
            };
            auto text = [ & ]( std::string* pFile ) {
                auto pStream = std::make_shared<StringStream>( sFastq );
                BatchTextReader xReader( xParams );
                xReader.uiBatchBytes = std::max<size_t>( 1, sFastq.size( ) / std::max<size_t>( n, 1 ) * uiBatchReads );
                return run(
                    [ & ]( size_t w, std::string* pKeep, uint64_t& ruiBytes ) {
                        auto pBatch = xReader.execute( pStream );
                        if( pBatch == nullptr )
                            return false;
                        auto pB = vAligners[ w ]->executeTextSamOn( pFM->pDev->p, pBatch );
                        ruiBytes += pB->samBytes( );
                        if( pKeep != nullptr )
                            pKeep->assign( pB->samText( ), pB->samBytes( ) );
                        return true;
                    },
                    pFile, uiBytesText );
            };
            if( bBgzfLeg )
            {
#ifdef MA_WITH_ZLIB
                const std::string sBgzf = bgzfOf( sFastq );
                const std::string sPath = std::string( argv[ 1 ] ) + ".boundary_bench.fq.gz";
                {
                    std::ofstream xOut( sPath, std::ios::binary );
                    xOut.write( sBgzf.data( ), (std::streamsize)sBgzf.size( ) );
                    if( !xOut )
                        throw std::runtime_error( "cannot write " + sPath );
                }
                uint64_t uiBytesBgzf = 0, uiBytesGz = 0;
                auto bgzf = [ & ]( std::string* pFile ) {
                    auto pStream = std::make_shared<StringStream>( sBgzf );
                    BatchBgzfReader xReader( xParams );
                    xReader.uiBatchBytes = std::max<size_t>( 1, sBgzf.size( ) / std::max<size_t>( n, 1 ) * uiBatchReads );
                    return run(
                        [ & ]( size_t w, std::string* pKeep, uint64_t& ruiBytes ) {
                            auto pBatch = xReader.execute( pStream );
                            if( pBatch == nullptr )
                                return false;
                            auto pB = vAligners[ w ]->executeBgzfSamOn( pFM->pDev->p, pBatch );
                            ruiBytes += pB->samBytes( );
                            if( pKeep != nullptr )
                                pKeep->assign( pB->samText( ), pB->samBytes( ) );
                            return true;
                        },
                        pFile, uiBytesBgzf );
                };
                auto gz = [ & ]( std::string* pFile ) {
                    std::shared_ptr<FileStream> pStream = std::make_shared<GzFileStream>( sPath );
                    BatchFileReader xReader( xParams );
                    xReader.uiBatchReads = uiBatchReads;
                    return run(
                        [ & ]( size_t w, std::string* pKeep, uint64_t& ruiBytes ) {
                            auto pBatch = xReader.execute( pStream );
                            if( pBatch == nullptr )
                                return false;
                            std::vector<AlignerTiming> vPer;
                            auto pFlat = vAligners[ w ]->executeFlatSamOn( pFM->pDev->all( ), pBatch, &vPer );
                            if( pKeep != nullptr )
                                pKeep->clear( );
                            for( auto& pB : *pFlat )
                            {
                                ruiBytes += pB->samBytes( );
                                if( pKeep != nullptr )
                                    pKeep->append( pB->samText( ), pB->samBytes( ) );
                            }
                            return true;
                        },
                        pFile, uiBytesGz );
                };
                // warm-up of all three: these runs keep their files, which must be the same bytes; the timed runs count theirs
                std::string sFileGz, sFileBgzf, sFilePlain;
                gz( &sFileGz ), bgzf( &sFileBgzf ), text( &sFilePlain );
                bool bSame = sFileGz == sFileBgzf && sFileGz == sFilePlain && !sFileGz.empty( );
                const uint64_t uiSamBytes = sFileGz.size( );
                std::string( ).swap( sFileGz ), std::string( ).swap( sFileBgzf ), std::string( ).swap( sFilePlain );
                std::vector<double> vA, vB, vC;
                for( int r = 0; r < iRepeats; r++ )
                {
                    vA.push_back( n / bgzf( nullptr ) ), vB.push_back( n / gz( nullptr ) ), vC.push_back( n / text( nullptr ) );
                    bSame = bSame && uiBytesBgzf == uiSamBytes && uiBytesGz == uiSamBytes && uiBytesText == uiSamBytes;
                }
                remove( sPath.c_str( ) );
                auto stats = []( std::vector<double> v ) {
                    std::string sAll;
                    for( double f : v )
                        sAll += ( sAll.empty( ) ? "" : ", " ) + std::to_string( f );
                    std::sort( v.begin( ), v.end( ) );
                    return "{\"median\": " + std::to_string( v[ v.size( ) / 2 ] ) + ", \"min\": " + std::to_string( v.front( ) ) +
                           ", \"max\": " + std::to_string( v.back( ) ) + ", \"all\": [" + sAll + "]}";
                };
                printf( "{\"bgzf\": {\"reads\": %zu, \"read_len\": %zu, \"repeats\": %d, \"batch_reads\": %zu, \"workers\": %zu, "
                        "\"bgzf_reader_bgzf_sam_reads_per_s\": %s, \"gz_stream_file_reader_flat_sam_reads_per_s\": %s, "
                        "\"text_reader_text_sam_reads_per_s\": %s, \"fastq_bytes\": %zu, \"bgzf_bytes\": %zu, \"sam_bytes\": %zu, \"equal\": %s}}\n",
                        n, uiLen, iRepeats, uiBatchReads, uiWorkers, stats( vA ).c_str( ), stats( vB ).c_str( ), stats( vC ).c_str( ), sFastq.size( ),
                        sBgzf.size( ), (size_t)uiSamBytes, bSame ? "true" : "false" );
                return bSame ? 0 : 1;
#else
                throw std::runtime_error( "the bgzf leg writes its file through zlib: build with -DMA_WITH_ZLIB -lz" );
#endif
            }
            // warm-up of both: these two runs keep their files, which must be the same bytes; the timed runs count theirs
            std::string sFileHost, sFileText;
            host( &sFileHost ), text( &sFileText );
            bool bEqual = sFileHost == sFileText && !sFileHost.empty( );
            const uint64_t uiFileBytes = sFileText.size( );
            std::string( ).swap( sFileHost ), std::string( ).swap( sFileText );
            std::vector<double> vH, vD;
            for( int r = 0; r < iRepeats; r++ )
            {
                vH.push_back( n / host( nullptr ) ), vD.push_back( n / text( nullptr ) );
                bEqual = bEqual && uiBytesHost == uiFileBytes && uiBytesText == uiFileBytes;
            }
            auto list = []( std::vector<double> v ) {
                std::string sAll;
                for( double f : v )
                    sAll += ( sAll.empty( ) ? "" : ", " ) + std::to_string( f );
                std::sort( v.begin( ), v.end( ) );
                return "{\"median\": " + std::to_string( v[ v.size( ) / 2 ] ) + ", \"min\": " + std::to_string( v.front( ) ) +
                       ", \"max\": " + std::to_string( v.back( ) ) + ", \"all\": [" + sAll + "]}";
            };
            printf( "{\"text\": {\"reads\": %zu, \"read_len\": %zu, \"repeats\": %d, \"batch_reads\": %zu, \"workers\": %zu, "
                    "\"file_reader_flat_sam_reads_per_s\": %s, \"text_reader_text_sam_reads_per_s\": %s, \"fastq_bytes\": %zu, "
                    "\"sam_bytes\": %zu, \"equal\": %s}}\n",
                    n, uiLen, iRepeats, uiBatchReads, uiWorkers, list( vH ).c_str( ), list( vD ).c_str( ), sFastq.size( ), (size_t)uiFileBytes,
                    bEqual ? "true" : "false" );
            return bEqual ? 0 : 1;
        }
        if( argc >= 7 && !strcmp( argv[ 6 ], "sam-bgzf" ) )
        {
            // ---- the compressed SAM leg: n single-end reads host to a FILE through BatchAligner::executeFlatSam + BatchFileWriter,
            // (a) plain: the text comes down and is written as it is; (b) SamOptions::bBgzf on aligner and writer: the text is
            // deflated on the device (ma_sam_bgzf_batch) and only its members come down and are written; (c) bBgzf on the writer
            // alone: the text comes down and up to 16 writer threads deflate it with the host statement of the same rules
            // (ma_bgzf::deflateHost) -- what a caller had before.  Alternating, <repeats> times each after one warm-up of each.
            // One more device run with ma_batch_enable_timing on an engine of its own gives the kernels' own time per batch.
            const int iRepeats = argc >= 8 ? std::max( 1, atoi( argv[ 7 ] ) ) : 5;
            ParameterSetManager xPacked = xParams;
            xPacked.xSam.bBgzf = true;
            BatchAligner xPlainAligner( xParams ), xPackedAligner( xPacked );
            for( BatchAligner* pA : { &xPlainAligner, &xPackedAligner } )
            {
                pA->uiBatchReads = std::min<size_t>( pReads->size( ), 1u << 18 );
                pA->uiInflight = 3;
                pA->warmUp( pFM, pReads );
            }
            // (MA_BOUNDARY_SAM_FILE: the file's name; it then stays, holding the last run's bytes -- the host-deflate variant's)
            const char* const sKeep = getenv( "MA_BOUNDARY_SAM_FILE" );
            const std::string sFile = sKeep != nullptr ? std::string( sKeep ) : "/tmp/ma_boundary_bench." + std::to_string( (long)getpid( ) ) + ".sam";
            struct Run
            {
                double fSeconds = 0, fWriter = 0;
                uint64_t uiFileBytes = 0, uiTextBytes = 0;
                AlignerTiming xTiming;
            };
            auto run = [ & ]( BatchAligner& rAligner, const ParameterSetManager& rWriterParams ) {
                Run r;
                const double t = now( );
                {
                    BatchFileWriter xWriter( rWriterParams, std::make_shared<FileWriter>( rWriterParams, sFile, pPack ), pPack );
                    xWriter.uiFormatThreads = std::min( 16u, uiHw );
                    auto pFlat = rAligner.executeFlatSam( pFM, pReads, pPack );
                    const double tW = now( );
                    for( auto& pB : *pFlat )
                        xWriter.write( *pB, pPack );
                    r.uiTextBytes = xWriter.uiBytes.load( );
                    r.fWriter = now( ) - tW;
                } // (the stream closes: the end-of-file marker)
                r.fSeconds = now( ) - t;
                r.xTiming = rAligner.xLast;
                std::ifstream xSize( sFile, std::ios::binary | std::ios::ate );
                r.uiFileBytes = (uint64_t)xSize.tellg( );
                return r;
            };
            Run xPlain = run( xPlainAligner, xParams ), xDevice = run( xPackedAligner, xPacked ), xHost = run( xPlainAligner, xPacked ); // warm-up
            std::vector<double> vP, vD, vH;
            for( int r = 0; r < iRepeats; r++ )
            {
                xPlain = run( xPlainAligner, xParams ), vP.push_back( n / xPlain.fSeconds );
                xDevice = run( xPackedAligner, xPacked ), vD.push_back( n / xDevice.fSeconds );
                xHost = run( xPlainAligner, xPacked ), vH.push_back( n / xHost.fSeconds );
            }
            if( sKeep == nullptr )
                remove( sFile.c_str( ) );
            // the kernels' own time: one batch of at most 2^18 reads on a batch object with timing on
            float aMs[ 8 ] = { 0, 0, 0, 0, 0, 0, 0, 0 };
            double fSamMs = 0;
            uint64_t uiOneText = 0, uiOneMembers = 0, uiOnePacked = 0;
            {
                const size_t uiOne = std::min<size_t>( pReads->size( ), 1u << 18 );
                std::vector<uint8_t> vCodes;
                std::vector<uint64_t> vOff( 1, 0 ), vNameOff( 1, 0 );
                std::string sNames;
                for( size_t i = 0; i < uiOne; i++ )
                {
                    const NucSeq& rQ = *( *pReads )[ i ];
                    vCodes.insert( vCodes.end( ), rQ.xCodes.begin( ), rQ.xCodes.end( ) );
                    vOff.push_back( vCodes.size( ) );
                    sNames += rQ.sName;
                    vNameOff.push_back( sNames.size( ) );
                }
                ma_batch* pB = nullptr;
                maCheck( ma_batch_create( pFM->pDev->p, &xParams.xSelected, uiOne, vCodes.size( ) + 64, &pB ) );
                maCheck( ma_batch_enable_timing( pB, 1 ) );
                maCheck( ma_batch_set_reads( pB, vCodes.data( ), vOff.data( ), uiOne ) );
                maCheck( ma_batch_set_read_text( pB, sNames.data( ), vNameOff.data( ), nullptr ) );
                maCheck( ma_align_batch( pB ) );
                maCheck( ma_batch_sync( pB ) );
                for( int k = 0; k < 2; k++ ) // (the second pass is the measured one)
                {
                    const double tS = now( );
                    maCheck( ma_sam_batch( pB, BatchAligner::samOptionBits( xParams.xSam ) ) );
                    maCheck( ma_batch_sync( pB ) );
                    fSamMs = 1e3 * ( now( ) - tS );
                    maCheck( ma_sam_bgzf_batch( pB, 0 ) );
                }
                maCheck( ma_batch_kernel_ms( pB, aMs ) );
                maCheck( ma_batch_sam_counts( pB, &uiOneText ) );
                maCheck( ma_batch_sam_bgzf_counts( pB, 0, &uiOneMembers, &uiOnePacked ) );
                maCheck( ma_batch_destroy( pB ) );
            }
            auto list = []( std::vector<double> v ) {
                std::sort( v.begin( ), v.end( ) );
                return "{\"median\": " + std::to_string( v[ v.size( ) / 2 ] ) + ", \"min\": " + std::to_string( v.front( ) ) +
                       ", \"max\": " + std::to_string( v.back( ) ) + "}";
            };
            auto phases = []( const Run& rR ) {
                char buf[ 320 ];
                snprintf( buf, sizeof( buf ), "{\"wall_s\": %.4f, \"batches\": %llu, \"h2d_s\": %.4f, \"stages_s\": %.4f, \"d2h_s\": %.4f, "
                          "\"writer_s\": %.4f, \"file_bytes\": %llu, \"text_bytes\": %llu}", rR.fSeconds, (unsigned long long)rR.xTiming.uiBatches,
                          rR.xTiming.fH2D, rR.xTiming.fKernels, rR.xTiming.fD2H, rR.fWriter, (unsigned long long)rR.uiFileBytes,
                          (unsigned long long)rR.uiTextBytes );
                return std::string( buf );
            };
            printf( "{\"sam_bgzf\": {\"reads\": %zu, \"read_len\": %zu, \"repeats\": %d, \"batch_reads\": %zu, \"in_flight\": 3, \"writer_threads\": %u, "
                    "\"plain_reads_per_s\": %s, \"device_deflate_reads_per_s\": %s, \"host_deflate_reads_per_s\": %s, \"phases_plain\": %s, "
                    "\"phases_device_deflate\": %s, \"phases_host_deflate\": %s, \"one_batch\": {\"reads\": %zu, \"text_bytes\": %llu, \"members\": %llu, "
                    "\"member_bytes\": %llu, \"sam_stage_ms\": %.3f, \"deflate_kernels_ms\": %.3f}}}\n",
                    n, uiLen, iRepeats, xPlainAligner.uiBatchReads, std::min( 16u, uiHw ), list( vP ).c_str( ), list( vD ).c_str( ), list( vH ).c_str( ),
                    phases( xPlain ).c_str( ), phases( xDevice ).c_str( ), phases( xHost ).c_str( ), std::min<size_t>( pReads->size( ), 1u << 18 ),
                    (unsigned long long)uiOneText, (unsigned long long)uiOneMembers, (unsigned long long)uiOnePacked, fSamMs, aMs[ 7 ] );
            return xDevice.uiTextBytes == xPlain.uiTextBytes && xHost.uiFileBytes == xDevice.uiFileBytes ? 0 : 1;
        }
        if( argc >= 7 && ( !strcmp( argv[ 6 ], "sam" ) || bSamTags ) )
        {
            // ---- the SAM leg: n single-end reads host to host INCLUDING SAM text through (a) BatchAligner::executeFlat +
            // BatchFileWriter -- records downloaded, formatted by up to 16 host threads -- and (b) executeFlatSam -- formatted on
            // the device, the text is what comes down; alternating, <repeats> times each after one warm-up of each.  The phase
            // sums of the last repeat of each (AlignerTiming; d2h of (b) holds ma_sam_batch and the text download) are the
            // step timeline.  sam-tags: the same reads and repeats with the NGMLR tag emulation -- (a) is then the per-read
            // FileWriter on Alignment containers (BatchFileWriter's path for the option), (b) ma_sam_batch with
            // MA_SAM_NGMLR_TAGS.
            const int iRepeats = argc >= 8 ? std::max( 1, atoi( argv[ 7 ] ) ) : 5;
            BatchAligner xAligner( xParams );
            xAligner.uiBatchReads = std::min<size_t>( pReads->size( ), 1u << 18 );
            xAligner.uiInflight = 3;
            xAligner.warmUp( pFM, pReads );
            uint64_t uiBytesHost = 0, uiBytesDevice = 0, uiRecordBytes = 0;
            double fWriterHost = 0, fWriterDevice = 0;
            AlignerTiming xHost, xDevice;
            auto host = [ & ]( ) {
                auto pSink = std::make_shared<CountingSink>( );
                BatchFileWriter xWriter( xParams, std::static_pointer_cast<OutStream>( pSink ), pPack );
                xWriter.uiFormatThreads = std::min( 16u, uiHw );
                const double t = now( );
                auto pFlat = xAligner.executeFlat( pFM, pReads );
                const double tW = now( );
                uiRecordBytes = 0;
                for( auto& pB : *pFlat )
                {
                    xWriter.write( *pB, pPack );
                    uiRecordBytes += ( pB->size( ) + 1 ) * 8 + pB->pResult->uiMqAlignments * sizeof( ma_alignment ) + pB->pResult->uiMqOps * 16;
                }
                const double f = now( ) - t;
                fWriterHost = now( ) - tW;
                xHost = xAligner.xLast;
                uiBytesHost = pSink->uiBytes.load( );
                return f;
            };
            auto device = [ & ]( ) {
                auto pSink = std::make_shared<CountingSink>( );
                BatchFileWriter xWriter( xParams, std::static_pointer_cast<OutStream>( pSink ), pPack );
                const double t = now( );
                auto pFlat = xAligner.executeFlatSam( pFM, pReads, pPack );
                const double tW = now( );
                for( auto& pB : *pFlat )
                    xWriter.write( *pB, pPack );
                const double f = now( ) - t;
                fWriterDevice = now( ) - tW;
                xDevice = xAligner.xLast;
                uiBytesDevice = pSink->uiBytes.load( );
                return f;
            };
            host( ), device( ); // warm-up of both
            std::vector<double> vH, vD;
            for( int r = 0; r < iRepeats; r++ )
                vH.push_back( n / host( ) ), vD.push_back( n / device( ) );
            auto list = []( std::vector<double> v ) {
                std::sort( v.begin( ), v.end( ) );
                return "{\"median\": " + std::to_string( v[ v.size( ) / 2 ] ) + ", \"min\": " + std::to_string( v.front( ) ) +
                       ", \"max\": " + std::to_string( v.back( ) ) + "}";
            };
            auto phases = []( const AlignerTiming& rT, double fWriter ) {
                char buf[ 256 ];
                snprintf( buf, sizeof( buf ), "{\"wall_s\": %.4f, \"batches\": %llu, \"pack_s\": %.4f, \"h2d_s\": %.4f, \"stages_s\": %.4f, "
                          "\"d2h_s\": %.4f, \"writer_s\": %.4f}", rT.fWall, (unsigned long long)rT.uiBatches, rT.fPack, rT.fH2D, rT.fKernels,
                          rT.fD2H, fWriter );
                return std::string( buf );
            };
            printf( "{\"%s\": {\"reads\": %zu, \"read_len\": %zu, \"repeats\": %d, \"batch_reads\": %zu, \"in_flight\": 3, "
                    "\"format_threads\": %u, \"execute_flat_plus_writer_reads_per_s\": %s, \"execute_flat_sam_reads_per_s\": %s, "
                    "\"sam_bytes_host\": %llu, \"sam_bytes_device\": %llu, \"record_bytes\": %llu, \"phases_host\": %s, "
                    "\"phases_device\": %s}}\n",
                    bSamTags ? "sam_tags" : "sam", n, uiLen, iRepeats, xAligner.uiBatchReads, std::min( 16u, uiHw ), list( vH ).c_str( ), list( vD ).c_str( ),
                    (unsigned long long)uiBytesHost, (unsigned long long)uiBytesDevice, (unsigned long long)uiRecordBytes,
                    phases( xHost, fWriterHost ).c_str( ), phases( xDevice, fWriterDevice ).c_str( ) );
            return uiBytesHost == uiBytesDevice ? 0 : 1;
        }
        if( getenv( "MA_BOUNDARY_ONLY_GRAPH" ) ) // diagnostics: the per-read graph with the prefetching reader alone
        {
            defaultBatcherOptions( ).bStages = false;
            double fBest = 0;
            int iBest = 0;
            const std::string sOnly = prefetchLeg( xParams, pReads, pFM, pPack, 0, fBest, iBest );
            printf( "{\"graph\": {\"reads_per_s\": %.1f, \"threads\": %d, %s}}\n", fBest, iBest, sOnly.c_str( ) );
            return 0;
        }
        // ---- leg 1: BatchAligner
        std::string sBatch;
        std::shared_ptr<BatchAligner::TP_RESULT> pRes;
        for( size_t uiInflight : { (size_t)1, (size_t)2 } )
        {
            BatchAligner xAligner( xParams );
            xAligner.uiInflight = uiInflight;
            xAligner.execute( pFM, pReads ); // warm-up: every engine allocates its device pools and page-locked staging once
            pRes = xAligner.execute( pFM, pReads );
            const AlignerTiming& T = xAligner.xLast;
            char buf[ 512 ];
            snprintf( buf, sizeof( buf ),
                      "%s\"inflight_%zu\": {\"reads_per_s\": %.1f, \"wall_s\": %.4f, \"h2d_s\": %.4f, \"kernels_s\": %.4f, \"d2h_s\": %.4f, "
                      "\"containers_s\": %.4f, \"device_batches\": %llu, \"aligned_reads\": %llu}",
                      sBatch.empty( ) ? "" : ", ", uiInflight, n / T.fWall, T.fWall, T.fH2D, T.fKernels, T.fD2H, T.fContainers,
                      (unsigned long long)T.uiBatches, (unsigned long long)T.uiAlignedReads );
            sBatch += buf;
        }
        // ---- leg 1b: the same with the results left flat (no Alignment containers), 1 .. 4 device batches in flight
        std::string sFlat;
        std::shared_ptr<BatchAligner::TP_FLAT> pFlat;
        for( size_t uiInflight : { (size_t)1, (size_t)2, (size_t)3, (size_t)4 } )
        {
            BatchAligner xAligner( xParams );
            xAligner.uiInflight = uiInflight;
            xAligner.executeFlat( pFM, pReads ); // warm-up: engines size their buffers, page-locked arenas are touched
            pFlat = xAligner.executeFlat( pFM, pReads );
            const AlignerTiming& T = xAligner.xLast;
            char buf[ 512 ];
            snprintf( buf, sizeof( buf ),
                      "%s\"inflight_%zu\": {\"reads_per_s\": %.1f, \"wall_s\": %.4f, \"gather_s\": %.4f, \"h2d_s\": %.4f, \"kernels_s\": %.4f, "
                      "\"d2h_s\": %.4f, \"device_batches\": %llu, \"aligned_reads\": %llu, \"slowest_batch_over_median\": %.2f}",
                      sFlat.empty( ) ? "" : ", ", uiInflight, n / T.fWall, T.fWall, T.fPack, T.fH2D, T.fKernels, T.fD2H,
                      (unsigned long long)T.uiBatches, (unsigned long long)T.uiAlignedReads, T.maxOverMedian( ) );
            sFlat += buf;
            // engines before admission: no batch of a timed leg may pay an engine's allocations (round 3: 2.9 s inside a 0.06 s leg)
            if( T.maxOverMedian( ) > 3.0 )
                fprintf( stderr, "WARNING: flat leg with %zu in flight: slowest device batch %.1fx the median\n", uiInflight, T.maxOverMedian( ) );
        }
        // ---- leg 1c: ONE process, several index replicas: MultiDeviceAligner::executeFlat with persistent engines.
        // On a node every replica is another GPU; on a one-GPU box the second replica is a "virtual shard" on the same device,
        // which must cost nothing: 2 replicas x 2 batches in flight against 1 replica x 4 in flight.
        std::string sMulti;
        {
            int nDev = 1;
            maCheck( ma_device_count( &nDev ) );
            const int iHere = atoi( argv[ 5 ] );
            double fOne = 0;
            for( int iReplicas : { 1, 2 } )
            {
                std::vector<int> vDevices;
                for( int g = 0; g < iReplicas; g++ )
                    vDevices.push_back( nDev >= iReplicas ? ( iHere + g ) % nDev : iHere );
                auto vReplicas = MultiDeviceAligner::replicate( pFM, vDevices, iHere );
                MultiDeviceAligner xMulti( xParams, vReplicas );
                xMulti.uiInflight = iReplicas == 1 ? 4 : 2;
                xMulti.warmUp( pReads );
                xMulti.executeFlat( pReads );
                const uint64_t uiEngines = detail::Engine::created( ).load( );
                auto pOut = xMulti.executeFlat( pReads );
                const AlignerTiming& T = xMulti.xLast;
                if( iReplicas == 1 )
                    fOne = n / T.fWall;
                char buf[ 512 ];
                snprintf( buf, sizeof( buf ),
                          "%s\"replicas_%d\": {\"reads_per_s\": %.1f, \"wall_s\": %.4f, \"inflight_per_replica\": %zu, \"devices\": \"%s\", "
                          "\"device_batches\": %llu, \"batches_of_last_replica\": %llu, \"engines_created_by_the_timed_run\": %llu, "
                          "\"over_one_replica\": %.3f, \"slowest_batch_over_median\": %.2f}",
                          sMulti.empty( ) ? "" : ", ", iReplicas, n / T.fWall, T.fWall, xMulti.uiInflight,
                          nDev >= iReplicas ? "distinct" : "virtual shards on one device", (unsigned long long)T.uiBatches,
                          (unsigned long long)xMulti.vLast.back( ).uiBatches,
                          (unsigned long long)( detail::Engine::created( ).load( ) - uiEngines ), fOne > 0 ? ( n / T.fWall ) / fOne : 0.0,
                          T.maxOverMedian( ) );
                sMulti += buf;
            }
        }
        // ---- leg 2b: SAM text of the flat batches (BatchFileWriter: arenas, one write per batch)
        double fSamFlat = 0;
        uint64_t uiSamFlatBytes = 0;
        {
            auto pSinkF = std::make_shared<CountingSink>( );
            BatchFileWriter xBatchWriter( xParams, std::static_pointer_cast<OutStream>( pSinkF ), pPack );
            xBatchWriter.uiFormatThreads = std::min( 32u, uiHw );
            t0 = now( );
            for( auto& pB : *pFlat )
            {
                auto pSlice = std::make_shared<ReadVec>( pReads->begin( ) + pB->uiFirst, pReads->begin( ) + pB->uiFirst + pB->size( ) );
                xBatchWriter.execute( pSlice, pB, pPack );
            }
            fSamFlat = now( ) - t0;
            uiSamFlatBytes = pSinkF->uiBytes.load( );
        }
        pFlat.reset( );
        // ---- leg 2c: the throughput path AS GRAPH NODES: source -> BatchAlign -> BatchFileWriter, T graph threads under
        // simultaneousGet (each thread = one device batch in flight), reads in host memory -> SAM bytes in the sink
        std::string sBatchGraph;
        for( int iT : { 2, 3, 4 } )
        {
            auto pSinkG = std::make_shared<CountingSink>( );
            auto pSource = std::make_shared<BatchSource>( pReads );
            pSource->uiBatchReads = 1u << 17;
            auto pAlign = std::make_shared<BatchAlign>( xParams );
            auto pBatchWriter = std::make_shared<BatchFileWriter>( xParams, std::static_pointer_cast<OutStream>( pSinkG ), pPack );
            pBatchWriter->uiFormatThreads = std::min( 16u, uiHw );
            auto pPackP = std::make_shared<Pledge<Pack>>( );
            pPackP->set( pPack );
            auto pFmP = std::make_shared<Pledge<FMIndex>>( );
            pFmP->set( pFM );
            std::vector<std::shared_ptr<BasePledge>> vSinks;
            for( int t = 0; t < iT; t++ )
            {
                auto pBatch = promiseMe( std::make_shared<Lock<ReadVec>>( ), promiseMe( pSource ) );
                auto pAligned = promiseMe( pAlign, pFmP, pBatch );
                auto pWritten = promiseMe( pBatchWriter, pBatch, pAligned, pPackP );
                vSinks.push_back( promiseMe( std::make_shared<UnLock<Container>>( pBatch ), pWritten ) );
            }
            {
                // warm-up: iT engines at once, each allocates its device pools and page-locked staging (they stay with pAlign)
                std::vector<std::thread> vWarm;
                for( int t = 0; t < iT; t++ )
                    vWarm.emplace_back( [ & ]( ) {
                        pAlign->execute( pFM, std::make_shared<ReadVec>( pReads->begin( ), pReads->begin( ) + std::min<size_t>( n, 1u << 17 ) ) );
                    } );
                for( auto& rT : vWarm )
                    rT.join( );
                pAlign->uiBatches = 0;
            }
            t0 = now( );
            BasePledge::simultaneousGet( vSinks );
            const double f = now( ) - t0;
            char buf[ 384 ];
            snprintf( buf, sizeof( buf ), "%s\"graph_threads_%d\": {\"reads_per_s\": %.1f, \"wall_s\": %.4f, \"device_batches\": %llu, \"sam_bytes\": %llu}",
                      sBatchGraph.empty( ) ? "" : ", ", iT, n / f, f, (unsigned long long)pAlign->uiBatches.load( ),
                      (unsigned long long)pSinkG->uiBytes.load( ) );
            sBatchGraph += buf;
        }
        // ---- leg 2d: the doAlign shape (execution-context.h:291-406) end to end: FASTQ TEXT -> BatchFileReader -> BatchAlign ->
        // BatchFileWriter -> SAM bytes, graph threads under simultaneousGet.  The text lives in memory (no disk in the timing).
        std::string sFastqGraph;
        {
            std::string sFastq;
            sFastq.reserve( n * ( 2 * uiLen + 24 ) );
            for( size_t i = 0; i < n; i++ )
            {
                const NucSeq& rQ = *( *pReads )[ i ];
                sFastq.push_back( '@' );
                sFastq += rQ.sName;
                sFastq.push_back( '\n' );
                for( uint8_t b : rQ.xCodes )
                    sFastq.push_back( "ACGTN"[ b < 4 ? b : 4 ] );
                sFastq += "\n+\n";
                sFastq.append( rQ.xCodes.size( ), 'F' );
                sFastq.push_back( '\n' );
            }
            for( int iT : { 3, 4, 6 } )
            {
                auto pSinkG = std::make_shared<CountingSink>( );
                auto pStream = std::make_shared<Pledge<FileStream>>( );
                pStream->set( std::make_shared<StringStream>( sFastq ) );
                auto pBatchReader = std::make_shared<BatchFileReader>( xParams );
                pBatchReader->uiBatchReads = 1u << 17;
                auto pAlign = std::make_shared<BatchAlign>( xParams );
                auto pBatchWriter = std::make_shared<BatchFileWriter>( xParams, std::static_pointer_cast<OutStream>( pSinkG ), pPack );
                pBatchWriter->uiFormatThreads = std::min( 16u, uiHw );
                auto pPackP = std::make_shared<Pledge<Pack>>( );
                pPackP->set( pPack );
                auto pFmP = std::make_shared<Pledge<FMIndex>>( );
                pFmP->set( pFM );
                std::vector<std::shared_ptr<BasePledge>> vSinks;
                for( int t = 0; t < iT; t++ )
                {
                    auto pBatch = promiseMe( std::make_shared<Lock<ReadVec>>( ), promiseMe( pBatchReader, pStream ) );
                    auto pAligned = promiseMe( pAlign, pFmP, pBatch );
                    auto pWritten = promiseMe( pBatchWriter, pBatch, pAligned, pPackP );
                    vSinks.push_back( promiseMe( std::make_shared<UnLock<Container>>( pBatch ), pWritten ) );
                }
                {
                    std::vector<std::thread> vWarm;
                    for( int t = 0; t < iT; t++ )
                        vWarm.emplace_back( [ & ]( ) {
                            pAlign->execute( pFM, std::make_shared<ReadVec>( pReads->begin( ), pReads->begin( ) + std::min<size_t>( n, 1u << 17 ) ) );
                        } );
                    for( auto& rT : vWarm )
                        rT.join( );
                    pAlign->uiBatches = 0;
                }
                t0 = now( );
                BasePledge::simultaneousGet( vSinks );
                const double f = now( ) - t0;
                char buf[ 384 ];
                snprintf( buf, sizeof( buf ), "%s\"graph_threads_%d\": {\"reads_per_s\": %.1f, \"wall_s\": %.4f, \"device_batches\": %llu, \"fastq_bytes\": %zu, \"sam_bytes\": %llu}",
                          sFastqGraph.empty( ) ? "" : ", ", iT, n / f, f, (unsigned long long)pAlign->uiBatches.load( ), sFastq.size( ),
                          (unsigned long long)pSinkG->uiBytes.load( ) );
                sFastqGraph += buf;
            }
        }
        // ---- leg 2: SAM text of every read
        auto pSink = std::make_shared<CountingSink>( );
        FileWriter xWriter( xParams, std::static_pointer_cast<OutStream>( pSink ), pPack );
        const unsigned uiSamThreads = std::min( 64u, uiHw );
        t0 = now( );
        {
            std::atomic<size_t> uiNext{ 0 };
            std::vector<std::thread> vT;
            for( unsigned t = 0; t < uiSamThreads; t++ )
                vT.emplace_back( [ & ]( ) {
                    for( size_t i = uiNext++; i < n; i = uiNext++ )
                        xWriter.execute( ( *pReads )[ i ], ( *pRes )[ i ], pPack );
                } );
            for( auto& t : vT )
                t.join( );
        }
        const double fSam = now( ) - t0;
        pRes.reset( );
        // ---- leg 3: the unchanged per-read graph with many graph threads
        auto pPackP = std::make_shared<Pledge<Pack>>( );
        pPackP->set( pPack );
        auto pFmP = std::make_shared<Pledge<FMIndex>>( );
        pFmP->set( pFM );
        auto pSai = std::make_shared<Pledge<SuffixArrayInterface>>( );
        pSai->set( pFM );
        // the chain of export.cpp:104-108 only hands its intermediate containers from one MI355X module to the next
        defaultBatcherOptions( ).bStages = false;
        auto pReader = std::make_shared<VecReader>( *pReads );
        auto pSeeding = std::make_shared<BinarySeeding>( xParams );
        auto pSOC = std::make_shared<StripOfConsideration>( xParams );
        auto pHarm = std::make_shared<Harmonization>( xParams );
        auto pDP = std::make_shared<NeedlemanWunsch>( xParams );
        auto pMq = std::make_shared<MappingQuality>( xParams );
        auto pSink2 = std::make_shared<CountingSink>( );
        auto pWriter = std::make_shared<FileWriter>( xParams, std::static_pointer_cast<OutStream>( pSink2 ), pPack );
        std::vector<std::shared_ptr<BasePledge>> vSinks;
        for( int t = 0; t < iGraphThreads; t++ )
        {
            auto pQuery = promiseMe( std::make_shared<Lock<NucSeq>>( ), promiseMe( pReader ) );
            auto pSeeds = promiseMe( pSeeding, pSai, pQuery );
            auto pSOCs = promiseMe( pSOC, pSeeds, pQuery, pPackP, pFmP );
            auto pHarmonized = promiseMe( pHarm, pSOCs, pQuery, pFmP );
            auto pAlignments = promiseMe( pDP, pHarmonized, pQuery, pPackP );
            auto pWithQuality = promiseMe( pMq, pQuery, pAlignments );
            auto pWritten = promiseMe( pWriter, pQuery, pWithQuality, pPackP );
            vSinks.push_back( promiseMe( std::make_shared<UnLock<Container>>( pQuery ), pWritten ) );
        }
        t0 = now( );
        BasePledge::simultaneousGet( vSinks );
        const double fGraph = now( ) - t0;
        auto xStat = pSeeding->batchStatistics( );
        double fRun = 0, fUp = 0, fKern = 0, fDown = 0;
        if( pSeeding->batcher( ) != nullptr )
            pSeeding->batcher( )->phaseSeconds( fRun, fUp, fKern, fDown );
        double aStage[ 4 ] = { 0, 0, 0, 0 };
        if( pSeeding->batcher( ) != nullptr )
            pSeeding->batcher( )->stageSeconds( aStage );
        fprintf( stderr, "graph leg: %.3f s wall; device batches: run %.3f s (h2d %.3f, kernels %.3f = seed %.3f + extract %.3f + chain %.3f + dp %.3f, d2h %.3f) summed over %llu batches\n",
                 fGraph, fRun, fUp, fKern, aStage[ 0 ], aStage[ 1 ], aStage[ 2 ], aStage[ 3 ], fDown, (unsigned long long)xStat.first );
        double fPrefetchBest = 0;
        int iPrefetchBestThreads = 0;
        const std::string sPrefetch = prefetchLeg( xParams, pReads, pFM, pPack, pSink2->uiBytes.load( ), fPrefetchBest, iPrefetchBestThreads );
        printf( "{\"reads\": %zu, \"read_len\": %zu, \"host_threads\": %u, \"index_load_s\": %.2f, "
                "\"batch_aligner\": {%s, \"what\": \"reads in host memory -> BatchAligner::execute (H2D, all stages, D2H, Alignment "
                "containers); 256 k reads per device batch; phase times summed over the batches\"}, "
                "\"batch_aligner_flat\": {%s, \"what\": \"BatchAligner::executeFlat: the same without Alignment containers -- the result "
                "of a device batch stays one header array + one ops array in page-locked memory\"}, "
                "\"multi_device_flat\": {%s, \"what\": \"MultiDeviceAligner::executeFlat: one process, device batches rotating over the "
                "replicas of the index, engines persistent (second run timed)\"}, "
                "\"sam_flat\": {\"reads_per_s\": %.1f, \"bytes\": %llu, \"what\": \"BatchFileWriter::execute on the flat batches: formatted by "
                "up to 32 threads into byte arenas, one write per batch\"}, "
                "\"batch_graph\": {%s, \"what\": \"BatchSource -> BatchAlign -> BatchFileWriter as graph nodes under promiseMe / "
                "simultaneousGet, 128 k reads per device batch, one device batch in flight per graph thread: reads in host memory -> SAM bytes\"}, "
                "\"fastq_to_sam_graph\": {%s, \"what\": \"FASTQ text in memory -> BatchFileReader (records cut out of the stream under its lock, "
                "reads built outside) -> BatchAlign -> BatchFileWriter -> SAM bytes: the shape of ExecutionContext::doAlign as batch graph nodes\"}, "
                "\"sam\": {\"reads_per_s\": %.1f, \"threads\": %u, \"bytes\": %llu, \"what\": \"FileWriter::execute per read into a "
                "counting sink\"}, "
                "\"graph\": {\"reads_per_s\": %.1f, \"threads\": %d, %s, \"what\": \"the per-read graph of export.cpp:99-126 (reader -> "
                "BinarySeeding -> StripOfConsideration -> Harmonization -> NeedlemanWunsch -> MappingQuality -> FileWriter), the reader "
                "node wrapped into PrefetchReader: it pulls 64 k reads ahead, sends them through all stages on the GPU and hands "
                "every graph thread reads that are aligned already; reads_per_s = the best of the thread counts\"}, "
                "\"graph_funnel\": {\"reads_per_s\": %.1f, \"graph_threads\": %d, \"device_batches\": %llu, \"mean_reads_per_device_batch\": %.1f, "
                "\"what\": \"the same graph with the plain reader: per-read execute() calls of that many graph threads funnelled into "
                "device batches (DeviceBatcher)\"}}\n",
                n, uiLen, uiHw, fLoad, sBatch.c_str( ), sFlat.c_str( ), sMulti.c_str( ), n / fSamFlat, (unsigned long long)uiSamFlatBytes, sBatchGraph.c_str( ),
                sFastqGraph.c_str( ), n / fSam, uiSamThreads, (unsigned long long)pSink->uiBytes.load( ), fPrefetchBest, iPrefetchBestThreads,
                sPrefetch.c_str( ), n / fGraph, iGraphThreads, (unsigned long long)xStat.first, xStat.first ? (double)xStat.second / xStat.first : 0.0 );
    }
    catch( const std::exception& e )
    {
        fprintf( stderr, "error: %s\n", e.what( ) );
        return 1;
    }
    return 0;
}
