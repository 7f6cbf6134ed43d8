// ma_engine.h -- the host-side machinery between MA's per-read Module graph and the batch-oriented C ABI:
//   Engine        one device batch (ma_batch) + one HIP stream on the device of its index: reads in host memory ->
//                 H2D -> all four stages -> D2H of every stage's records (BatchResult), with the time of each phase
//   PrefetchQueue the funnel turned round (round 4): a volatile SOURCE of the graph reads AHEAD -- it pulls a device batch
//                 worth of reads from the reader it wraps, sends them through all stages and hands every graph thread one
//                 read of a FINISHED batch with its ticket, so that no graph thread ever blocks per read and a few dozen
//                 graph threads keep the GPU busy (the per-read funnel needs a thousand)
//   DeviceBatcher thread-safe funnel: the graph threads of libMA::setUpCompGraph (export.cpp:84-126, one graph copy per
//                 thread, every copy calling BinarySeeding::execute concurrently and lock-free, module.h:303-369) hand in
//                 ONE read each and block; the reads that arrive while the GPU is busy form the next device batch, whose
//                 results every waiting thread then picks its slice from (SURVEY 8(b) "Threading")
// Nothing here computes: every stage runs on the GPU behind include/ma_amd.h; a non-zero status becomes
// std::runtime_error like in the module wrappers.
#pragma once
#include "../../include/ma_amd.h"
#include "ma_bgzf_dev.h"
#include <algorithm>
#include <atomic>
#include <climits>
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace ma_amd
{
namespace engine
{
// a read in host memory: codes A0 C1 G2 T3 N4; the owner keeps it alive while its batch is in flight
struct ReadRef
{
    const uint8_t* pCodes = nullptr;
    size_t uiLength = 0;
    ReadRef( )
    {}
    ReadRef( const uint8_t* pCodes, size_t uiLength ) : pCodes( pCodes ), uiLength( uiLength )
    {}
    ReadRef( const std::vector<uint8_t>& rCodes ) : pCodes( rCodes.data( ) ), uiLength( rCodes.size( ) )
    {}
};

// QNAME and QUAL of a read for the SAM mode of Engine::run (pQuality: nullptr or one character per base)
struct ReadText
{
    const char* pName = nullptr;
    size_t uiNameLen = 0;
    const uint8_t* pQuality = nullptr;
};
// SAM mode of Engine::run: the text of the batch's reads (one entry per read) and the MA_SAM_* bits of ma_sam_batch
// Beside the MA_SAM_* bits in a run's SAM options: the text stays on the device, is deflated there (ma_sam_bgzf_batch) and only its
// BGZF members come down (BatchResult::bSamBgzf).  The bit is the host layer's: it never reaches the library.
static const uint32_t SAM_AS_BGZF = 0x80000000u;
// (The three calls behind the bit are weak references: a program that stands in for the library without them still links --
// tests/emul/engine_calls_test.cpp stubs exactly the calls its golden trace holds -- and the bit then throws.)
#pragma weak ma_sam_bgzf_batch
#pragma weak ma_batch_sam_bgzf_counts
#pragma weak ma_batch_get_sam_bgzf
struct SamMode
{
    const std::vector<ReadText>* pText = nullptr;
    uint32_t uiOptions = 0;
};

inline void engineCheck( int rc )
{
    if( rc != 0 )
        throw std::runtime_error( ma_last_error( ) );
}
inline double secondsSince( const std::chrono::steady_clock::time_point& t0 )
{
    return std::chrono::duration<double>( std::chrono::steady_clock::now( ) - t0 ).count( );
}

// Copies of an index on the devices of vDevices (the index is replicated per GPU, 11.9 GB of 288 GB; the arrays are
// downloaded once and uploaded per device, each upload on a thread bound to its device).  The caller owns the handles
// (ma_index_destroy).  A device may be named more than once and may be the original's own ("virtual shards" in tests).
inline std::vector<ma_index*> replicateOnDevices( const ma_index* pOriginal, const std::vector<int>& vDevices )
{
    std::vector<ma_index*> vNew;
    if( vDevices.empty( ) )
        return vNew;
    uint64_t nWords = 0, nSa = 0, uiN = 0;
    int32_t nContigs = 0;
    engineCheck( ma_index_sizes( pOriginal, &nWords, &nSa, &uiN, &nContigs ) );
    std::vector<uint32_t> vBwt( nWords );
    std::vector<int64_t> vSa( nSa );
    std::vector<uint8_t> vPac( ( uiN / 2 + 3 ) / 4 + 1 );
    std::vector<uint64_t> vStarts( nContigs ), vLens( nContigs );
    uint64_t L2[ 5 ];
    int64_t primary = 0;
    engineCheck( ma_index_download( pOriginal, vBwt.data( ), vSa.data( ), L2, &primary, vPac.data( ), vStarts.data( ), vLens.data( ) ) );
    for( int iDev : vDevices )
    {
        ma_index* pCopy = nullptr;
        std::string sFailure;
        std::thread xCreator( [ & ]( ) { // the upload binds its own thread to the target device
            if( ma_set_device( iDev ) != 0 ||
                ma_index_create( vBwt.data( ), nWords, vSa.data( ), nSa, L2, primary, uiN, vPac.data( ), nContigs, vStarts.data( ),
                                 vLens.data( ), &pCopy ) != 0 )
                sFailure = ma_last_error( );
        } );
        xCreator.join( );
        if( !sFailure.empty( ) )
        {
            for( ma_index* p : vNew )
                ma_index_destroy( p );
            throw std::runtime_error( "replicateOnDevices: device " + std::to_string( iDev ) + ": " + sFailure );
        }
        vNew.push_back( pCopy );
    }
    return vNew;
}

// Page-locked host array that only grows (ma_host_alloc): the arrays a device batch is uploaded from and downloaded into.
// Not value-initialised: a download overwrites what it needs.
template <typename T> class HostBuf
{
    T* p = nullptr;
    size_t uiCap = 0;
    bool bPinned = false;

    void release( )
    {
        if( p != nullptr && bPinned )
            ma_host_free( p );
        else if( p != nullptr )
            free( p );
        p = nullptr;
        uiCap = 0;
    }

  public:
    HostBuf( )
    {}
    HostBuf( const HostBuf& ) = delete;
    HostBuf& operator=( const HostBuf& ) = delete;
    ~HostBuf( )
    {
        release( );
    }
    T* need( size_t n ) // at least n elements (contents are lost when it grows)
    {
        if( n > uiCap )
        {
            // the new block first, into locals: a failed (page-locked) allocation throws and must leave the buffer as it was,
            // not with p == nullptr and the new capacity (the engine is reused after a failed batch)
            const size_t uiNewCap = n + n / 4 + 64;
            // page-locking pays for the MB-sized arrays of a throughput batch; the few KB of a small batch of the per-read
            // funnel stay ordinary memory (page-locking and unlocking go through the driver and stall other streams)
            const bool bNewPinned = uiNewCap * sizeof( T ) >= ( 1u << 20 );
            void* q = nullptr;
            if( bNewPinned )
                engineCheck( ma_host_alloc( uiNewCap * sizeof( T ), &q ) );
            else if( ( q = malloc( uiNewCap * sizeof( T ) ) ) == nullptr )
                throw std::bad_alloc( );
            release( );
            p = static_cast<T*>( q );
            uiCap = uiNewCap;
            bPinned = bNewPinned;
        }
        return p;
    }
    T* data( )
    {
        return p;
    }
    const T* data( ) const
    {
        return p;
    }
    const T& operator[]( size_t i ) const
    {
        return p[ i ];
    }
};

// Host copies of the records of one device batch, CSR by read (offset arrays have n + 1 entries).
struct BatchResult
{
    size_t uiReads = 0;
    bool bStages = false; // segments / seeds / harmonized sets / unsorted-quality alignments present?
    std::vector<uint64_t> vSegOff, vSeedOff, vHsetOff, vHseedOff, vAlnOff;
    std::vector<ma_segment> vSegs;
    std::vector<ma_seed> vSeeds, vHseeds;
    std::vector<uint32_t> vHsetSoc;
    // the SoC queue of every read as the sweep leaves it (ma_batch_get_soc_heap): strips CSR by vSocOff, the read's seeds
    // re-sorted by reference position at vSeedOff (what a binding on the reference's own SoCPriorityQueue fills it with)
    std::vector<uint64_t> vSocOff;
    std::vector<ma_soc> vSocHeap;
    std::vector<ma_seed> vSortedSeeds;
    bool bSocQueues = false;
    std::vector<ma_alignment> vAlns; // NeedlemanWunsch output (bStages)
    std::vector<uint64_t> vAlnOps; // (type, length) pairs
    // MappingQuality output = the result of the path: a FLAT view, one header array + one ops array per device batch in
    // page-locked memory that the engine recycles; Alignment containers are built from it only where somebody asks for them
    HostBuf<uint64_t> vMqOff; // n + 1
    HostBuf<ma_alignment> vMq;
    HostBuf<uint64_t> vMqOps; // (type, length) pairs
    uint64_t uiMqAlignments = 0, uiMqOps = 0;
    uint64_t uiAlignedReads = 0;
    // Paired batches (Engine::run with bPairs: reads 2k, 2k + 1 are the mates of pair k): INSTEAD of the MappingQuality
    // records the records PairedReads leaves per pair (ma_pair_batch / ma_batch_get_pairs), CSR by pair, with the two columns
    // mate (1 = record of the first mate) and other (index of the partner's record within the pair, -1: none)
    bool bPairs = false;
    HostBuf<uint64_t> vPairOff; // uiReads / 2 + 1
    HostBuf<ma_alignment> vPair;
    HostBuf<uint64_t> vPairOps;
    HostBuf<int32_t> vPairMate, vPairOther;
    uint64_t uiPairRecords = 0, uiPairOps = 0, uiPairsOnHost = 0; // (uiPairsOnHost: pairs the library finished on the host)
    // SAM batches (Engine::run with a SamMode): INSTEAD of the MappingQuality records the SAM text the device formatted from
    // them (ma_sam_batch / ma_batch_get_sam): read r's records are vSam[ vSamOff[r] .. vSamOff[r+1] ), what FileWriter::execute
    // prints for it.  A batch the device does not serve (some reads with qualities, some without) keeps bSam false and
    // carries the records as usual.  With bPairs as well (ma_pair_sam_batch / ma_batch_get_pair_sam) the text is that of the
    // PAIRS, what PairedFileWriter::execute prints: pair k's records are vSam[ vSamOff[k] .. vSamOff[k+1] ), and there are no pair
    // records.
    bool bSam = false;
    uint32_t uiSamOptions = 0; // the MA_SAM_* bits the text was made with (bSam)
    HostBuf<uint64_t> vSamOff; // uiReads + 1 (pairs: uiReads / 2 + 1)
    HostBuf<char> vSam;
    uint64_t uiSamBytes = 0;
    // with SAM_AS_BGZF among the options: INSTEAD of the text its BGZF members as the device deflated them, packed back to back
    // (uiSamBytes is still the size of the text; vSamOff and vSam are not filled)
    bool bSamBgzf = false;
    HostBuf<uint8_t> vSamBgzf;
    uint64_t uiSamBgzfBytes = 0, uiSamBgzfMembers = 0;
    double fPack = 0, fH2D = 0, fKernels = 0, fD2H = 0; // seconds: gathering the reads, upload, all stages, download
    float aStageMs[ 8 ] = { 0, 0, 0, 0, 0, 0, 0, 0 }; // host wall time of seed / extract / chain / dp (ma_batch_host_ms)
};

class Engine
{
    const ma_index* pIndex;
    const ma_params xP;
    ma_batch* pBatch = nullptr;
    void* pStream = nullptr;
    uint64_t uiCapReads = 0, uiCapBases = 0;
    HostBuf<uint8_t> vCodes; // page-locked staging of the reads
    HostBuf<uint64_t> vOff;
    HostBuf<char> vNames; // SAM mode: QNAMEs, their CSR offsets and the qualities of the batch
    HostBuf<uint64_t> vNameOff;
    HostBuf<uint8_t> vQual;
    const bool bBlocking; // waits sleep instead of spinning (hosts that run far more threads than cores)
    // results are handed out as shared_ptr; one that nobody holds any more is reused (its page-locked arrays are kept)
    std::vector<std::shared_ptr<BatchResult>> vPool;

    std::shared_ptr<BatchResult> freshResult( )
    {
        for( auto& pR : vPool )
            if( pR.use_count( ) == 1 )
                return pR;
        if( vPool.size( ) < 64 )
        {
            vPool.push_back( std::make_shared<BatchResult>( ) );
            return vPool.back( );
        }
        return std::make_shared<BatchResult>( ); // the caller keeps many results alive: not pooled
    }

  public:
    bool bFetchSocQueues = false; // run(): with bStages also fetch every read's SoC queue (one extra kernel per batch)
    // batches this engine has completed.  Its FIRST batch allocates the device pools (GBs) and page-locks the staging
    // arrays, which stalls every stream of the process: callers run first batches one at a time, before they admit
    // concurrent work (primed( ), BatchAligner::alignRange, BatchAlign::execute, DeviceBatcher's constructor)
    uint64_t uiRuns = 0;
    bool primed( uint64_t uiReads ) const
    {
        return uiRuns != 0 && pBatch != nullptr && uiReads <= uiCapReads;
    }

  private:
    void fit( uint64_t uiReads, uint64_t uiBases )
    {
        if( pBatch != nullptr && uiReads <= uiCapReads && uiBases <= uiCapBases )
            return;
        if( pBatch != nullptr )
            ma_batch_destroy( pBatch );
        pBatch = nullptr;
        uiCapReads = std::max<uint64_t>( uiReads + uiReads / 4, 64 );
        uiCapBases = std::max<uint64_t>( uiBases + uiBases / 4, 4096 );
        engineCheck( ma_batch_create( pIndex, &xP, uiCapReads, uiCapBases + 64, &pBatch ) );
        engineCheck( ma_batch_set_stream( pBatch, pStream ) );
        engineCheck( ma_batch_set_blocking_sync( pBatch, bBlocking ? 1 : 0 ) );
    }

  public:
    Engine( const ma_index* pIndex, const ma_params& rP, bool bBlocking = false ) : pIndex( pIndex ), xP( rP ), bBlocking( bBlocking )
    {
        engineCheck( ma_stream_create( pIndex, &pStream ) );
        created( )++;
    }
    // engines constructed by this process so far (tests: a second run of a persistent aligner must not create any)
    static std::atomic<uint64_t>& created( )
    {
        static std::atomic<uint64_t> uiCreated{ 0 };
        return uiCreated;
    }
    const ma_index* index( ) const
    {
        return pIndex;
    }
    Engine( const Engine& ) = delete;
    Engine& operator=( const Engine& ) = delete;
    ~Engine( )
    {
        if( pBatch != nullptr )
            ma_batch_destroy( pBatch );
        ma_stream_destroy( pIndex, pStream );
    }

    // device batch and pools for batches of up to that size, now (instead of inside the first run)
    void reserve( uint64_t uiReads, uint64_t uiBases )
    {
        fit( uiReads, uiBases );
    }

    // vReads[i] = codes of read i (A0 C1 G2 T3 N4).  bStages: also fetch the records of the intermediate stages.
    std::shared_ptr<BatchResult> run( const std::vector<const std::vector<uint8_t>*>& vReads, bool bStages )
    {
        std::vector<ReadRef> vRefs;
        vRefs.reserve( vReads.size( ) );
        for( const std::vector<uint8_t>* pRead : vReads )
            vRefs.emplace_back( *pRead );
        return run( vRefs, bStages );
    }
    // pSam: SAM mode -- the result carries the SAM text of the reads instead of their MappingQuality records; with bPairs the
    // text of the PAIRS (PairedFileWriter's records, one vSamOff entry per pair) instead of the pair records; bInversions: see runFlat
    std::shared_ptr<BatchResult> run( const std::vector<ReadRef>& vReads, bool bStages, bool bPairs = false, const SamMode* pSam = nullptr,
                                      bool bInversions = false )
    {
        const size_t n = vReads.size( );
        auto tPack = std::chrono::steady_clock::now( );
        uint64_t* pOff = vOff.need( n + 1 );
        pOff[ 0 ] = 0;
        for( size_t i = 0; i < n; i++ )
            pOff[ i + 1 ] = pOff[ i ] + vReads[ i ].uiLength;
        uint8_t* pCodes = vCodes.need( pOff[ n ] + 1 );
        // gather the reads into the staging array; large batches on a few threads (10^6 scattered 150-byte copies)
        auto gather = [ & ]( size_t lo, size_t hi ) {
            for( size_t i = lo; i < hi; i++ )
                if( vReads[ i ].uiLength != 0 )
                    memcpy( pCodes + pOff[ i ], vReads[ i ].pCodes, vReads[ i ].uiLength );
        };
        const size_t uiThreads = n >= ( 1u << 16 ) ? 4 : 1;
        if( uiThreads == 1 )
            gather( 0, n );
        else
        {
            std::vector<std::thread> vT;
            for( size_t t = 1; t < uiThreads; t++ )
                vT.emplace_back( gather, n * t / uiThreads, n * ( t + 1 ) / uiThreads );
            gather( 0, n / uiThreads );
            for( auto& rT : vT )
                rT.join( );
        }
        // SAM mode: names and qualities next to the codes.  The device takes qualities for all reads of a batch or for none
        // (ma_batch_set_read_text); a batch that mixes the two is not served and comes back as records.
        SamText xText;
        if( pSam != nullptr )
        {
            if( pSam->pText == nullptr || pSam->pText->size( ) != n )
                throw std::runtime_error( "Engine::run: the SAM mode needs one ReadText per read" );
            const std::vector<ReadText>& rT = *pSam->pText;
            size_t uiWithQual = 0;
            uint64_t* pNameOff = vNameOff.need( n + 1 );
            pNameOff[ 0 ] = 0;
            for( size_t i = 0; i < n; i++ )
            {
                pNameOff[ i + 1 ] = pNameOff[ i ] + rT[ i ].uiNameLen;
                uiWithQual += rT[ i ].pQuality != nullptr;
            }
            if( uiWithQual == 0 || uiWithQual == n )
            {
                char* pNames = vNames.need( pNameOff[ n ] + 1 );
                uint8_t* pQual = uiWithQual ? vQual.need( pOff[ n ] + 1 ) : nullptr;
                for( size_t i = 0; i < n; i++ )
                {
                    if( rT[ i ].uiNameLen != 0 )
                        memcpy( pNames + pNameOff[ i ], rT[ i ].pName, rT[ i ].uiNameLen );
                    if( pQual != nullptr && vReads[ i ].uiLength != 0 )
                        memcpy( pQual + pOff[ i ], rT[ i ].pQuality, vReads[ i ].uiLength );
                }
                xText.pNames = pNames, xText.pNameOff = pNameOff, xText.pQual = pQual, xText.uiOptions = pSam->uiOptions;
                xText.bOn = true;
            }
        }
        const double fPack = secondsSince( tPack );
        auto pRes = runFlat( pCodes, pOff, n, bStages, bPairs, xText.bOn ? &xText : nullptr, bInversions );
        pRes->fPack = fPack;
        return pRes;
    }
    // SAM mode of runFlat: the reads' names (CSR, n + 1 offsets), their qualities (nullptr, or one character per base in the
    // reads' CSR) and the MA_SAM_* bits
    struct SamText
    {
        const char* pNames = nullptr;
        const uint64_t* pNameOff = nullptr;
        const uint8_t* pQual = nullptr;
        uint32_t uiOptions = 0;
        bool bOn = false;
    };
    // reads that already are one array of codes + CSR offsets (n + 1), e.g. in page-locked memory the caller filled
    // bPairs: the reads are mate pairs (2k, 2k + 1); the result carries the pair records instead of the MappingQuality ones
    // pSam: the result carries the SAM text (BatchResult::vSamOff / vSam) instead of the MappingQuality records
    // both: the pairs' SAM text (ma_pair_sam_batch), vSamOff per PAIR, instead of the pair records; bPairs and bSam are both set
    // bInversions: "Detect Small Inversions" on the device (ma_inversions_batch) between the alignment and all of the above: the
    // MappingQuality records, the pairs and both texts are then those of the lists with the inversion records in them
    std::shared_ptr<BatchResult> runFlat( const uint8_t* pCodes, const uint64_t* pOff, size_t n, bool bStages, bool bPairs = false,
                                          const SamText* pSam = nullptr, bool bInversions = false )
    {
        const uint32_t uiSamOptions = pSam != nullptr ? pSam->uiOptions : 0;
        auto pRes = beginRun( bStages, bPairs, pSam != nullptr, uiSamOptions );
        BatchResult& R = *pRes;
        R.uiReads = n;
        fit( n, pOff[ n ] );
        auto t0 = std::chrono::steady_clock::now( );
        engineCheck( ma_batch_set_reads( pBatch, pCodes, pOff, n ) );
        if( pSam != nullptr )
            engineCheck( ma_batch_set_read_text( pBatch, pSam->pNames, pSam->pNameOff, pSam->pQual ) );
        R.fH2D = secondsSince( t0 );
        t0 = runStages( R, bInversions );
        uint64_t nSeg = 0, nSeed = 0, nHset = 0, nHseed = 0, nAln = 0, nOps = 0;
        engineCheck( ma_batch_counts( pBatch, &nSeg, &nSeed, &nHset, &nHseed, &nAln, &nOps, &R.uiAlignedReads ) );
        if( bStages )
            fetchStageRecords( R, nSeg, nSeed, nHset, nHseed, nAln, nOps );
        if( bPairs && pSam != nullptr )
            fetchPairSam( R, uiSamOptions );
        else if( bPairs )
            fetchPairRecords( R );
        else if( pSam != nullptr )
            fetchSam( R, uiSamOptions );
        else
            fetchMqRecords( R, nAln, nOps );
        endRun( R, t0, [ & ]( char* p, size_t c ) { snprintf( p, c, "%zu reads, h2d", n ); } );
        return pRes;
    }
    // A FASTQ / FASTA text instead of reads (ma_batch_set_reads_text: the device parses it, strict form only) through all stages to
    // the SAM text of its reads: the result of runFlat's SAM mode (bSam, vSamOff, vSam; uiReads from the device), with no NucSeq,
    // no gather and no separate upload of names and qualities.  A text the device refuses throws the library's message, which
    // names the line.  The device batch is sized by the text: bases for its bytes, reads as the last texts held (a first text
    // that holds more is parsed twice).
    std::shared_ptr<BatchResult> runText( const char* pText, size_t uiBytes, uint32_t uiSamOptions, bool bInversions = false )
    {
        return runTextBy( uiBytes, uiSamOptions, bInversions,
                          [ & ]( uint64_t* pReads ) { return ma_batch_set_reads_text( pBatch, pText, uiBytes, pReads ); } );
    }
    // runText for a batch of a BGZF-compressed file: the text is pHead followed by what the members inflate to, minus its last
    // uiDrop bytes (ma_batch_set_reads_bgzf: the device inflates the members and parses the text).  The member headers are walked
    // here as well, for the size of the text the device batch is sized by.
    std::shared_ptr<BatchResult> runBgzf( const char* pHead, size_t uiHeadBytes, const char* pMembers, size_t uiMemberBytes, uint64_t uiDrop,
                                          uint32_t uiSamOptions, bool bInversions = false )
    {
        ma_bgzf::Result xWalk;
        ma_bgzf::inflateHost( (const uint8_t*)pMembers, uiMemberBytes, nullptr, &xWalk ); // (a bad header: the library refuses it by name)
        const size_t uiBytes = uiHeadBytes + xWalk.uiBytes - std::min<uint64_t>( uiDrop, xWalk.uiBytes );
        return runTextBy( uiBytes, uiSamOptions, bInversions, [ & ]( uint64_t* pReads ) {
            return ma_batch_set_reads_bgzf( pBatch, pHead, uiHeadBytes, pMembers, uiMemberBytes, uiDrop, pReads );
        } );
    }
    // runText for mate pairs: the texts of the two read files (ma_batch_set_mates_text: the device parses both, interleaves the
    // mates and, with bRevCompMates, reverse-complements every second one) through all stages, the pairing and the pairs'
    // formatting: the result of runFlat's paired SAM mode (bPairs, bSam, vSamOff per PAIR, vSam; uiReads = 2 x the pairs the device
    // found).  Records one text has beyond the other's are dropped as PairedFileReader drops them.  Sized like runText.
    std::shared_ptr<BatchResult> runMatesText( const char* pText1, size_t uiBytes1, const char* pText2, size_t uiBytes2, bool bRevCompMates,
                                               uint32_t uiSamOptions, bool bInversions = false )
    {
        auto pRes = beginRun( false, true, true, uiSamOptions );
        BatchResult& R = *pRes;
        auto t0 = std::chrono::steady_clock::now( );
        uint64_t aConsumed[ 2 ];
        const uint64_t nPairs = setText( uiBytes1 + uiBytes2, 2, [ & ]( uint64_t* pPairs ) {
            return ma_batch_set_mates_text( pBatch, pText1, uiBytes1, pText2, uiBytes2, bRevCompMates ? 1 : 0, pPairs, aConsumed );
        } );
        R.uiReads = 2 * nPairs;
        R.fH2D = secondsSince( t0 );
        t0 = runStages( R, bInversions );
        engineCheck( ma_batch_counts( pBatch, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &R.uiAlignedReads ) );
        fetchPairSam( R, uiSamOptions );
        endRun( R, t0, [ & ]( char* p, size_t c ) { snprintf( p, c, "%zu + %zu bytes of mate text, %llu pairs, h2d+parse", uiBytes1, uiBytes2, (unsigned long long)nPairs ); } );
        return pRes;
    }
    // runMatesText for a batch of two BGZF-compressed files: text i is aSide[ i ]'s head followed by what its members inflate to,
    // minus its last n_drop bytes (ma_batch_set_mates_bgzf).  The two texts need not hold equally many records: directly after
    // the set call succeeded -- once, also when the call ran twice for the capacity -- and before the stages, rOnRest gets what
    // of either text lies beyond the last pair (ma_batch_get_mates_rest): the front of the caller's next heads.  The member
    // headers are walked here as well, for the size of the texts the device batch is sized by.
    template <typename ON_REST>
    std::shared_ptr<BatchResult> runMatesBgzf( const ma_bgzf_text aSide[ 2 ], bool bRevCompMates, uint32_t uiSamOptions, bool bInversions, ON_REST&& rOnRest )
    {
        auto pRes = beginRun( false, true, true, uiSamOptions );
        BatchResult& R = *pRes;
        auto t0 = std::chrono::steady_clock::now( );
        size_t uiBytes = 0;
        for( int i = 0; i < 2; i++ )
        {
            ma_bgzf::Result xWalk;
            ma_bgzf::inflateHost( (const uint8_t*)aSide[ i ].members, aSide[ i ].n_bytes, nullptr, &xWalk ); // (a bad header: the library refuses it by name)
            uiBytes += aSide[ i ].n_head + xWalk.uiBytes - std::min<uint64_t>( aSide[ i ].n_drop, xWalk.uiBytes );
        }
        uint64_t aConsumed[ 2 ], aTextBytes[ 2 ];
        const uint64_t nPairs = setText( uiBytes, 2, [ & ]( uint64_t* pPairs ) {
            return ma_batch_set_mates_bgzf( pBatch, aSide, bRevCompMates ? 1 : 0, pPairs, aTextBytes, aConsumed );
        } );
        std::string asRest[ 2 ];
        for( int i = 0; i < 2; i++ )
        {
            uint64_t n = 0;
            engineCheck( ma_batch_get_mates_rest( pBatch, i, &n, nullptr ) );
            asRest[ i ].resize( n );
            if( n )
                engineCheck( ma_batch_get_mates_rest( pBatch, i, &n, &asRest[ i ][ 0 ] ) );
        }
        rOnRest( asRest[ 0 ], asRest[ 1 ] );
        R.uiReads = 2 * nPairs;
        R.fH2D = secondsSince( t0 );
        t0 = runStages( R, bInversions );
        engineCheck( ma_batch_counts( pBatch, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &R.uiAlignedReads ) );
        fetchPairSam( R, uiSamOptions );
        endRun( R, t0, [ & ]( char* p, size_t c ) { snprintf( p, c, "%zu bytes of compressed mate text, %llu pairs, h2d+inflate+parse", uiBytes, (unsigned long long)nPairs ); } );
        return pRes;
    }

  private:
    // uiBytes of text that rSet puts into pBatch (it returns the library's status and the reads it found)
    template <typename SET> std::shared_ptr<BatchResult> runTextBy( size_t uiBytes, uint32_t uiSamOptions, bool bInversions, SET&& rSet )
    {
        auto pRes = beginRun( false, false, true, uiSamOptions );
        BatchResult& R = *pRes;
        auto t0 = std::chrono::steady_clock::now( );
        R.uiReads = setText( uiBytes, 1, rSet );
        R.fH2D = secondsSince( t0 );
        t0 = runStages( R, bInversions );
        engineCheck( ma_batch_counts( pBatch, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &R.uiAlignedReads ) );
        fetchSam( R, uiSamOptions );
        endRun( R, t0, [ & ]( char* p, size_t c ) { snprintf( p, c, "%zu bytes of text, %llu reads, h2d+parse", uiBytes, (unsigned long long)R.uiReads ); } );
        return pRes;
    }

    // ---- the pieces of a run: beginRun, the form's input, runStages, the form's output (fetch...), endRun ----
    std::shared_ptr<BatchResult> beginRun( bool bStages, bool bPairs, bool bSam, uint32_t uiSamOptions )
    {
        auto pRes = freshResult( );
        BatchResult& R = *pRes;
        R.bStages = bStages, R.bPairs = bPairs, R.bSam = bSam;
        R.bSocQueues = false;
        R.uiSamOptions = uiSamOptions;
        R.uiSamBytes = 0;
        R.bSamBgzf = false;
        R.uiSamBgzfBytes = R.uiSamBgzfMembers = 0;
        R.fPack = 0;
        return pRes;
    }
    // rLead writes the front of the MA_ENGINE_TRACE line, up to and including the name of the first phase (h2d+parse: the upload of
    // a text, its parse and the parse's two read-backs)
    template <typename LEAD> void endRun( BatchResult& R, const std::chrono::steady_clock::time_point& tD2H, LEAD&& rLead )
    {
        R.fD2H = secondsSince( tD2H );
        uiRuns++;
        if( getenv( "MA_ENGINE_TRACE" ) ) // diagnostics: the phases of every device batch
        {
            char aLead[ 160 ];
            rLead( aLead, sizeof( aLead ) );
            fprintf( stderr, "engine %p: %s %.4f s, stages %.4f s (seed %.1f extract %.1f chain %.1f dp %.1f ms), d2h %.4f s\n", (void*)this, aLead,
                     R.fH2D, R.fKernels, R.aStageMs[ 0 ], R.aStageMs[ 1 ], R.aStageMs[ 2 ], R.aStageMs[ 3 ], R.fD2H );
        }
    }
    // A text form's input: the device batch sized by the text, then rSet, which returns the library's status and the count it
    // found (reads, or pairs: uiReadsPerCount reads each).  Only "batch capacity exceeded" fails WITH a count: the batch is then
    // made to hold it and rSet runs again; every other failure throws the library's message.
    template <typename SET> uint64_t setText( size_t uiBytes, uint64_t uiReadsPerCount, SET&& rSet )
    {
        fit( std::max<uint64_t>( uiCapReads, uiBytes / 32 ), std::max<uint64_t>( uiCapBases, uiBytes ) );
        uint64_t n = 0;
        if( rSet( &n ) != 0 )
        {
            if( n == 0 )
                engineCheck( 1 );
            fit( uiReadsPerCount * n, uiBytes );
            engineCheck( rSet( &n ) );
        }
        return n;
    }
    // the device stages of every form; returns the start of the download phase
    std::chrono::steady_clock::time_point runStages( BatchResult& R, bool bInversions )
    {
        const auto t0 = std::chrono::steady_clock::now( );
        engineCheck( ma_align_batch( pBatch ) );
        if( bInversions )
            engineCheck( ma_inversions_batch( pBatch ) );
        engineCheck( ma_batch_sync( pBatch ) );
        R.fKernels = secondsSince( t0 );
        engineCheck( ma_batch_host_ms( pBatch, R.aStageMs ) );
        return std::chrono::steady_clock::now( );
    }
    // no per-read records in this result (pairs, either text): a recycled result may hold old offsets
    void noMqRecords( BatchResult& R )
    {
        memset( R.vMqOff.need( R.uiReads + 1 ), 0, ( R.uiReads + 1 ) * sizeof( uint64_t ) );
        R.uiMqAlignments = R.uiMqOps = 0;
    }
    void fetchStageRecords( BatchResult& R, uint64_t nSeg, uint64_t nSeed, uint64_t nHset, uint64_t nHseed, uint64_t nAln, uint64_t nOps )
    {
        const size_t n = R.uiReads;
        R.vSegOff.resize( n + 1 );
        R.vSegs.resize( nSeg + 1 );
        engineCheck( ma_batch_get_segments( pBatch, R.vSegOff.data( ), R.vSegs.data( ) ) );
        R.vSeedOff.resize( n + 1 );
        R.vSeeds.resize( nSeed + 1 );
        engineCheck( ma_batch_get_seeds( pBatch, R.vSeedOff.data( ), R.vSeeds.data( ) ) );
        R.vHsetOff.resize( n + 1 );
        R.vHseedOff.resize( nHset + 1 );
        R.vHsetSoc.resize( nHset + 1 );
        R.vHseeds.resize( nHseed + 1 );
        engineCheck( ma_batch_get_hsets( pBatch, R.vHsetOff.data( ), R.vHseedOff.data( ), R.vHsetSoc.data( ), R.vHseeds.data( ) ) );
        if( bFetchSocQueues )
        {
            uint64_t nSocs = 0;
            engineCheck( ma_batch_get_soc_heap( pBatch, &nSocs, nullptr, nullptr, nullptr, nullptr ) );
            R.vSocOff.resize( n + 1 );
            R.vSocHeap.resize( nSocs + 1 );
            R.vSortedSeeds.resize( nSeed + 1 );
            std::vector<uint64_t> vSeedOffAgain( n + 1 );
            engineCheck( ma_batch_get_soc_heap( pBatch, &nSocs, R.vSocOff.data( ), R.vSocHeap.data( ), vSeedOffAgain.data( ),
                                                R.vSortedSeeds.data( ) ) );
            R.bSocQueues = true;
        }
        R.vAlnOff.resize( n + 1 );
        R.vAlns.resize( nAln + 1 );
        R.vAlnOps.resize( 2 * nOps + 2 );
        engineCheck( ma_batch_get_alignments( pBatch, R.vAlnOff.data( ), R.vAlns.data( ), R.vAlnOps.data( ) ) );
    }
    void fetchMqRecords( BatchResult& R, uint64_t nAln, uint64_t nOps )
    {
        uint64_t* pMqOff = R.vMqOff.need( R.uiReads + 1 );
        engineCheck( ma_batch_get_mapq_alignments( pBatch, pMqOff, R.vMq.need( nAln + 1 ), R.vMqOps.need( 2 * nOps + 2 ) ) );
        R.uiMqAlignments = R.uiReads ? pMqOff[ R.uiReads ] : 0;
        R.uiMqOps = 0;
        if( R.uiMqAlignments )
        {
            const ma_alignment& rLast = R.vMq[ R.uiMqAlignments - 1 ];
            R.uiMqOps = rLast.ops_off + rLast.n_ops;
        }
    }
    void fetchPairRecords( BatchResult& R )
    {
        uint64_t nPairs = 0;
        engineCheck( ma_pair_batch( pBatch ) );
        engineCheck( ma_batch_pair_counts( pBatch, &nPairs, &R.uiPairRecords, &R.uiPairOps, &R.uiPairsOnHost ) );
        engineCheck( ma_batch_get_pairs( pBatch, R.vPairOff.need( nPairs + 1 ), R.vPair.need( R.uiPairRecords + 1 ),
                                         R.vPairOps.need( 2 * R.uiPairOps + 2 ), R.vPairMate.need( R.uiPairRecords + 1 ),
                                         R.vPairOther.need( R.uiPairRecords + 1 ) ) );
        noMqRecords( R );
    }
    // the text replaces the record download: ma_sam_batch waits once for the size, then one copy of offsets + bytes
    void fetchSam( BatchResult& R, uint32_t uiSamOptions )
    {
        engineCheck( ma_sam_batch( pBatch, uiSamOptions & ~SAM_AS_BGZF ) );
        engineCheck( ma_batch_sam_counts( pBatch, &R.uiSamBytes ) );
        if( uiSamOptions & SAM_AS_BGZF )
            fetchSamBgzf( R, 0 );
        else
            engineCheck( ma_batch_get_sam( pBatch, R.vSamOff.need( R.uiReads + 1 ), R.vSam.need( R.uiSamBytes + 1 ) ) );
        noMqRecords( R );
    }
    // the text deflated where it is: only its members come down
    void fetchSamBgzf( BatchResult& R, int32_t iPair )
    {
        if( &ma_sam_bgzf_batch == nullptr || &ma_batch_sam_bgzf_counts == nullptr || &ma_batch_get_sam_bgzf == nullptr )
            throw std::runtime_error( "Engine: SAM_AS_BGZF without ma_sam_bgzf_batch in the library" );
        engineCheck( ma_sam_bgzf_batch( pBatch, iPair ) );
        engineCheck( ma_batch_sam_bgzf_counts( pBatch, iPair, &R.uiSamBgzfMembers, &R.uiSamBgzfBytes ) );
        engineCheck( ma_batch_get_sam_bgzf( pBatch, iPair, nullptr, R.vSamBgzf.need( R.uiSamBgzfBytes + 1 ) ) );
        R.bSamBgzf = true;
    }
    // pairing and formatting behind the alignment: the text replaces the download of records, ops, mate and other
    void fetchPairSam( BatchResult& R, uint32_t uiSamOptions )
    {
        uint64_t nPairs = 0;
        R.uiPairRecords = R.uiPairOps = 0;
        engineCheck( ma_pair_batch( pBatch ) );
        engineCheck( ma_batch_pair_counts( pBatch, &nPairs, nullptr, nullptr, &R.uiPairsOnHost ) );
        engineCheck( ma_pair_sam_batch( pBatch, uiSamOptions & ~SAM_AS_BGZF ) );
        engineCheck( ma_batch_pair_sam_counts( pBatch, &nPairs, &R.uiSamBytes ) );
        if( uiSamOptions & SAM_AS_BGZF )
            fetchSamBgzf( R, 1 );
        else
            engineCheck( ma_batch_get_pair_sam( pBatch, R.vSamOff.need( nPairs + 1 ), R.vSam.need( R.uiSamBytes + 1 ) ) );
        memset( R.vPairOff.need( nPairs + 1 ), 0, ( nPairs + 1 ) * sizeof( uint64_t ) ); // no pair records either (a recycled result)
        noMqRecords( R );
    }
};

// One read's place in a finished device batch.
struct Ticket
{
    std::shared_ptr<const BatchResult> pResult;
    size_t uiRead = 0;
    explicit operator bool( ) const
    {
        return pResult != nullptr;
    }
};

struct BatcherOptions
{
    size_t uiMaxBatch = 1u << 18; // reads per device batch at most
    size_t uiEngines = 2; // device batches in flight (own stream each).  Measured with 2048 graph threads: 2 -> 109 k reads/s, 4 -> 63 k: with
                          // an engine always free a batch is sealed after xGather, while it is small, and small batches pay the fixed cost
    std::chrono::microseconds xGather{ 40 }; // an idle GPU still waits this long for more reads to arrive
    std::chrono::microseconds xMaxWait{ 20000 }; // a read never waits longer than this for its batch to be sealed
    std::chrono::microseconds xFill{ 3000 }; // while another batch runs, a batch smaller than half the last one waits this long for more
    // true: every stage's records are fetched, so SegmentVector / SoCPriorityQueue / seed sets / NeedlemanWunsch's
    // alignments carry their content (what a graph needs whose nodes are not all MI355X modules).  false: only the
    // MappingQuality-annotated alignments are fetched; the intermediate containers are empty shells that just pass the
    // ticket on -- enough for the chain of export.cpp:104-108 and several times cheaper per read.
    bool bStages = true;
    // with bStages: also fetch every read's SoC queue (needed by bindings whose SoCPriorityQueue is the reference's own
    // type and must therefore be filled eagerly; the mirror types of ma_modules.h compute it on demand)
    bool bSocQueues = false;
    // bases per read the engines' device pools are sized for when the batcher is constructed (a funnel batch holds at most
    // min( uiMaxBatch, 4096 ) reads); a long-read graph sets its expected read length
    size_t uiReserveBasesPerRead = 512;
};

// One-shot gate many threads sleep at until it opens.  A condition variable makes every woken thread re-acquire the mutex it
// waited with: the ~600 graph threads of one device batch then leave one by one (and fight the threads that are entering the
// next batch for the same mutex) -- measured as ~45 ms per cycle of a graph thread, against 5 ms on the GPU.  A futex wakes
// them all at once and none of them needs a lock afterwards.
class Gate
{
    std::atomic<int> iOpen{ 0 };

  public:
    void wait( )
    {
        while( iOpen.load( std::memory_order_acquire ) == 0 )
            syscall( SYS_futex, reinterpret_cast<int*>( &iOpen ), FUTEX_WAIT_PRIVATE, 0, nullptr, nullptr, 0 );
    }
    void open( )
    {
        iOpen.store( 1, std::memory_order_release );
        syscall( SYS_futex, reinterpret_cast<int*>( &iOpen ), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0 );
    }
};

class DeviceBatcher
{
    struct Slot
    {
        std::vector<ReadRef> vReads;
        std::shared_ptr<const BatchResult> pResult;
        std::string sError;
        bool bSealed = false;
        Gate xDone; // only this batch's readers wait here: a finished batch wakes nobody else
    };
    const ma_index* pIndex;
    const ma_params xP;
    const BatcherOptions xOpt;
    std::mutex xMutex;
    std::condition_variable xChanged;
    std::shared_ptr<Slot> pOpen;
    std::vector<std::unique_ptr<Engine>> vIdle; // engines not running a batch
    size_t uiEnginesMade = 0, uiRunning = 0, uiLastSealed = 0;
    uint64_t uiBatches = 0, uiReadsTotal = 0;
    double fSumH2D = 0, fSumKernels = 0, fSumD2H = 0, fSumRun = 0; // seconds over all batches
    double aSumStageMs[ 4 ] = { 0, 0, 0, 0 };

    // called with the lock held by the thread that sealed the slot; releases the lock while the GPU works
    void runSealed( std::unique_lock<std::mutex>& rLock, const std::shared_ptr<Slot>& pSlot )
    {
        xChanged.wait( rLock, [ & ]( ) { return !vIdle.empty( ) || uiEnginesMade < xOpt.uiEngines; } );
        std::unique_ptr<Engine> pEngine;
        if( !vIdle.empty( ) )
        {
            pEngine = std::move( vIdle.back( ) );
            vIdle.pop_back( );
        }
        else
            uiEnginesMade++; // constructed below, outside the lock
        uiRunning++;
        rLock.unlock( );
        const auto tRun = std::chrono::steady_clock::now( );
        try
        {
            if( pEngine == nullptr )
            {
                pEngine.reset( new Engine( pIndex, xP, true ) );
                pEngine->bFetchSocQueues = xOpt.bSocQueues;
            }
            pSlot->pResult = pEngine->run( pSlot->vReads, xOpt.bStages );
        }
        catch( const std::exception& rE )
        {
            pSlot->sError = rE.what( );
            if( pSlot->sError.empty( ) )
                pSlot->sError = "device batch failed";
        }
        rLock.lock( );
        if( pEngine != nullptr )
            vIdle.push_back( std::move( pEngine ) );
        else
            uiEnginesMade--;
        uiRunning--;
        uiBatches++;
        uiReadsTotal += pSlot->vReads.size( );
        fSumRun += secondsSince( tRun );
        if( pSlot->pResult != nullptr )
        {
            fSumH2D += pSlot->pResult->fH2D, fSumKernels += pSlot->pResult->fKernels, fSumD2H += pSlot->pResult->fD2H;
            for( int k = 0; k < 4; k++ )
                aSumStageMs[ k ] += pSlot->pResult->aStageMs[ k ];
        }
        xChanged.notify_all( ); // leaders of open batches and sealers waiting for a device slot
        pSlot->xDone.open( ); // result and error of the slot are published by the release store inside
    }

  public:
    // Engines before admission: all uiEngines engines (stream + device batch sized for the batches a funnel sees) exist when
    // the constructor returns; none is created while reads are being aligned.  Constructing a batcher therefore allocates
    // device memory and streams even if no read ever arrives (the per-read modules construct theirs on the first execute( ) of a
    // graph thread, BinarySeeding::batcherFor); a device that is short of memory fails HERE, with a message that says so.
    DeviceBatcher( const ma_index* pIndex, const ma_params& rP, const BatcherOptions& rOpt = BatcherOptions( ) )
        : pIndex( pIndex ), xP( rP ), xOpt( rOpt )
    {
        const uint64_t uiReads = std::min<uint64_t>( std::max<uint64_t>( xOpt.uiMaxBatch, 1 ), 4096 );
        for( size_t k = 0; k < xOpt.uiEngines; k++ )
        {
            try
            {
                std::unique_ptr<Engine> pEngine( new Engine( pIndex, xP, true ) );
                pEngine->bFetchSocQueues = xOpt.bSocQueues;
                pEngine->reserve( uiReads, uiReads * std::max<size_t>( xOpt.uiReserveBasesPerRead, 1 ) );
                vIdle.push_back( std::move( pEngine ) );
                uiEnginesMade++;
            }
            catch( const std::exception& rE )
            {
                throw std::runtime_error( "DeviceBatcher: engine " + std::to_string( k ) + " of " + std::to_string( xOpt.uiEngines ) + " (" +
                                          std::to_string( uiReads ) + " reads x " + std::to_string( xOpt.uiReserveBasesPerRead ) +
                                          " bases): " + rE.what( ) );
            }
        }
    }
    DeviceBatcher( const DeviceBatcher& ) = delete;

    // Blocks until the batch that contains this read has been through all stages.  rCodes must stay alive meanwhile
    // (the caller holds the NucSeq).  Re-entrant: called concurrently by all graph threads.
    Ticket align( const std::vector<uint8_t>& rCodes )
    {
        return align( ReadRef( rCodes ) );
    }
    Ticket align( const ReadRef& rRead )
    {
        std::unique_lock<std::mutex> xLock( xMutex );
        if( pOpen == nullptr )
            pOpen = std::make_shared<Slot>( );
        std::shared_ptr<Slot> pSlot = pOpen;
        const size_t uiMine = pSlot->vReads.size( );
        pSlot->vReads.push_back( rRead );
        auto seal = [ & ]( ) {
            pSlot->bSealed = true;
            uiLastSealed = pSlot->vReads.size( );
            if( pOpen == pSlot )
                pOpen = nullptr;
        };
        if( pSlot->vReads.size( ) >= xOpt.uiMaxBatch )
        {
            seal( );
            runSealed( xLock, pSlot );
        }
        else if( uiMine == 0 )
        {
            // the first read of a batch leads it: it seals the batch once a device slot is free and the arrivals have had
            // a moment to gather (while all device slots are busy the batch simply keeps growing), or after xMaxWait
            // While ANOTHER batch is on the device a free engine is no reason to leave with a handful of reads: the readers of
            // the batch that just finished are only now coming back, and a batch of 30 reads costs the same ~4 ms as one of 600
            // (measured: the batches alternated between ~1100 and ~40 reads, and less than one of them was in flight on average).
            // Such a batch waits until it holds half of what the last sealed batch held, or xFill.
            const auto tOpened = std::chrono::steady_clock::now( );
            while( !pSlot->bSealed )
            {
                const auto tNow = std::chrono::steady_clock::now( );
                const bool bGathered = tNow - tOpened >= xOpt.xGather;
                const bool bFilled = uiRunning == 0 || pSlot->vReads.size( ) >= uiLastSealed / 2 || tNow - tOpened >= xOpt.xFill;
                if( ( bGathered && bFilled && uiRunning < xOpt.uiEngines ) || tNow - tOpened >= xOpt.xMaxWait )
                    break;
                xChanged.wait_for( xLock, bGathered ? std::chrono::microseconds( 200 ) : xOpt.xGather );
            }
            if( !pSlot->bSealed )
            {
                seal( );
                runSealed( xLock, pSlot );
            }
        }
        xLock.unlock( );
        pSlot->xDone.wait( );
        if( !pSlot->sError.empty( ) )
            throw std::runtime_error( pSlot->sError );
        Ticket xT;
        xT.pResult = pSlot->pResult;
        xT.uiRead = uiMine;
        return xT;
    }

    // statistics: device batches run so far, reads they carried
    void stats( uint64_t& rBatches, uint64_t& rReads )
    {
        std::lock_guard<std::mutex> xLock( xMutex );
        rBatches = uiBatches;
        rReads = uiReadsTotal;
    }
    // seconds summed over all device batches: whole run() calls, and inside them upload / kernels / download
    void phaseSeconds( double& rRun, double& rH2D, double& rKernels, double& rD2H )
    {
        std::lock_guard<std::mutex> xLock( xMutex );
        rRun = fSumRun, rH2D = fSumH2D, rKernels = fSumKernels, rD2H = fSumD2H;
    }
    void stageSeconds( double aOut[ 4 ] ) // host wall time of the four stage calls, summed over all batches
    {
        std::lock_guard<std::mutex> xLock( xMutex );
        for( int k = 0; k < 4; k++ )
            aOut[ k ] = aSumStageMs[ k ] / 1e3;
    }
};

struct PrefetchOptions
{
    size_t uiBatchReads = 1u << 16; // reads per device batch pulled ahead
    size_t uiDepth = 2; // device batches ahead of the graph threads (in flight or finished and not yet handed out): one engine each
    // reads of a finished batch a graph thread takes at a time: the queue's lock is taken once per slice, not once per read
    // (with more graph threads than the host grants cores, a thread that is descheduled while it holds a lock stalls them all)
    size_t uiSlice = 128;
    bool bStages = false, bSocQueues = false; // as in BatcherOptions
    // bases per read the engines' device pools and staging arrays are sized for up front (short reads: 256; a long-read graph
    // sets its expected read length, otherwise the first batch re-allocates inside the run)
    size_t uiReserveBasesPerRead = 256;
};

// Reads pulled AHEAD of the graph threads.  TP_ITEM is the read handle of the host layer (shared_ptr to its NucSeq type).
//   next( out, pull, ref ): the next read of a finished device batch with its ticket; false = the source is exhausted and
//   everything pulled has been handed out.  `pull` returns the next read of the wrapped source or an empty handle at its
//   end; it is called by ONE thread at a time (the wrapped reader need not be re-entrant).  A caller that finds fewer than
//   uiDepth batches ahead pulls and runs the next batch itself (it blocks for one device batch, the others keep being
//   served from the finished ones), so there is no thread of our own and nothing runs when nobody asks.
// The reads a batch pulled stay with the batch until its last slice is done and are then released together by ONE thread: the
// host layer hands the graph threads COPIES (made, and later freed, by the consuming thread).  Handing out the pulled objects
// themselves was measured at a third of the rate: they are allocated by the thread that pulled the batch and would be freed
// by 8-16 others, all contending for that one thread's malloc arena (13.4 vs 5.1 us of thread time per read).
// Order: reads are handed out batch by batch in pull order, within a batch in pull order; which graph thread gets which
// read is as arbitrary as in the reference (every graph thread takes the next read from the shared reader, export.cpp:99-126).
// TP_ENGINE: Engine; the CPU test of the queue's bookkeeping (tests/emul/prefetch_queue_test.cpp) puts a stand-in there.
template <typename TP_ITEM, typename TP_ENGINE = Engine> class PrefetchQueue
{
    struct Batch
    {
        std::vector<TP_ITEM> vItems;
        std::shared_ptr<const BatchResult> pResult;
        size_t uiNext = 0;
    };
    const ma_params xP;
    const PrefetchOptions xOpt;
    std::mutex xMutex; // state below
    std::condition_variable xChanged;
    std::vector<std::shared_ptr<Batch>> vReady; // finished batches, oldest first
    // engines not running a batch.  With several index replicas (one per GPU of the node) every replica has uiDepth
    // engines of its own and the device batches rotate over them: whoever pulls the next batch takes the engine that has been
    // idle longest, so G GPUs are fed by the unchanged graph of export.cpp:99-126 -- tickets carry their batch's result, the
    // modules downstream never ask which device computed it
    std::vector<std::unique_ptr<TP_ENGINE>> vIdle;
    size_t uiDepthTotal = 1; // uiDepth per replica
    size_t uiLoading = 0; // batches being pulled or on the device
    bool bEof = false;
    std::string sError;
    std::mutex xPullMutex; // the wrapped source is read by one thread at a time, batches are pulled in order
    bool bSourceEnded = false; // (under xPullMutex) the source has returned its end marker: it is not asked again
    // what a thread's unfinished slice checks before it touches its queue's batch: a queue that was destroyed (an aborted
    // graph) leaves stale slices behind in the threads that served it; they are dropped the next time the thread looks
    const std::shared_ptr<int> pAlive = std::make_shared<int>( 0 );
    static uint64_t nextId( )
    {
        static std::atomic<uint64_t> uiNext{ 1 };
        return uiNext++;
    }
    const uint64_t uiId = nextId( ); // what a thread's slice remembers of its queue
    uint64_t uiBatches = 0, uiReadsTotal = 0;
    double fSumRun = 0, fSumPull = 0;

  public:
    // Constructing a queue creates uiDepth engines per index replica -- a stream, device pools for uiBatchReads reads of
    // uiReserveBasesPerRead bases (GBs for long reads) and page-locked staging each: before the first read is asked for, not
    // inside the first timed batch.  A device that is short of memory makes the constructor throw (with the replica's number).
    PrefetchQueue( const std::vector<const ma_index*>& vIndices, const ma_params& rP, const PrefetchOptions& rOpt = PrefetchOptions( ) )
        : xP( rP ), xOpt( rOpt )
    {
        if( vIndices.empty( ) )
            throw std::runtime_error( "PrefetchQueue: no index" );
        uiDepthTotal = std::max<size_t>( xOpt.uiDepth, 1 ) * vIndices.size( );
        // round k holds the k-th engine of every replica: vIdle is served from its front, so consecutive batches go to
        // different devices
        for( size_t k = 0; k < std::max<size_t>( xOpt.uiDepth, 1 ); k++ )
            for( size_t g = 0; g < vIndices.size( ); g++ )
            {
                try
                {
                    std::unique_ptr<TP_ENGINE> pEngine( new TP_ENGINE( vIndices[ g ], xP, true ) );
                    pEngine->bFetchSocQueues = xOpt.bSocQueues;
                    pEngine->reserve( xOpt.uiBatchReads, xOpt.uiBatchReads * std::max<size_t>( xOpt.uiReserveBasesPerRead, 1 ) );
                    vIdle.push_back( std::move( pEngine ) );
                }
                catch( const std::exception& rE )
                {
                    throw std::runtime_error( "PrefetchQueue: engine " + std::to_string( k ) + " of index replica " + std::to_string( g ) +
                                              " (" + std::to_string( xOpt.uiBatchReads ) + " reads x " +
                                              std::to_string( xOpt.uiReserveBasesPerRead ) + " bases): " + rE.what( ) );
                }
            }
    }
    PrefetchQueue( const ma_index* pIndex, const ma_params& rP, const PrefetchOptions& rOpt = PrefetchOptions( ) )
        : PrefetchQueue( std::vector<const ma_index*>( 1, pIndex ), rP, rOpt )
    {}
    PrefetchQueue( const PrefetchQueue& ) = delete;

    // the calling thread's slice of a finished batch (thread-local: no lock while it lasts)
    struct Slice
    {
        uint64_t uiOwner = 0; // id of the queue the slice belongs to (not its address: a later queue may be allocated there)
        std::weak_ptr<int> pOwnerAlive;
        std::shared_ptr<Batch> pBatch;
        // the batch's result behind a control block of THIS thread's own: the tickets of a slice are copied a dozen times per
        // read (query -> segments -> ... -> alignments), and reference counts that 16 threads keep bumping on ONE control
        // block bounce its cache line between the cores (measured: half of a graph thread's time per read)
        std::shared_ptr<const BatchResult> pResult;
        size_t uiNext = 0, uiEnd = 0;
        void take( const std::shared_ptr<Batch>& pB, size_t uiFrom, size_t uiTo, uint64_t uiQueue, const std::shared_ptr<int>& pAliveOfQueue )
        {
            uiOwner = uiQueue, pOwnerAlive = pAliveOfQueue, pBatch = pB, uiNext = uiFrom, uiEnd = uiTo;
            std::shared_ptr<const BatchResult> pKeep = pB->pResult;
            pResult = std::shared_ptr<const BatchResult>( pKeep.get( ), [ pKeep ]( const BatchResult* ) {} );
        }
        void drop( )
        {
            pBatch.reset( );
            pResult.reset( );
            uiNext = uiEnd = 0;
        }
        bool empty( ) const
        {
            return uiNext >= uiEnd;
        }
    };
    // One slice PER QUEUE the thread serves: a graph thread that alternates between two PrefetchReaders -- two
    // wrapped files, two aligners in one process -- keeps its unfinished slice of queue A while it takes reads of queue B; with
    // one slice per thread the reads of A's slice, already taken out of A's batch, were lost.  Finished slices and slices of
    // queues that no longer exist are removed on the way.
    static Slice& mySlice( uint64_t uiQueue )
    {
        static thread_local std::vector<Slice> vSlices;
        Slice* pFound = nullptr;
        for( size_t k = 0; k < vSlices.size( ); )
        {
            if( vSlices[ k ].uiOwner == uiQueue )
                pFound = &vSlices[ k ];
            else if( vSlices[ k ].empty( ) || vSlices[ k ].pOwnerAlive.expired( ) )
            {
                if( pFound == &vSlices.back( ) )
                    pFound = &vSlices[ k ];
                vSlices[ k ] = std::move( vSlices.back( ) );
                vSlices.pop_back( );
                continue;
            }
            k++;
        }
        if( pFound != nullptr )
            return *pFound;
        vSlices.emplace_back( );
        vSlices.back( ).uiOwner = uiQueue;
        return vSlices.back( );
    }

    template <typename TP_PULL, typename TP_REF> bool next( TP_ITEM& rItem, Ticket& rTicket, TP_PULL&& fPull, TP_REF&& fRef )
    {
        Slice& rMine = mySlice( uiId );
        if( rMine.uiNext < rMine.uiEnd )
        {
            const size_t k = rMine.uiNext++;
            rItem = rMine.pBatch->vItems[ k ];
            rTicket.pResult = rMine.pResult;
            rTicket.uiRead = k;
            if( rMine.uiNext >= rMine.uiEnd )
                rMine.drop( );
            return true;
        }
        std::unique_lock<std::mutex> xLock( xMutex );
        for( ;; )
        {
            if( !sError.empty( ) )
                throw std::runtime_error( sError );
            // keep uiDepth batches ahead: this caller pulls and runs the next one, the others are served meanwhile
            if( !bEof && uiLoading + vReady.size( ) < uiDepthTotal && !vIdle.empty( ) )
            {
                uiLoading++;
                std::unique_ptr<TP_ENGINE> pEngine = std::move( vIdle.front( ) ); // idle longest: batches rotate over the replicas
                vIdle.erase( vIdle.begin( ) );
                xLock.unlock( );
                auto pBatch = std::make_shared<Batch>( );
                std::string sFailed;
                bool bEnd = false;
                const auto tPull = std::chrono::steady_clock::now( );
                double fPullS = 0, fRun = 0;
                try
                {
                    {
                        std::lock_guard<std::mutex> xPull( xPullMutex );
                        // a source that has ended is not asked again (it need not be idempotent at its end): a second puller
                        // may have been waiting for this lock while the first one met the end
                        bEnd = bSourceEnded;
                        if( !bEnd )
                            pBatch->vItems.reserve( xOpt.uiBatchReads );
                        while( !bEnd && pBatch->vItems.size( ) < xOpt.uiBatchReads )
                        {
                            TP_ITEM xItem = fPull( );
                            if( !xItem )
                                bEnd = bSourceEnded = true;
                            else
                                pBatch->vItems.push_back( std::move( xItem ) );
                        }
                    }
                    fPullS = secondsSince( tPull );
                    if( !pBatch->vItems.empty( ) )
                    {
                        const auto tRun = std::chrono::steady_clock::now( );
                        std::vector<ReadRef> vRefs;
                        vRefs.reserve( pBatch->vItems.size( ) );
                        for( const TP_ITEM& rI : pBatch->vItems )
                            vRefs.push_back( fRef( rI ) );
                        pBatch->pResult = pEngine->run( vRefs, xOpt.bStages );
                        fRun = secondsSince( tRun );
                    }
                }
                catch( const std::exception& rE )
                {
                    sFailed = rE.what( );
                    if( sFailed.empty( ) )
                        sFailed = "device batch failed";
                }
                catch( ... ) // whatever the wrapped source throws: the queue's state is restored and every waiter sees the failure
                {
                    sFailed = "PrefetchQueue: the wrapped source or the device batch threw an exception that is not a std::exception";
                }
                xLock.lock( );
                vIdle.push_back( std::move( pEngine ) );
                uiLoading--;
                if( bEnd )
                    bEof = true;
                if( !sFailed.empty( ) )
                {
                    bEof = true;
                    if( sError.empty( ) )
                        sError = sFailed;
                }
                else if( !pBatch->vItems.empty( ) )
                {
                    // (with several batches ahead they may finish, and are handed out, in another order than they were pulled)
                    vReady.push_back( pBatch );
                    uiBatches++, uiReadsTotal += pBatch->vItems.size( );
                    fSumRun += fRun, fSumPull += fPullS;
                }
                xChanged.notify_all( );
                continue;
            }
            if( !vReady.empty( ) )
            {
                std::shared_ptr<Batch> pB = vReady.front( );
                const size_t k = pB->uiNext;
                pB->uiNext = std::min( pB->vItems.size( ), k + std::max<size_t>( xOpt.uiSlice, 1 ) );
                const size_t uiEnd = pB->uiNext;
                if( pB->uiNext >= pB->vItems.size( ) )
                {
                    vReady.erase( vReady.begin( ) );
                    xChanged.notify_all( ); // room for another batch ahead
                }
                xLock.unlock( );
                rMine.take( pB, k + 1, uiEnd, uiId, pAlive );
                rItem = pB->vItems[ k ];
                rTicket.pResult = rMine.pResult;
                rTicket.uiRead = k;
                if( rMine.uiNext >= rMine.uiEnd )
                    rMine.drop( );
                return true;
            }
            if( bEof && uiLoading == 0 )
                return false;
            xChanged.wait( xLock );
        }
    }
    void stats( uint64_t& rBatches, uint64_t& rReads, double& rRunSeconds, double& rPullSeconds )
    {
        std::lock_guard<std::mutex> xLock( xMutex );
        rBatches = uiBatches, rReads = uiReadsTotal, rRunSeconds = fSumRun, rPullSeconds = fSumPull;
    }
};
} // namespace engine
} // namespace ma_amd
