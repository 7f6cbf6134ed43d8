// pipeline.hip -- the batch pipeline behind the C ABI: BinarySeeding -> ExtractSeeds -> SoC sweep +
// Harmonization -> NeedlemanWunsch (job enumeration, batched ksw, stitch) -> MappingQuality, wired as in
// libMA::setUpCompGraph (libs/ma/src/util/export.cpp:104-108) but over a whole batch of reads resident
// in HBM.  Every stage is a HIP kernel; there is no host fallback.
#include "chain.h"
#include "wave_sort.h"
#include "ksw_launch.h"
#include "nw.h"
#include "seeding.h"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstring>
#include <chrono>
#include <memory>
#include <mutex>

using namespace ma;

// ------------------------------------------------------------------------------------------------
// device-side counters of a batch
// ------------------------------------------------------------------------------------------------
enum : int
{
    CTR_SEG_USED = 0, // segment pool bump pointer
    CTR_NEXT_READ = 1, // seeding read queue
    CTR_STEPS = 2, // extend_backward steps
    CTR_BLOCKS = 3, // distinct occ blocks touched
    CTR_LF_STEPS = 4,
    CTR_SA_ROWS = 5,
    CTR_HSEED_USED = 6, // harmonized seed pool bump pointer
    CTR_ERR = 7,
    CTR_CIG_USED = 8,
    CTR_CELLS = 9,
    CTR_KSW_JOBS = 10,
    CTR_NEXT_SLOT = 11,
    CTR_MAX_STATE = 12, // ksw sizing (atomicMax)
    CTR_MAX_H = 13,
    CTR_MAX_P = 14,
    CTR_MAX_CIG = 15,
    CTR_N_JOBS = 16,
    CTR_N_ALIGNED = 17,
    CTR_SEQ_BYTES = 18, // sum of qlen+tlen over DP jobs
    CTR_PATH_BYTES = 19, // back-trace steps (direction bytes read back)
    CTR_CLS0 = 20, // DP jobs per kernel class (KSW_N_CLASSES consecutive words, indexed by KSW_CLS_*)
    CTR_MAX_QLEN = CTR_CLS0 + KSW_N_CLASSES,
    CTR_NEXT_SLOTS, // KSW_N_NEXT x u32 job queues / list counters of the ksw launches (ksw_run_all: `next`, KSW_NX_*)
    CTR_N_REDO = CTR_NEXT_SLOTS + KSW_N_NEXT / 2, // u32: jobs the extension kernels (and the band of 120) handed back
    CTR_CIG_WORDS, // cigar words written (CTR_CIG_USED counts pool words reserved)
    CTR_NEXT_SEED, // queue of k_lf_walk
    CTR_OPS_ALL, // alignment ops of all alignments / of the MappingQuality selection (exact sizes of the downloads)
    CTR_OPS_MQ,
    CTR_ALN_MQ, // alignments MappingQuality keeps
    CTR_MAX_PC0, // per kernel class: largest direction-byte scratch of a job (KSW_N_CLASSES words) ...
    CTR_MAX_CIGC0 = CTR_MAX_PC0 + KSW_N_CLASSES, // ... and largest cigar scratch in words (KSW_N_CLASSES words)
    CTR_MAX_P_REDO = CTR_MAX_CIGC0 + KSW_N_CLASSES, // the same two for the extension kernels' jobs if they are handed back to the exact kernel
    CTR_MAX_CIG_REDO,
    CTR_NEXT_BIG, // KSW_N_NEXT_BIG x u32 job queues of the second (few waves, large scratch) launch of a class
    CTR_N_1X1 = CTR_NEXT_BIG + KSW_N_NEXT_BIG / 2, // 1 x 1 gap fills answered by k_dp_enum itself (counted as ksw calls of one cell each)
    CTR_MAX_BANDL, // largest min(qlen, tlen) of the long jobs on the band of 120 (scratch rows of their launch)
    CTR_PAIR_RECS, // ma_pair_batch: records / ops of the picked pairs (exact sizes of the pair download) ...
    CTR_PAIR_OPS,
    CTR_PAIR_OVER, // ... pairs k_pair_pick left to the host, pairs without any candidate (stage_pair.h)
    CTR_PAIR_ERR,
    CTR_COUNT
};
static_assert( CTR_COUNT == 96 && KSW_N_NEXT % 2 == 0 && KSW_N_NEXT_BIG % 2 == 0, "the counter block is 96 words; the u32 queues fill whole words" );

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
#include "stage_seed.h"

#include "stage_extract.h"

#include "stage_chain.h"

#include "stage_dp.h"

#include "stage_output.h"

#include "../host/ma_pair_flat.h"
#include "stage_pair.h"

#include "../host/ma_sam_dev.h"
#include "stage_sam.h"
#include "stage_pair_sam.h"

#include "../host/ma_inv_dev.h"
#include "stage_inv.h"

#include "../host/ma_text_dev.h"
#include "stage_text.h"
#include "../host/ma_genome_dev.h"
#include "stage_genome.h"

#include "../host/ma_bgzf_dev.h"
#include "stage_bgzf.h"
// the device deflate of the SAM texts into BGZF members: ma_sam_bgzf_batch (launch_deflate.h)
#include "../host/ma_deflate_dev.h"
#include "stage_deflate.h"
// what of a batch is valid, and what a call takes away (every entry point: drop on entry, finish on success)
#include "../host/ma_batch_state.h"
#include "../host/ma_seed_contract.h"

// ------------------------------------------------------------------------------------------------
// batch object
// ------------------------------------------------------------------------------------------------
// One SAM text of a batch (launch_sam.h): per item -- a read, or a pair -- the bytes of its records and their scan, where SEQ
// of every record goes, the text, the statistics of the one read-back (SAM_STAT_*)
// What a deflate needs beside the text (launch_deflate.h), sized by the members (slots, sizes, flags) and by the grid (tokens),
// and the members of one text: their offsets (members + 1) and their bytes
struct DeflateBufs
{
    DevBuf tokens, slots, sizes, flags, cub;
};
struct DeflateMembers
{
    DevBuf off, bytes;
};
// z: the text's BGZF members (ma_sam_bgzf_batch).  id: the text's product in the batch's state (ma_state::SAM or PAIR_SAM), where
// its validity, its bytes and the members' counts are
struct SamTextState
{
    const ma_state::Product id;
    DevBuf cnt, off, seqPos, text, stat;
    DeflateMembers z;
};

struct ma_batch
{
    const ma_index* idx = nullptr;
    int device = 0; // the index's device: every entry point binds the calling thread to it
    ma_params P;
    hipStream_t stream = nullptr;
    u64 max_reads = 0, max_bases = 0;
    u64 n_reads = 0, n_bases = 0;
    u32 max_qlen = 0;
    bool reads_external = false;
    const uint8_t* d_reads = nullptr;
    const u64* d_roff = nullptr;
    DevBuf reads, roff, ctr, seedStack, seedRow, seedSteps, seedSeg, hlocal, hdense, hseedCnt, hseedOff;
    // seeding
    DevBuf stage, smemA, smemB, segPool, segRead, segOff, segCnt, memsCnt, memsOff;
    DevBuf taskA, taskB, taskCnt, taskKey, taskKey2, taskPerm, taskPerm2, taskStage; // (taskStage: per-lane segments of an SMEM task) // area tasks of long reads (seed_tasks)
    u64 segPoolCap = 0, segPoolMin = 0;
    // extraction
    DevBuf segSeedCnt, segSeedOff, seedOff, seedCnt, seeds, cubTmp;
    // chaining
    DevBuf cWork, cMax, cMm, cA, cB, cOut, cSh1, cSh2, cVx, cVy, cMed, cInl, cBest, hpool, setTab, nsets, hsetOff,
        hsetFlat, hsetRead;
    u64 hpoolCap = 0;
    DevBuf socIn, socInCnt; // SoC queues swept elsewhere (ma_batch_set_soc_heap), carved by seed offset
    DevBuf preNmx, preSorted; // long reads: strips per read after k_soc_windows, which sorts k_sort_seeds_wave did
    DevBuf cPack, cList; // short reads: the thirteen scratch arrays as one block per read; the reads with two or more seeds
    DevBuf cRng; // the first draws of the RANSAC generator (ChainParams::rng_tab), uploaded once per srand seed from rngTabHost
    u32 rngTabHost[ MA_RNG_TAB_WORDS( MA_RNG_TAB ) ];
    u32 rngTabSeed = 0;
    bool rngTabValid = false;
    // dp
    DevBuf jobs, info, ez, cigOff, cigPool, kswScratch, clsLists, opsCap, opsOff, ops, hdr, order, mqOrder, mqCnt;
    DevBuf outCnt, outOps, outAlnOff, outOpsOff, outAlns, outOpsPairs; // packed results (get_alns)
    DevBuf sortKey, sortKey2, sortVal2; // longest-job-first order of the DP job lists
    // pairing (ma_pair_batch): per pair its pick and sizes, the pairs left to the host and their round trip, the packed columns
    DevBuf pairPick, pairCnt, pairOps, pairOver, pairHostOff, pairHostLists, pairHostPick, pairMate, pairOther;
    // SAM text: the reads' names and qualities (ma_batch_set_read_text; dropped when reads are set), the single-end text per
    // read (ma_sam_batch) and the paired-end text per pair (ma_pair_sam_batch), each all of its own: one never touches the other
    DevBuf txtNames, txtNameOff, txtQual;
    // read text parsed on the device (ma_batch_set_reads_text, launch_text.h), reserved on first use: the text, the statistics of
    // the call, line feeds per workgroup, and per line its start, header flag | name bytes, bases (both scanned in place) and
    // per record its header line.  ma_batch_set_mates_text parses two texts: they share txtIn (the second at an aligned offset)
    // and txtStat; the second text has its own per-workgroup and per-line scratch (txtMate)
    DevBuf txtIn, txtStat;
    struct TextScratch
    {
        DevBuf block, start, hdrName, bases, recLine;
    } txtOne, txtMate;
    // BGZF members inflated into txtIn (ma_batch_set_reads_bgzf, launch_bgzf.h): the compressed bytes and the member table; the
    // call's statistics follow the parse's in txtStat
    DevBuf bgzIn, bgzMembers;
    SamTextState sam{ ma_state::SAM }, pairSam{ ma_state::PAIR_SAM };
    DeflateBufs zScratch; // of ma_sam_bgzf_batch, shared by both texts
    // small inversions (ma_inversions_batch, launch_inv.h): the statistics of the call, per MappingQuality slot its candidates, per
    // candidate its record, DP job, shape, window and result, and the FINAL lists the later stages see through mq_view
    DevBuf invStat, invSlotCnt, invSlotFirst, invCand, invJobs, invShapes, invWin, invEz, invCigOff, invCigPool, invCtr, invHdr;
    DevBuf finOff, finHdr, finOrder, finCnt;
    u64 invCandCap = 0, invWinCap = 0;
    u64 cigPoolCap = 0, cigPoolMin = 0, nOpsCap = 0;
    KswSide kswSide; // created on first use
    // double-buffered I/O (ma_batch_stage_reads / ma_batch_start_mapq_download): the next reads are uploaded into reads2 / roff2
    // and the packed results of the last step downloaded on ioStream while the batch's own stream runs kernels
    DevBuf reads2, roff2;
    hipStream_t ioStream = nullptr;
    hipEvent_t evReadsFree = nullptr, evStaged = nullptr, evPacked = nullptr, evDown = nullptr;
    bool stagedPending = false, downPending = false;
    u64 stN = 0, stBases = 0;
    u32 stMaxQ = 0;
    ma_state::BatchState st; // what of all this is valid, and the counts that go with it
    bool timing = false;
    bool blocking = false; // batch_wait: sleep on an event instead of spinning
    hipEvent_t waitEv = nullptr;
    hipEvent_t ev[ 16 ];
    bool evInit = false;
    float kms[ 8 ] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    float hostMs[ 8 ] = { 0, 0, 0, 0, 0, 0, 0, 0 }; // wall time of the last stage calls on the host: seed, extract, chain, dp
    unsigned long long hctr[ CTR_COUNT ];
};

// The lists "after MappingQuality" as every later stage sees them -- pairing, both SAM texts, the packed download: read r's
// records are hdr[ off[ r ] + order[ off[ r ] + k ] ], k < cnt[ r ]; slots = off[ n_reads ].  The MappingQuality arrays themselves,
// or the final lists of a ma_inversions_batch that kept at least one record (launch_inv.h); whatever drops the inversions puts
// the view back.
struct MqView
{
    const u64* off;
    const AlnHeader* hdr;
    const u32* order;
    const u32* cnt;
    u64 slots;
};
static MqView mq_view( const ma_batch* b )
{
    if( b->st.invFinal( ) )
        return MqView{ b->finOff.as<u64>( ), b->finHdr.as<AlnHeader>( ), b->finOrder.as<u32>( ), b->finCnt.as<u32>( ), b->st.nHsets + b->st.invRecs };
    return MqView{ b->hsetOff.as<u64>( ), b->hdr.as<AlnHeader>( ), b->mqOrder.as<u32>( ), b->mqCnt.as<u32>( ), b->st.nHsets };
}

// Waits for the batch's stream.  Default: hipStreamSynchronize (the runtime spins: lowest latency, one host core busy).
// With blocking waits (ma_batch_set_blocking_sync) the host thread sleeps on an interrupt-driven event instead: the mode for
// hosts that run many more threads than cores (the per-read graph funnel), where a spinning runner burns the time slice
// it then lacks for the next launch.
static int batch_wait( ma_batch* b )
{
    if( !b->blocking )
    {
        MA_HIP( hipStreamSynchronize( b->stream ) );
        return 0;
    }
    if( !b->waitEv )
        MA_HIP( hipEventCreateWithFlags( &b->waitEv, hipEventBlockingSync | hipEventDisableTiming ) );
    MA_HIP( hipEventRecord( b->waitEv, b->stream ) );
    MA_HIP( hipEventSynchronize( b->waitEv ) );
    return 0;
}

static void batch_own_reads( ma_batch* b )
{
    b->d_reads = b->reads.as<uint8_t>( );
    b->d_roff = b->roff.as<u64>( );
    b->reads_external = false;
}

static u32 longest_read( const uint64_t* offsets, u64 n )
{
    u32 mq = 0;
    for( u64 i = 0; i < n; i++ )
        mq = std::max<u32>( mq, (u32)( offsets[ i + 1 ] - offsets[ i ] ) );
    return mq;
}

static int read_ctr( ma_batch* b )
{
    MA_HIP( hipMemcpyAsync( b->hctr, b->ctr.p, sizeof( b->hctr ), hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    return 0;
}

static int check_err( ma_batch* b, const char* where )
{
    const u32 e = (u32)b->hctr[ CTR_ERR ];
    if( !e )
        return 0;
    std::string s = std::string( where ) + ": device capacity overflow:";
    if( e & MA_ERR_SEG_OVERFLOW )
        s += " segments";
    if( e & MA_ERR_SEED_OVERFLOW )
        s += " seeds";
    if( e & MA_ERR_STACK_OVERFLOW )
        s += " interval-stack";
    if( e & MA_ERR_CIGAR_OVERFLOW )
        s += " cigar";
    if( e & MA_ERR_OPS_OVERFLOW )
        s += " alignment-ops";
    if( e & MA_ERR_SCRATCH_OVERFLOW )
        s += " scratch";
    if( e & MA_ERR_SMEM_OVERFLOW )
        s += " smem-lists";
    return fail( s );
}

template <typename T> static int scan_exclusive( ma_batch* b, const T* in, T* out, u64 n )
{
    size_t tb = 0;
    MA_HIP( hipcub::DeviceScan::ExclusiveSum( nullptr, tb, in, out, (int)n, b->stream ) );
    if( b->cubTmp.reserve( tb + 256 ) )
        return 1;
    MA_HIP( hipcub::DeviceScan::ExclusiveSum( b->cubTmp.p, tb, in, out, (int)n, b->stream ) );
    return 0;
}

struct EvTimer
{
    ma_batch* b;
    int slot;
    EvTimer( ma_batch* b_, int s ) : b( b_ ), slot( s )
    {
        if( b->timing )
            (void)hipEventRecord( b->ev[ 2 * slot ], b->stream );
    }
    ~EvTimer( )
    {
        if( b->timing )
            (void)hipEventRecord( b->ev[ 2 * slot + 1 ], b->stream );
    }
};

extern "C" {

int ma_batch_create( const ma_index* idx, const ma_params* P, uint64_t max_reads, uint64_t max_bases, ma_batch** out )
{
    if( !idx || !P || !out )
        return fail( "ma_batch_create: null argument" );
    if( P->seeding_technique < 0 || P->seeding_technique > 2 )
        return fail( "ma_batch_create: unknown seeding technique " + std::to_string( P->seeding_technique ) +
                     " (0 maxSpan, 1 SMEMs, 2 MEMs; binarySeeding.h:560-561)" );
    MA_BIND_DEVICE( idx->device );
    std::unique_ptr<ma_batch> b( new ma_batch( ) );
    b->idx = idx;
    b->device = idx->device;
    b->P = *P;
    b->max_reads = max_reads;
    b->max_bases = max_bases;
    if( b->ctr.reserve( CTR_COUNT * 8 ) || b->reads.reserve( max_bases + 64 ) || b->roff.reserve( ( max_reads + 1 ) * 8 ) )
        return 1;
    *out = b.release( );
    return 0;
}

int ma_batch_destroy( ma_batch* b )
{
    if( !b )
        return 0;
    MA_BIND_DEVICE( b->device );
    if( b->evInit )
        for( int i = 0; i < 16; i++ )
            (void)hipEventDestroy( b->ev[ i ] );
    if( b->waitEv )
        (void)hipEventDestroy( b->waitEv );
    if( b->ioStream )
    {
        (void)hipStreamSynchronize( b->ioStream );
        (void)hipStreamDestroy( b->ioStream );
        for( hipEvent_t e : { b->evReadsFree, b->evStaged, b->evPacked, b->evDown } )
            if( e )
                (void)hipEventDestroy( e );
    }
    if( b->kswSide.fork )
    {
        (void)hipEventDestroy( b->kswSide.fork );
        if( b->kswSide.band )
            (void)hipEventDestroy( b->kswSide.band );
        for( int l = 0; l < 3; l++ )
        {
            if( b->kswSide.stream[ l ] )
                (void)hipStreamDestroy( b->kswSide.stream[ l ] );
            if( b->kswSide.join[ l ] )
                (void)hipEventDestroy( b->kswSide.join[ l ] );
        }
    }
    delete b;
    return 0;
}

int ma_batch_set_stream( ma_batch* b, void* s )
{
    if( !b )
        return fail( "ma_batch_set_stream: null batch" );
    b->stream = (hipStream_t)s;
    return 0;
}

int ma_batch_set_blocking_sync( ma_batch* b, int on )
{
    if( !b )
        return fail( "ma_batch_set_blocking_sync: null batch" );
    b->blocking = on != 0;
    return 0;
}

int ma_batch_enable_timing( ma_batch* b, int on )
{
    if( !b )
        return fail( "null batch" );
    MA_BIND_DEVICE( b->device );
    if( on && !b->evInit )
    {
        for( int i = 0; i < 16; i++ )
            MA_HIP( hipEventCreate( &b->ev[ i ] ) );
        b->evInit = true;
    }
    b->timing = on != 0;
    return 0;
}

// ---- double-buffered I/O ------------------------------------------------------------------------------------------------
static int io_init( ma_batch* b )
{
    if( b->ioStream )
        return 0;
    MA_HIP( hipStreamCreateWithFlags( &b->ioStream, hipStreamNonBlocking ) );
    const unsigned fl = hipEventDisableTiming | ( b->blocking ? hipEventBlockingSync : 0u );
    MA_HIP( hipEventCreateWithFlags( &b->evReadsFree, hipEventDisableTiming ) );
    MA_HIP( hipEventCreateWithFlags( &b->evStaged, fl ) );
    MA_HIP( hipEventCreateWithFlags( &b->evPacked, hipEventDisableTiming ) );
    MA_HIP( hipEventCreateWithFlags( &b->evDown, fl ) );
    return 0;
}

// The download slot.  A batch has ONE I/O stream and ONE pending download (downPending, evDown), whatever was started:
// MappingQuality records, pair records, either SAM text.  Every download, and everything that overwrites what a download
// reads, goes through these:
//   download_wait    waits for the pending download, if any
//   download_begin   async (ma_batch_start_*_download, named by `start`): refused while one is pending, else the I/O stream is
//                    made; the synchronous form waits for the pending one
//   download_stream  the stream of the copies: the batch's own, or the I/O stream behind what the batch's stream holds so far
//   download_end     async: the download is pending from here on; else waits for the copies
// An early return between begin and end (nothing to copy) leaves nothing pending.
static int download_wait( ma_batch* b )
{
    if( b->downPending )
    {
        MA_HIP( hipEventSynchronize( b->evDown ) );
        b->downPending = false;
    }
    return 0;
}

static int download_begin( ma_batch* b, bool async, const char* start )
{
    if( async && b->downPending )
        return fail( std::string( start ) + ": the download started before was not finished (ma_batch_finish_download)" );
    return download_wait( b ) || ( async && io_init( b ) );
}

static int download_stream( ma_batch* b, bool async, hipStream_t* cs )
{
    *cs = b->stream;
    if( async )
    {
        *cs = b->ioStream;
        MA_HIP( hipEventRecord( b->evPacked, b->stream ) );
        MA_HIP( hipStreamWaitEvent( *cs, b->evPacked, 0 ) );
    }
    return 0;
}

static int download_end( ma_batch* b, bool async, hipStream_t cs )
{
    if( !async )
        return batch_wait( b );
    MA_HIP( hipEventRecord( b->evDown, cs ) );
    b->downPending = true;
    return 0;
}

int ma_batch_stage_reads( ma_batch* b, const uint8_t* codes, const uint64_t* offsets, uint64_t n )
{
    if( !b || !offsets || ( n && !codes ) )
        return fail( "ma_batch_stage_reads: null argument" );
    MA_BIND_DEVICE( b->device );
    if( n > b->max_reads || offsets[ n ] > b->max_bases )
        return fail( "ma_batch_stage_reads: batch capacity exceeded" );
    if( b->stagedPending )
        return fail( "ma_batch_stage_reads: the reads staged before were not taken (ma_batch_use_staged_reads)" );
    if( io_init( b ) || b->reads2.reserve( b->max_bases + 64 ) || b->roff2.reserve( ( b->max_reads + 1 ) * 8 ) )
        return 1;
    b->stN = n, b->stBases = offsets[ n ], b->stMaxQ = longest_read( offsets, n );
    // the second buffer held the reads of the step before the current one: everything that was enqueued on the batch's stream
    // up to the last swap may still read it
    if( b->evReadsFree )
        MA_HIP( hipStreamWaitEvent( b->ioStream, b->evReadsFree, 0 ) );
    if( b->stBases )
        MA_HIP( hipMemcpyAsync( b->reads2.p, codes, b->stBases, hipMemcpyHostToDevice, b->ioStream ) );
    MA_HIP( hipMemcpyAsync( b->roff2.p, offsets, ( n + 1 ) * 8, hipMemcpyHostToDevice, b->ioStream ) );
    MA_HIP( hipEventRecord( b->evStaged, b->ioStream ) );
    b->stagedPending = true;
    return 0;
}

int ma_batch_use_staged_reads( ma_batch* b )
{
    if( !b )
        return fail( "ma_batch_use_staged_reads: null batch" );
    if( !b->stagedPending )
        return fail( "ma_batch_use_staged_reads: no reads staged (ma_batch_stage_reads)" );
    MA_BIND_DEVICE( b->device );
    MA_HIP( hipEventSynchronize( b->evStaged ) );
    MA_HIP( hipEventRecord( b->evReadsFree, b->stream ) ); // what runs on the stream now is the last reader of the old buffer
    b->st.newReads( );
    std::swap( b->reads, b->reads2 );
    std::swap( b->roff, b->roff2 );
    b->n_reads = b->stN;
    b->n_bases = b->stBases;
    b->max_qlen = b->stMaxQ;
    batch_own_reads( b );
    b->stagedPending = false;
    return 0;
}

int ma_batch_set_reads( ma_batch* b, const uint8_t* codes, const uint64_t* offsets, uint64_t n )
{
    if( !b || !offsets || ( n && !codes ) )
        return fail( "ma_batch_set_reads: null argument" );
    MA_BIND_DEVICE( b->device );
    if( n > b->max_reads || offsets[ n ] > b->max_bases )
        return fail( "ma_batch_set_reads: batch capacity exceeded" );
    b->st.newReads( );
    b->n_reads = n;
    b->n_bases = offsets[ n ];
    b->max_qlen = longest_read( offsets, n );
    if( b->n_bases )
        MA_HIP( hipMemcpyAsync( b->reads.p, codes, b->n_bases, hipMemcpyHostToDevice, b->stream ) );
    MA_HIP( hipMemcpyAsync( b->roff.p, offsets, ( n + 1 ) * 8, hipMemcpyHostToDevice, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    batch_own_reads( b );
    return 0;
}

// longest read of the batch.  A million same-address atomics serialise in L2 (182 us per 1 M reads in
// profiles/r05_step_timeline_150bp.txt; one per wavefront: still 16 k of them, 180 us): a fixed grid strides over the reads and
// every wavefront issues ONE atomic (1 024 in all).
__global__ void k_max_qlen( const u64* roff, u64 n, unsigned long long* out )
{
    u32 v = 0;
    for( u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x )
        v = max( v, (u32)std::min<u64>( roff[ i + 1 ] - roff[ i ], 0xffffffffull ) );
    for( int m = 32; m; m >>= 1 )
        v = max( v, (u32)__shfl_xor( (int)v, m, 64 ) );
    if( ( threadIdx.x & 63 ) == 0 && v )
        atomicMax( out, (unsigned long long)v );
}

int ma_batch_set_reads_device( ma_batch* b, const void* d_codes, const void* d_offsets, uint64_t n, uint64_t n_bases )
{
    if( !b || !d_offsets || ( n && !d_codes ) )
        return fail( "ma_batch_set_reads_device: null argument" );
    MA_BIND_DEVICE( b->device );
    // the longest read first, from the caller's offsets (the counter block is its scratch: every stage's counters go, so the
    // products go before it); the caller's arrays are installed last, so a failure up to there leaves the reads that were set
    b->st.newReads( );
    MA_HIP( hipMemsetAsync( b->ctr.p, 0, CTR_COUNT * 8, b->stream ) );
    if( n )
        hipLaunchKernelGGL( k_max_qlen, dim3( (unsigned)std::min<u64>( 256, ( n + 255 ) / 256 ) ), dim3( 256 ), 0, b->stream, (const u64*)d_offsets, n,
                            b->ctr.as<unsigned long long>( ) );
    if( read_ctr( b ) )
        return 1;
    b->n_reads = n;
    b->n_bases = n_bases;
    b->d_reads = (const uint8_t*)d_codes;
    b->d_roff = (const u64*)d_offsets;
    b->reads_external = true;
    b->max_qlen = (u32)b->hctr[ 0 ];
    return 0;
}

#include "launch_seed.h"

#include "launch_extract.h"

#include "launch_chain.h"

#include "launch_dp.h"

// ---- streams -----------------------------------------------------------------------------------------------
int ma_stream_create( const ma_index* x, void** out )
{
    if( !x || !out )
        return fail( "ma_stream_create: null argument" );
    MA_BIND_DEVICE( x->device );
    hipStream_t s = nullptr;
    MA_HIP( hipStreamCreateWithFlags( &s, hipStreamNonBlocking ) );
    *out = (void*)s;
    return 0;
}
int ma_stream_destroy( const ma_index* x, void* s )
{
    if( !x )
        return fail( "ma_stream_destroy: null index" );
    if( !s )
        return 0;
    MA_BIND_DEVICE( x->device );
    MA_HIP( hipStreamDestroy( (hipStream_t)s ) );
    return 0;
}

// ---- stage inputs from the host -------------------------------------------------------------------------------
static int reset_ctr( ma_batch* b )
{
    MA_HIP( hipMemsetAsync( b->ctr.p, 0, CTR_COUNT * 8, b->stream ) );
    return 0;
}
// per-read counts (u32) and exclusive offsets (u64) from a host CSR
static void csr_parts( const uint64_t* off, u64 n, std::vector<u64>& o, std::vector<u32>& c )
{
    o.resize( n + 1 );
    c.resize( n + 1 );
    for( u64 r = 0; r < n; r++ )
    {
        o[ r ] = off[ r ];
        c[ r ] = (u32)( off[ r + 1 ] - off[ r ] );
    }
    o[ n ] = off[ n ];
    c[ n ] = 0;
}

// What ma_extract_seeds_batch relies on in segments handed in (include/ma_amd.h): checked on the host, before anything is
// uploaded -- a decreasing seg_off would make the loop below write beyond `rd`, a negative sa_size becomes a huge seed count in
// k_seg_seed_counts, a row beyond n an out-of-bounds read of k_lf_walk, a segment beyond its read an underflow of delta in
// k_seed_final.  A negative sa_start is the pool's own "this segment carries its position" form (seeding.h: text mode), which no
// getter returns and no caller may hand in.  sa_start_rc is not read by extraction and not checked: the MEMs seeding and the
// reference's SAInterval::do_for_difference (fMIndex.h:145-148) set it to -1.  A refusal is the early return of
// ma_batch_state.h: the batch is left without segments (as before ma_seed_batch) and otherwise usable.
static int segments_refuse( ma_batch* b, const std::string& what )
{
    b->st.drop( ma_state::SEEDED );
    return fail( "ma_batch_set_segments: " + what );
}
static int segments_check( ma_batch* b, const u64* roff, const uint64_t* seg_off, const ma_segment* segs )
{
    const u64 n = b->n_reads, rows = b->idx->v.n + 1; // rows 0 .. n of the BWT; row 0 is the sentinel's
    if( seg_off[ 0 ] != 0 )
        return segments_refuse( b, "seg_off does not start at 0" );
    for( u64 r = 0; r < n; r++ )
        if( seg_off[ r + 1 ] < seg_off[ r ] )
            return segments_refuse( b, "seg_off decreases at read " + std::to_string( r ) );
    if( seg_off[ n ] > 0xffffffffull )
        return segments_refuse( b, "more than 2^32 - 1 segments" );
    if( seg_off[ n ] && !segs )
        return fail( "ma_batch_set_segments: null argument" );
    for( u64 r = 0; r < n; r++ )
    {
        const u64 qlen = roff[ r + 1 ] - roff[ r ];
        for( u64 k = seg_off[ r ]; k < seg_off[ r + 1 ]; k++ )
        {
            const ma_segment& x = segs[ k ];
            const std::string where = " (read " + std::to_string( r ) + ", segment " + std::to_string( k - seg_off[ r ] ) + ")";
            if( x.q_start < 0 || x.q_size < 0 || x.sa_start < 0 || x.sa_size < 0 )
                return segments_refuse( b, "negative field" + where );
            if( x.sa_size < 1 )
                return segments_refuse( b, "empty interval" + where );
            // no interval of the seeding starts at row 0: FMIndex::init_interval starts at L2[c] + 1 (fMIndex.h:772)
            if( x.sa_start < 1 || (u64)x.sa_start > rows || (u64)x.sa_size > rows - (u64)x.sa_start )
                return segments_refuse( b, "interval outside rows 1 .. " + std::to_string( rows - 1 ) + where );
            if( (u64)x.q_start > qlen || (u64)x.q_size >= qlen - (u64)x.q_start )
                return segments_refuse( b, "segment ends beyond its read of " + std::to_string( qlen ) + " bases" + where );
        }
    }
    return 0;
}

int ma_batch_set_segments( ma_batch* b, const uint64_t* seg_off, const ma_segment* segs )
{
    if( !b || !b->d_roff || !seg_off )
        return fail( "ma_batch_set_segments: no reads set or null argument" );
    MA_BIND_DEVICE( b->device );
    const u64 n = b->n_reads;
    // the reads' lengths: the offsets live on the device, however the reads were set (as in ma_batch_set_hsets)
    std::vector<u64> roff( n + 1, 0 );
    MA_HIP( hipMemcpyAsync( roff.data( ), b->d_roff, ( n + 1 ) * 8, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    if( segments_check( b, roff.data( ), seg_off, segs ) )
        return 1;
    const u64 ns = seg_off[ n ];
    b->st.drop( ma_state::SEEDED );
    std::vector<u64> o;
    std::vector<u32> c, rd( ns + 1 );
    csr_parts( seg_off, n, o, c );
    for( u64 r = 0; r < n; r++ )
        for( u64 k = seg_off[ r ]; k < seg_off[ r + 1 ]; k++ )
            rd[ k ] = (u32)r;
    b->segPoolCap = std::max<u64>( ns + 1024, b->segPoolCap );
    if( reset_ctr( b ) || b->segPool.reserve( b->segPoolCap * sizeof( ma_segment ) ) || b->segRead.reserve( b->segPoolCap * 4 ) ||
        b->segOff.reserve( ( n + 1 ) * 8 ) || b->segCnt.reserve( ( n + 1 ) * 4 ) )
        return 1;
    if( ns )
    {
        MA_HIP( hipMemcpyAsync( b->segPool.p, segs, ns * sizeof( ma_segment ), hipMemcpyHostToDevice, b->stream ) );
        MA_HIP( hipMemcpyAsync( b->segRead.p, rd.data( ), ns * 4, hipMemcpyHostToDevice, b->stream ) );
    }
    MA_HIP( hipMemcpyAsync( b->segOff.p, o.data( ), ( n + 1 ) * 8, hipMemcpyHostToDevice, b->stream ) );
    MA_HIP( hipMemcpyAsync( b->segCnt.p, c.data( ), ( n + 1 ) * 4, hipMemcpyHostToDevice, b->stream ) );
    const unsigned long long used = ns;
    MA_HIP( hipMemcpyAsync( b->ctr.as<unsigned long long>( ) + CTR_SEG_USED, &used, 8, hipMemcpyHostToDevice, b->stream ) );
    if( batch_wait( b ) )
        return 1; // the host vectors go out of scope
    b->st.nSegs = ns;
    b->st.finish( ma_state::SEEDED );
    return 0;
}

// What ma_chain_batch relies on in seeds handed in (include/ma_amd.h, ../host/ma_seed_contract.h): checked on the host, before
// anything is uploaded.  A refusal is the early return of ma_batch_state.h: the batch is left without seeds and strips (as before
// ma_extract_seeds_batch) and otherwise usable.
static int seeds_check( ma_batch* b, const char* fn, const uint64_t* seed_off, const ma_seed* seeds )
{
    const u64 n = b->n_reads;
    std::vector<u64> roff( n + 1, 0 );
    MA_HIP( hipMemcpyAsync( roff.data( ), b->d_roff, ( n + 1 ) * 8, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    const std::string what = ma_contract::seeds_violation( seed_off, seeds, n, roff.data( ), b->idx->h_cstart.data( ), b->idx->h_cstart.size( ),
                                                           b->idx->v.F );
    return what.empty( ) ? 0 : fail( std::string( fn ) + ": " + what );
}

static int set_seeds( ma_batch* b, const char* fn, const uint64_t* seed_off, const ma_seed* seeds )
{
    MA_BIND_DEVICE( b->device );
    const u64 n = b->n_reads;
    b->st.drop( ma_state::EXTRACTED );
    if( seeds_check( b, fn, seed_off, seeds ) )
        return 1;
    const u64 total = seed_off[ n ];
    std::vector<u64> o;
    std::vector<u32> c;
    csr_parts( seed_off, n, o, c );
    if( reset_ctr( b ) || b->seeds.reserve( ( total + 1 ) * sizeof( ma_seed ) ) || b->seedOff.reserve( ( n + 1 ) * 8 ) ||
        b->seedCnt.reserve( ( n + 1 ) * 4 ) )
        return 1;
    if( total )
        MA_HIP( hipMemcpyAsync( b->seeds.p, seeds, total * sizeof( ma_seed ), hipMemcpyHostToDevice, b->stream ) );
    MA_HIP( hipMemcpyAsync( b->seedOff.p, o.data( ), ( n + 1 ) * 8, hipMemcpyHostToDevice, b->stream ) );
    MA_HIP( hipMemcpyAsync( b->seedCnt.p, c.data( ), ( n + 1 ) * 4, hipMemcpyHostToDevice, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    b->st.nSeeds = total;
    b->st.finish( ma_state::EXTRACTED );
    return 0;
}

int ma_batch_set_seeds( ma_batch* b, const uint64_t* seed_off, const ma_seed* seeds )
{
    if( !b || !b->d_roff || !seed_off )
        return fail( "ma_batch_set_seeds: no reads set or null argument" );
    // (a seed_off that decreases is the check's to name; seeds may be null only where there are none)
    if( !seeds && seed_off[ 0 ] == 0 && seed_off[ b->n_reads ] != 0 )
        return fail( "ma_batch_set_seeds: no reads set or null argument" );
    return set_seeds( b, "ma_batch_set_seeds", seed_off, seeds );
}

// A SoC queue per read that was swept elsewhere -- the reference's StripOfConsideration in a mixed graph -- as input of
// ma_chain_batch, which then only harmonizes: sorted_seeds = the read's seeds as rectangularSoC left them (pSeeds of the
// SoCPriorityQueue), socs = its array vMaxima (score triple + seed range), both CSR per read (the layout
// ma_batch_get_soc_heap returns).
int ma_batch_set_soc_heap( ma_batch* b, const uint64_t* soc_off, const ma_soc* socs, const uint64_t* seed_off, const ma_seed* sorted_seeds )
{
    if( !b || !b->d_roff || !soc_off || !seed_off )
        return fail( "ma_batch_set_soc_heap: no reads set or null argument" );
    const u64 n = b->n_reads;
    if( ( soc_off[ n ] && !socs ) || ( seed_off[ n ] && !sorted_seeds ) )
        return fail( "ma_batch_set_soc_heap: null argument" );
    {
        const std::string what = ma_contract::socs_violation( soc_off, socs, seed_off, n );
        if( !what.empty( ) )
        {
            b->st.drop( ma_state::EXTRACTED );
            return fail( "ma_batch_set_soc_heap: " + what );
        }
    }
    if( set_seeds( b, "ma_batch_set_soc_heap", seed_off, sorted_seeds ) )
        return 1;
    const u64 total = seed_off[ n ];
    std::vector<ma_soc> q( total + 1 ); // the strips of read r at its SEED offset: the carving every chain scratch uses
    std::vector<u32> c( n + 1 );
    for( u64 r = 0; r < n; r++ )
    {
        c[ r ] = (u32)( soc_off[ r + 1 ] - soc_off[ r ] );
        for( u32 k = 0; k < c[ r ]; k++ )
            q[ seed_off[ r ] + k ] = socs[ soc_off[ r ] + k ];
    }
    if( b->socIn.reserve( ( total + 1 ) * sizeof( ma_soc ) ) || b->socInCnt.reserve( ( n + 1 ) * 4 ) )
        return 1;
    if( total )
        MA_HIP( hipMemcpyAsync( b->socIn.p, q.data( ), total * sizeof( ma_soc ), hipMemcpyHostToDevice, b->stream ) );
    MA_HIP( hipMemcpyAsync( b->socInCnt.p, c.data( ), ( n + 1 ) * 4, hipMemcpyHostToDevice, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    b->st.giveSocs( );
    return 0;
}

// What ma_dp_batch relies on in sets handed in (include/ma_amd.h): checked on the host, before anything is uploaded -- a seed
// beyond its read or beyond the text would be an out-of-bounds read of k_dp_enum and the ksw kernels.  A refusal leaves the batch
// without harmonized sets (as before ma_chain_batch) and otherwise usable.
static int hsets_refuse( ma_batch* b, const std::string& what )
{
    b->st.drop( ma_state::CHAINED );
    return fail( "ma_batch_set_hsets: " + what );
}
static int hsets_check( ma_batch* b, const u64* roff, const uint64_t* hset_off, const uint64_t* hseed_off, const uint32_t* hset_soc, const ma_seed* hseeds )
{
    const u64 n = b->n_reads, textLen = b->idx->v.n;
    if( hset_off[ 0 ] != 0 )
        return hsets_refuse( b, "hset_off does not start at 0" );
    for( u64 r = 0; r < n; r++ )
        if( hset_off[ r + 1 ] < hset_off[ r ] )
            return hsets_refuse( b, "hset_off decreases at read " + std::to_string( r ) );
    const u64 nh = hset_off[ n ];
    if( nh == 0 )
        return 0;
    if( !hseed_off || !hset_soc )
        return fail( "ma_batch_set_hsets: null argument" );
    if( nh > 0xffffffffull )
        return hsets_refuse( b, "more than 2^32 - 1 sets" );
    if( hseed_off[ 0 ] != 0 )
        return hsets_refuse( b, "hseed_off does not start at 0" );
    for( u64 r = 0; r < n; r++ )
    {
        const u64 qlen = roff[ r + 1 ] - roff[ r ];
        for( u64 s = hset_off[ r ]; s < hset_off[ r + 1 ]; s++ )
        {
            const std::string where = "read " + std::to_string( r ) + ", set " + std::to_string( s - hset_off[ r ] );
            if( hseed_off[ s + 1 ] < hseed_off[ s ] )
                return hsets_refuse( b, "hseed_off decreases (" + where + ")" );
            if( hseed_off[ s + 1 ] - hseed_off[ s ] > 0x7fffffffull )
                return hsets_refuse( b, "too many seeds (" + where + ")" );
            if( hseed_off[ s + 1 ] > hseed_off[ s ] && !hseeds )
                return fail( "ma_batch_set_hsets: null argument" );
            for( u64 k = hseed_off[ s ]; k < hseed_off[ s + 1 ]; k++ )
            {
                const ma_seed& x = hseeds[ k ];
                const std::string seed = where + ", seed " + std::to_string( k - hseed_off[ s ] ) + ")";
                if( x.q_start < 0 || x.len < 0 || x.r_start < 0 || x.delta < 0 )
                    return hsets_refuse( b, "negative field (" + seed );
                if( (u64)x.q_start > qlen || (u64)x.len > qlen - (u64)x.q_start )
                    return hsets_refuse( b, "seed ends beyond its read of " + std::to_string( qlen ) + " bases (" + seed );
                if( (u64)x.r_start > textLen || (u64)x.len > textLen - (u64)x.r_start )
                    return hsets_refuse( b, "seed ends beyond the doubled text of " + std::to_string( textLen ) + " bases (" + seed );
            }
        }
    }
    return 0;
}

int ma_batch_set_hsets( ma_batch* b, const uint64_t* hset_off, const uint64_t* hseed_off, const uint32_t* hset_soc,
                        const ma_seed* hseeds )
{
    if( !b || !b->d_roff || !hset_off )
        return fail( "ma_batch_set_hsets: no reads set or null argument" );
    const u64 n = b->n_reads;
    MA_BIND_DEVICE( b->device );
    // the reads' lengths: the offsets live on the device, however the reads were set (this call is no part of the aligned path: a
    // small copy and a wait more do not matter here, a host copy of the offsets per ma_batch_set_reads would)
    std::vector<u64> roff( n + 1, 0 );
    MA_HIP( hipMemcpyAsync( roff.data( ), b->d_roff, ( n + 1 ) * 8, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    if( hsets_check( b, roff.data( ), hset_off, hseed_off, hset_soc, hseeds ) )
        return 1;
    b->st.drop( ma_state::CHAINED );
    const u64 nh = hset_off[ n ];
    const u64 nhs = nh ? hseed_off[ nh ] : 0;
    std::vector<HSet> flat( nh + 1 );
    std::vector<u32> rd( nh + 1 );
    for( u64 r = 0; r < n; r++ )
        for( u64 s = hset_off[ r ]; s < hset_off[ r + 1 ]; s++ )
        {
            flat[ s ].off = hseed_off[ s ];
            flat[ s ].cnt = (u32)( hseed_off[ s + 1 ] - hseed_off[ s ] );
            flat[ s ].soc = hset_soc[ s ];
            rd[ s ] = (u32)r;
        }
    if( reset_ctr( b ) || b->hsetFlat.reserve( ( nh + 1 ) * sizeof( HSet ) ) || b->hsetRead.reserve( ( nh + 1 ) * 4 ) ||
        b->hdense.reserve( ( nhs + 1 ) * sizeof( ma_seed ) ) || b->hsetOff.reserve( ( n + 2 ) * 8 ) )
        return 1;
    if( nh )
    {
        MA_HIP( hipMemcpyAsync( b->hsetFlat.p, flat.data( ), nh * sizeof( HSet ), hipMemcpyHostToDevice, b->stream ) );
        MA_HIP( hipMemcpyAsync( b->hsetRead.p, rd.data( ), nh * 4, hipMemcpyHostToDevice, b->stream ) );
    }
    if( nhs )
        MA_HIP( hipMemcpyAsync( b->hdense.p, hseeds, nhs * sizeof( ma_seed ), hipMemcpyHostToDevice, b->stream ) );
    MA_HIP( hipMemcpyAsync( b->hsetOff.p, hset_off, ( n + 1 ) * 8, hipMemcpyHostToDevice, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    b->st.nHsets = nh;
    b->st.nHseeds = nhs;
    b->st.finish( ma_state::CHAINED );
    return 0;
}

// ---- the SoC queue across the boundary ------------------------------------------------------------------------
static int get_socs( ma_batch* b, int heap_layout, uint64_t* n_socs, uint64_t* soc_off, ma_soc* socs, uint64_t* seed_off,
                     ma_seed* sorted_seeds );
int ma_batch_get_socs( ma_batch* b, uint64_t* n_socs, uint64_t* soc_off, ma_soc* socs, uint64_t* seed_off, ma_seed* sorted_seeds )
{
    return get_socs( b, 0, n_socs, soc_off, socs, seed_off, sorted_seeds );
}
int ma_batch_get_soc_heap( ma_batch* b, uint64_t* n_socs, uint64_t* soc_off, ma_soc* socs, uint64_t* seed_off, ma_seed* sorted_seeds )
{
    return get_socs( b, 1, n_socs, soc_off, socs, seed_off, sorted_seeds );
}
} // extern "C"
static int get_socs( ma_batch* b, int heap_layout, uint64_t* n_socs, uint64_t* soc_off, ma_soc* socs, uint64_t* seed_off,
                     ma_seed* sorted_seeds )
{
    if( !b || !b->st.has( ma_state::EXTRACTED ) )
        return fail( "ma_batch_get_socs: run ma_extract_seeds_batch first" );
    MA_BIND_DEVICE( b->device );
    const u64 n = b->n_reads, ts = b->st.nSeeds + 1;
    if( n_socs )
        *n_socs = 0;
    if( soc_off )
        soc_off[ 0 ] = 0;
    if( seed_off )
        seed_off[ 0 ] = 0;
    if( n == 0 )
        return 0;
    DevBuf dSocs, dN;
    if( b->cWork.reserve( ts * sizeof( ma_seed ) ) || b->cMax.reserve( ts * sizeof( SoCEntry ) ) ||
        b->cMm.reserve( ts * sizeof( RefMinMax ) ) || dSocs.reserve( ts * sizeof( ma_soc ) ) || dN.reserve( ( n + 1 ) * 4 ) )
        return 1;
    hipLaunchKernelGGL( k_soc_dump, dim3( (unsigned)( ( n + 63 ) / 64 ) ), dim3( 64 ), 0, b->stream, b->idx->v, chain_params( b->P ),
                        (u32)n, b->d_roff, b->seedOff.as<u64>( ), b->seedCnt.as<u32>( ), b->seeds.as<ma_seed>( ),
                        b->cWork.as<ma_seed>( ), b->cMax.as<SoCEntry>( ), b->cMm.as<RefMinMax>( ), dSocs.as<ma_soc>( ),
                        dN.as<u32>( ), heap_layout );
    MA_HIP( hipGetLastError( ) );
    std::vector<u32> cnt( n ), scnt( n );
    std::vector<u64> off( n );
    MA_HIP( hipMemcpyAsync( cnt.data( ), dN.p, n * 4, hipMemcpyDeviceToHost, b->stream ) );
    MA_HIP( hipMemcpyAsync( scnt.data( ), b->seedCnt.p, n * 4, hipMemcpyDeviceToHost, b->stream ) );
    MA_HIP( hipMemcpyAsync( off.data( ), b->seedOff.p, n * 8, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    u64 total = 0;
    for( u64 r = 0; r < n; r++ )
        total += cnt[ r ];
    if( n_socs )
        *n_socs = total;
    if( !soc_off && !socs && !seed_off && !sorted_seeds )
        return 0;
    std::vector<ma_soc> hs( b->st.nSeeds + 1 );
    std::vector<ma_seed> hw( b->st.nSeeds + 1 );
    if( b->st.nSeeds )
    {
        MA_HIP( hipMemcpy( hs.data( ), dSocs.p, b->st.nSeeds * sizeof( ma_soc ), hipMemcpyDeviceToHost ) );
        MA_HIP( hipMemcpy( hw.data( ), b->cWork.p, b->st.nSeeds * sizeof( ma_seed ), hipMemcpyDeviceToHost ) );
    }
    u64 so = 0, sd = 0;
    for( u64 r = 0; r < n; r++ )
    {
        if( socs )
            for( u32 k = 0; k < cnt[ r ]; k++ )
                socs[ so + k ] = hs[ off[ r ] + k ];
        if( sorted_seeds )
            for( u32 k = 0; k < scnt[ r ]; k++ )
                sorted_seeds[ sd + k ] = hw[ off[ r ] + k ];
        so += cnt[ r ];
        sd += scnt[ r ];
        if( soc_off )
            soc_off[ r + 1 ] = so;
        if( seed_off )
            seed_off[ r + 1 ] = sd;
    }
    return 0;
}
extern "C" {

int ma_align_batch( ma_batch* b )
{
    if( !b )
        return fail( "ma_align_batch: null batch" );
    int ( *const stage[ 4 ] )( ma_batch* ) = { ma_seed_batch, ma_extract_seeds_batch, ma_chain_batch, ma_dp_batch };
    for( int k = 0; k < 4; k++ )
    {
        const auto t0 = std::chrono::steady_clock::now( );
        if( stage[ k ]( b ) )
            return 1;
        b->hostMs[ k ] = std::chrono::duration<float, std::milli>( std::chrono::steady_clock::now( ) - t0 ).count( );
    }
    if( getenv( "MA_MEM_REPORT" ) ) // diagnostics: device bytes this batch holds after a full pass
    {
        struct Row
        {
            const char* name;
            size_t cap;
        };
#define MA_ROW( x ) Row{ #x, b->x.cap }
        std::vector<Row> rows = { MA_ROW( reads ), MA_ROW( roff ), MA_ROW( seedStack ), MA_ROW( seedRow ), MA_ROW( seedSteps ), MA_ROW( seedSeg ),
            MA_ROW( hlocal ), MA_ROW( hdense ), MA_ROW( hseedCnt ), MA_ROW( hseedOff ), MA_ROW( stage ), MA_ROW( smemA ), MA_ROW( smemB ),
            MA_ROW( segPool ), MA_ROW( segRead ), MA_ROW( segOff ), MA_ROW( segCnt ), MA_ROW( memsCnt ), MA_ROW( memsOff ), MA_ROW( taskA ),
            MA_ROW( taskB ), MA_ROW( taskCnt ), MA_ROW( taskKey ), MA_ROW( taskKey2 ), MA_ROW( taskPerm ), MA_ROW( taskPerm2 ),
            MA_ROW( segSeedCnt ), MA_ROW( segSeedOff ), MA_ROW( seedOff ), MA_ROW( seedCnt ), MA_ROW( seeds ), MA_ROW( cubTmp ), MA_ROW( cWork ),
            MA_ROW( cMax ), MA_ROW( cMm ), MA_ROW( cA ), MA_ROW( cB ), MA_ROW( cOut ), MA_ROW( cSh1 ), MA_ROW( cSh2 ), MA_ROW( cVx ), MA_ROW( cVy ),
            MA_ROW( cMed ), MA_ROW( cInl ), MA_ROW( cBest ), MA_ROW( cPack ), MA_ROW( cList ), MA_ROW( hpool ), MA_ROW( setTab ), MA_ROW( nsets ), MA_ROW( hsetOff ),
            MA_ROW( hsetFlat ), MA_ROW( hsetRead ), MA_ROW( jobs ), MA_ROW( info ), MA_ROW( ez ), MA_ROW( cigOff ), MA_ROW( cigPool ),
            MA_ROW( kswScratch ), MA_ROW( clsLists ), MA_ROW( opsCap ), MA_ROW( opsOff ), MA_ROW( ops ), MA_ROW( hdr ), MA_ROW( order ),
            MA_ROW( mqOrder ), MA_ROW( mqCnt ), MA_ROW( outCnt ), MA_ROW( outOps ), MA_ROW( outAlnOff ), MA_ROW( outOpsOff ), MA_ROW( outAlns ),
            MA_ROW( outOpsPairs ) };
#undef MA_ROW
        std::sort( rows.begin( ), rows.end( ), []( const Row& a, const Row& c ) { return a.cap > c.cap; } );
        size_t total = 0;
        for( const Row& r : rows )
            total += r.cap;
        fprintf( stderr, "[ma_amd] batch of %llu reads / %llu bases holds %.2f GB on the device:", (unsigned long long)b->n_reads,
                 (unsigned long long)b->n_bases, total / 1e9 );
        for( size_t i = 0; i < rows.size( ) && i < 14; i++ )
            fprintf( stderr, " %s %.2f", rows[ i ].name, rows[ i ].cap / 1e9 );
        fprintf( stderr, "\n" );
    }
    return 0;
}

int ma_batch_host_ms( ma_batch* b, float out[ 8 ] )
{
    if( !b )
        return fail( "null batch" );
    for( int i = 0; i < 8; i++ )
        out[ i ] = b->hostMs[ i ];
    return 0;
}

int ma_batch_sync( ma_batch* b )
{
    if( !b )
        return fail( "ma_batch_sync: null batch" );
    MA_BIND_DEVICE( b->device );
    if( read_ctr( b ) )
        return 1;
    if( b->timing && b->evInit )
        for( int i = 0; i < 6; i++ )
        {
            float ms = 0;
            if( hipEventElapsedTime( &ms, b->ev[ 2 * i ], b->ev[ 2 * i + 1 ] ) == hipSuccess )
                b->kms[ i ] = ms;
        }
    return check_err( b, "ma_batch_sync" );
}

int ma_batch_kernel_ms( ma_batch* b, float out[ 8 ] )
{
    if( !b )
        return fail( "null batch" );
    for( int i = 0; i < 8; i++ )
        out[ i ] = b->kms[ i ];
    return 0;
}

int ma_batch_counters( ma_batch* b, uint64_t out[ 8 ] )
{
    if( ma_batch_sync( b ) )
        return 1;
    out[ 0 ] = b->hctr[ CTR_STEPS ];
    out[ 1 ] = b->hctr[ CTR_BLOCKS ];
    out[ 2 ] = b->hctr[ CTR_LF_STEPS ];
    out[ 3 ] = b->st.nSeeds;
    out[ 4 ] = b->hctr[ CTR_CELLS ] + b->hctr[ CTR_N_1X1 ];
    out[ 5 ] = b->hctr[ CTR_KSW_JOBS ] + b->hctr[ CTR_N_1X1 ];
    out[ 6 ] = b->hctr[ CTR_SEQ_BYTES ];
    out[ 7 ] = b->hctr[ CTR_PATH_BYTES ] + 4 * b->hctr[ CTR_CIG_WORDS ] + 5 * b->hctr[ CTR_N_1X1 ]; // (a 1 x 1 job: one back-trace step, one cigar word)
    return 0;
}

int ma_batch_counts( ma_batch* b, uint64_t* n_segments, uint64_t* n_seeds, uint64_t* n_hsets, uint64_t* n_hseeds,
                     uint64_t* n_alignments, uint64_t* n_ops, uint64_t* n_aligned_reads )
{
    if( ma_batch_sync( b ) )
        return 1;
    if( b->st.has( ma_state::SEEDED ) && b->st.nSegs == 0 )
        b->st.nSegs = b->hctr[ CTR_SEG_USED ];
    if( n_segments )
        *n_segments = b->st.nSegs;
    if( n_seeds )
        *n_seeds = b->st.nSeeds;
    if( n_hsets )
        *n_hsets = b->st.nHsets;
    if( n_hseeds )
        *n_hseeds = b->st.nHseeds;
    if( n_alignments )
        *n_alignments = b->st.has( ma_state::ALIGNED ) ? mq_view( b ).slots : 0;
    if( n_ops ) // exact: the ops of all alignments (the MappingQuality selection has at most as many) and of the inversion records
        *n_ops = b->st.has( ma_state::ALIGNED ) ? b->hctr[ CTR_OPS_ALL ] + ( b->st.invFinal( ) ? b->st.invOps : 0 ) : 0;
    if( n_aligned_reads )
        *n_aligned_reads = b->hctr[ CTR_N_ALIGNED ];
    return 0;
}

// The public segment record holds rows.  The text mode of k_seed leaves segments that carry their position instead; whoever hands
// segments out calls this first.  Not part of the aligned path: extraction takes the position as it is.
static int seg_materialise( ma_batch* b, u64 ns )
{
    if( !b->st.segMarked || ns == 0 )
        return 0;
    hipLaunchKernelGGL( k_seg_materialise, dim3( (unsigned)( ( ns + 255 ) / 256 ) ), dim3( 256 ), 0, b->stream, b->idx->v, b->d_reads, b->d_roff,
                        b->segRead.as<u32>( ), b->segPool.as<ma_segment>( ), ns );
    MA_HIP( hipGetLastError( ) );
    if( batch_wait( b ) )
        return 1;
    b->st.markSegments( false );
    return 0;
}

// Downloads gather the per-read ranges (pools are in completion order) into read-order CSR arrays.
int ma_batch_get_segments( ma_batch* b, uint64_t* seg_off, ma_segment* segs )
{
    if( !b || !b->st.has( ma_state::SEEDED ) )
        return fail( "ma_batch_get_segments: stage not run" );
    MA_BIND_DEVICE( b->device );
    if( ma_batch_sync( b ) )
        return 1;
    const u64 n = b->n_reads, ns = b->hctr[ CTR_SEG_USED ];
    if( seg_materialise( b, ns ) )
        return 1;
    std::vector<u64> off( n );
    std::vector<u32> cnt( n );
    std::vector<ma_segment> pool( ns );
    if( n )
    {
        MA_HIP( hipMemcpy( off.data( ), b->segOff.p, n * 8, hipMemcpyDeviceToHost ) );
        MA_HIP( hipMemcpy( cnt.data( ), b->segCnt.p, n * 4, hipMemcpyDeviceToHost ) );
    }
    if( ns )
        MA_HIP( hipMemcpy( pool.data( ), b->segPool.p, ns * sizeof( ma_segment ), hipMemcpyDeviceToHost ) );
    u64 o = 0;
    for( u64 r = 0; r < n; r++ )
    {
        if( seg_off )
            seg_off[ r ] = o;
        if( segs )
            for( u32 k = 0; k < cnt[ r ]; k++ )
                segs[ o + k ] = pool[ off[ r ] + k ];
        o += cnt[ r ];
    }
    if( seg_off )
        seg_off[ n ] = o;
    return 0;
}

int ma_batch_get_seeds( ma_batch* b, uint64_t* seed_off, ma_seed* seeds )
{
    if( !b || !b->st.has( ma_state::EXTRACTED ) )
        return fail( "ma_batch_get_seeds: stage not run" );
    MA_BIND_DEVICE( b->device );
    if( ma_batch_sync( b ) )
        return 1;
    const u64 n = b->n_reads;
    std::vector<u64> off( n );
    std::vector<u32> cnt( n );
    std::vector<ma_seed> pool( b->st.nSeeds );
    if( n )
    {
        MA_HIP( hipMemcpy( off.data( ), b->seedOff.p, n * 8, hipMemcpyDeviceToHost ) );
        MA_HIP( hipMemcpy( cnt.data( ), b->seedCnt.p, n * 4, hipMemcpyDeviceToHost ) );
    }
    if( b->st.nSeeds )
        MA_HIP( hipMemcpy( pool.data( ), b->seeds.p, b->st.nSeeds * sizeof( ma_seed ), hipMemcpyDeviceToHost ) );
    u64 o = 0;
    for( u64 r = 0; r < n; r++ )
    {
        if( seed_off )
            seed_off[ r ] = o;
        if( seeds )
            for( u32 k = 0; k < cnt[ r ]; k++ )
                seeds[ o + k ] = pool[ off[ r ] + k ];
        o += cnt[ r ];
    }
    if( seed_off )
        seed_off[ n ] = o;
    return 0;
}

int ma_batch_get_hsets( ma_batch* b, uint64_t* hset_off, uint64_t* hseed_off, uint32_t* hset_soc, ma_seed* hseeds )
{
    if( !b || !b->st.has( ma_state::CHAINED ) )
        return fail( "ma_batch_get_hsets: stage not run" );
    MA_BIND_DEVICE( b->device );
    if( ma_batch_sync( b ) )
        return 1;
    const u64 n = b->n_reads, nh = b->st.nHsets;
    if( hset_off && n )
        MA_HIP( hipMemcpy( hset_off, b->hsetOff.p, ( n + 1 ) * 8, hipMemcpyDeviceToHost ) );
    if( hset_off && !n )
        hset_off[ 0 ] = 0;
    std::vector<HSet> flat( nh );
    std::vector<ma_seed> pool( b->st.nHseeds );
    if( nh )
        MA_HIP( hipMemcpy( flat.data( ), b->hsetFlat.p, nh * sizeof( HSet ), hipMemcpyDeviceToHost ) );
    if( b->st.nHseeds )
        MA_HIP( hipMemcpy( pool.data( ), b->hdense.p, b->st.nHseeds * sizeof( ma_seed ), hipMemcpyDeviceToHost ) );
    u64 o = 0;
    for( u64 s = 0; s < nh; s++ )
    {
        if( hseed_off )
            hseed_off[ s ] = o;
        if( hset_soc )
            hset_soc[ s ] = flat[ s ].soc;
        if( hseeds )
            for( u32 k = 0; k < flat[ s ].cnt; k++ )
                hseeds[ o + k ] = pool[ flat[ s ].off + k ];
        o += flat[ s ].cnt;
    }
    if( hseed_off )
        hseed_off[ nh ] = o;
    return 0;
}

// async = the double-buffered form: the copies go to the I/O stream behind the pack kernels and nobody waits here
static int get_alns( ma_batch* b, bool mq, uint64_t* aln_off, ma_alignment* alns, uint64_t* ops, bool async = false )
{
    if( !b || !b->st.has( ma_state::ALIGNED ) )
        return fail( "ma_batch_get_alignments: stage not run" );
    MA_BIND_DEVICE( b->device );
    if( ma_batch_sync( b ) )
        return 1;
    if( download_begin( b, async, "ma_batch_start_mapq_download" ) ) // (the packed arrays may be overwritten only behind it)
        return 1;
    const u64 n = b->n_reads, nh = b->st.nHsets;
    if( aln_off )
        aln_off[ 0 ] = 0;
    if( n == 0 )
        return 0;
    if( nh == 0 )
    {
        if( aln_off )
            memset( aln_off, 0, ( n + 1 ) * 8 );
        return 0;
    }
    // (the MappingQuality form serves the list view: the final lists after a ma_inversions_batch that kept records)
    const MqView V = mq_view( b );
    const u64 invA = mq && b->st.invFinal( ) ? b->st.invRecs : 0, invO = mq && b->st.invFinal( ) ? b->st.invOps : 0;
    const u64 totalA = mq ? b->hctr[ CTR_ALN_MQ ] + invA : nh, totalO = mq ? b->hctr[ CTR_OPS_MQ ] + invO : b->hctr[ CTR_OPS_ALL ];
    if( b->outCnt.reserve( ( n + 2 ) * 8 ) || b->outOps.reserve( ( n + 2 ) * 8 ) || b->outAlnOff.reserve( ( n + 2 ) * 8 ) ||
        b->outOpsOff.reserve( ( n + 2 ) * 8 ) || b->outAlns.reserve( ( totalA + 1 ) * sizeof( ma_alignment ) ) ||
        b->outOpsPairs.reserve( ( totalO + 1 ) * 16 ) )
        return 1;
    const u64* off = mq ? V.off : b->hsetOff.as<u64>( );
    const AlnHeader* hdr = mq ? V.hdr : b->hdr.as<AlnHeader>( );
    const u32* ord = mq ? V.order : b->order.as<u32>( );
    const dim3 grid( (unsigned)( ( n + 255 ) / 256 ) ), block( 256 );
    hipLaunchKernelGGL( k_aln_sizes, grid, block, 0, b->stream, (u32)n, off, hdr, ord, mq ? V.cnt : b->mqCnt.as<u32>( ), mq ? 1 : 0,
                        b->outCnt.as<u64>( ), b->outOps.as<u64>( ) );
    MA_HIP( hipMemsetAsync( (char*)b->outCnt.p + n * 8, 0, 8, b->stream ) );
    MA_HIP( hipMemsetAsync( (char*)b->outOps.p + n * 8, 0, 8, b->stream ) );
    if( scan_exclusive<u64>( b, b->outCnt.as<u64>( ), b->outAlnOff.as<u64>( ), n + 1 ) ||
        scan_exclusive<u64>( b, b->outOps.as<u64>( ), b->outOpsOff.as<u64>( ), n + 1 ) )
        return 1;
    hipLaunchKernelGGL( k_aln_pack, grid, block, 0, b->stream, (u32)n, off, hdr, ord, b->ops.as<u64>( ), mq ? 1 : 0, b->outAlnOff.as<u64>( ), b->outOpsOff.as<u64>( ), b->outAlns.as<ma_alignment>( ),
                        b->outOpsPairs.as<u64>( ) );
    MA_HIP( hipGetLastError( ) );
    hipStream_t cs;
    if( download_stream( b, async, &cs ) )
        return 1;
    if( aln_off )
        MA_HIP( hipMemcpyAsync( aln_off, b->outAlnOff.p, ( n + 1 ) * 8, hipMemcpyDeviceToHost, cs ) );
    if( alns && totalA )
        MA_HIP( hipMemcpyAsync( alns, b->outAlns.p, totalA * sizeof( ma_alignment ), hipMemcpyDeviceToHost, cs ) );
    if( ops && totalO )
        MA_HIP( hipMemcpyAsync( ops, b->outOpsPairs.p, totalO * 16, hipMemcpyDeviceToHost, cs ) );
    return download_end( b, async, cs );
}

int ma_batch_start_mapq_download( ma_batch* b, uint64_t* aln_off, ma_alignment* alns, uint64_t* ops )
{
    return get_alns( b, true, aln_off, alns, ops, true );
}

int ma_batch_finish_download( ma_batch* b )
{
    if( !b )
        return fail( "ma_batch_finish_download: null batch" );
    if( !b->downPending )
        return 0;
    MA_BIND_DEVICE( b->device );
    return download_wait( b );
}

int ma_batch_get_alignments( ma_batch* b, uint64_t* aln_off, ma_alignment* alns, uint64_t* ops )
{
    return get_alns( b, false, aln_off, alns, ops );
}
int ma_batch_get_mapq_alignments( ma_batch* b, uint64_t* aln_off, ma_alignment* alns, uint64_t* ops )
{
    return get_alns( b, true, aln_off, alns, ops );
}

int ma_batch_get_dp_jobs( ma_batch* b, uint64_t* n_jobs, int32_t* shapes /* 8 x i32 per job */, uint64_t cap )
{
    if( !b || !b->st.has( ma_state::ALIGNED ) )
        return fail( "ma_batch_get_dp_jobs: stage not run" );
    MA_BIND_DEVICE( b->device );
    if( ma_batch_sync( b ) )
        return 1;
    const u64 nSlots = b->st.nJobSlots;
    std::vector<DpJob> jobs( nSlots + 1 );
    std::vector<ma_ez> ez( nSlots + 1 );
    if( nSlots )
    {
        MA_HIP( hipMemcpy( jobs.data( ), b->jobs.p, nSlots * sizeof( DpJob ), hipMemcpyDeviceToHost ) );
        MA_HIP( hipMemcpy( ez.data( ), b->ez.p, nSlots * sizeof( ma_ez ), hipMemcpyDeviceToHost ) );
    }
    u64 n = 0;
    for( u64 i = 0; i < nSlots; i++ )
    {
        const DpJob& j = jobs[ i ];
        if( j.q_to <= j.q_from )
            continue;
        if( shapes && n < cap )
        {
            int32_t* o = shapes + 8 * n;
            o[ 0 ] = (int32_t)( j.q_to - j.q_from );
            o[ 1 ] = (int32_t)( j.r_to - j.r_from );
            o[ 2 ] = j.w;
            o[ 3 ] = j.zdrop;
            o[ 4 ] = j.flag;
            o[ 5 ] = ez[ i ].zdropped;
            o[ 6 ] = ez[ i ].max_q;
            o[ 7 ] = ez[ i ].max_t;
        }
        n++;
    }
    if( n_jobs )
        *n_jobs = n;
    return 0;
}

// diagnostics: what became of the extension jobs tried on the proven narrow band (ksw_band.h) since the library was loaded:
// tried, proved, failed check 1 / 2 / 3 / 4, handed back for another reason, diagonals run
int ma_debug_band_stats( unsigned long long out[ 8 ] )
{
    if( !out )
        return fail( "ma_debug_band_stats: null argument" );
    // (a static __device__ array per translation unit: the pipeline's kernels count here, those of ma_ksw_ext_batch in prims.hip)
    unsigned long long other[ 8 ];
    MA_HIP( hipMemcpyFromSymbol( out, HIP_SYMBOL( ma::g_band_stats ), 8 * 8 ) );
    if( ma::band_stats_of_prims( other ) )
        return 1;
    for( int i = 0; i < 8; i++ )
        out[ i ] += other[ i ];
    return 0;
}

// the same for the LONG extension jobs, one per wavefront on the band of 120 (ksw_band.h, G = 1)
int ma_debug_band_long_stats( unsigned long long out[ 8 ] )
{
    if( !out )
        return fail( "ma_debug_band_long_stats: null argument" );
    unsigned long long other[ 8 ];
    MA_HIP( hipMemcpyFromSymbol( out, HIP_SYMBOL( ma::g_band_stats ), 8 * 8, 8 * 8 ) );
    if( ma::band_long_stats_of_prims( other ) )
        return 1;
    for( int i = 0; i < 8; i++ )
        out[ i ] += other[ i ];
    return 0;
}

// diagnostics: DP cells computed and jobs finished per kernel family since the library was loaded (ksw_launch.h: g_dp_family):
// out[ 2 f ], out[ 2 f + 1 ] for f = 0 k_ksw_ext<1>, 1 k_ksw_ext<2>, 2 k_ksw_grp<2>, 3 k_ksw_grp<4>, 4 k_ksw_band (four short jobs per wave),
// 5 k_ksw_pk, 6 k_ksw, 7 k_ksw_band (one long job per wave)
int ma_debug_dp_family_stats( unsigned long long out[ 16 ] )
{
    if( !out )
        return fail( "ma_debug_dp_family_stats: null argument" );
    unsigned long long other[ 2 * KSW_N_FAMILIES ];
    MA_HIP( hipMemcpyFromSymbol( out, HIP_SYMBOL( ma::g_dp_family ), 2 * KSW_N_FAMILIES * 8 ) );
    if( ma::dp_family_stats_of_prims( other ) )
        return 1;
    for( int i = 0; i < 2 * KSW_N_FAMILIES; i++ )
        out[ i ] += other[ i ];
    return 0;
}

#if defined( MA_CHAIN_PROF )
int ma_debug_chain_prof( unsigned long long* out )
{
    MA_HIP( hipMemcpyFromSymbol( out, HIP_SYMBOL( ma::g_chain_prof ), 16 * 8 ) );
    return 0;
}
#endif

#if defined( MA_KSW_PROF )
int ma_debug_ksw_prof( unsigned long long* out )
{
    MA_HIP( hipMemcpyFromSymbol( out, HIP_SYMBOL( ma::g_ksw_prof ), 16 * 8 ) );
    return 0;
}
int ma_debug_pk_prof( unsigned long long* out )
{
    MA_HIP( hipMemcpyFromSymbol( out, HIP_SYMBOL( ma::g_pk_prof ), 16 * 8 ) );
    return 0;
}
int ma_debug_grp_prof( unsigned long long* out ) // 24 words (ksw_grp.h)
{
    MA_HIP( hipMemcpyFromSymbol( out, HIP_SYMBOL( ma::g_grp_prof ), 24 * 8 ) );
    return 0;
}
int ma_debug_seed_prof( unsigned long long* out )
{
    MA_HIP( hipMemcpyFromSymbol( out, HIP_SYMBOL( g_seed_prof ), 8 * 8 ) );
    return 0;
}
#endif

} // extern "C"

#include "launch_pair.h"

#include "launch_sam.h"

#include "launch_inv.h"

#include "launch_text.h"
#include "launch_genome.h"

#include "launch_bgzf.h"

#include "../host/ma_mates_bgzf_dev.h"
#include "launch_mates_bgzf.h"

#include "launch_deflate.h"
