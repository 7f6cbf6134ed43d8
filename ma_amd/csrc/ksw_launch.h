// ksw_launch.h -- persistent-wave driver around ksw_wave_core: every 64-thread workgroup (= one
// wavefront) pulls DP job slots from an atomic counter until none are left.  Also the kernel classes of the DP jobs (KSW_CLS_*), the
// one router that assigns them (ksw_route_job), the job population the launches are sized for (KswSizing), the table of a stage's
// launches (KswLaunch rows in issue order inside a KswStagePlan: kernel, job list, queue, lane, waves, LDS, scratch), the pure function
// that plans it (ksw_plan_stage) and the loop that reads the two environment hooks, plans, and issues the rows (ksw_run_all).
#pragma once
#include "internal.h"
#include "ksw_wave.h"
#include "ksw_reg.h"
#include "ksw_ext.h"
#include "ksw_pk.h"
#include "nw.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace ma
{
struct KswWaveScratch
{
    uint8_t* base; // per-wave HBM scratch
    u64 stride; // bytes per wave
    u64 state_cap; // bytes reserved for u|v|..|qr (used in HBM mode)
    u64 h_cap; // bytes for H
    u64 p_cap; // direction bytes
    u64 cig_cap; // cigar entries
    u32 use_lds; // state + H in dynamic LDS
};

struct KswOut
{
    ma_ez* ez; // per slot
    u64* cig_off; // per slot
    u32* cig_pool;
    u64 cig_pool_cap;
    unsigned long long* cig_used;
    unsigned long long* cells; // sum of band cells
    unsigned long long* njobs;
    unsigned long long* path; // back-trace steps
    unsigned long long* cig_words; // cigar words written (may be null)
    u32* err;
    u32 cig_chunk; // 0: one pool atomic per job (dense pool); else each wave reserves pool space this many words at a time
};

// Per-wave running totals and the wave's current cigar-pool reservation: the device-wide counters sit in one cache
// line, and same-line atomics serialise in L2 (~9 ns each), so they are touched once per wave, not once per job.
struct KswWaveAcc
{
    u64 cells = 0, njobs = 0, path = 0, cig_words = 0;
    u64 chunk_off = 0;
    u32 chunk_left = 0;
};
#define KSW_JOBS_PER_FETCH 8u // queue entries a wave takes per atomic
// ... when the launch has jobs in plenty.  With few jobs per wave -- the long junk extensions of a 10 kb batch on k_ksw_pk<5> (8.5 k jobs
// of ~8 ms on 4 096 waves), the handful of jobs the band of 120 hands back -- eight at a time leaves most waves without work and
// makes the launch as long as eight jobs in a row (10 kb: the 150 handed-back jobs were a tail of 40 ms on 19 waves): one at a time.
__device__ __forceinline__ u32 ksw_fetch_size( u32 n )
{
    return n / gridDim.x >= 32u ? KSW_JOBS_PER_FETCH : 1u;
}

// exact jobs by the number of 128-cell ring slots they need (ksw_pk_slots): 1, 2, 3, <= 5, else the LDS kernel
#define KSW_S0 1
#define KSW_S1 2
#define KSW_S2 3
#define KSW_S3 5
// Kernel classes of the DP jobs.  A job list, a launch and a word of every per-class counter bank (KswSizing, CTR_CLS0 /
// CTR_MAX_PC0 / CTR_MAX_CIGC0 of the pipeline) are indexed by these.
enum : int
{
    KSW_CLS_PK0 = 0, // exact register kernel k_ksw_pk<S> (ksw_pk.h), S = KSW_S0 .. KSW_S3 ring slots
    KSW_CLS_PK1 = 1,
    KSW_CLS_PK2 = 2,
    KSW_CLS_PK3 = 3,
    KSW_CLS_LDS = 4, // exact kernel with its state in LDS / HBM, k_ksw (ksw_wave.h): whatever fits no register kernel
    KSW_CLS_EXT1 = 5, // extension kernel k_ksw_ext<R> (ksw_ext.h) with R = 1 / 2 slots
    KSW_CLS_EXT2 = 6,
    KSW_CLS_GRP0 = 7, // first of the KSW_GRP_LISTS lists of extensions that share a wavefront; from here on the scratch per wave is fixed
    KSW_CLS_NARROW_L = 7, // the proven narrow band k_ksw_band (ksw_band.h): 4 jobs of up to 254 query bases per wave, left / right
    KSW_CLS_NARROW_R = 8,
    KSW_CLS_GRP2_L = 9, // query-stationary k_ksw_grp<2> (ksw_grp.h): 2 jobs of up to 64 query bases per wave, left / right
    KSW_CLS_GRP2_R = 10,
    KSW_CLS_GRP4_L = 11, // k_ksw_grp<4>: 4 jobs of up to 32 query bases per wave, left / right
    KSW_CLS_GRP4_R = 12,
    KSW_CLS_BANDL = 13, // LONG extension jobs on the proven band of 120, k_ksw_band<.., 1>: one per wave, left / right
    KSW_CLS_BANDL_L = 13,
    KSW_CLS_BANDL_R = 14,
    KSW_N_CLASSES = 15
};
// Words of `next`, the zeroed u32 counters of ksw_run_all: one job queue per launch, and the lengths of the lists the kernels append to
enum : int
{
    KSW_NX_CLS = 0, // + class, KSW_CLS_PK0 .. KSW_CLS_EXT2: queue of the class's own launch
    KSW_NX_REDO = 7, // + k: queue of k_ksw_pk<k> over the jobs handed back to the exact kernels (second pass)
    KSW_NX_GRP = 11, // + list, 0 .. KSW_GRP_LISTS - 1: queues of the wavefront-sharing launches
    KSW_NX_BAND_EXT = 17, // + 0 / 1: jobs the narrow band appended to the lists of KSW_CLS_EXT1 / EXT2
    KSW_NX_BANDL = 19, // + 0 / 1: queues of the two launches on the band of 120
    KSW_NX_REDOL = 21, // + k: queue of k_ksw_pk<k> over the long jobs the band of 120 handed back (when they have a stream of their own)
    KSW_NX_N_REDOL = 25, // ... and the number of those jobs
    KSW_N_NEXT = 28, // words of `next` (the last two are spare)
    KSW_N_NEXT_BIG = 4 // words of `nextBig`: + k, queue of the huge tier of class k
};
MA_HD int ksw_job_class( i32 qlen, i32 tlen, i32 w )
{
    if( qlen > 150000 )
        return KSW_CLS_LDS; // the register kernels keep the reversed query in LDS (160 KB per CU)
    const i32 n = ksw_pk_slots( qlen, tlen, w ); // 128-cell slots of the two-cells-per-lane kernel (ksw_pk.h)
    return n <= KSW_S0 ? KSW_CLS_PK0 : ( n <= KSW_S1 ? KSW_CLS_PK1 : ( n <= KSW_S2 ? KSW_CLS_PK2 : ( n <= KSW_S3 ? KSW_CLS_PK3 : KSW_CLS_LDS ) ) );
}
// per-wave scratch of one job: direction bytes of the exact kernels (n_col bytes per diagonal) / of the extension kernel
// (one ring row per diagonal)
MA_HD u64 ksw_p_bytes( i32 qlen, i32 tlen, i32 w )
{
    return (u64)ksw_max_diags( qlen, tlen, w ) * (u64)( ksw_ncol( qlen, tlen, w ) * 16 ) + 16;
}
MA_HD u64 ksw_ext_p_bytes( i32 qlen, i32 tlen, int R )
{
    return (u64)( (i64)qlen + tlen - 1 ) * (u64)( 128 * R ) + 16;
}

// result record + cigar of one finished job -> output arrays (all 64 lanes call this)
__device__ __forceinline__ void ksw_publish( const KswOut& O, KswWaveAcc& A, u32 slot, const KswEz& ez, u32 nCig, u64 cells,
                                             u64 path, const u32* cig, unsigned long long* sOff )
{
    A.cells += cells;
    A.njobs += 1;
    A.path += path;
    A.cig_words += nCig;
    u64 off;
    if( O.cig_chunk == 0 || nCig > O.cig_chunk )
    {
        if( threadIdx.x == 0 )
            *sOff = atomicAdd( O.cig_used, (unsigned long long)nCig );
        __syncthreads( );
        off = *sOff;
        __syncthreads( );
    }
    else
    {
        if( nCig > A.chunk_left )
        {
            if( threadIdx.x == 0 )
                *sOff = atomicAdd( O.cig_used, (unsigned long long)O.cig_chunk );
            __syncthreads( );
            A.chunk_off = *sOff;
            A.chunk_left = O.cig_chunk;
            __syncthreads( );
        }
        off = A.chunk_off;
        A.chunk_off += nCig;
        A.chunk_left -= nCig;
    }
    const bool fits = off + nCig <= O.cig_pool_cap;
    if( threadIdx.x == 0 )
    {
        ma_ez r;
        r.max = (i32)ez.max;
        r.zdropped = ez.zdropped;
        r.max_q = ez.max_q;
        r.max_t = ez.max_t;
        r.mqe = ez.mqe;
        r.mqe_t = ez.mqe_t;
        r.mte = ez.mte;
        r.mte_q = ez.mte_q;
        r.score = ez.score;
        r.reach_end = ez.reach_end;
        r.n_cigar = (i32)nCig;
        O.ez[ slot ] = r;
        O.cig_off[ slot ] = off;
        if( !fits )
            atomicOr( O.err, MA_ERR_CIGAR_OVERFLOW );
    }
    if( fits )
        for( u32 i = threadIdx.x; i < nCig; i += 64 )
            O.cig_pool[ off + i ] = cig[ i ];
    __syncthreads( ); // the scratch cigar may be overwritten by the next job
}
// cells computed and jobs finished per DP kernel FAMILY since the library was loaded (ma_debug_dp_family_stats; bench.py divides a
// family's VALU instructions of the PMC pass by ITS cells): 0 k_ksw_ext<1>, 1 k_ksw_ext<2>, 2 k_ksw_grp<2>, 3 k_ksw_grp<4>,
// 4 k_ksw_band (four short jobs per wave), 5 k_ksw_pk, 6 k_ksw (LDS), 7 k_ksw_band (one long job per wave)
#define KSW_N_FAMILIES 8
static __device__ unsigned long long g_dp_family[ 2 * KSW_N_FAMILIES ];
__device__ __forceinline__ void ksw_flush( const KswOut& O, const KswWaveAcc& A, int family )
{
    if( threadIdx.x == 0 && A.njobs )
    {
        atomicAdd( g_dp_family + 2 * family, (unsigned long long)A.cells );
        atomicAdd( g_dp_family + 2 * family + 1, (unsigned long long)A.njobs );
        atomicAdd( O.cells, (unsigned long long)A.cells );
        atomicAdd( O.njobs, (unsigned long long)A.njobs );
        if( O.path )
            atomicAdd( O.path, (unsigned long long)A.path );
        if( O.cig_words )
            atomicAdd( O.cig_words, (unsigned long long)A.cig_words );
    }
}
// next queue position of this wave: KSW_JOBS_PER_FETCH entries per atomic
__device__ __forceinline__ bool ksw_next( unsigned int* nextSlot, u32 n, u32& cur, u32& end, u32* sSlot, u32& at )
{
    if( cur == end )
    {
        const u32 fetch = ksw_fetch_size( n );
        if( threadIdx.x == 0 )
            *sSlot = atomicAdd( nextSlot, fetch );
        __syncthreads( );
        cur = *sSlot;
        __syncthreads( );
        end = cur + fetch < n ? cur + fetch : n;
        if( cur >= n )
            return false;
    }
    at = cur++;
    return true;
}

} // namespace ma
#include "ksw_grp.h"
#include "ksw_band.h"
namespace ma
{
// pipeline mode: extensions whose callers read only max_q / max_t / cigar go to the extension kernels.  KswScoring carries the
// switches (grp: MA_KSW_GRP, 0 keeps the short extensions on the one-job-per-wavefront kernel; band_long: MA_KSW_BANDL) as a kernel
// argument of everything that classifies jobs, so host and device classify alike.
MA_HD int ksw_job_class_pipe( const KswScoring& SC, i32 qlen, i32 tlen, i32 w, i32 zdrop, i32 flag )
{
    const int e = ksw_ext_slots( SC, qlen, tlen, w, zdrop, flag );
    const int right = ( flag & KSW_EZ_RIGHT ) ? 1 : 0;
    if( e && SC.grp >= 1000 && ksw_band_ok( SC, qlen, tlen, w, zdrop, flag, SC.grp - 1000 ) )
        return KSW_CLS_NARROW_L + right;
    if( e == 1 && SC.grp != 0 )
        if( const int G = ksw_grp_size( SC, qlen, tlen, w, zdrop, flag ) )
            return ( G == 4 ? KSW_CLS_GRP4_L : KSW_CLS_GRP2_L ) + right;
    if( !e && SC.band_long && ksw_bandl_ok( SC, qlen, tlen, w, zdrop, flag ) )
        return KSW_CLS_BANDL_L + right;
    return e ? KSW_CLS_EXT1 + ( e - 1 ) : ksw_job_class( qlen, tlen, w );
}

// THE routing of a pipeline job: its final class, and what the sizing of the launches takes from it.  k_dp_enum (through
// ksw_route_slot) and the host path of ma_ksw_ext_batch (prims.hip) both come here.
struct KswRoute
{
    int cls; // class after both demotions
    u32 cig; // cigar words of the job's scratch
    u64 p; // direction bytes in its class's kernel (0 from KSW_CLS_GRP0 on: fixed scratch per wave)
    u64 pk; // direction bytes in the exact kernels (ksw_p_bytes) ...
    bool redo; // ... which count when its kernel may hand it back to them (pRedo / cigRedo)
    u32 bandlN; // a job on the band of 120: its min(qlen, tlen), else 0
    int ext; // a job on the narrow band: the extension class it goes on to if it fails its checks, else 0 ...
    u64 pExt; // ... and its direction bytes there
};
// qf / tf: base i of the query / target in DP order.  tryAll (MA_KSW_BAND_ALL, host only): no pre-filters, every eligible job is tried
// on its band.
template <typename QF, typename TF>
MA_HD KswRoute ksw_route_job( const KswScoring& SC, i32 qlen, i32 tlen, i32 w, i32 zdrop, i32 flag, const QF& qf, const TF& tf, bool tryAll )
{
    KswRoute R;
    R.cls = ksw_job_class_pipe( SC, qlen, tlen, w, zdrop, flag );
    // the narrow band is tried on the jobs whose query follows the target's main diagonal, the band of 120 on the long extensions whose
    // first bases follow the target with few edits; the others go to the kernels they would go to without the band
    if( !tryAll && SC.grp >= 1000 && ( R.cls == KSW_CLS_NARROW_L || R.cls == KSW_CLS_NARROW_R ) && !ksw_band_likely( qf, tf, qlen, tlen, SC.band_mis ) )
    {
        KswScoring S1 = SC;
        S1.grp = 1;
        R.cls = ksw_job_class_pipe( S1, qlen, tlen, w, zdrop, flag );
    }
    if( !tryAll && ( R.cls == KSW_CLS_BANDL_L || R.cls == KSW_CLS_BANDL_R ) && !ksw_bandl_likely( qf, tf, qlen, tlen ) )
    {
        KswScoring S1 = SC;
        S1.band_long = 0;
        R.cls = ksw_job_class_pipe( S1, qlen, tlen, w, zdrop, flag );
    }
    R.cig = (u32)( qlen + tlen + 2 );
    R.pk = ksw_p_bytes( qlen, tlen, w );
    R.p = R.cls >= KSW_CLS_GRP0 ? 0 : ( R.cls >= KSW_CLS_EXT1 ? ksw_ext_p_bytes( qlen, tlen, R.cls - KSW_CLS_EXT1 + 1 ) : R.pk );
    R.redo = R.cls >= KSW_CLS_EXT1;
    R.bandlN = R.cls == KSW_CLS_BANDL_L || R.cls == KSW_CLS_BANDL_R ? (u32)( qlen < tlen ? qlen : tlen ) : 0u;
    R.ext = 0, R.pExt = 0;
    if( SC.grp >= 1000 && ( R.cls == KSW_CLS_NARROW_L || R.cls == KSW_CLS_NARROW_R ) )
    {
        const int e = ksw_ext_slots( SC, qlen, tlen, w, zdrop, flag );
        R.ext = KSW_CLS_EXT1 + ( e - 1 );
        R.pExt = ksw_ext_p_bytes( qlen, tlen, e );
    }
    return R;
}
// ... of a job slot of the pipeline: the bases come from the batch's reads and the packed reference
MA_HD KswRoute ksw_route_slot( const KswScoring& SC, const IndexView& X, const uint8_t* reads, const DpJob& j )
{
    const uint8_t* qb = reads + j.read_off;
    auto qf = [ & ]( i32 i ) -> u32 { return j.rev ? qb[ j.q_to - 1 - (u32)i ] : qb[ j.q_from + (u32)i ]; };
    auto tf = [ & ]( i32 i ) -> u32 { return text_base( X, j.win_begin + ( j.rev ? j.r_to - 1 - (u32)i : j.r_from + (u32)i ) ); };
    return ksw_route_job( SC, (i32)( j.q_to - j.q_from ), (i32)( j.r_to - j.r_from ), j.w, j.zdrop, j.flag, qf, tf, false );
}

// job source of a launch: mode 0 = list[0..n), 1 = every slot 0..n that is valid and of class cls,
// 2 = list[0..*nDev) filtered by class cls (the jobs the extension kernel handed back)
struct KswJobs
{
    const u32* list;
    u32 n;
    const unsigned int* nDev;
    int mode, cls;
    // a class with a few huge jobs is run as two launches: tier 1 takes the jobs with ksw_p_bytes <= pSplit and
    // ksw_q_lds <= qSplit (scratch and LDS of a full set of waves), tier 2 the others on fewer waves; tier 0 takes all
    int tier;
    u64 pSplit;
    i32 qSplit;
};
MA_HD bool ksw_tier_takes( const KswJobs& JB, i32 qlen, i32 tlen, i32 w )
{
    if( JB.tier == 0 )
        return true;
    const bool small = ksw_p_bytes( qlen, tlen, w ) <= JB.pSplit && ksw_q_lds( qlen, tlen, w ) <= (i64)JB.qSplit;
    return JB.tier == 1 ? small : !small;
}

#if defined( MA_KSW_PROF )
#define KSW_PROF_T( v ) const unsigned long long v = clock64( )
#define KSW_PROF_ADD( i, a, b ) prof[ i ] += ( b ) - ( a )
#define KSW_PROF_ARG , prof
#else
#define KSW_PROF_ARG
#define KSW_PROF_T( v )
#define KSW_PROF_ADD( i, a, b )
#endif

template <typename FETCH, int R>
__global__ void __launch_bounds__( 64 ) __attribute__( ( amdgpu_waves_per_eu( R == 1 ? 7 : 4 ) ) ) k_ksw_ext( FETCH F, KswScoring SC, const u32* list, u32 n, unsigned int* nextSlot,
                                                  uint8_t* scratch, u64 stride, u64 p_cap, u32 ldsBytes, KswOut O,
                                                  u32* redo, unsigned int* nRedo, const unsigned int* nMore /*jobs k_ksw_band appended to the list, or null*/ )
{
    extern __shared__ __attribute__( ( aligned( 16 ) ) ) char lds[];
    if( nMore )
        n += *nMore;
    __shared__ u32 sSlot;
    __shared__ unsigned long long sOff;
    __shared__ uint2 sSnap[ 64 * R ]; // the lanes' H of the diagonal that raised ez.max last (ksw_ext.h)
    uint8_t* my = scratch + (u64)blockIdx.x * stride;
    u32* cig = (u32*)( my + p_cap );
#if defined( MA_KSW_PROF )
    unsigned long long prof[ 16 ] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
#endif
    KswWaveAcc acc;
    u32 qCur = 0, qEnd = 0;
    while( true )
    {
        KSW_PROF_T( t0 );
        u32 at;
        if( !ksw_next( nextSlot, n, qCur, qEnd, &sSlot, at ) )
            break;
        const u32 slot = list[ at ];
        const KswJobView J = F.view( slot );
        KswEz ez;
        u32 nCig = 0;
        u64 cells = 0, path = 0;
        auto qf = F.qfetch( slot );
        auto tf = F.tfetch( slot );
        bool ok;
        KSW_PROF_T( t1 );
        if( !( J.flag & KSW_EZ_EXTZ_ONLY ) )
        {
            if( J.flag & KSW_EZ_RIGHT )
                ok = ksw_ext_core<R, false, true>( SC, J, qf, tf, (uint8_t*)lds, ldsBytes, my, cig, ez, nCig, cells, path, sSnap KSW_PROF_ARG );
            else
                ok = ksw_ext_core<R, true, true>( SC, J, qf, tf, (uint8_t*)lds, ldsBytes, my, cig, ez, nCig, cells, path, sSnap KSW_PROF_ARG );
        }
        else if( J.flag & KSW_EZ_RIGHT )
            ok = ksw_ext_core<R, false, false>( SC, J, qf, tf, (uint8_t*)lds, ldsBytes, my, cig, ez, nCig, cells, path, sSnap KSW_PROF_ARG );
        else
            ok = ksw_ext_core<R, true, false>( SC, J, qf, tf, (uint8_t*)lds, ldsBytes, my, cig, ez, nCig, cells, path, sSnap KSW_PROF_ARG );
        if( !ok )
        {
            if( threadIdx.x == 0 )
                redo[ atomicAdd( nRedo, 1u ) ] = slot;
            continue;
        }
        KSW_PROF_T( t2 );
        ksw_publish( O, acc, slot, ez, nCig, cells, path, cig, &sOff );
        KSW_PROF_T( t3 );
        KSW_PROF_ADD( 0, t0, t1 );
        KSW_PROF_ADD( 1, t1, t2 );
        KSW_PROF_ADD( 2, t2, t3 );
        KSW_PROF_ADD( 3, 0ull, 1ull );
#if defined( MA_KSW_PROF )
        // wave time (fetch .. publish) of the jobs that would fit HALF a wavefront (two jobs per wave: qlen + 2 <= 64 cells),
        // of those that would fit a quarter, and their numbers: the upper bound of what packing several jobs into one
        // wavefront can save (profiles/r03_ext_pairing_bound.txt)
        if( J.qlen + 2 <= 64 || J.tlen <= 64 )
        {
            prof[ 14 ] += t3 - t0;
            prof[ 15 ] += 1;
        }
        if( J.qlen + 2 <= 32 || J.tlen <= 32 )
        {
            prof[ 10 ] += t3 - t0; // (the GLOBAL slots 10 / 11 are re-used: see tools/ksw_prof.py)
            prof[ 11 ] += 1;
        }
        prof[ 9 ] += t3 - t0;
#endif
    }
    ksw_flush( O, acc, R == 1 ? 0 : 1 );
#if defined( MA_KSW_PROF )
    if( threadIdx.x == 0 )
        for( int i = 0; i < 16; i++ )
            atomicAdd( &g_ksw_prof[ i ], prof[ i ] );
#endif
}

#if !defined( MA_PK5_WAVES )
#define MA_PK5_WAVES 4
#endif
template <typename FETCH, int S>
__global__ void __launch_bounds__( 64 ) __attribute__( ( amdgpu_waves_per_eu( S >= 5 ? MA_PK5_WAVES : 3 ) ) ) k_ksw_pk( FETCH F, KswScoring SC, KswJobs JB, unsigned int* nextSlot,
                                                  uint8_t* scratch, u64 stride, u64 p_cap, u32 ldsBytes, KswOut O )
{
    extern __shared__ __attribute__( ( aligned( 16 ) ) ) char lds[];
    __shared__ u32 sSlot;
    __shared__ unsigned long long sOff;
    __shared__ int2 sSnap[ 64 * S ]; // the lanes' H of the diagonal that raised ez.max last (ksw_pk.h)
    uint8_t* my = scratch + (u64)blockIdx.x * stride;
    uint8_t* P = my;
    u32* cig = (u32*)( my + p_cap );
    const u32 n = JB.mode == 2 ? *JB.nDev : JB.n;
    KswWaveAcc acc;
    u32 qCur = 0, qEnd = 0;
    while( true )
    {
        u32 at;
        if( !ksw_next( nextSlot, n, qCur, qEnd, &sSlot, at ) )
            break;
        const u32 slot = JB.mode == 1 ? at : JB.list[ at ];
        if( JB.mode == 1 && !F.valid( slot ) )
            continue;
        const KswJobView J = F.view( slot );
        if( JB.mode != 0 && ksw_job_class( J.qlen, J.tlen, J.w ) != JB.cls )
            continue;
        if( !ksw_tier_takes( JB, J.qlen, J.tlen, J.w ) )
            continue;
        KswEz ez;
        u32 nCig = 0;
        u64 cells = 0, path = 0;
        auto qf = F.qfetch( slot );
        auto tf = F.tfetch( slot );
        ksw_pk_core<S, FETCH::EARLY>( SC, J, qf, tf, (uint8_t*)lds, P, cig, ez, nCig, cells, path, ldsBytes, sSnap );
        ksw_publish( O, acc, slot, ez, nCig, cells, path, cig, &sOff );
    }
    ksw_flush( O, acc, 5 );
}

template <typename FETCH>
__global__ void __launch_bounds__( 64 ) k_ksw( FETCH F, KswScoring SC, KswJobs JB, unsigned int* nextSlot,
                                              KswWaveScratch WS, u32 ldsBytes, KswOut O )
{
    extern __shared__ __attribute__( ( aligned( 16 ) ) ) char lds[];
    __shared__ u32 sSlot;
    uint8_t* my = WS.base + (u64)blockIdx.x * WS.stride;
    KswMem M;
    if( WS.use_lds )
    {
        M.u = (int8_t*)lds;
        M.H = (void*)( lds + WS.state_cap );
        M.p = my;
        M.cig = (u32*)( my + WS.p_cap );
        M.stage = (uint8_t*)lds;
        M.stageBytes = ldsBytes;
    }
    else
    {
        M.u = (int8_t*)my;
        M.H = (void*)( my + WS.state_cap );
        M.p = my + WS.state_cap + WS.h_cap;
        M.cig = (u32*)( my + WS.state_cap + WS.h_cap + WS.p_cap );
        M.stage = nullptr;
        M.stageBytes = 0;
    }
    __shared__ unsigned long long sOff;
    const u32 n = JB.mode == 2 ? *JB.nDev : JB.n;
    KswWaveAcc acc;
    u32 qCur = 0, qEnd = 0;
    while( true )
    {
        u32 at;
        if( !ksw_next( nextSlot, n, qCur, qEnd, &sSlot, at ) )
            break;
        const u32 slot = JB.mode == 1 ? at : JB.list[ at ];
        if( JB.mode == 1 && !F.valid( slot ) )
            continue;
        const KswJobView J = F.view( slot );
        if( JB.mode != 0 && ksw_job_class( J.qlen, J.tlen, J.w ) != KSW_CLS_LDS )
            continue; // handled by a register-resident launch
        M.L = ( ( J.tlen + 15 ) / 16 ) * 16;
        KswEz ez;
        u32 nCig = 0;
        u64 cells = 0, path = 0;
        auto qf = F.qfetch( slot );
        auto tf = F.tfetch( slot );
        if( ksw_h16( SC, J.qlen, J.tlen ) )
            ksw_wave_core<int16_t, 8>( SC, J, qf, tf, M, ez, nCig, cells, path );
        else
            ksw_wave_core<int32_t, 4>( SC, J, qf, tf, M, ez, nCig, cells, path );
        ksw_publish( O, acc, slot, ez, nCig, cells, path, M.cig, &sOff );
    }
    ksw_flush( O, acc, 6 );
}

inline i32 ksw_grp_env( ) // KswScoring::grp (read on every call: the tests switch it inside one process)
{
    const char* e = getenv( "MA_KSW_GRP" );
    // 0: one job per wavefront; 1: queries of up to 64 bases share a wavefront (2, once the four-rows-per-lane experiment of DESIGN.md
    // section 3.4, reads as 1); 3 (or 1000 + n): extensions of 65 (n) .. 254 query bases on the proven narrow band, four per wave
    // (ksw_band.h).  Default: 1033 (150 bp: DP 19.0 ms with 1, 16.4 with 3, 15.7 with 1033)
    const i32 v = e ? std::max( 0, atoi( e ) ) : 1033;
    return v == 3 ? 1065 : ( v >= 1000 ? std::min( v, 1000 + KSW_BAND_QMAX ) : std::min( v, 1 ) );
}
inline i32 ksw_bandl_env( ) // KswScoring::band_long
{
    const char* e = getenv( "MA_KSW_BANDL" );
    return e ? ( atoi( e ) != 0 ? 1 : 0 ) : 1;
}
inline i32 ksw_band_mis_env( )
{
    const char* e = getenv( "MA_KSW_BAND_MAXMIS" );
    return e ? std::max( 0, std::min( 64, atoi( e ) ) ) : KSW_BAND_MAXMIS;
}
// sizes for a job population (host side)
struct KswSizing
{
    u64 state = 0, h = 0, p = 0, cig = 0;
    u64 qlen = 0; // longest query (LDS bytes of the register kernels)
    u64 cls[ KSW_N_CLASSES ] = { }; // jobs per class
    u64 pc[ KSW_N_CLASSES ] = { }; // largest direction-byte scratch of a job, per class (0: use p)
    u64 cigc[ KSW_N_CLASSES ] = { }; // largest cigar scratch in words, per class (0: use cig)
    u64 pRedo = 0, cigRedo = 0; // the same for jobs the extension kernel hands back to the exact kernels (0: use p / cig)
    u64 bandlN = 0; // largest min(qlen, tlen) of the long jobs on the band of 120 (their scratch: KSW_BANDL_ROWS( N ) direction rows per wave)
};
inline void ksw_size_job( KswSizing& S, i32 qlen, i32 tlen, i32 w )
{
    if( qlen <= 0 || tlen <= 0 )
        return;
    const int k = ksw_job_class( qlen, tlen, w );
    S.cls[ k ]++;
    S.qlen = S.qlen > (u64)qlen ? S.qlen : (u64)qlen;
    const u64 st = ksw_state_bytes( qlen, tlen );
    const u64 L = (u64)( ( tlen + 15 ) / 16 ) * 16;
    const u64 p = ksw_p_bytes( qlen, tlen, w );
    S.pc[ k ] = S.pc[ k ] > p ? S.pc[ k ] : p;
    S.cigc[ k ] = S.cigc[ k ] > (u64)qlen + tlen + 2 ? S.cigc[ k ] : (u64)qlen + tlen + 2;
    S.state = S.state > st ? S.state : st;
    S.h = S.h > L * 4 ? S.h : L * 4;
    S.p = S.p > p ? S.p : p;
    const u64 c = (u64)qlen + tlen + 2;
    S.cig = S.cig > c ? S.cig : c;
}
// ... and what a routed pipeline job adds to the per-class part (k_dp_enum does the same with atomics on the batch's counters)
inline void ksw_size_route( KswSizing& S, const KswRoute& R )
{
    S.cls[ R.cls ]++;
    S.pc[ R.cls ] = std::max( S.pc[ R.cls ], R.p );
    S.cigc[ R.cls ] = std::max<u64>( S.cigc[ R.cls ], R.cig );
    S.bandlN = std::max<u64>( S.bandlN, R.bandlN );
    if( R.redo )
    {
        S.pRedo = std::max( S.pRedo, R.pk );
        S.cigRedo = std::max<u64>( S.cigRedo, R.cig );
    }
    if( R.ext )
    {
        S.pc[ R.ext ] = std::max( S.pc[ R.ext ], R.pExt );
        S.cigc[ R.ext ] = std::max<u64>( S.cigc[ R.ext ], R.cig );
    }
}

// ---- The launches of one DP stage as a table: ksw_plan_stage writes it (no HIP call: tests/emul/dp_plan_test.cpp runs it on the
// CPU), ksw_run_all issues it row by row.  A row names its kernel by family and instantiation and its pointers by index.
enum : int
{
    KSW_FAM_PK = 0, // k_ksw_pk<S>; inst = the class, KSW_CLS_PK0 .. PK3
    KSW_FAM_EXT, // k_ksw_ext<R>; inst = R
    KSW_FAM_GRP, // k_ksw_grp<G, 1, LEFT>; inst = the class, KSW_CLS_GRP2_L .. GRP4_R
    KSW_FAM_BAND4, // k_ksw_band<.., 4>, the narrow band; inst = 1 left, 0 right
    KSW_FAM_BAND1, // k_ksw_band<.., 1>, the band of 120; inst = 1 left, 0 right
    KSW_FAM_LDS // k_ksw; inst = the class, KSW_CLS_LDS
};
// A counter of a row is a word of `next` (KSW_NX_*) or one of KSW_CT_*; a list is lists + index * list_stride, the index a class (its jobs)
// or one of KSW_LIST_*.
enum : int
{
    KSW_NONE = -1, // no counter, no list: null
    KSW_CT_BIG = KSW_N_NEXT, // + k: word k of `nextBig`
    KSW_CT_NREDO = KSW_N_NEXT + KSW_N_NEXT_BIG, // *nRedo
    KSW_LIST_REDO = KSW_N_CLASSES, // the jobs handed back to the exact kernels
    KSW_LIST_REDOL = KSW_N_CLASSES + 1 // the long jobs the band of 120 handed back, when they have a stream of their own
};
struct KswLaunch
{
    int family = 0, inst = 0; // KSW_FAM_*
    int lane = 0; // 0 .. 3: stream and scratch region (KswSide)
    u32 waves = 0; // grid (0: nothing planned)
    u32 lds = 0; // dynamic LDS bytes of the launch (register kernels: reversed query of ITS longest job)
    int queue = KSW_NONE; // counter: the launch's job queue
    int list = KSW_NONE; // list: its jobs (KSW_NONE: it scans the slots)
    int nDev = KSW_NONE; // counter: KswJobs::nDev
    KswJobs jb = { }; // n, mode, cls, tier, pSplit, qSplit; of the kernels that take no KswJobs: n (list and nDev: set from the indices when launching)
    u64 stride = 0, p_cap = 0; // scratch bytes per wave, direction bytes among them
    int out1 = KSW_NONE, out2 = KSW_NONE; // lists: where the kernel appends the jobs it hands back (narrow band: hands on to k_ksw_ext<1> / <2>) ...
    u32 nOut1 = 0, nOut2 = 0; // ... the entries there before the launch (narrow band) ...
    int outCtr = KSW_NONE; // ... counter: of the appended ones
    int nMore = KSW_NONE; // counter: jobs the narrow band appended to the list (k_ksw_ext)
    KswWaveScratch ws = { }; // k_ksw (base: set when launching)
};
#define KSW_MAX_LAUNCHES 27 // exact kernels 4 x (huge tier, own, handed back, handed back by the band of 120), band 2 + 2, k_ksw_grp 4, k_ksw_ext 2, k_ksw
struct KswStagePlan
{
    KswLaunch launch[ KSW_MAX_LAUNCHES ]; // in issue order
    int n = 0;
    u64 laneBase[ 4 ] = { }, total = 0; // byte offsets of the lanes' scratch regions; bytes of all four
    bool laneUsed[ 4 ] = { true, false, false, false }; // lanes 1 .. 3: fork from and join the batch's stream
    int bandAfter = -1; // after this row the event `band` is recorded and lane 3 waits for it (-1: no such event)
    u32 ldsPk = 0, ldsLds = 0; // LDS limit to set on the k_ksw_pk instantiations / on k_ksw (0: the default of 48 KB is enough)
};
// Scratch: every wave owns `stride` bytes (direction bytes + cigar of the job it is working on) of one allocation that
// the launches of a lane, which run back to back on one stream, share.  Each launch is sized for ITS class: the classes differ
// by orders of magnitude (gap between two seeds: KBs; end extension of a 50 kb read: 27 MB), and one stride for all
// would cut every launch down to the few hundred waves the largest job allows -- less than one wave per SIMD
// (50 kb reads: DP stage 2.4 s -> see DESIGN.md 3.6).  A class whose own largest job still does not leave room for a
// full set of waves is run as two launches: the jobs that fit a full set, then the few huge ones on fewer waves.
#define KSW_REG_LDS 6144u // per-wave LDS of the exact register kernels: reversed query, later the back-trace staging block
#define KSW_EXT_LDS 4096u // extension kernel: back-trace staging only (8 waves per SIMD fit)
// per-wave scratch of all resident waves of a launch may take this much HBM (MA_KSW_SCRATCH_MB: test hook that makes small
// batches take the paths of the large ones -- fewer waves, classes split in two launches, the side stream).
// B bounds ONE launch.  With the kernel classes on their own streams (the default for batches with job lists) four lanes of
// launches run side by side, each in its own region of B/4, 5B/12, B/3 and B/4 bytes: a batch whose DP stage needs more than
// 2 GB of scratch then holds 1.25 B (30 GB at the default), once per batch in flight -- DESIGN.md section 2 counts it that way.
inline u64 ksw_scratch_budget( )
{
    const char* e = getenv( "MA_KSW_SCRATCH_MB" ); // (read on every call: the tests switch it inside one process)
    return e && atoi( e ) > 0 ? (u64)atoi( e ) << 20 : 24ull << 30;
}
// scratch and waves of a launch whose waves each work on one job of up to p direction bytes and cigWords cigar words
inline KswLaunch ksw_plan_launch( u64 p, u64 cigWords, u64 jobs, u64 wantWaves, u64 budget )
{
    auto al = []( u64 x ) { return ( x + 255 ) / 256 * 256; };
    KswLaunch L;
    L.p_cap = al( p );
    L.stride = al( L.p_cap + al( cigWords * 4 ) );
    u64 waves = std::max<u64>( 1, std::min<u64>( wantWaves, jobs ) );
    if( L.stride * waves > budget )
        waves = std::max<u64>( 1, budget / L.stride );
    L.waves = (u32)waves;
    return L;
}
// ... of k_ksw: state and H of the longest job in LDS, or with the direction bytes in the wave's scratch
inline KswLaunch ksw_plan( const KswSizing& S, u64 nJobs, u64 budget )
{
    auto al = []( u64 x ) { return ( x + 255 ) / 256 * 256; };
    const u64 state = al( S.state ), h = al( S.h ), ldsNeed = state + h;
    const bool useLds = ldsNeed <= 64 * 1024;
    u64 waves = 256ull * 16; // 16 single-wave workgroups per CU
    if( useLds )
    {
        const u64 perCu = ( 160 * 1024 ) / ( ldsNeed ? ldsNeed : 1 );
        waves = 256ull * ( perCu > 16 ? 16 : ( perCu < 1 ? 1 : perCu ) );
    }
    KswLaunch P = ksw_plan_launch( ( useLds ? 0 : ldsNeed ) + al( S.p ), S.cig, nJobs, waves, budget );
    P.p_cap = al( S.p );
    P.lds = useLds ? (u32)ldsNeed : 0;
    P.ws = KswWaveScratch{ nullptr, P.stride, state, h, P.p_cap, S.cig, useLds ? 1u : 0u };
    return P;
}
// Streams of one DP stage.  The kernel classes of a stage are independent of each other, and each is a persistent launch
// that ends in a tail -- a few waves still working on their last jobs while the rest of the machine idles.  On ONE stream
// the tails add up (50 kb reads: five launches, five tails); on separate streams, each launch with its own scratch region,
// the next class's waves take the SIMDs the moment a class's waves retire, so only the last tail of the stage is paid.
//   lane 0 (the batch's stream): extension kernel classes, then the jobs they handed back, then the LDS kernel
//   lane 1: k_ksw_pk<5>            lane 2: k_ksw_pk<3>, <2>, <1>            lane 3: the huge tiers of split classes
struct KswSide
{
    hipStream_t stream[ 3 ] = { nullptr, nullptr, nullptr };
    hipEvent_t fork = nullptr, join[ 3 ] = { nullptr, nullptr, nullptr };
    hipEvent_t band = nullptr; // the long jobs' band kernels are done: their handed-back jobs start on lane 3 (KswStagePlan::bandAfter)
    bool ready( ) const
    {
        return stream[ 0 ] && stream[ 1 ] && stream[ 2 ];
    }
};
#define KSW_SIDE_WAVES 512u
// LDS bytes of a job's query window (ksw_q_lds) up to which it runs in the class's first tier: the register kernels'
// minimum per-wave LDS, so that 16 waves take 96 KB of a CU's 160 KB and the extension kernels' waves still fit beside them
#define KSW_Q_SPLIT KSW_REG_LDS

// Plans every launch of a stage whose job population is SZ.  `lists`: there are per-class job lists (without them every launch scans
// nSlots and there are no extension-kernel classes); `nextBig`: there are queues for huge tiers; side3 / side2 / sideBand: KswSide has
// all three streams / stream[ 2 ] / the event `band`; B: scratch budget of one launch (ksw_scratch_budget); perCu: waves per CU of
// the persistent launches.
inline KswStagePlan ksw_plan_stage( const KswSizing& SZ, const KswScoring& SC, u32 nSlots, bool lists, bool nextBig, bool side3, bool side2, bool sideBand,
                                    u64 B, u64 perCu )
{
    auto al = []( u64 x ) { return ( x + 255 ) / 256 * 256; };
    KswStagePlan P;
    u64 nJobs = 0;
    for( int k = 0; k < KSW_N_CLASSES; k++ )
        nJobs += SZ.cls[ k ];
    if( nJobs == 0 )
        return P;
    u64 nGrp = 0;
    for( int k = 0; k < KSW_GRP_LISTS; k++ )
        nGrp += SZ.cls[ KSW_CLS_GRP0 + k ];
    // jobs on the proven narrow band (ksw_band.h): those that fail a check are appended to the lists of k_ksw_ext<1> / <2>, which
    // run after them (next[ KSW_NX_BAND_EXT + 0 / 1 ] count them)
    const u64 nBand = SC.grp >= 1000 ? SZ.cls[ KSW_CLS_NARROW_L ] + SZ.cls[ KSW_CLS_NARROW_R ] : 0;
    const u64 nBandL = SZ.cls[ KSW_CLS_BANDL_L ] + SZ.cls[ KSW_CLS_BANDL_R ]; // long jobs on the band of 120; those that fail go to `redo`
    const u64 nExt = SZ.cls[ KSW_CLS_EXT1 ] + SZ.cls[ KSW_CLS_EXT2 ] + nGrp + nBandL;
    const bool conc = side3 && lists; // classes on their own streams
    const u64 wantWaves = 256ull * perCu;
    // Concurrent launches each own a scratch region, so each asks only for the waves that can be RESIDENT (registers:
    // k_ksw_pk<1> 74 VGPRs = 6 waves per SIMD, <2> 99, <3> 122, <5> 128 = 4; the extension kernels 7 / 4): a persistent wave
    // beyond that would only start when another one retires and its scratch would sit idle until then.
    const u64 resident[ KSW_CLS_GRP0 ] = { 256 * 24, 256 * 16, 256 * 16, 256 * 16, 0, 256 * 28, 256 * 16 };
    auto wantOf = [ & ]( int k ) { return conc ? std::min<u64>( wantWaves, resident[ k ] ) : wantWaves; };
    // budgets of the scratch regions: lane 0 / 1 / 2 (sequential launches of a lane share its region)
    const u64 budgetOf[ KSW_CLS_GRP0 ] = { conc ? B / 3 : B, conc ? B / 3 : B, conc ? B / 3 : B, conc ? 5 * B / 12 : B, B, conc ? B / 4 : B, conc ? B / 4 : B };
    auto ldsOf = []( u64 qBytes ) { return std::max<u32>( (u32)( ( ( std::min<u64>( qBytes, 150000 + 64 ) + 15 ) / 16 ) * 16 ), KSW_REG_LDS ); };
    // ---- sizes.  Register kernels: the classes' own launches (KSW_CLS_PK0 .. PK3 exact, KSW_CLS_EXT1 / EXT2 extension), the exact
    // classes' huge tiers, their second pass over the jobs handed back (RD: the same plan for the four), and the one over the long
    // jobs the band of 120 handed back (LPR).  Lanes: sequential mode, one region for all launches (+ one for the huge tiers when
    // they have a stream); concurrent mode, lane 0 = extension classes, handed-back jobs, LDS kernel; lane 1 = KSW_CLS_PK3;
    // lane 2 = KSW_CLS_PK0 .. PK2; lane 3 = huge tiers.
    KswLaunch own[ KSW_CLS_GRP0 ], big[ 4 ], RD, LPR, LG, LBL, LL;
    // k_ksw_grp: fixed scratch per wave (KSW_GRP_ROWS direction rows; the cigars stay in LDS), 5 waves per SIMD
    if( nGrp )
    {
        const u64 sets = ( SZ.cls[ KSW_CLS_NARROW_L ] + 1 ) / ( SC.grp >= 1000 ? 4 : 2 ) + ( SZ.cls[ KSW_CLS_NARROW_R ] + 1 ) / ( SC.grp >= 1000 ? 4 : 2 ) +
                         ( SZ.cls[ KSW_CLS_GRP2_L ] + 1 ) / 2 + ( SZ.cls[ KSW_CLS_GRP2_R ] + 1 ) / 2 + ( SZ.cls[ KSW_CLS_GRP4_L ] + 3 ) / 4 + ( SZ.cls[ KSW_CLS_GRP4_R ] + 3 ) / 4;
        LG = ksw_plan_launch( (u64)KSW_GRP_ROWS * 128, 0, sets, std::min<u64>( wantWaves, 256 * 20 ), conc ? B / 4 : B );
    }
    // LBL: k_ksw_band<.., 1>, KSW_BANDL_ROWS direction rows per wave, 5 waves per SIMD.
    // The few long jobs the band hands back (0.1 % of a 10 kb batch, and the long ones among them: queries AND targets of thousands of
    // bases) take tens of ms each in k_ksw_pk<5>.  Behind the extension kernels on the batch's stream they were a tail of their own
    // (10 kb: 38 of 161 ms); with streams they get their own list and start on lane 3 the moment the band kernels are done.
    const bool ownRedo = nBandL && conc && sideBand;
    if( nBandL )
    {
        // rows for the largest job of the batch, but no more than leave a full set of waves their scratch: the few larger jobs are handed
        // on by the kernel (a 7 900 x 7 900 job needs 2 MB of direction rows; sized for it, a launch of 10^5 jobs of 2 500 x 1 000 would
        // run on half its waves)
        const u64 wavesL = std::min<u64>( std::min<u64>( wantWaves, 256 * 20 ), nBandL );
        const u64 rowsFull = std::max<u64>( KSW_BANDL_ROWS( 2048 ), ( ( conc ? B / 4 : B ) / std::max<u64>( wavesL, 1 ) ) / 128 );
        const u64 rows = std::min<u64>( KSW_BANDL_ROWS( SZ.bandlN ? std::min<u64>( SZ.bandlN, KSW_BANDL_NMAX ) : KSW_BANDL_NMAX ), rowsFull );
        LBL = ksw_plan_launch( rows * 128, 0, nBandL, wavesL, conc ? B / 4 : B );
    }
    if( ownRedo )
    {
        LPR = ksw_plan_launch( SZ.pRedo ? SZ.pRedo : SZ.p, SZ.cigRedo ? SZ.cigRedo : SZ.cig, std::min<u64>( nBandL / 4 + 64, 256 * 8 ), wantWaves, B / 4 );
        LPR.lds = ldsOf( std::min<u64>( SZ.qlen, SZ.cigRedo ? SZ.cigRedo : SZ.qlen ) + 48 );
        LPR.lane = 3;
    }
    for( int k = 0; k < KSW_CLS_GRP0; k++ )
    {
        const bool isExt = k >= KSW_CLS_EXT1;
        if( k == KSW_CLS_LDS || ( SZ.cls[ k ] == 0 && !( isExt && nBand ) ) )
            continue;
        const u64 pk = SZ.pc[ k ] ? SZ.pc[ k ] : ( isExt ? std::max( SZ.p, ksw_ext_p_bytes( 256, 2048, k - KSW_CLS_EXT1 + 1 ) ) : SZ.p );
        const u64 cg = SZ.cigc[ k ] ? SZ.cigc[ k ] : SZ.cig;
        // (the narrow band hands on a few per cent of its jobs: the extension kernels' waves are planned for their own jobs plus a
        // sixteenth of the band's -- more of them would only wait their turn)
        own[ k ] = ksw_plan_launch( pk, cg, SZ.cls[ k ] + ( isExt && nBand ? nBand / 16 + 64 : 0 ), wantOf( k ), budgetOf[ k ] );
        if( isExt )
        {
            own[ k ].lds = KSW_EXT_LDS;
            own[ k ].nMore = nBand ? KSW_NX_BAND_EXT + ( k - KSW_CLS_EXT1 ) : KSW_NONE;
            continue;
        }
        // LDS bytes of the longest query of the class (ksw_q_lds <= round16( qlen ) + 32; qlen + tlen + 2 <= cigc[k])
        const u64 qMaxK = std::min<u64>( SZ.qlen, SZ.cigc[ k ] ? SZ.cigc[ k ] : SZ.qlen ) + 48;
        own[ k ].lds = ldsOf( qMaxK );
        const u64 full = std::min<u64>( wantOf( k ), SZ.cls[ k ] );
        const bool fewWaves = own[ k ].waves < full && own[ k ].waves < 256 * 16;
        // The reversed query of a job lives in LDS, sized for the longest job of the LAUNCH: one 49 kb end extension in a
        // class of 10^5 gap fills would leave 3 waves per CU to all of them (this, not the tails, held the exact kernels of the
        // 50 kb workload at a fifth of the issue rate).  Jobs whose query or direction matrix does not leave room for a full
        // set of waves go to the class's second tier: few waves, own scratch, own stream.
        const bool splitQ = qMaxK > KSW_Q_SPLIT;
        bool splitP = false;
        u64 pSmall = pk;
        if( fewWaves )
        {
            // direction bytes one wave of a full set can have, after its cigar scratch (a job of the small tier has
            // qlen + tlen <= pSmall / 16 + 1: a diagonal stores 16 bytes at least)
            const u64 room = budgetOf[ k ] / std::min<u64>( full, 256 * 16 );
            if( room > 8192 )
            {
                pSmall = std::min<u64>( pk, ( room - room / 5 - 512 ) / 256 * 256 ); // stride = p + 4 * (p / 16 + 3) + padding
                splitP = pSmall < pk;
            }
        }
        if( nextBig && ( splitP || splitQ ) )
        {
            big[ k ] = own[ k ]; // the huge jobs: what the small tier leaves
            big[ k ].jb.tier = 2;
            if( conc ) // their region is a fixed quarter of the budget (a region that follows the largest job of every batch
                       // would be re-allocated -- seconds, device-wide -- whenever a later batch brings a larger one)
                big[ k ].waves = (u32)std::max<u64>( 1, std::min<u64>( std::min<u32>( big[ k ].waves, KSW_SIDE_WAVES ), ( B / 4 ) / std::max<u64>( big[ k ].stride, 1 ) ) );
            const u64 cgSmall = splitP ? std::min<u64>( cg, pSmall / 16 + 3 ) : cg;
            own[ k ] = ksw_plan_launch( pSmall, cgSmall, SZ.cls[ k ], wantOf( k ), budgetOf[ k ] );
            own[ k ].jb.tier = 1;
            own[ k ].lds = ldsOf( std::min<u64>( qMaxK, KSW_Q_SPLIT ) );
            own[ k ].jb.pSplit = big[ k ].jb.pSplit = pSmall;
        }
    }
    if( nExt )
    {
        // (the band of 120 proves nearly all of its jobs: a quarter of them as waves of the second pass is plenty)
        RD = ksw_plan_launch( SZ.pRedo ? SZ.pRedo : SZ.p, SZ.cigRedo ? SZ.cigRedo : SZ.cig, std::min<u64>( nExt, 256 * 4 ) + std::min<u64>( nBandL / 4, 256 * 12 ),
                              wantWaves, conc ? B / 4 : B );
        RD.lds = ldsOf( std::min<u64>( SZ.qlen, SZ.cigRedo ? SZ.cigRedo : SZ.qlen ) + 48 );
    }
    if( SZ.cls[ KSW_CLS_LDS ] )
        LL = ksw_plan( SZ, SZ.cls[ KSW_CLS_LDS ], conc ? B / 4 : B );
    for( int k = KSW_CLS_PK0; k <= KSW_CLS_PK3; k++ )
        own[ k ].lane = !conc ? 0 : ( k == KSW_CLS_PK3 ? 1 : 2 ), big[ k ].lane = conc || side2 ? 3 : 0;
    // ---- scratch regions: a lane's region holds the largest of its launches
    u64 needLane[ 4 ] = { 0, 0, 0, 0 };
    u32 ldsMax = std::max( RD.lds, LPR.lds );
    auto need = [ & ]( const KswLaunch& L ) { needLane[ L.lane ] = std::max<u64>( needLane[ L.lane ], L.stride * L.waves ); };
    for( const KswLaunch* L : { &LL, &LG, &LBL, &LPR, &RD, own + KSW_CLS_EXT1, own + KSW_CLS_EXT2 } )
        need( *L );
    for( int k = KSW_CLS_PK0; k <= KSW_CLS_PK3; k++ )
    {
        need( own[ k ] ), need( big[ k ] );
        ldsMax = std::max( ldsMax, std::max( own[ k ].lds, big[ k ].lds ) );
    }
    // the per-wave scratch follows the largest jobs of the batch, which vary a lot from batch to batch for long
    // reads: once it is in the GB range take the whole budget so that later batches never re-allocate mid-step
    if( !conc && needLane[ 0 ] > ( 2ull << 30 ) )
        needLane[ 0 ] = std::max<u64>( needLane[ 0 ], B );
    if( conc && needLane[ 0 ] + needLane[ 1 ] + needLane[ 2 ] + needLane[ 3 ] > ( 2ull << 30 ) )
    {
        needLane[ 0 ] = std::max<u64>( needLane[ 0 ], B / 4 );
        needLane[ 1 ] = std::max<u64>( needLane[ 1 ], 5 * B / 12 );
        needLane[ 2 ] = std::max<u64>( needLane[ 2 ], B / 3 );
        needLane[ 3 ] = std::max<u64>( needLane[ 3 ], B / 4 );
    }
    for( int l = 0; l < 4; l++ )
    {
        P.laneBase[ l ] = P.total;
        P.total += al( needLane[ l ] );
    }
    P.ldsPk = ldsMax > 48 * 1024 ? ldsMax : 0;
    P.ldsLds = LL.lds > 48 * 1024 ? LL.lds : 0;
    // ---- the rows, in issue order
    auto push = [ & ]( const KswLaunch& L ) {
        if( L.waves == 0 )
            return;
        P.laneUsed[ L.lane ] = true;
        P.launch[ P.n++ ] = L;
    };
    // a launch of exact class k over its own list (the class's launch or its huge tier) or over a list of handed-back jobs (second pass)
    auto pushExact = [ & ]( KswLaunch L, int k, int queue, int list ) {
        const bool ownList = list == k, redoL = list == KSW_LIST_REDOL;
        L.family = k == KSW_CLS_LDS ? KSW_FAM_LDS : KSW_FAM_PK, L.inst = L.jb.cls = k, L.queue = queue;
        L.list = lists ? list : KSW_NONE;
        L.nDev = redoL ? KSW_NX_N_REDOL : KSW_CT_NREDO;
        L.jb.n = redoL ? 0u : ( lists ? (u32)SZ.cls[ k ] : nSlots );
        L.jb.mode = !ownList ? 2 : ( lists ? 0 : 1 );
        L.jb.pSplit = redoL ? 0 : own[ k ].jb.pSplit;
        L.jb.qSplit = k == KSW_CLS_LDS ? 0 : KSW_Q_SPLIT; // (k_ksw takes all the jobs of its class)
        push( L );
    };
    // a launch of an extension class over its list, on `waves` waves
    auto pushExt = [ & ]( KswLaunch L, int family, int inst, int cls, int queue, u64 waves, int out1, int outCtr ) {
        L.family = family, L.inst = inst, L.list = cls, L.queue = queue, L.out1 = out1, L.outCtr = outCtr;
        L.jb.n = (u32)SZ.cls[ cls ];
        L.waves = (u32)std::max<u64>( 1, waves );
        if( family != KSW_FAM_EXT )
            L.p_cap = 0; // (only k_ksw_ext takes it: the others' scratch is direction rows alone)
        push( L );
    };
    // longest jobs first: the huge tiers, then the wide classes; the extension kernels' small jobs fill the tails
    for( int k = KSW_CLS_PK3; k >= KSW_CLS_PK0; k-- )
        pushExact( big[ k ], k, KSW_CT_BIG + k, k );
    if( conc )
        for( int k = KSW_CLS_PK3; k >= KSW_CLS_PK0; k-- )
            pushExact( own[ k ], k, KSW_NX_CLS + k, k );
    for( int k = 0; k < 2; k++ ) // the long extensions on the band of 120 first: they are the longest jobs of lane 0
        if( SZ.cls[ KSW_CLS_BANDL + k ] )
            pushExt( LBL, KSW_FAM_BAND1, k == 0, KSW_CLS_BANDL + k, KSW_NX_BANDL + k, std::min<u64>( LBL.waves, SZ.cls[ KSW_CLS_BANDL + k ] ),
                     ownRedo ? KSW_LIST_REDOL : KSW_LIST_REDO, ownRedo ? KSW_NX_N_REDOL : KSW_CT_NREDO );
    // The jobs handed back are drained by k_ksw_pk alone (these rows and the last four): a long-band job of class KSW_CLS_LDS that is
    // handed back is run by no second-pass launch -- no row reads KSW_LIST_REDO / REDOL with cls == KSW_CLS_LDS.
    if( ownRedo )
    {
        P.bandAfter = P.n - 1;
        for( int k = KSW_CLS_PK3; k >= KSW_CLS_PK0; k-- )
            pushExact( LPR, k, KSW_NX_REDOL + k, KSW_LIST_REDOL );
    }
    // the short extensions, several per wavefront (lane 0 of the streams, like the other extension kernels); longest first
    for( int k = 0; k < KSW_GRP_LISTS; k++ )
    {
        const int cls = KSW_CLS_GRP0 + k;
        const u64 nk = SZ.cls[ cls ], Gk = k < 2 && SC.grp >= 1000 ? 4u : ( k < 4 ? 2u : 4u ), waves = std::min<u64>( LG.waves, ( nk + Gk - 1 ) / Gk );
        KswLaunch L = LG;
        L.out2 = KSW_CLS_EXT2, L.nOut1 = (u32)SZ.cls[ KSW_CLS_EXT1 ], L.nOut2 = (u32)SZ.cls[ KSW_CLS_EXT2 ]; // (the narrow band's)
        if( nk && k >= 2 )
            pushExt( LG, KSW_FAM_GRP, cls, cls, KSW_NX_GRP + k, waves, KSW_LIST_REDO, KSW_CT_NREDO );
        else if( nk && SC.grp >= 1000 ) // (without the narrow band its two lists stay empty)
            pushExt( L, KSW_FAM_BAND4, k == 0, cls, KSW_NX_GRP + k, waves, KSW_CLS_EXT1, KSW_NX_BAND_EXT );
    }
    for( int c = KSW_CLS_EXT1; c <= KSW_CLS_EXT2; c++ ) // k_ksw_ext<1>, k_ksw_ext<2>
        if( own[ c ].waves )
            pushExt( own[ c ], KSW_FAM_EXT, c - KSW_CLS_EXT1 + 1, c, KSW_NX_CLS + c, own[ c ].waves, KSW_LIST_REDO, KSW_CT_NREDO );
    if( !conc )
        for( int k = KSW_CLS_PK0; k <= KSW_CLS_PK3; k++ )
            pushExact( own[ k ], k, KSW_NX_CLS + k, k );
    pushExact( LL, KSW_CLS_LDS, KSW_NX_CLS + KSW_CLS_LDS, KSW_CLS_LDS ); // k_ksw (a handed-back job always fits a register kernel)
    for( int k = KSW_CLS_PK0; k <= KSW_CLS_PK3; k++ )
        pushExact( RD, k, KSW_NX_REDO + k, KSW_LIST_REDO ); // on the batch's stream, behind the extension kernels that fill the list
    return P;
}

// the instantiations a launch picks from by a run-time index: exact class k, list k of the wavefront-sharing classes, direction
template <typename FETCH> auto ksw_pk_kernel( int k ) -> decltype( &k_ksw_pk<FETCH, KSW_S0> )
{
    return k == KSW_CLS_PK0 ? k_ksw_pk<FETCH, KSW_S0>
                            : ( k == KSW_CLS_PK1 ? k_ksw_pk<FETCH, KSW_S1> : ( k == KSW_CLS_PK2 ? k_ksw_pk<FETCH, KSW_S2> : k_ksw_pk<FETCH, KSW_S3> ) );
}
template <typename FETCH> auto ksw_grp_kernel( int cls ) -> decltype( &k_ksw_grp<FETCH, 2, 1, true> )
{
    return cls == KSW_CLS_GRP2_L ? k_ksw_grp<FETCH, 2, 1, true>
                                 : ( cls == KSW_CLS_GRP2_R ? k_ksw_grp<FETCH, 2, 1, false> : ( cls == KSW_CLS_GRP4_L ? k_ksw_grp<FETCH, 4, 1, true> : k_ksw_grp<FETCH, 4, 1, false> ) );
}
template <typename FETCH, int G> auto ksw_band_kernel( bool left ) -> decltype( &k_ksw_band<FETCH, true, G> )
{
    return left ? k_ksw_band<FETCH, true, G> : k_ksw_band<FETCH, false, G>;
}
// Launches every class that has jobs.  `next` = KSW_N_NEXT zeroed counters (KSW_NX_*), `nextBig` = KSW_N_NEXT_BIG more (or null).
// `lists` (device, or null) holds the job slots of class k at lists + k * list_stride, SZ.cls[k] entries, and room for the jobs the
// kernels hand back at lists + KSW_LIST_REDO * list_stride (counted in *nRedo) and lists + KSW_LIST_REDOL * list_stride; `side`
// (or null): the streams the classes fork to.
template <typename FETCH>
int ksw_run_all( const FETCH& F, const KswScoring& SC, u32 nSlots, const KswSizing& SZ, DevBuf& scratch, unsigned int* next, KswOut O, hipStream_t stream,
                 u32* lists, u64 list_stride, unsigned int* nRedo, unsigned int* nextBig, const KswSide* side )
{
    u64 perCu = 32; // waves per CU of the persistent ksw launches (MA_KSW_WAVES_PER_CU: tuning hook)
    if( const char* e = getenv( "MA_KSW_WAVES_PER_CU" ) )
        perCu = (u64)std::max( 1, atoi( e ) );
    const bool side3 = side && side->ready( );
    const KswStagePlan P = ksw_plan_stage( SZ, SC, nSlots, lists != nullptr, nextBig != nullptr, side3, side && side->stream[ 2 ], side && side->band,
                                           ksw_scratch_budget( ), perCu ); // one reading of the hooks per call
    if( P.n == 0 )
        return 0;
    if( scratch.reserve( P.total ) )
        return 1;
    if( P.ldsPk )
        for( int k = KSW_CLS_PK0; k <= KSW_CLS_PK3; k++ )
            MA_HIP( hipFuncSetAttribute( (const void*)ksw_pk_kernel<FETCH>( k ), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.ldsPk ) );
    if( P.ldsLds )
        MA_HIP( hipFuncSetAttribute( (const void*)k_ksw<FETCH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.ldsLds ) );
    hipStream_t laneStream[ 4 ] = { stream, side3 ? side->stream[ 0 ] : stream, side3 ? side->stream[ 1 ] : stream,
                                    side && side->stream[ 2 ] ? side->stream[ 2 ] : stream }; // (lanes 1 and 2 have rows only when there are lists, too)
    const bool forked = P.laneUsed[ 1 ] || P.laneUsed[ 2 ] || P.laneUsed[ 3 ];
    if( forked )
    {
        MA_HIP( hipEventRecord( side->fork, stream ) );
        for( int l = 1; l < 4; l++ )
            if( P.laneUsed[ l ] )
                MA_HIP( hipStreamWaitEvent( laneStream[ l ], side->fork, 0 ) );
    }
    auto listAt = [ & ]( int i ) -> u32* { return lists && i != KSW_NONE ? lists + (u64)i * list_stride : nullptr; };
    auto ctrAt = [ & ]( int w ) -> unsigned int* { return w == KSW_NONE ? nullptr : ( w < KSW_CT_BIG ? next + w : ( w < KSW_CT_NREDO ? nextBig + ( w - KSW_CT_BIG ) : nRedo ) ); };
    for( int i = 0; i < P.n; i++ )
    {
        const KswLaunch& L = P.launch[ i ];
        const dim3 grid( L.waves ), block( 64 );
        hipStream_t st = laneStream[ L.lane ];
        uint8_t* sb = scratch.as<uint8_t>( ) + P.laneBase[ L.lane ];
        unsigned int* const queue = ctrAt( L.queue );
        KswJobs JB = L.jb;
        JB.list = listAt( L.list );
        JB.nDev = ctrAt( L.nDev );
        KswWaveScratch WS = L.ws;
        WS.base = sb;
        switch( L.family )
        {
        case KSW_FAM_PK:
            hipLaunchKernelGGL( ksw_pk_kernel<FETCH>( L.inst ), grid, block, L.lds, st, F, SC, JB, queue, sb, L.stride, L.p_cap, L.lds, O );
            break;
        case KSW_FAM_EXT:
            hipLaunchKernelGGL( ( L.inst == 1 ? k_ksw_ext<FETCH, 1> : k_ksw_ext<FETCH, 2> ), grid, block, L.lds, st, F, SC, JB.list, JB.n, queue, sb, L.stride, L.p_cap,
                                L.lds, O, listAt( L.out1 ), ctrAt( L.outCtr ), ctrAt( L.nMore ) );
            break;
        case KSW_FAM_GRP:
            hipLaunchKernelGGL( ksw_grp_kernel<FETCH>( L.inst ), grid, block, 0, st, F, SC, JB.list, JB.n, queue, sb, L.stride, O, listAt( L.out1 ), ctrAt( L.outCtr ) );
            break;
        case KSW_FAM_BAND4:
            hipLaunchKernelGGL( ( ksw_band_kernel<FETCH, 4>( L.inst != 0 ) ), grid, block, 0, st, F, SC, JB.list, JB.n, queue, sb, L.stride, O, listAt( L.out1 ), L.nOut1,
                                listAt( L.out2 ), L.nOut2, ctrAt( L.outCtr ) );
            break;
        case KSW_FAM_BAND1:
            hipLaunchKernelGGL( ( ksw_band_kernel<FETCH, 1>( L.inst != 0 ) ), grid, block, 0, st, F, SC, JB.list, JB.n, queue, sb, L.stride, O, listAt( L.out1 ), L.nOut1,
                                listAt( L.out2 ), L.nOut2, ctrAt( L.outCtr ) );
            break;
        case KSW_FAM_LDS:
            hipLaunchKernelGGL( k_ksw<FETCH>, grid, block, L.lds, st, F, SC, JB, queue, WS, L.lds, O );
            break;
        }
        if( i == P.bandAfter )
        {
            MA_HIP( hipEventRecord( side->band, stream ) );
            MA_HIP( hipStreamWaitEvent( laneStream[ 3 ], side->band, 0 ) );
        }
    }
    if( forked )
        for( int l = 1; l < 4; l++ )
            if( P.laneUsed[ l ] )
            {
                MA_HIP( hipEventRecord( side->join[ l - 1 ], laneStream[ l ] ) );
                MA_HIP( hipStreamWaitEvent( stream, side->join[ l - 1 ], 0 ) );
            }
    MA_HIP( hipGetLastError( ) );
    return 0;
}
} // namespace ma
