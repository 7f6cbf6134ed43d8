// prims.hip -- batched primitive operations behind the C ABI (kernel-level parity seams):
// FMIndex::extend_backward (fMIndex.cpp:21-101), FMIndex::bwt_sa (fMIndex.h:788-814) and
// kswcpp_dispatch (kswcpp.h:165-190).
#include "ksw_launch.h"
#include "fm_device.h"
#include <cstring>

using namespace ma;

__global__ void k_extend( IndexView X, const i64* ik, const uint8_t* c, u64 n, i64* ok )
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n )
        return;
    i64 a[ 3 ] = { ik[ 3 * i ], ik[ 3 * i + 1 ], ik[ 3 * i + 2 ] }, o[ 3 ];
    u32 nb;
    extend_backward( X, a, c[ i ], o, nb );
    ok[ 3 * i ] = o[ 0 ];
    ok[ 3 * i + 1 ] = o[ 1 ];
    ok[ 3 * i + 2 ] = o[ 2 ];
}

__global__ void k_bwt_sa( IndexView X, const i64* rows, u64 n, i64* pos )
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n )
        return;
    u32 steps;
    pos[ i ] = bwt_sa( X, rows[ i ], steps );
}

extern "C" int ma_extend_backward_batch( const ma_index* x, const int64_t* ik, const uint8_t* c, uint64_t n, int64_t* ok )
{
    if( !x )
        return fail( "ma_extend_backward_batch: null index" );
    MA_BIND_DEVICE( x->device );
    if( n == 0 )
        return 0;
    DevBuf dik, dc, dok;
    if( dik.reserve( n * 24 ) || dc.reserve( n ) || dok.reserve( n * 24 ) )
        return 1;
    MA_HIP( hipMemcpy( dik.p, ik, n * 24, hipMemcpyHostToDevice ) );
    MA_HIP( hipMemcpy( dc.p, c, n, hipMemcpyHostToDevice ) );
    hipLaunchKernelGGL( k_extend, dim3( (unsigned)( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, 0, x->v, dik.as<i64>( ),
                        dc.as<uint8_t>( ), n, dok.as<i64>( ) );
    MA_HIP( hipGetLastError( ) );
    MA_HIP( hipMemcpy( ok, dok.p, n * 24, hipMemcpyDeviceToHost ) );
    return 0;
}

extern "C" int ma_bwt_sa_batch( const ma_index* x, const int64_t* rows, uint64_t n, int64_t* pos )
{
    if( !x )
        return fail( "ma_bwt_sa_batch: null index" );
    MA_BIND_DEVICE( x->device );
    if( n == 0 )
        return 0;
    DevBuf dr, dp;
    if( dr.reserve( n * 8 ) || dp.reserve( n * 8 ) )
        return 1;
    MA_HIP( hipMemcpy( dr.p, rows, n * 8, hipMemcpyHostToDevice ) );
    hipLaunchKernelGGL( k_bwt_sa, dim3( (unsigned)( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, 0, x->v, dr.as<i64>( ), n,
                        dp.as<i64>( ) );
    MA_HIP( hipGetLastError( ) );
    MA_HIP( hipMemcpy( pos, dp.p, n * 8, hipMemcpyDeviceToHost ) );
    return 0;
}

namespace
{
struct ByteFetch
{
    static const bool EARLY = false; // ma_ksw_batch returns every ez field of kswcpp_dispatch
    const ma_ksw_job* jobs;
    const uint8_t* qb;
    const uint8_t* tb;
    __device__ bool valid( u32 ) const
    {
        return true;
    }
    __device__ KswJobView view( u32 s ) const
    {
        KswJobView v;
        v.qlen = jobs[ s ].qlen;
        v.tlen = jobs[ s ].tlen;
        v.w = jobs[ s ].w;
        v.zdrop = jobs[ s ].zdrop;
        v.flag = jobs[ s ].flag;
        return v;
    }
    struct Q
    {
        const uint8_t* p;
        __device__ u32 operator( )( i32 i ) const
        {
            return p[ i ];
        }
        static const bool CLEAN = false; // bytes as given: 4 (and above) = N
        __device__ u32 pair( i32 i ) const // cells i, i + 1 (the byte arrays are padded: reading one past the end is safe)
        {
            return (u32)p[ i ] | (u32)p[ i + 1 ] << 16;
        }
    };
    __device__ Q qfetch( u32 s ) const
    {
        return Q{ qb + jobs[ s ].q_off };
    }
    __device__ Q tfetch( u32 s ) const
    {
        return Q{ tb + jobs[ s ].t_off };
    }
};
struct ByteFetchPipe : ByteFetch
{
    static const bool EARLY = true; // what NeedlemanWunsch reads: max, max_q, max_t, cigar
};
} // namespace

// the 64-bit device counters of one call
enum : int
{
    PC_CIG_USED = 0,
    PC_CELLS,
    PC_NJOBS,
    PC_ERR,
    PC_NEXT, // ksw_run_all's `next`: KSW_N_NEXT x u32
    PC_N_REDO = PC_NEXT + KSW_N_NEXT / 2,
    PC_NEXT_BIG, // KSW_N_NEXT_BIG x u32
    PC_COUNT = PC_NEXT_BIG + KSW_N_NEXT_BIG / 2
};
static_assert( PC_CIG_USED == KSW_BYTES_CIG_USED && PC_ERR == KSW_BYTES_ERR && PC_COUNT <= KSW_BYTES_CTR_WORDS, "internal.h names these words" );

// The device-resident middle of a call: n jobs whose records and bytes are in device memory (F), their result records, cigar
// offsets and the dense cigar pool of cigar_cap words, the PC_COUNT counters of the call; everything is enqueued on `stream`
// and nobody waits.  ctr[ PC_CIG_USED ] is the pool's fill, ctr[ PC_ERR ] holds MA_ERR_CIGAR_OVERFLOW if it did not fit.
template <typename FETCH>
static int ksw_bytes_launch( const FETCH& F, const KswScoring& SC, uint64_t n, const KswSizing& S, u32* lists, ma_ez* ez, u64* cig_off,
                             u32* cig_pool, uint64_t cigar_cap, unsigned long long* ctr, DevBuf& scratch, hipStream_t stream )
{
    MA_HIP( hipMemsetAsync( ctr, 0, PC_COUNT * 8, stream ) );
    MA_HIP( hipMemsetAsync( ez, 0, n * sizeof( ma_ez ), stream ) );
    MA_HIP( hipMemsetAsync( cig_off, 0, ( n + 1 ) * 8, stream ) );
    KswOut O;
    O.ez = ez;
    O.cig_off = cig_off;
    O.cig_pool = cig_pool;
    O.cig_pool_cap = cigar_cap;
    O.cig_used = ctr + PC_CIG_USED;
    O.cells = ctr + PC_CELLS;
    O.njobs = ctr + PC_NJOBS;
    O.err = (u32*)( ctr + PC_ERR );
    O.path = nullptr;
    O.cig_words = nullptr;
    O.cig_chunk = 0; // dense pool: cigar_off[n] is the total
    return ksw_run_all( F, SC, (u32)n, S, scratch, (unsigned int*)( ctr + PC_NEXT ), O, stream, lists, n, (unsigned int*)( ctr + PC_N_REDO ),
                        (unsigned int*)( ctr + PC_NEXT_BIG ), nullptr );
}

// ma_ksw_batch's kernels (every ez field, no early stop) over jobs that are in device memory already: the DP of the pipeline's
// small-inversion stage (launch_inv.h).  shapes: qlen, tlen, w of every job on the host, for the sizing of the launches.
int ma::ksw_bytes_device( const ma_params& P, const ma_ksw_job* d_jobs, uint64_t n, const int32_t* shapes, const uint8_t* d_q,
                          const uint8_t* d_t, ma_ez* d_ez, uint64_t* d_cig_off, uint32_t* d_cig_pool, uint64_t cigar_cap,
                          unsigned long long* d_ctr, DevBuf& scratch, hipStream_t stream )
{
    KswScoring SC{ P.match, P.mismatch, P.gap, P.extend, P.gap2, P.extend2 };
    SC.grp = ksw_grp_env( );
    SC.band_mis = ksw_band_mis_env( );
    SC.band_long = ksw_bandl_env( );
    KswSizing S;
    for( uint64_t i = 0; i < n; i++ )
        ksw_size_job( S, shapes[ 3 * i ], shapes[ 3 * i + 1 ], shapes[ 3 * i + 2 ] );
    ByteFetch F;
    F.jobs = d_jobs;
    F.qb = d_q;
    F.tb = d_t;
    return ksw_bytes_launch( F, SC, n, S, nullptr, d_ez, d_cig_off, d_cig_pool, cigar_cap, d_ctr, scratch, stream );
}

// FETCH::EARLY selects the pipeline semantics (extension kernel + early stop, see ksw_ext.h)
template <typename FETCH>
static int ksw_batch_impl( const ma_params* P, const ma_ksw_job* jobs, uint64_t n, const uint8_t* q_bytes, uint64_t q_len,
                           const uint8_t* t_bytes, uint64_t t_len, ma_ez* ez, uint64_t* cigar_off, uint32_t* cigar,
                           uint64_t cigar_cap )
{
    if( !P || !jobs || !ez || !cigar_off )
        return fail( "ma_ksw_batch: null argument" );
    if( n == 0 )
        return 0;
    KswScoring SC{ P->match, P->mismatch, P->gap, P->extend, P->gap2, P->extend2 };
    SC.grp = ksw_grp_env( );
    SC.band_mis = ksw_band_mis_env( );
    SC.band_long = ksw_bandl_env( );
    KswSizing S;
    for( uint64_t i = 0; i < n; i++ )
        ksw_size_job( S, jobs[ i ].qlen, jobs[ i ].tlen, jobs[ i ].w );
    // pipeline semantics: per-class job lists and sizes by the router k_dp_enum builds them with on the device (ksw_route_job)
    std::vector<u32> lists;
    DevBuf dlists;
    if( FETCH::EARLY )
    {
        for( int k = 0; k < KSW_N_CLASSES; k++ )
            S.cls[ k ] = S.pc[ k ] = S.cigc[ k ] = 0;
        lists.assign( (size_t)( KSW_N_CLASSES + 2 ) * n, 0u );
        const bool tryAll = getenv( "MA_KSW_BAND_ALL" ) != nullptr; // the tests try every eligible job on its band: no pre-filters
        for( uint64_t i = 0; i < n; i++ )
        {
            const ma_ksw_job& j = jobs[ i ];
            if( j.qlen <= 0 || j.tlen <= 0 )
                continue;
            const uint8_t *qp = q_bytes + j.q_off, *tp = t_bytes + j.t_off;
            auto qf = [ & ]( i32 k ) -> u32 { return qp[ k ]; };
            auto tf = [ & ]( i32 k ) -> u32 { return tp[ k ]; };
            const KswRoute R = ksw_route_job( SC, j.qlen, j.tlen, j.w, j.zdrop, j.flag, qf, tf, tryAll );
            lists[ (size_t)R.cls * n + S.cls[ R.cls ] ] = (u32)i;
            ksw_size_route( S, R );
        }
        if( dlists.reserve( lists.size( ) * 4 + 16 ) )
            return 1;
        MA_HIP( hipMemcpy( dlists.p, lists.data( ), lists.size( ) * 4, hipMemcpyHostToDevice ) );
    }
    DevBuf dj, dq, dt, dez, doff, dpool, dscr, dctr;
    if( dj.reserve( n * sizeof( ma_ksw_job ) ) || dq.reserve( q_len + 16 ) || dt.reserve( t_len + 16 ) ||
        dez.reserve( n * sizeof( ma_ez ) ) || doff.reserve( ( n + 1 ) * 8 ) || dpool.reserve( cigar_cap * 4 + 16 ) ||
        dctr.reserve( PC_COUNT * 8 ) )
        return 1;
    MA_HIP( hipMemcpy( dj.p, jobs, n * sizeof( ma_ksw_job ), hipMemcpyHostToDevice ) );
    MA_HIP( hipMemcpy( dq.p, q_bytes, q_len, hipMemcpyHostToDevice ) );
    MA_HIP( hipMemcpy( dt.p, t_bytes, t_len, hipMemcpyHostToDevice ) );
    FETCH F;
    F.jobs = dj.as<ma_ksw_job>( );
    F.qb = dq.as<uint8_t>( );
    F.tb = dt.as<uint8_t>( );
    if( ksw_bytes_launch( F, SC, n, S, FETCH::EARLY ? dlists.as<u32>( ) : nullptr, dez.as<ma_ez>( ), doff.as<u64>( ), dpool.as<u32>( ), cigar_cap,
                          dctr.as<unsigned long long>( ), dscr, 0 ) )
        return 1;
    MA_HIP( hipDeviceSynchronize( ) );
    unsigned long long h[ PC_NEXT ];
    MA_HIP( hipMemcpy( h, dctr.p, sizeof( h ), hipMemcpyDeviceToHost ) );
    int rc = 0;
    if( ( (u32)h[ PC_ERR ] ) & MA_ERR_CIGAR_OVERFLOW )
        rc = fail( "ma_ksw_batch: cigar capacity too small" );
    else
    {
        MA_HIP( hipMemcpy( ez, dez.p, n * sizeof( ma_ez ), hipMemcpyDeviceToHost ) );
        MA_HIP( hipMemcpy( cigar_off, doff.p, n * 8, hipMemcpyDeviceToHost ) );
        cigar_off[ n ] = h[ PC_CIG_USED ];
        if( cigar && h[ PC_CIG_USED ] )
            MA_HIP( hipMemcpy( cigar, dpool.p, h[ PC_CIG_USED ] * 4, hipMemcpyDeviceToHost ) );
    }
    return rc;
}

extern "C" int ma_ksw_batch( const ma_params* P, const ma_ksw_job* jobs, uint64_t n, const uint8_t* q_bytes,
                             uint64_t q_len, const uint8_t* t_bytes, uint64_t t_len, ma_ez* ez, uint64_t* cigar_off,
                             uint32_t* cigar, uint64_t cigar_cap )
{
    return ksw_batch_impl<ByteFetch>( P, jobs, n, q_bytes, q_len, t_bytes, t_len, ez, cigar_off, cigar, cigar_cap );
}

extern "C" int ma_ksw_ext_batch( const ma_params* P, const ma_ksw_job* jobs, uint64_t n, const uint8_t* q_bytes,
                                 uint64_t q_len, const uint8_t* t_bytes, uint64_t t_len, ma_ez* ez, uint64_t* cigar_off,
                                 uint32_t* cigar, uint64_t cigar_cap )
{
    return ksw_batch_impl<ByteFetchPipe>( P, jobs, n, q_bytes, q_len, t_bytes, t_len, ez, cigar_off, cigar, cigar_cap );
}

// ---- diagnostics: the device libm values the chaining stage decides with (chain.h: tan, sin, atan, log), evaluated
// exactly like there (same translation-unit flags, -ffp-contract=off), so a test can compare their bits with glibc's
// (harmonization.h:82-89 and ransac.cpp:112,131-135 run on glibc in the reference)
__global__ void k_libm_probe( int op, const double* in, u64 n, double* out )
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if( i >= n )
        return;
    const double x = in[ i ];
    out[ i ] = op == 0 ? tan( x ) : op == 1 ? sin( x ) : op == 2 ? atan( x ) : log( x );
}
namespace ma
{
int band_stats_of_prims( unsigned long long out[ 8 ] )
{
    MA_HIP( hipMemcpyFromSymbol( out, HIP_SYMBOL( ma::g_band_stats ), 8 * 8 ) );
    return 0;
}
int band_long_stats_of_prims( unsigned long long out[ 8 ] )
{
    MA_HIP( hipMemcpyFromSymbol( out, HIP_SYMBOL( ma::g_band_stats ), 8 * 8, 8 * 8 ) );
    return 0;
}
int dp_family_stats_of_prims( unsigned long long out[ 2 * KSW_N_FAMILIES ] )
{
    MA_HIP( hipMemcpyFromSymbol( out, HIP_SYMBOL( ma::g_dp_family ), 2 * KSW_N_FAMILIES * 8 ) );
    return 0;
}
} // namespace ma

extern "C" int ma_debug_libm( int op, const double* in, uint64_t n, double* out )
{
    if( !in || !out || op < 0 || op > 3 )
        return fail( "ma_debug_libm: bad argument" );
    if( n == 0 )
        return 0;
    DevBuf di, dout;
    if( di.reserve( n * 8 ) || dout.reserve( n * 8 ) )
        return 1;
    MA_HIP( hipMemcpy( di.p, in, n * 8, hipMemcpyHostToDevice ) );
    hipLaunchKernelGGL( k_libm_probe, dim3( (unsigned)( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, 0, op, di.as<double>( ), n,
                        dout.as<double>( ) );
    MA_HIP( hipGetLastError( ) );
    MA_HIP( hipMemcpy( out, dout.p, n * 8, hipMemcpyDeviceToHost ) );
    return 0;
}
