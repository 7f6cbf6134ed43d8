// launch_inv.h -- ma_inversions_batch and its counts.  Textually part of pipeline.hip.
//
// One sequence behind the DP stage on the batch's stream: k_inv_scan, then the wait with the ONE sizing read-back -- the
// stage's statistics (candidates, window bytes, ops bound, errors) and the candidates' shapes, three int32 each, which size
// the DP launches on the host (KswSizing).  A batch without a candidate ends there.  Otherwise the DP kernels of ma_ksw_batch
// run over the device-resident jobs (ksw_bytes_device, prims.hip), k_inv_assemble writes the records' ops behind the end of
// the batch's ops pool, a scan of the per-read counts gives the final lists' offsets, k_inv_merge writes them, and a second
// wait brings the records and ops kept (the sizes of the downloads).  The capacities of the candidate arrays persist and grow:
// only a batch that brings more candidates than any before pays a second k_inv_scan and a third wait.
namespace
{
struct U32AsU64
{
    __host__ __device__ __forceinline__ u64 operator( )( const u32& x ) const
    {
        return (u64)x;
    }
};

InvKernelArgs inv_args( ma_batch* b )
{
    InvKernelArgs A;
    memset( &A, 0, sizeof( A ) );
    A.X = b->idx->v;
    A.P = ma_inv::params( b->P );
    A.NP = nw_params( b->P );
    A.n_reads = (u32)b->n_reads;
    A.n_slots = b->st.nHsets;
    A.off = b->hsetOff.as<u64>( ); // always the MappingQuality output itself, never the final lists of a call before
    A.hdr = b->hdr.as<AlnHeader>( );
    A.order = b->mqOrder.as<u32>( );
    A.cnt = b->mqCnt.as<u32>( );
    A.roff = b->d_roff;
    A.reads = b->d_reads;
    A.pool = b->ops.as<u64>( );
    A.pool_used = b->nOpsCap;
    A.slot_cnt = b->invSlotCnt.as<u32>( );
    A.slot_first = b->invSlotFirst.as<u64>( );
    A.cand = b->invCand.as<InvCand>( );
    A.jobs = b->invJobs.as<ma_ksw_job>( );
    A.shapes = b->invShapes.as<i32>( );
    A.win = b->invWin.as<uint8_t>( );
    A.cand_cap = b->invCandCap;
    A.win_cap = b->invWinCap;
    A.stat = b->invStat.as<unsigned long long>( );
    return A;
}

// the message for the first bad stretch (error path only): key = slot << 2 | ma_inv::ERR_*
int inv_fail( ma_batch* b, u64 key )
{
    const u64 n = b->n_reads, slot = key >> 2;
    std::vector<u64> hoff( n + 1 );
    MA_HIP( hipMemcpyAsync( hoff.data( ), b->hsetOff.p, ( n + 1 ) * 8, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    const u64 r = (u64)( std::upper_bound( hoff.begin( ), hoff.end( ), slot ) - hoff.begin( ) ) - 1;
    const u32 kind = (u32)( key & 3 );
    return fail( "ma_inversions_batch: record " + std::to_string( slot - hoff[ r ] ) + " of read " + std::to_string( r ) + ": a stretch between two seeds " +
                 ( kind == ma_inv::ERR_BEYOND_READ
                       ? "ends beyond the read"
                       : ( kind == ma_inv::ERR_BRIDGING ? "has its reverse-strand window on both strands ((vExtractSubsection) Try to extract bridging sequence)"
                                                        : "has its reverse-strand window outside the doubled text" ) ) );
}
} // namespace

extern "C" {

int ma_inversions_batch( ma_batch* b )
{
    if( !b )
        return fail( "ma_inversions_batch: null batch" );
    if( !b->st.has( ma_state::ALIGNED ) )
        return fail( "ma_inversions_batch: no MappingQuality output to scan (run ma_dp_batch / ma_align_batch / ma_batch_set_alignments first)" );
    MA_BIND_DEVICE( b->device );
    // pairs and texts made before are of other lists; the list view (mq_view) is back on the MappingQuality arrays
    b->st.drop( ma_state::INVERSIONS );
    const u64 n = b->n_reads, nh = b->st.nHsets;
    if( n == 0 || nh == 0 )
    {
        b->st.finish( ma_state::INVERSIONS );
        return 0;
    }
    if( b->invStat.reserve( INV_STAT_COUNT * 8 ) || b->invSlotCnt.reserve( ( nh + 1 ) * 4 ) || b->invSlotFirst.reserve( ( nh + 1 ) * 8 ) )
        return 1;
    unsigned long long stat[ INV_STAT_COUNT ];
    std::vector<i32> shapes;
    for( int attempt = 0;; attempt++ )
    {
        b->invCandCap = std::max<u64>( b->invCandCap, 1024 );
        b->invWinCap = std::max<u64>( b->invWinCap, 256 * 1024 );
        if( b->invCand.reserve( b->invCandCap * sizeof( InvCand ) ) || b->invJobs.reserve( b->invCandCap * sizeof( ma_ksw_job ) ) ||
            b->invShapes.reserve( b->invCandCap * 12 ) || b->invWin.reserve( b->invWinCap + 16 ) )
            return 1;
        unsigned long long init[ INV_STAT_COUNT ] = { };
        init[ INV_STAT_FIRST ] = ~0ull;
        MA_HIP( hipMemcpyAsync( b->invStat.p, init, sizeof( init ), hipMemcpyHostToDevice, b->stream ) );
        hipLaunchKernelGGL( k_inv_scan, dim3( (unsigned)( ( nh + 255 ) / 256 ) ), dim3( 256 ), 0, b->stream, inv_args( b ) );
        MA_HIP( hipGetLastError( ) );
        shapes.resize( 3 * b->invCandCap );
        MA_HIP( hipMemcpyAsync( stat, b->invStat.p, sizeof( stat ), hipMemcpyDeviceToHost, b->stream ) );
        MA_HIP( hipMemcpyAsync( shapes.data( ), b->invShapes.p, shapes.size( ) * 4, hipMemcpyDeviceToHost, b->stream ) );
        if( batch_wait( b ) ) // (init goes out of scope as well)
            return 1;
        if( stat[ INV_STAT_ERRORS ] )
            return inv_fail( b, stat[ INV_STAT_FIRST ] );
        if( stat[ INV_STAT_CAND ] <= b->invCandCap && stat[ INV_STAT_WIN ] <= b->invWinCap )
            break;
        if( attempt == 1 )
            return fail( "ma_inversions_batch: the candidates of two scans of the same lists differ" );
        b->invCandCap = std::max<u64>( b->invCandCap, stat[ INV_STAT_CAND ] + stat[ INV_STAT_CAND ] / 4 );
        b->invWinCap = std::max<u64>( b->invWinCap, stat[ INV_STAT_WIN ] + stat[ INV_STAT_WIN ] / 4 );
    }
    const u64 nc = stat[ INV_STAT_CAND ];
    b->st.invCands = nc;
    b->st.invJobsN = stat[ INV_STAT_JOBS ];
    if( nc == 0 ) // nothing found: the view stays on the MappingQuality arrays
    {
        b->st.finish( ma_state::INVERSIONS );
        return 0;
    }
    // the DP of all candidates at once: kswcpp_dispatch( ..., uiBandwidth, uiZDrop, 0, ... ) (smallInversions.h:131-133)
    const u64 cigCap = stat[ INV_STAT_OPS ] + 16;
    if( b->invEz.reserve( ( nc + 1 ) * sizeof( ma_ez ) ) || b->invCigOff.reserve( ( nc + 2 ) * 8 ) || b->invCigPool.reserve( cigCap * 4 + 16 ) ||
        b->invCtr.reserve( KSW_BYTES_CTR_WORDS * 8 ) )
        return 1;
    if( ksw_bytes_device( b->P, b->invJobs.as<ma_ksw_job>( ), nc, shapes.data( ), b->d_reads, b->invWin.as<uint8_t>( ), b->invEz.as<ma_ez>( ),
                          b->invCigOff.as<u64>( ), b->invCigPool.as<u32>( ), cigCap, b->invCtr.as<unsigned long long>( ), b->kswScratch, b->stream ) )
        return 1;
    // room for the records' ops behind the pool's end; a pool that is too small grows with its contents kept
    const u64 poolNeed = ( b->nOpsCap + stat[ INV_STAT_OPS ] + 2 ) * 8;
    if( poolNeed > b->ops.cap )
    {
        DevBuf grown;
        if( grown.reserve( poolNeed ) )
            return 1;
        if( b->nOpsCap )
            MA_HIP( hipMemcpyAsync( grown.p, b->ops.p, b->nOpsCap * 8, hipMemcpyDeviceToDevice, b->stream ) );
        if( batch_wait( b ) ) // (the old pool is freed here; only a batch whose pool has no headroom comes this way)
            return 1;
        b->ops = std::move( grown );
    }
    if( b->invHdr.reserve( nc * sizeof( AlnHeader ) ) || b->finCnt.reserve( ( n + 2 ) * 4 ) || b->finOff.reserve( ( n + 2 ) * 8 ) ||
        b->finHdr.reserve( ( nh + nc + 1 ) * sizeof( AlnHeader ) ) || b->finOrder.reserve( ( nh + nc + 1 ) * 4 ) )
        return 1;
    InvKernelArgs A = inv_args( b );
    A.n_cand = nc;
    A.ez = b->invEz.as<ma_ez>( );
    A.cig_off = b->invCigOff.as<u64>( );
    A.cig_pool = b->invCigPool.as<u32>( );
    A.inv_hdr = b->invHdr.as<AlnHeader>( );
    A.fin_cnt = b->finCnt.as<u32>( );
    A.fin_off = b->finOff.as<u64>( );
    A.fin_hdr = b->finHdr.as<AlnHeader>( );
    A.fin_order = b->finOrder.as<u32>( );
    MA_HIP( hipMemcpyAsync( b->finCnt.p, b->mqCnt.p, n * 4, hipMemcpyDeviceToDevice, b->stream ) );
    MA_HIP( hipMemsetAsync( (char*)b->finCnt.p + n * 4, 0, 4, b->stream ) );
    hipLaunchKernelGGL( k_inv_assemble, dim3( (unsigned)( ( nc + 63 ) / 64 ) ), dim3( 64 ), 0, b->stream, A );
    MA_HIP( hipGetLastError( ) );
    {
        hipcub::TransformInputIterator<u64, U32AsU64, const u32*> in( b->finCnt.as<u32>( ), U32AsU64( ) );
        size_t tb = 0;
        MA_HIP( hipcub::DeviceScan::ExclusiveSum( nullptr, tb, in, b->finOff.as<u64>( ), (int)( n + 1 ), b->stream ) );
        if( b->cubTmp.reserve( tb + 256 ) )
            return 1;
        MA_HIP( hipcub::DeviceScan::ExclusiveSum( b->cubTmp.p, tb, in, b->finOff.as<u64>( ), (int)( n + 1 ), b->stream ) );
    }
    hipLaunchKernelGGL( k_inv_merge, dim3( (unsigned)( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, b->stream, A );
    MA_HIP( hipGetLastError( ) );
    unsigned long long kctr[ KSW_BYTES_CTR_WORDS ];
    MA_HIP( hipMemcpyAsync( stat, b->invStat.p, sizeof( stat ), hipMemcpyDeviceToHost, b->stream ) );
    MA_HIP( hipMemcpyAsync( kctr, b->invCtr.p, sizeof( kctr ), hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    if( (u32)kctr[ KSW_BYTES_ERR ] & MA_ERR_CIGAR_OVERFLOW )
        return fail( "ma_inversions_batch: cigar capacity too small" );
    if( stat[ INV_STAT_SYMBOL ] )
        return fail( "obtained wierd symbol from ksw" ); // (the host module's text, smallInversions.h:167)
    if( stat[ INV_STAT_FLAGS ] )
        return fail( "ma_inversions_batch: device capacity overflow: alignment-ops" );
    b->st.invRecs = stat[ INV_STAT_RECS ];
    b->st.invOps = stat[ INV_STAT_REC_OPS ];
    b->st.finish( ma_state::INVERSIONS ); // (no record kept: the view stays on the MappingQuality lists, BatchState::invFinal)
    return 0;
}

int ma_batch_inversion_counts( ma_batch* b, uint64_t* n_candidates, uint64_t* n_jobs, uint64_t* n_records )
{
    if( !b || !b->st.has( ma_state::INVERSIONS ) )
        return fail( "ma_batch_inversion_counts: run ma_inversions_batch first" );
    if( n_candidates )
        *n_candidates = b->st.invCands;
    if( n_jobs )
        *n_jobs = b->st.invJobsN;
    if( n_records )
        *n_records = b->st.invRecs;
    return 0;
}
} // extern "C"
