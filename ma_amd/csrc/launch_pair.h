// launch_pair.h -- ma_pair_batch and the download of its records.  Textually part of pipeline.hip.
//
// ma_pair_batch runs k_pair_pick behind the DP stage on the batch's stream and waits for it with the ONE read-back of the
// batch's counters that sizes the download (records, ops) and reports the two things only the device knows: a pair without
// any candidate (the reference's error) and the pairs left to the host.  The pairs left to the host are the tied ones with
// more than PAIR_TIE_CAP candidates (stage_pair.h): their lists come down as PairCompact records, ma_pair_flat.h picks
// (through the real std::sort), k_pair_apply puts the picks beside the device's own.  ma_batch_get_pairs /
// ma_batch_start_pair_download then scan the per-pair sizes and pack the records without reading anything back.
namespace
{
struct PairCompactList // a list of ma_pair_flat.h over PairCompact records
{
    const PairCompact* c;
    u32 n;
    uint32_t size( ) const
    {
        return n;
    }
    int64_t score( uint32_t k ) const
    {
        return c[ k ].score;
    }
    uint64_t begin( uint32_t k ) const
    {
        return c[ k ].begin;
    }
    bool nonzero( uint32_t k ) const
    {
        return c[ k ].nonzero != 0;
    }
    uint32_t seeds( uint32_t k ) const
    {
        return c[ k ].seeds;
    }
};

PairKernelArgs pair_args( ma_batch* b )
{
    PairKernelArgs A;
    A.pp.P = ma_pair::params( b->P, b->idx->v.n );
    A.pp.n_pairs = (u32)( b->n_reads / 2 );
    const MqView V = mq_view( b );
    A.hset_off = V.off;
    A.roff = b->d_roff;
    A.hdr = V.hdr;
    A.pool = b->ops.as<u64>( );
    A.mq_order = V.order;
    A.mq_cnt = V.cnt;
    A.pick = b->pairPick.as<ma_pair::Pick>( );
    A.cnt = b->pairCnt.as<u64>( );
    A.nops = b->pairOps.as<u64>( );
    A.over = b->pairOver.as<u32>( );
    A.ctr = b->ctr.as<unsigned long long>( );
    return A;
}

// the pairs k_pair_pick left to the host (b->hctr is current)
int pair_finish_on_host( ma_batch* b, const PairKernelArgs& A )
{
    const u32 nOver = (u32)b->hctr[ CTR_PAIR_OVER ];
    const u64 n = b->n_reads;
    std::vector<u32> over( nOver ), cnt( n );
    std::vector<u64> roff( n + 1 );
    MA_HIP( hipMemcpyAsync( over.data( ), b->pairOver.p, nOver * 4ull, hipMemcpyDeviceToHost, b->stream ) );
    MA_HIP( hipMemcpyAsync( cnt.data( ), mq_view( b ).cnt, n * 4, hipMemcpyDeviceToHost, b->stream ) );
    MA_HIP( hipMemcpyAsync( roff.data( ), b->d_roff, ( n + 1 ) * 8, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    std::vector<u64> off( nOver + 1, 0 );
    for( u32 t = 0; t < nOver; t++ )
        off[ t + 1 ] = off[ t ] + cnt[ 2 * (u64)over[ t ] ] + cnt[ 2 * (u64)over[ t ] + 1 ];
    std::vector<PairCompact> lists( off[ nOver ] );
    if( b->pairHostOff.reserve( ( nOver + 1 ) * 8ull ) || b->pairHostLists.reserve( ( off[ nOver ] + 1 ) * sizeof( PairCompact ) ) ||
        b->pairHostPick.reserve( nOver * sizeof( ma_pair::Pick ) ) )
        return 1;
    const dim3 grid( ( nOver + 63 ) / 64 ), block( 64 );
    MA_HIP( hipMemcpyAsync( b->pairHostOff.p, off.data( ), ( nOver + 1 ) * 8ull, hipMemcpyHostToDevice, b->stream ) );
    hipLaunchKernelGGL( k_pair_gather, grid, block, 0, b->stream, A, nOver, b->pairHostOff.as<u64>( ), b->pairHostLists.as<PairCompact>( ) );
    MA_HIP( hipGetLastError( ) );
    MA_HIP( hipMemcpyAsync( lists.data( ), b->pairHostLists.p, off[ nOver ] * sizeof( PairCompact ), hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    std::vector<ma_pair::Pick> picks( nOver );
    for( u32 t = 0; t < nOver; t++ )
    {
        const u64 k = over[ t ];
        const PairCompactList a{ lists.data( ) + off[ t ], cnt[ 2 * k ] }, c{ lists.data( ) + off[ t ] + cnt[ 2 * k ], cnt[ 2 * k + 1 ] };
        picks[ t ] = ma_pair::pick( a, c, A.pp.P, roff[ 2 * k + 1 ] - roff[ 2 * k ], roff[ 2 * k + 2 ] - roff[ 2 * k + 1 ] );
    }
    MA_HIP( hipMemcpyAsync( b->pairHostPick.p, picks.data( ), nOver * sizeof( ma_pair::Pick ), hipMemcpyHostToDevice, b->stream ) );
    hipLaunchKernelGGL( k_pair_apply, grid, block, 0, b->stream, A, nOver, b->pairHostPick.as<ma_pair::Pick>( ) );
    MA_HIP( hipGetLastError( ) );
    return read_ctr( b ); // (waits: the host vectors go out of scope)
}
} // namespace

extern "C" {

int ma_pair_batch( ma_batch* b )
{
    if( !b )
        return fail( "ma_pair_batch: null batch" );
    if( !b->st.has( ma_state::ALIGNED ) )
        return fail( "ma_pair_batch: no MappingQuality output to pair (run ma_dp_batch / ma_align_batch first)" );
    if( b->n_reads % 2 )
        return fail( "ma_pair_batch: odd number of reads (" + std::to_string( b->n_reads ) +
                     "): reads 2k and 2k+1 of a batch are the mates of pair k" );
    MA_BIND_DEVICE( b->device );
    const u64 np = b->n_reads / 2;
    b->st.drop( ma_state::PAIRS ); // (a pairs' text printed before is of other picks; the single-end text does not read them)
    if( np && b->st.nHsets )
    {
        if( b->pairPick.reserve( np * sizeof( ma_pair::Pick ) ) || b->pairCnt.reserve( ( np + 2 ) * 8 ) || b->pairOps.reserve( ( np + 2 ) * 8 ) ||
            b->pairOver.reserve( ( np + 1 ) * 4 ) )
            return 1;
        MA_HIP( hipMemsetAsync( b->ctr.as<unsigned long long>( ) + CTR_PAIR_RECS, 0, ( CTR_COUNT - CTR_PAIR_RECS ) * 8, b->stream ) );
        const PairKernelArgs A = pair_args( b );
        hipLaunchKernelGGL( k_pair_pick, dim3( (unsigned)( ( np + 63 ) / 64 ) ), dim3( 64 ), 0, b->stream, A );
        MA_HIP( hipGetLastError( ) );
        if( read_ctr( b ) || check_err( b, "ma_pair_batch" ) )
            return 1;
        if( b->hctr[ CTR_PAIR_ERR ] )
            return fail( ma_pair::noCandidateText( ) );
        b->st.pairOnHost = b->hctr[ CTR_PAIR_OVER ];
        if( b->st.pairOnHost && pair_finish_on_host( b, A ) )
            return 1;
        b->st.pairRecs = b->hctr[ CTR_PAIR_RECS ];
        b->st.pairNOps = b->hctr[ CTR_PAIR_OPS ];
    }
    b->st.finish( ma_state::PAIRS );
    return 0;
}

int ma_batch_pair_counts( ma_batch* b, uint64_t* n_pairs, uint64_t* n_records, uint64_t* n_ops, uint64_t* n_host_pairs )
{
    if( !b || !b->st.has( ma_state::PAIRS ) )
        return fail( "ma_batch_pair_counts: run ma_pair_batch first" );
    if( n_pairs )
        *n_pairs = b->n_reads / 2;
    if( n_records )
        *n_records = b->st.pairRecs;
    if( n_ops )
        *n_ops = b->st.pairNOps;
    if( n_host_pairs )
        *n_host_pairs = b->st.pairOnHost;
    return 0;
}
} // extern "C"

// async: see get_alns
static int get_pairs( ma_batch* b, uint64_t* pair_off, ma_alignment* alns, uint64_t* ops, int32_t* mate, int32_t* other, bool async )
{
    if( !b || !b->st.has( ma_state::PAIRS ) )
        return fail( "ma_batch_get_pairs: run ma_pair_batch first" );
    MA_BIND_DEVICE( b->device );
    if( download_begin( b, async, "ma_batch_start_pair_download" ) )
        return 1;
    const u64 np = b->n_reads / 2, totalA = b->st.pairRecs, totalO = b->st.pairNOps;
    if( totalA == 0 )
    {
        if( pair_off )
            memset( pair_off, 0, ( np + 1 ) * 8 );
        return 0;
    }
    if( b->outAlnOff.reserve( ( np + 2 ) * 8 ) || b->outOpsOff.reserve( ( np + 2 ) * 8 ) ||
        b->outAlns.reserve( ( totalA + 1 ) * sizeof( ma_alignment ) ) || b->outOpsPairs.reserve( ( totalO + 1 ) * 16 ) ||
        b->pairMate.reserve( ( totalA + 1 ) * 4 ) || b->pairOther.reserve( ( totalA + 1 ) * 4 ) )
        return 1;
    MA_HIP( hipMemsetAsync( (char*)b->pairCnt.p + np * 8, 0, 8, b->stream ) );
    MA_HIP( hipMemsetAsync( (char*)b->pairOps.p + np * 8, 0, 8, b->stream ) );
    if( scan_exclusive<u64>( b, b->pairCnt.as<u64>( ), b->outAlnOff.as<u64>( ), np + 1 ) ||
        scan_exclusive<u64>( b, b->pairOps.as<u64>( ), b->outOpsOff.as<u64>( ), np + 1 ) )
        return 1;
    hipLaunchKernelGGL( k_pair_pack, dim3( (unsigned)( ( np + 255 ) / 256 ) ), dim3( 256 ), 0, b->stream, pair_args( b ),
                        b->outAlnOff.as<u64>( ), b->outOpsOff.as<u64>( ), b->outAlns.as<ma_alignment>( ), b->outOpsPairs.as<u64>( ),
                        b->pairMate.as<i32>( ), b->pairOther.as<i32>( ) );
    MA_HIP( hipGetLastError( ) );
    hipStream_t cs;
    if( download_stream( b, async, &cs ) )
        return 1;
    if( pair_off )
        MA_HIP( hipMemcpyAsync( pair_off, b->outAlnOff.p, ( np + 1 ) * 8, hipMemcpyDeviceToHost, cs ) );
    if( alns )
        MA_HIP( hipMemcpyAsync( alns, b->outAlns.p, totalA * sizeof( ma_alignment ), hipMemcpyDeviceToHost, cs ) );
    if( ops && totalO )
        MA_HIP( hipMemcpyAsync( ops, b->outOpsPairs.p, totalO * 16, hipMemcpyDeviceToHost, cs ) );
    if( mate )
        MA_HIP( hipMemcpyAsync( mate, b->pairMate.p, totalA * 4, hipMemcpyDeviceToHost, cs ) );
    if( other )
        MA_HIP( hipMemcpyAsync( other, b->pairOther.p, totalA * 4, hipMemcpyDeviceToHost, cs ) );
    return download_end( b, async, cs );
}

extern "C" {
int ma_batch_get_pairs( ma_batch* b, uint64_t* pair_off, ma_alignment* alns, uint64_t* ops, int32_t* mate, int32_t* other )
{
    return get_pairs( b, pair_off, alns, ops, mate, other, false );
}
int ma_batch_start_pair_download( ma_batch* b, uint64_t* pair_off, ma_alignment* alns, uint64_t* ops, int32_t* mate, int32_t* other )
{
    return get_pairs( b, pair_off, alns, ops, mate, other, true );
}
} // extern "C"
