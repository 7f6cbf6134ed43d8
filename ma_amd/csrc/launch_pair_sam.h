// launch_pair_sam.h -- ma_pair_sam_batch and the download of its text.  Textually part of pipeline.hip.
//
// ma_pair_sam_batch has the shape of ma_sam_batch (launch_sam.h): k_pair_sam_size behind the pairing on the batch's stream, a
// scan of the per-pair byte counts into offsets, the ONE read-back of the statistics -- the bytes of the text and the records
// that end beyond their mate, the host formatter's exception, which the call then fails with, launching nothing more -- and
// k_pair_sam_write with nobody waiting.  Its state (pairSamDone, offsets, counts, text) is its own: the single-end text of
// ma_sam_batch on the same object is never touched.
namespace
{
PairSamKernelArgs pair_sam_args( ma_batch* b, u32 options )
{
    const ma_index* x = b->idx;
    PairSamKernelArgs A;
    A.contigs = ma_sam::Contigs{ x->cnames.as<char>( ), x->cnameOff.as<u64>( ), x->v.cstart, x->v.clen, (u32)x->v.n_contigs };
    A.options = options;
    A.n_pairs = (u32)( b->n_reads / 2 );
    A.picks_valid = b->nHsets ? 1u : 0u; // (ma_pair_batch launches nothing without harmonized sets)
    A.hset_off = b->hsetOff.as<u64>( );
    A.roff = b->d_roff;
    A.reads = b->d_reads;
    A.hdr = b->hdr.as<AlnHeader>( );
    A.pool = b->ops.as<u64>( );
    A.mq_order = b->mqOrder.as<u32>( );
    A.mq_cnt = b->mqCnt.as<u32>( );
    A.pick = b->pairPick.as<ma_pair::Pick>( );
    A.names = b->txtNames.as<char>( );
    A.name_off = b->txtNameOff.as<u64>( );
    A.qual = b->txtHasQual ? b->txtQual.as<uint8_t>( ) : nullptr;
    A.cnt = b->pairSamCnt.as<u64>( );
    A.off = b->pairSamOff.as<u64>( );
    A.seq_pos = b->pairSamSeqPos.as<u64>( );
    A.text = b->pairSamText.as<char>( );
    A.stat = b->pairSamStat.as<unsigned long long>( );
    return A;
}

// the host formatter's text for the first bad record (error path only): key = pair << 32 | index in the pair's records
int pair_sam_fail( ma_batch* b, u64 key )
{
    const u64 p = key >> 32;
    const u32 k = (u32)key;
    ma_pair::Pick pick;
    u64 hoff[ 2 ], roff[ 3 ];
    MA_HIP( hipMemcpyAsync( &pick, b->pairPick.as<ma_pair::Pick>( ) + p, sizeof( pick ), hipMemcpyDeviceToHost, b->stream ) );
    MA_HIP( hipMemcpyAsync( hoff, b->hsetOff.as<u64>( ) + 2 * p, 16, hipMemcpyDeviceToHost, b->stream ) );
    MA_HIP( hipMemcpyAsync( roff, b->d_roff + 2 * p, 24, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    // the record's mate and its place in that mate's MappingQuality order
    const bool first = pick.kind == ma_pair::PICKED ? k == 0 : pick.kind == ma_pair::FIRST_LIST;
    const u64 idx = pick.kind == ma_pair::PICKED ? ( k == 0 ? pick.i : pick.j ) : k;
    const u64 base = hoff[ first ? 0 : 1 ];
    u32 ord = 0;
    AlnHeader h;
    MA_HIP( hipMemcpyAsync( &ord, b->mqOrder.as<u32>( ) + base + idx, 4, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    MA_HIP( hipMemcpyAsync( &h, b->hdr.as<AlnHeader>( ) + base + ord, sizeof( h ), hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    char text[ 64 ];
    const bool rev = h.begin_ref >= b->idx->v.F;
    const u64 len = first ? roff[ 1 ] - roff[ 0 ] : roff[ 2 ] - roff[ 1 ];
    ma_sam::errorText( text, rev ? ma_sam::ERR_COMP_CHAR_AT : ma_sam::ERR_QUERY_LENGTH, (i64)len - (i64)h.end_q );
    return fail( text );
}
} // namespace

extern "C" {

int ma_pair_sam_batch( ma_batch* b, uint32_t options )
{
    if( !b )
        return fail( "ma_pair_sam_batch: null batch" );
    if( b->stage_done < 5 )
        return fail( "ma_pair_sam_batch: no pairs to print (run ma_pair_batch first)" );
    if( options & ~(uint32_t)ma_sam::ALL_OPTIONS )
        return fail( "ma_pair_sam_batch: unknown option bits " + std::to_string( options & ~(uint32_t)ma_sam::ALL_OPTIONS ) );
    if( !b->idx->namesSet )
        return fail( "ma_pair_sam_batch: the index has no contig names (ma_index_set_contig_names)" );
    if( !b->txtSet )
        return fail( "ma_pair_sam_batch: the reads have no names (ma_batch_set_read_text after the reads were set)" );
    MA_BIND_DEVICE( b->device );
    if( b->downPending ) // the text of the last call may still be on its way down
    {
        MA_HIP( hipEventSynchronize( b->evDown ) );
        b->downPending = false;
    }
    const u64 np = b->n_reads / 2;
    b->pairSamDone = false;
    b->pairSamBytes = 0;
    if( np )
    {
        if( b->pairSamCnt.reserve( ( np + 2 ) * 8 ) || b->pairSamOff.reserve( ( np + 2 ) * 8 ) || b->pairSamStat.reserve( PSAM_STAT_COUNT * 8 ) ||
            b->pairSamSeqPos.reserve( ( b->nHsets + 1 ) * 8 ) )
            return 1;
        const unsigned long long init[ PSAM_STAT_COUNT ] = { 0, 0, ~0ull, 0 };
        MA_HIP( hipMemcpyAsync( b->pairSamStat.p, init, sizeof( init ), hipMemcpyHostToDevice, b->stream ) );
        MA_HIP( hipMemsetAsync( (char*)b->pairSamCnt.p + np * 8, 0, 8, b->stream ) );
        PairSamKernelArgs A = pair_sam_args( b, options );
        const dim3 grid( (unsigned)( ( np + 255 ) / 256 ) ), block( 256 );
        hipLaunchKernelGGL( k_pair_sam_size, grid, block, 0, b->stream, A );
        MA_HIP( hipGetLastError( ) );
        if( scan_exclusive<u64>( b, b->pairSamCnt.as<u64>( ), b->pairSamOff.as<u64>( ), np + 1 ) )
            return 1;
        MA_HIP( hipMemcpyAsync( b->pairSamStat.as<unsigned long long>( ) + PSAM_STAT_BYTES, b->pairSamOff.as<u64>( ) + np, 8, hipMemcpyDeviceToDevice,
                                b->stream ) );
        unsigned long long stat[ PSAM_STAT_COUNT ];
        MA_HIP( hipMemcpyAsync( stat, b->pairSamStat.p, sizeof( stat ), hipMemcpyDeviceToHost, b->stream ) );
        if( batch_wait( b ) ) // (init goes out of scope as well)
            return 1;
        if( stat[ PSAM_STAT_ERRORS ] )
            return pair_sam_fail( b, stat[ PSAM_STAT_FIRST ] );
        if( b->pairSamText.reserve( stat[ PSAM_STAT_BYTES ] + 64 ) )
            return 1;
        A.text = b->pairSamText.as<char>( );
        hipLaunchKernelGGL( k_pair_sam_write, grid, block, 0, b->stream, A );
        MA_HIP( hipGetLastError( ) );
        b->pairSamBytes = stat[ PSAM_STAT_BYTES ];
    }
    b->pairSamDone = true;
    return 0;
}

int ma_batch_pair_sam_counts( ma_batch* b, uint64_t* n_pairs, uint64_t* n_bytes )
{
    if( !b || !b->pairSamDone )
        return fail( "ma_batch_pair_sam_counts: run ma_pair_sam_batch first" );
    if( n_pairs )
        *n_pairs = b->n_reads / 2;
    if( n_bytes )
        *n_bytes = b->pairSamBytes;
    return 0;
}
} // extern "C"

// async: see get_alns
static int get_pair_sam( ma_batch* b, uint64_t* pair_off, char* text, bool async )
{
    if( !b || !b->pairSamDone )
        return fail( "ma_batch_get_pair_sam: run ma_pair_sam_batch first" );
    MA_BIND_DEVICE( b->device );
    if( b->downPending )
    {
        if( async )
            return fail( "ma_batch_start_pair_sam_download: the download started before was not finished (ma_batch_finish_download)" );
        MA_HIP( hipEventSynchronize( b->evDown ) );
        b->downPending = false;
    }
    if( async && io_init( b ) )
        return 1;
    const u64 np = b->n_reads / 2;
    if( np == 0 )
    {
        if( pair_off )
            pair_off[ 0 ] = 0;
        return 0;
    }
    hipStream_t cs = b->stream;
    if( async )
    {
        cs = b->ioStream;
        MA_HIP( hipEventRecord( b->evPacked, b->stream ) );
        MA_HIP( hipStreamWaitEvent( cs, b->evPacked, 0 ) );
    }
    if( pair_off )
        MA_HIP( hipMemcpyAsync( pair_off, b->pairSamOff.p, ( np + 1 ) * 8, hipMemcpyDeviceToHost, cs ) );
    if( text && b->pairSamBytes )
        MA_HIP( hipMemcpyAsync( text, b->pairSamText.p, b->pairSamBytes, hipMemcpyDeviceToHost, cs ) );
    if( async )
    {
        MA_HIP( hipEventRecord( b->evDown, cs ) );
        b->downPending = true;
        return 0;
    }
    return batch_wait( b );
}

extern "C" {
int ma_batch_get_pair_sam( ma_batch* b, uint64_t* pair_off, char* text )
{
    return get_pair_sam( b, pair_off, text, false );
}
int ma_batch_start_pair_sam_download( ma_batch* b, uint64_t* pair_off, char* text )
{
    return get_pair_sam( b, pair_off, text, true );
}
} // extern "C"
