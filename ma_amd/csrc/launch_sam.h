// launch_sam.h -- ma_batch_set_read_text, ma_sam_batch and the download of its text.  Textually part of pipeline.hip.
//
// ma_sam_batch runs k_sam_size behind the MappingQuality stage on the batch's stream, scans the per-read byte counts into
// offsets and waits with the ONE read-back of the batch's SAM statistics: the bytes of the text (the size of the download) and
// the records that end beyond their read -- the host formatter's exception, which the call then fails with, launching nothing
// more.  k_sam_write follows on the stream; ma_batch_get_sam / ma_batch_start_sam_download are two plain copies.
namespace
{
SamKernelArgs sam_args( ma_batch* b, u32 options )
{
    const ma_index* x = b->idx;
    SamKernelArgs A;
    A.contigs = ma_sam::Contigs{ x->cnames.as<char>( ), x->cnameOff.as<u64>( ), x->v.cstart, x->v.clen, (u32)x->v.n_contigs };
    A.options = options;
    A.n_reads = (u32)b->n_reads;
    A.hset_off = b->hsetOff.as<u64>( );
    A.roff = b->d_roff;
    A.reads = b->d_reads;
    A.hdr = b->hdr.as<AlnHeader>( );
    A.pool = b->ops.as<u64>( );
    A.mq_order = b->mqOrder.as<u32>( );
    A.mq_cnt = b->mqCnt.as<u32>( );
    A.names = b->txtNames.as<char>( );
    A.name_off = b->txtNameOff.as<u64>( );
    A.qual = b->txtHasQual ? b->txtQual.as<uint8_t>( ) : nullptr;
    A.cnt = b->samCnt.as<u64>( );
    A.off = b->samOff.as<u64>( );
    A.seq_pos = b->samSeqPos.as<u64>( );
    A.text = b->samText.as<char>( );
    A.stat = b->samStat.as<unsigned long long>( );
    return A;
}

// the host formatter's text for the first bad record (error path only: both CSR offset arrays, (n + 1) * 8 bytes each, and the
// record's place in the MappingQuality order come down behind one wait, its header behind a second)
int sam_fail( ma_batch* b, u64 slot )
{
    const u64 n = b->n_reads;
    std::vector<u64> hoff( n + 1 ), roff( n + 1 );
    u32 ord = 0;
    AlnHeader h;
    MA_HIP( hipMemcpyAsync( hoff.data( ), b->hsetOff.p, ( n + 1 ) * 8, hipMemcpyDeviceToHost, b->stream ) );
    MA_HIP( hipMemcpyAsync( roff.data( ), b->d_roff, ( n + 1 ) * 8, hipMemcpyDeviceToHost, b->stream ) );
    MA_HIP( hipMemcpyAsync( &ord, b->mqOrder.as<u32>( ) + slot, 4, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    const u64 r = (u64)( std::upper_bound( hoff.begin( ), hoff.end( ), slot ) - hoff.begin( ) ) - 1;
    MA_HIP( hipMemcpyAsync( &h, b->hdr.as<AlnHeader>( ) + hoff[ r ] + ord, sizeof( h ), hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    char text[ 64 ];
    const bool rev = h.begin_ref >= b->idx->v.F;
    ma_sam::errorText( text, rev ? ma_sam::ERR_COMP_CHAR_AT : ma_sam::ERR_QUERY_LENGTH,
                       (i64)( roff[ r + 1 ] - roff[ r ] ) - (i64)h.end_q );
    return fail( text );
}
} // namespace

extern "C" {

int ma_index_set_contig_names( ma_index* x, const char* names, const uint64_t* name_off )
{
    if( !x || !name_off || x->v.n_contigs < 1 )
        return fail( "ma_index_set_contig_names: null argument or an index without contigs" );
    const u64 nc = (u64)x->v.n_contigs;
    if( name_off[ 0 ] != 0 || ( name_off[ nc ] && !names ) )
        return fail( "ma_index_set_contig_names: null names or offsets that do not start at 0" );
    for( u64 i = 0; i < nc; i++ )
        if( name_off[ i + 1 ] < name_off[ i ] )
            return fail( "ma_index_set_contig_names: offsets decrease" );
    MA_BIND_DEVICE( x->device );
    x->namesSet = false;
    if( x->cnames.reserve( name_off[ nc ] + 1 ) || x->cnameOff.reserve( ( nc + 1 ) * 8 ) )
        return 1;
    if( name_off[ nc ] )
        MA_HIP( hipMemcpy( x->cnames.p, names, name_off[ nc ], hipMemcpyHostToDevice ) );
    MA_HIP( hipMemcpy( x->cnameOff.p, name_off, ( nc + 1 ) * 8, hipMemcpyHostToDevice ) );
    x->namesSet = true;
    return 0;
}

int ma_batch_set_read_text( ma_batch* b, const char* names, const uint64_t* name_off, const uint8_t* qual )
{
    if( !b || !b->d_roff || !name_off )
        return fail( "ma_batch_set_read_text: no reads set or null argument" );
    const u64 n = b->n_reads;
    if( name_off[ 0 ] != 0 || ( name_off[ n ] && !names ) )
        return fail( "ma_batch_set_read_text: null names or offsets that do not start at 0" );
    for( u64 i = 0; i < n; i++ )
        if( name_off[ i + 1 ] < name_off[ i ] )
            return fail( "ma_batch_set_read_text: offsets decrease" );
    MA_BIND_DEVICE( b->device );
    b->txtSet = b->samDone = b->pairSamDone = false;
    if( b->txtNames.reserve( name_off[ n ] + 1 ) || b->txtNameOff.reserve( ( n + 1 ) * 8 ) || ( qual && b->txtQual.reserve( b->n_bases + 1 ) ) )
        return 1;
    if( name_off[ n ] )
        MA_HIP( hipMemcpyAsync( b->txtNames.p, names, name_off[ n ], hipMemcpyHostToDevice, b->stream ) );
    MA_HIP( hipMemcpyAsync( b->txtNameOff.p, name_off, ( n + 1 ) * 8, hipMemcpyHostToDevice, b->stream ) );
    if( qual && b->n_bases )
        MA_HIP( hipMemcpyAsync( b->txtQual.p, qual, b->n_bases, hipMemcpyHostToDevice, b->stream ) );
    if( batch_wait( b ) )
        return 1; // the caller's arrays are free again
    b->txtHasQual = qual != nullptr;
    b->txtSet = true;
    return 0;
}

int ma_sam_batch( ma_batch* b, uint32_t options )
{
    if( !b )
        return fail( "ma_sam_batch: null batch" );
    if( b->stage_done < 4 )
        return fail( "ma_sam_batch: no MappingQuality output to print (run ma_dp_batch / ma_align_batch / ma_batch_set_alignments first)" );
    if( options & ~(uint32_t)ma_sam::ALL_OPTIONS )
        return fail( "ma_sam_batch: unknown option bits " + std::to_string( options & ~(uint32_t)ma_sam::ALL_OPTIONS ) );
    if( !b->idx->namesSet )
        return fail( "ma_sam_batch: the index has no contig names (ma_index_set_contig_names)" );
    if( !b->txtSet )
        return fail( "ma_sam_batch: the reads have no names (ma_batch_set_read_text after the reads were set)" );
    MA_BIND_DEVICE( b->device );
    if( b->downPending ) // the text of the last call may still be on its way down
    {
        MA_HIP( hipEventSynchronize( b->evDown ) );
        b->downPending = false;
    }
    const u64 n = b->n_reads;
    b->samDone = false;
    b->samBytes = 0;
    if( n )
    {
        if( b->samCnt.reserve( ( n + 2 ) * 8 ) || b->samOff.reserve( ( n + 2 ) * 8 ) || b->samStat.reserve( SAM_STAT_COUNT * 8 ) ||
            b->samSeqPos.reserve( ( b->nHsets + 1 ) * 8 ) )
            return 1;
        const unsigned long long init[ SAM_STAT_COUNT ] = { 0, 0, ~0ull, 0 };
        MA_HIP( hipMemcpyAsync( b->samStat.p, init, sizeof( init ), hipMemcpyHostToDevice, b->stream ) );
        MA_HIP( hipMemsetAsync( (char*)b->samCnt.p + n * 8, 0, 8, b->stream ) );
        SamKernelArgs A = sam_args( b, options );
        const dim3 grid( (unsigned)( ( n + 255 ) / 256 ) ), block( 256 );
        hipLaunchKernelGGL( k_sam_size, grid, block, 0, b->stream, A );
        MA_HIP( hipGetLastError( ) );
        if( scan_exclusive<u64>( b, b->samCnt.as<u64>( ), b->samOff.as<u64>( ), n + 1 ) )
            return 1;
        MA_HIP( hipMemcpyAsync( b->samStat.as<unsigned long long>( ) + SAM_STAT_BYTES, b->samOff.as<u64>( ) + n, 8, hipMemcpyDeviceToDevice, b->stream ) );
        unsigned long long stat[ SAM_STAT_COUNT ];
        MA_HIP( hipMemcpyAsync( stat, b->samStat.p, sizeof( stat ), hipMemcpyDeviceToHost, b->stream ) );
        if( batch_wait( b ) ) // (init goes out of scope as well)
            return 1;
        if( stat[ SAM_STAT_ERRORS ] )
            return sam_fail( b, stat[ SAM_STAT_FIRST ] );
        if( b->samText.reserve( stat[ SAM_STAT_BYTES ] + 64 ) )
            return 1;
        A.text = b->samText.as<char>( );
        hipLaunchKernelGGL( k_sam_write, grid, block, 0, b->stream, A );
        MA_HIP( hipGetLastError( ) );
        b->samBytes = stat[ SAM_STAT_BYTES ];
    }
    b->samDone = true;
    return 0;
}

int ma_batch_sam_counts( ma_batch* b, uint64_t* n_bytes )
{
    if( !b || !b->samDone )
        return fail( "ma_batch_sam_counts: run ma_sam_batch first" );
    if( n_bytes )
        *n_bytes = b->samBytes;
    return 0;
}
} // extern "C"

// async: see get_alns
static int get_sam( ma_batch* b, uint64_t* rec_off, char* text, bool async )
{
    if( !b || !b->samDone )
        return fail( "ma_batch_get_sam: run ma_sam_batch first" );
    MA_BIND_DEVICE( b->device );
    if( b->downPending )
    {
        if( async )
            return fail( "ma_batch_start_sam_download: the download started before was not finished (ma_batch_finish_download)" );
        MA_HIP( hipEventSynchronize( b->evDown ) );
        b->downPending = false;
    }
    if( async && io_init( b ) )
        return 1;
    const u64 n = b->n_reads;
    if( n == 0 )
    {
        if( rec_off )
            rec_off[ 0 ] = 0;
        return 0;
    }
    hipStream_t cs = b->stream;
    if( async )
    {
        cs = b->ioStream;
        MA_HIP( hipEventRecord( b->evPacked, b->stream ) );
        MA_HIP( hipStreamWaitEvent( cs, b->evPacked, 0 ) );
    }
    if( rec_off )
        MA_HIP( hipMemcpyAsync( rec_off, b->samOff.p, ( n + 1 ) * 8, hipMemcpyDeviceToHost, cs ) );
    if( text && b->samBytes )
        MA_HIP( hipMemcpyAsync( text, b->samText.p, b->samBytes, hipMemcpyDeviceToHost, cs ) );
    if( async )
    {
        MA_HIP( hipEventRecord( b->evDown, cs ) );
        b->downPending = true;
        return 0;
    }
    return batch_wait( b );
}

extern "C" {
int ma_batch_get_sam( ma_batch* b, uint64_t* rec_off, char* text )
{
    return get_sam( b, rec_off, text, false );
}
int ma_batch_start_sam_download( ma_batch* b, uint64_t* rec_off, char* text )
{
    return get_sam( b, rec_off, text, true );
}
} // extern "C"
