// launch_sam.h -- ma_batch_set_read_text, ma_sam_batch, ma_pair_sam_batch and the downloads of their texts.  Textually part of
// pipeline.hip.
//
// Both calls are one sequence (sam_text_launch) over a SamTextState of their own: the size kernel behind the stage before on the
// batch's stream, a scan of the per-item byte counts into offsets, and the wait with the ONE read-back of the text's
// statistics: its bytes (the size of the download) and the records that end beyond their read -- the host formatter's
// exception, which the call then fails with, launching nothing more.  The write kernel follows on the stream with nobody
// waiting; the gets and downloads (get_sam_text) are two plain copies.  The calls differ in their items (reads / pairs), their
// kernels and arguments (stage_sam.h / stage_pair_sam.h) and in how the first bad record is found again.
namespace
{
// (cnt, off, seq_pos, text and stat are the launcher's to fill)
SamKernelArgs sam_args( ma_batch* b, u32 options )
{
    const ma_index* x = b->idx;
    SamKernelArgs A;
    A.contigs = ma_sam::Contigs{ x->cnames.as<char>( ), x->cnameOff.as<u64>( ), x->v.cstart, x->v.clen, (u32)x->v.n_contigs };
    A.options = options;
    const MqView V = mq_view( b );
    A.n_reads = (u32)b->n_reads;
    A.hset_off = V.off;
    A.roff = b->d_roff;
    A.reads = b->d_reads;
    A.hdr = V.hdr;
    A.pool = b->ops.as<u64>( );
    A.mq_order = V.order;
    A.mq_cnt = V.cnt;
    A.names = b->txtNames.as<char>( );
    A.name_off = b->txtNameOff.as<u64>( );
    A.qual = b->st.hasQual ? b->txtQual.as<uint8_t>( ) : nullptr;
    A.ref = ma_sam::Ref{ x->v.pac, x->holeStart.as<u64>( ), x->holeLen.as<u64>( ), x->nHoles, x->v.F };
    return A;
}

// the host formatter's text for the first bad record (error path only: both CSR offset arrays, (n + 1) * 8 bytes each, and the
// record's place in the MappingQuality order come down behind one wait, its header behind a second)
int sam_fail( ma_batch* b, u64 slot )
{
    const u64 n = b->n_reads;
    const MqView V = mq_view( b );
    std::vector<u64> hoff( n + 1 ), roff( n + 1 );
    u32 ord = 0;
    AlnHeader h;
    MA_HIP( hipMemcpyAsync( hoff.data( ), V.off, ( n + 1 ) * 8, hipMemcpyDeviceToHost, b->stream ) );
    MA_HIP( hipMemcpyAsync( roff.data( ), b->d_roff, ( n + 1 ) * 8, hipMemcpyDeviceToHost, b->stream ) );
    MA_HIP( hipMemcpyAsync( &ord, V.order + slot, 4, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    const u64 r = (u64)( std::upper_bound( hoff.begin( ), hoff.end( ), slot ) - hoff.begin( ) ) - 1;
    MA_HIP( hipMemcpyAsync( &h, V.hdr + hoff[ r ] + ord, sizeof( h ), hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    char text[ 64 ];
    const bool rev = h.begin_ref >= b->idx->v.F;
    ma_sam::errorText( text, rev ? ma_sam::ERR_COMP_CHAR_AT : ma_sam::ERR_QUERY_LENGTH,
                       (i64)( roff[ r + 1 ] - roff[ r ] ) - (i64)h.end_q );
    return fail( text );
}

// the same for a text with tags: key = slot * 4 + kind - 1 (SamTagCountSink).  The two kinds of the tags: the reference's text for
// a record across the strands, the library's own -- naming the record -- for ops that do not cover the record's intervals
int sam_tag_fail( ma_batch* b, u64 key )
{
    const u64 slot = key >> 2;
    const u32 kind = (u32)( key & 3 ) + 1;
    if( kind == ma_sam::ERR_QUERY_LENGTH || kind == ma_sam::ERR_COMP_CHAR_AT )
        return sam_fail( b, slot );
    char text[ 96 ];
    ma_sam::errorText( text, kind, 0 );
    if( kind == ma_sam::ERR_BRIDGING )
        return fail( text );
    const u64 n = b->n_reads;
    std::vector<u64> hoff( n + 1 );
    MA_HIP( hipMemcpyAsync( hoff.data( ), mq_view( b ).off, ( n + 1 ) * 8, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    const u64 r = (u64)( std::upper_bound( hoff.begin( ), hoff.end( ), slot ) - hoff.begin( ) ) - 1;
    return fail( "ma_sam_batch: record " + std::to_string( slot - hoff[ r ] ) + " of read " + std::to_string( r ) + ": " + text +
                 " (MA_SAM_NGMLR_TAGS reads the reference along them)" );
}

PairSamKernelArgs pair_sam_args( ma_batch* b, u32 options )
{
    const ma_index* x = b->idx;
    PairSamKernelArgs A;
    A.contigs = ma_sam::Contigs{ x->cnames.as<char>( ), x->cnameOff.as<u64>( ), x->v.cstart, x->v.clen, (u32)x->v.n_contigs };
    A.options = options;
    A.n_pairs = (u32)( b->n_reads / 2 );
    A.picks_valid = b->st.nHsets ? 1u : 0u; // (ma_pair_batch launches nothing without harmonized sets)
    const MqView V = mq_view( b );
    A.hset_off = V.off;
    A.roff = b->d_roff;
    A.reads = b->d_reads;
    A.hdr = V.hdr;
    A.pool = b->ops.as<u64>( );
    A.mq_order = V.order;
    A.mq_cnt = V.cnt;
    A.pick = b->pairPick.as<ma_pair::Pick>( );
    A.names = b->txtNames.as<char>( );
    A.name_off = b->txtNameOff.as<u64>( );
    A.qual = b->st.hasQual ? b->txtQual.as<uint8_t>( ) : nullptr;
    return A;
}

// the host formatter's text for the first bad record (error path only): key = pair << 32 | index in the pair's records
int pair_sam_fail( ma_batch* b, u64 key )
{
    const u64 p = key >> 32;
    const u32 k = (u32)key;
    const MqView V = mq_view( b );
    ma_pair::Pick pick;
    u64 hoff[ 2 ], roff[ 3 ];
    MA_HIP( hipMemcpyAsync( &pick, b->pairPick.as<ma_pair::Pick>( ) + p, sizeof( pick ), hipMemcpyDeviceToHost, b->stream ) );
    MA_HIP( hipMemcpyAsync( hoff, V.off + 2 * p, 16, hipMemcpyDeviceToHost, b->stream ) );
    MA_HIP( hipMemcpyAsync( roff, b->d_roff + 2 * p, 24, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    // the record's mate and its place in that mate's MappingQuality order
    const bool first = pick.kind == ma_pair::PICKED ? k == 0 : pick.kind == ma_pair::FIRST_LIST;
    const u64 idx = pick.kind == ma_pair::PICKED ? ( k == 0 ? pick.i : pick.j ) : k;
    const u64 base = hoff[ first ? 0 : 1 ];
    u32 ord = 0;
    AlnHeader h;
    MA_HIP( hipMemcpyAsync( &ord, V.order + base + idx, 4, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    MA_HIP( hipMemcpyAsync( &h, V.hdr + base + ord, sizeof( h ), hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    char text[ 64 ];
    const bool rev = h.begin_ref >= b->idx->v.F;
    const u64 len = first ? roff[ 1 ] - roff[ 0 ] : roff[ 2 ] - roff[ 1 ];
    ma_sam::errorText( text, rev ? ma_sam::ERR_COMP_CHAR_AT : ma_sam::ERR_QUERY_LENGTH, (i64)len - (i64)h.end_q );
    return fail( text );
}

// The text of n items into s.  A: the stage's arguments but for the state's arrays.
template <typename Args, void ( *SizeKernel )( Args ), void ( *WriteKernel )( Args ), int ( *Fail )( ma_batch*, u64 )>
int sam_text_launch( ma_batch* b, SamTextState& s, u64 n, Args A )
{
    if( download_wait( b ) ) // the text of the last call may still be on its way down
        return 1;
    b->st.drop( s.id ); // (the members of ma_sam_bgzf_batch are of the text before)
    if( n )
    {
        if( s.cnt.reserve( ( n + 2 ) * 8 ) || s.off.reserve( ( n + 2 ) * 8 ) || s.stat.reserve( SAM_STAT_COUNT * 8 ) ||
            s.seqPos.reserve( ( mq_view( b ).slots + 1 ) * 8 ) )
            return 1;
        const unsigned long long init[ SAM_STAT_COUNT ] = { 0, 0, ~0ull, 0 };
        MA_HIP( hipMemcpyAsync( s.stat.p, init, sizeof( init ), hipMemcpyHostToDevice, b->stream ) );
        MA_HIP( hipMemsetAsync( (char*)s.cnt.p + n * 8, 0, 8, b->stream ) );
        A.cnt = s.cnt.as<u64>( );
        A.off = s.off.as<u64>( );
        A.seq_pos = s.seqPos.as<u64>( );
        A.text = s.text.as<char>( );
        A.stat = s.stat.as<unsigned long long>( );
        const dim3 grid( (unsigned)( ( n + 255 ) / 256 ) ), block( 256 );
        hipLaunchKernelGGL( SizeKernel, grid, block, 0, b->stream, A );
        MA_HIP( hipGetLastError( ) );
        if( scan_exclusive<u64>( b, s.cnt.as<u64>( ), s.off.as<u64>( ), n + 1 ) )
            return 1;
        MA_HIP( hipMemcpyAsync( A.stat + SAM_STAT_BYTES, s.off.as<u64>( ) + n, 8, hipMemcpyDeviceToDevice, b->stream ) );
        unsigned long long stat[ SAM_STAT_COUNT ];
        MA_HIP( hipMemcpyAsync( stat, s.stat.p, sizeof( stat ), hipMemcpyDeviceToHost, b->stream ) );
        if( batch_wait( b ) ) // (init goes out of scope as well)
            return 1;
        if( stat[ SAM_STAT_ERRORS ] )
            return Fail( b, stat[ SAM_STAT_FIRST ] );
        if( s.text.reserve( stat[ SAM_STAT_BYTES ] + 64 ) )
            return 1;
        A.text = s.text.as<char>( );
        hipLaunchKernelGGL( WriteKernel, grid, block, 0, b->stream, A );
        MA_HIP( hipGetLastError( ) );
        b->st.text( s.id ).bytes = stat[ SAM_STAT_BYTES ];
    }
    b->st.finish( s.id );
    return 0;
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

int ma_index_set_holes( ma_index* x, const uint64_t* start, const uint64_t* length, uint64_t n )
{
    if( !x || ( n && ( !start || !length ) ) )
        return fail( "ma_index_set_holes: null argument" );
    for( u64 i = 0; i < n; i++ )
    {
        if( length[ i ] == 0 || start[ i ] >= x->v.F || length[ i ] > x->v.F - start[ i ] )
            return fail( "ma_index_set_holes: hole " + std::to_string( i ) + " is empty or not inside the forward strand" );
        if( i && start[ i ] < start[ i - 1 ] + length[ i - 1 ] )
            return fail( "ma_index_set_holes: hole " + std::to_string( i ) + " starts before the one before it ends (sorted, not overlapping)" );
    }
    MA_BIND_DEVICE( x->device );
    x->nHoles = 0;
    if( n )
    {
        if( x->holeStart.reserve( n * 8 ) || x->holeLen.reserve( n * 8 ) )
            return 1;
        MA_HIP( hipMemcpy( x->holeStart.p, start, n * 8, hipMemcpyHostToDevice ) );
        MA_HIP( hipMemcpy( x->holeLen.p, length, n * 8, hipMemcpyHostToDevice ) );
    }
    x->nHoles = n;
    return 0;
}

int ma_debug_ngmlr_floats( int kind, const uint64_t* num, const uint64_t* den, uint64_t n, char* out )
{
    if( !num || !den || !out || kind < 0 || kind > 1 )
        return fail( "ma_debug_ngmlr_floats: bad argument" );
    if( n == 0 )
        return 0;
    DevBuf dn, dd, dout;
    if( dn.reserve( n * 8 ) || dd.reserve( n * 8 ) || dout.reserve( n * 16 ) )
        return 1;
    MA_HIP( hipMemcpy( dn.p, num, n * 8, hipMemcpyHostToDevice ) );
    MA_HIP( hipMemcpy( dd.p, den, n * 8, hipMemcpyHostToDevice ) );
    hipLaunchKernelGGL( k_ngmlr_float_probe, dim3( (unsigned)( ( n + 255 ) / 256 ) ), dim3( 256 ), 0, 0, kind, dn.as<u64>( ), dd.as<u64>( ), n,
                        dout.as<char>( ) );
    MA_HIP( hipGetLastError( ) );
    MA_HIP( hipMemcpy( out, dout.p, n * 16, hipMemcpyDeviceToHost ) );
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
    b->st.drop( ma_state::NAMES ); // (both texts were printed with the names before)
    if( b->txtNames.reserve( name_off[ n ] + 1 ) || b->txtNameOff.reserve( ( n + 1 ) * 8 ) || ( qual && b->txtQual.reserve( b->n_bases + 1 ) ) )
        return 1;
    if( name_off[ n ] )
        MA_HIP( hipMemcpyAsync( b->txtNames.p, names, name_off[ n ], hipMemcpyHostToDevice, b->stream ) );
    MA_HIP( hipMemcpyAsync( b->txtNameOff.p, name_off, ( n + 1 ) * 8, hipMemcpyHostToDevice, b->stream ) );
    if( qual && b->n_bases )
        MA_HIP( hipMemcpyAsync( b->txtQual.p, qual, b->n_bases, hipMemcpyHostToDevice, b->stream ) );
    if( batch_wait( b ) )
        return 1; // the caller's arrays are free again
    b->st.hasQual = qual != nullptr;
    b->st.nameBytes = name_off[ n ];
    b->st.finish( ma_state::NAMES );
    return 0;
}

int ma_sam_batch( ma_batch* b, uint32_t options )
{
    if( !b )
        return fail( "ma_sam_batch: null batch" );
    if( !b->st.has( ma_state::ALIGNED ) )
        return fail( "ma_sam_batch: no MappingQuality output to print (run ma_dp_batch / ma_align_batch / ma_batch_set_alignments first)" );
    if( options & ~(uint32_t)ma_sam::ALL_OPTIONS )
        return fail( "ma_sam_batch: unknown option bits " + std::to_string( options & ~(uint32_t)ma_sam::ALL_OPTIONS ) );
    if( !b->idx->namesSet )
        return fail( "ma_sam_batch: the index has no contig names (ma_index_set_contig_names)" );
    if( !b->st.has( ma_state::NAMES ) )
        return fail( "ma_sam_batch: the reads have no names (ma_batch_set_read_text after the reads were set)" );
    MA_BIND_DEVICE( b->device );
    if( options & ma_sam::NGMLR_TAGS )
        return sam_text_launch<SamKernelArgs, k_sam_size<true>, k_sam_write<true>, sam_tag_fail>( b, b->sam, b->n_reads, sam_args( b, options ) );
    return sam_text_launch<SamKernelArgs, k_sam_size<false>, k_sam_write<false>, sam_fail>( b, b->sam, b->n_reads, sam_args( b, options ) );
}

int ma_pair_sam_batch( ma_batch* b, uint32_t options )
{
    if( !b )
        return fail( "ma_pair_sam_batch: null batch" );
    if( !b->st.has( ma_state::PAIRS ) )
        return fail( "ma_pair_sam_batch: no pairs to print (run ma_pair_batch first)" );
    if( options & ~(uint32_t)ma_sam::PAIR_OPTIONS ) // (the tag emulation is the single-end writer's)
        return fail( "ma_pair_sam_batch: unknown option bits " + std::to_string( options & ~(uint32_t)ma_sam::PAIR_OPTIONS ) );
    if( !b->idx->namesSet )
        return fail( "ma_pair_sam_batch: the index has no contig names (ma_index_set_contig_names)" );
    if( !b->st.has( ma_state::NAMES ) )
        return fail( "ma_pair_sam_batch: the reads have no names (ma_batch_set_read_text after the reads were set)" );
    MA_BIND_DEVICE( b->device );
    return sam_text_launch<PairSamKernelArgs, k_pair_sam_size, k_pair_sam_write, pair_sam_fail>( b, b->pairSam, b->n_reads / 2,
                                                                                                 pair_sam_args( b, options ) );
}

int ma_batch_sam_counts( ma_batch* b, uint64_t* n_bytes )
{
    if( !b || !b->st.has( ma_state::SAM ) )
        return fail( "ma_batch_sam_counts: run ma_sam_batch first" );
    if( n_bytes )
        *n_bytes = b->st.sam.bytes;
    return 0;
}

int ma_batch_pair_sam_counts( ma_batch* b, uint64_t* n_pairs, uint64_t* n_bytes )
{
    if( !b || !b->st.has( ma_state::PAIR_SAM ) )
        return fail( "ma_batch_pair_sam_counts: run ma_pair_sam_batch first" );
    if( n_pairs )
        *n_pairs = b->n_reads / 2;
    if( n_bytes )
        *n_bytes = b->st.pairSam.bytes;
    return 0;
}
} // extern "C"

// The download of one text of n items and of its offsets; async and start: see get_alns, download_begin
static int get_sam_text( ma_batch* b, const SamTextState& s, u64 n, const char* start, uint64_t* off, char* text, bool async )
{
    MA_BIND_DEVICE( b->device );
    const u64 bytes = b->st.text( s.id ).bytes;
    if( download_begin( b, async, start ) )
        return 1;
    if( n == 0 )
    {
        if( off )
            off[ 0 ] = 0;
        return 0;
    }
    hipStream_t cs;
    if( download_stream( b, async, &cs ) )
        return 1;
    if( off )
        MA_HIP( hipMemcpyAsync( off, s.off.p, ( n + 1 ) * 8, hipMemcpyDeviceToHost, cs ) );
    if( text && bytes )
        MA_HIP( hipMemcpyAsync( text, s.text.p, bytes, hipMemcpyDeviceToHost, cs ) );
    return download_end( b, async, cs );
}

static int get_sam( ma_batch* b, uint64_t* rec_off, char* text, bool async )
{
    if( !b || !b->st.has( ma_state::SAM ) )
        return fail( "ma_batch_get_sam: run ma_sam_batch first" );
    return get_sam_text( b, b->sam, b->n_reads, "ma_batch_start_sam_download", rec_off, text, async );
}
static int get_pair_sam( ma_batch* b, uint64_t* pair_off, char* text, bool async )
{
    if( !b || !b->st.has( ma_state::PAIR_SAM ) )
        return fail( "ma_batch_get_pair_sam: run ma_pair_sam_batch first" );
    return get_sam_text( b, b->pairSam, b->n_reads / 2, "ma_batch_start_pair_sam_download", pair_off, text, async );
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
int ma_batch_get_pair_sam( ma_batch* b, uint64_t* pair_off, char* text )
{
    return get_pair_sam( b, pair_off, text, false );
}
int ma_batch_start_pair_sam_download( ma_batch* b, uint64_t* pair_off, char* text )
{
    return get_pair_sam( b, pair_off, text, true );
}
} // extern "C"
