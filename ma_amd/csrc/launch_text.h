// launch_text.h -- ma_batch_set_reads_text and the getters of a batch's reads and read text.  Textually part of pipeline.hip;
// the kernels are in stage_text.h, the rules in ma_amd/host/ma_text_dev.h.

// the batch holds no reads and no text (what a failed ma_batch_set_reads_text leaves, and what it starts from)
static int text_no_reads( ma_batch* b )
{
    b->n_reads = b->n_bases = 0;
    b->max_qlen = 0;
    b->d_reads = b->reads.as<uint8_t>( );
    b->d_roff = b->roff.as<u64>( );
    b->reads_external = false;
    b->stage_done = 0;
    b->txtSet = b->txtHasQual = b->sam.done = b->pairSam.done = false;
    b->txtNameBytes = 0;
    inv_reset( b );
    MA_HIP( hipMemsetAsync( b->roff.p, 0, 8, b->stream ) );
    return 0;
}

static int text_refuse( u64 line, u64 byte, u32 reason )
{
    char msg[ 256 ];
    ma_text::message( msg, sizeof( msg ), line, byte, reason );
    return fail( msg );
}

extern "C" {

int ma_batch_set_reads_text( ma_batch* b, const char* text, uint64_t n, uint64_t* n_reads )
{
    if( !b || ( n && !text ) )
        return fail( "ma_batch_set_reads_text: null argument" );
    MA_BIND_DEVICE( b->device );
    if( n_reads )
        *n_reads = 0;
    if( text_no_reads( b ) )
        return 1;
    if( n > ma_text::MAX_TEXT_BYTES )
        return batch_wait( b ) || text_refuse( 0, 0, ma_text::ERR_TOO_LARGE );
    if( n && text[ 0 ] != '@' && text[ 0 ] != '>' )
        return batch_wait( b ) || text_refuse( 0, 0, ma_text::ERR_KIND );
    if( b->txtNameOff.reserve( ( b->max_reads + 1 ) * 8 ) )
        return 1;
    MA_HIP( hipMemsetAsync( b->txtNameOff.p, 0, 8, b->stream ) );
    if( n == 0 )
    {
        if( batch_wait( b ) )
            return 1;
        b->txtSet = true;
        return 0;
    }
    const u32 kind = text[ 0 ] == '@' ? ma_text::KIND_FASTQ : ma_text::KIND_FASTA;
    const u64 nBlocks = ( n + TEXT_BLOCK_BYTES - 1 ) / TEXT_BLOCK_BYTES;
    if( b->txtIn.reserve( n + 64 ) || b->txtStat.reserve( TXT_WORDS * 8 ) || b->txtBlock.reserve( ( nBlocks + 1 ) * 4 ) )
        return 1;
    unsigned long long* const stat = b->txtStat.as<unsigned long long>( );
    unsigned long long h[ TXT_WORDS ];
    MA_HIP( hipMemcpyAsync( b->txtIn.p, text, n, hipMemcpyHostToDevice, b->stream ) );
    MA_HIP( hipMemsetAsync( stat, 0, TXT_WORDS * 8, b->stream ) );
    MA_HIP( hipMemsetAsync( stat + TXT_LONE_CR, 0xff, 2 * 8, b->stream ) ); // TXT_LONE_CR, TXT_VIOLATION: none
    const dim3 textGrid( (unsigned)nBlocks ), textBlock( TEXT_BLOCK );
    hipLaunchKernelGGL( k_text_count, textGrid, textBlock, 0, b->stream, b->txtIn.as<char>( ), n, b->txtBlock.as<u32>( ), stat );
    MA_HIP( hipGetLastError( ) );
    // read-back 1: the number of lines sizes the per-line scratch and launches
    MA_HIP( hipMemcpyAsync( h, stat, 8, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    const u64 feeds = h[ TXT_FEEDS ], lines = ma_text::nLines( feeds, text[ n - 1 ] );
    if( b->txtStart.reserve( ( lines + 2 ) * 4 ) || b->txtHdrName.reserve( ( lines + 2 ) * 8 ) || b->txtBases.reserve( ( lines + 2 ) * 4 ) ||
        b->txtRecLine.reserve( ( lines + 2 ) * 4 ) || b->txtNames.reserve( n + 1 ) ||
        ( kind == ma_text::KIND_FASTQ && b->txtQual.reserve( b->max_bases + 1 ) ) )
        return 1;
    if( scan_exclusive<u32>( b, b->txtBlock.as<u32>( ), b->txtBlock.as<u32>( ), nBlocks ) )
        return 1;
    hipLaunchKernelGGL( k_text_lines, textGrid, textBlock, 0, b->stream, b->txtIn.as<char>( ), n, b->txtBlock.as<u32>( ), feeds, b->txtStart.as<u32>( ) );
    const dim3 lineGrid( (unsigned)( ( lines + 1 + 255 ) / 256 ) ), lineBlock( 256 );
    hipLaunchKernelGGL( k_text_classify, lineGrid, lineBlock, 0, b->stream, kind, b->txtIn.as<char>( ), b->txtStart.as<u32>( ), lines, stat,
                        b->txtHdrName.as<u64>( ), b->txtBases.as<u32>( ) );
    MA_HIP( hipGetLastError( ) );
    if( scan_exclusive<u64>( b, b->txtHdrName.as<u64>( ), b->txtHdrName.as<u64>( ), lines + 1 ) ||
        scan_exclusive<u32>( b, b->txtBases.as<u32>( ), b->txtBases.as<u32>( ), lines + 1 ) )
        return 1;
    hipLaunchKernelGGL( k_text_rec_lines, lineGrid, lineBlock, 0, b->stream, lines, b->txtHdrName.as<u64>( ), b->txtRecLine.as<u32>( ) );
    hipLaunchKernelGGL( k_text_records, dim3( (unsigned)std::min<u64>( 256, ( lines + 255 ) / 256 ) ), lineBlock, 0, b->stream, kind, lines,
                        b->txtHdrName.as<u64>( ), b->txtBases.as<u32>( ), b->txtRecLine.as<u32>( ), stat );
    hipLaunchKernelGGL( k_text_stat, dim3( 1 ), dim3( 1 ), 0, b->stream, lines, b->txtHdrName.as<u64>( ), b->txtBases.as<u32>( ),
                        b->txtStart.as<u32>( ), b->max_reads, b->max_bases, stat );
    TextEmitArgs A;
    A.kind = kind;
    A.text = b->txtIn.as<char>( );
    A.n = n, A.lines = lines;
    A.start = b->txtStart.as<u32>( );
    A.hdrName = b->txtHdrName.as<u64>( );
    A.bases = b->txtBases.as<u32>( );
    A.stat = stat;
    A.roff = b->roff.as<u64>( );
    A.codes = b->reads.as<uint8_t>( );
    A.nameOff = b->txtNameOff.as<u64>( );
    A.names = b->txtNames.as<char>( );
    A.qual = kind == ma_text::KIND_FASTQ ? b->txtQual.as<uint8_t>( ) : nullptr;
    hipLaunchKernelGGL( k_text_emit, textGrid, textBlock, 0, b->stream, A );
    MA_HIP( hipGetLastError( ) );
    // read-back 2: reads, bases, name bytes, the longest read, the refusal
    MA_HIP( hipMemcpyAsync( h, stat, TXT_WORDS * 8, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    if( h[ TXT_VIOLATION ] != ma_text::NO_VIOLATION )
        return text_refuse( h[ TXT_VIOLATION ] >> 8, h[ TXT_BYTE ], (u32)( h[ TXT_VIOLATION ] & 0xffu ) );
    if( !h[ TXT_EMIT ] )
    {
        if( n_reads )
            *n_reads = h[ TXT_READS ]; // (what a caller sizes the next batch object by)
        return fail( "ma_batch_set_reads_text: batch capacity exceeded" );
    }
    b->n_reads = h[ TXT_READS ];
    b->n_bases = h[ TXT_BASES ];
    b->max_qlen = (u32)h[ TXT_MAX_LEN ];
    b->txtNameBytes = h[ TXT_NAME_BYTES ];
    b->txtHasQual = kind == ma_text::KIND_FASTQ;
    b->txtSet = true;
    if( n_reads )
        *n_reads = b->n_reads;
    return 0;
}

int ma_batch_read_counts( ma_batch* b, uint64_t* n_reads, uint64_t* n_bases, uint64_t* n_name_bytes, int32_t* has_qual )
{
    if( !b )
        return fail( "ma_batch_read_counts: null batch" );
    if( n_reads )
        *n_reads = b->d_roff ? b->n_reads : 0;
    if( n_bases )
        *n_bases = b->d_roff ? b->n_bases : 0;
    if( n_name_bytes )
        *n_name_bytes = b->txtSet ? b->txtNameBytes : 0;
    if( has_qual )
        *has_qual = b->txtSet && b->txtHasQual ? 1 : 0;
    return 0;
}

int ma_batch_get_reads( ma_batch* b, uint64_t* offsets, uint8_t* codes )
{
    if( !b || !b->d_roff )
        return fail( "ma_batch_get_reads: no reads set" );
    MA_BIND_DEVICE( b->device );
    if( offsets )
        MA_HIP( hipMemcpyAsync( offsets, b->d_roff, ( b->n_reads + 1 ) * 8, hipMemcpyDeviceToHost, b->stream ) );
    if( codes && b->n_bases )
        MA_HIP( hipMemcpyAsync( codes, b->d_reads, b->n_bases, hipMemcpyDeviceToHost, b->stream ) );
    return batch_wait( b );
}

int ma_batch_get_read_text( ma_batch* b, uint64_t* name_off, char* names, uint8_t* qual )
{
    if( !b || !b->d_roff || !b->txtSet )
        return fail( "ma_batch_get_read_text: the reads have no names (ma_batch_set_read_text or ma_batch_set_reads_text)" );
    if( qual && !b->txtHasQual )
        return fail( "ma_batch_get_read_text: the reads have no qualities" );
    MA_BIND_DEVICE( b->device );
    if( name_off )
        MA_HIP( hipMemcpyAsync( name_off, b->txtNameOff.p, ( b->n_reads + 1 ) * 8, hipMemcpyDeviceToHost, b->stream ) );
    if( names && b->txtNameBytes )
        MA_HIP( hipMemcpyAsync( names, b->txtNames.p, b->txtNameBytes, hipMemcpyDeviceToHost, b->stream ) );
    if( qual && b->n_bases )
        MA_HIP( hipMemcpyAsync( qual, b->txtQual.p, b->n_bases, hipMemcpyDeviceToHost, b->stream ) );
    return batch_wait( b );
}
} // extern "C"
