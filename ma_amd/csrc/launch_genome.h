// launch_genome.h -- ma_genome_*: a genome read from FASTA text on the device and turned into an index.  Textually part of
// pipeline.hip; the kernels are in stage_genome.h (and stage_text.h), the rules in ma_amd/host/ma_genome_dev.h.

struct ma_genome
{
    int device = 0;
    hipStream_t stream = nullptr;
    u64 max_bases = 0;
    ma_genome_dev::Genome g; // the contig table, the holes and what one chunk hands to the next (no codes: they are in `codes`)
    DevBuf codes; // 1 byte per base, max_bases + 64
    // scratch of a chunk: the text, the statistics (TXT_WORDS + GEN_WORDS), line feeds per workgroup, per line its start, header
    // flag | name bytes and bases (both scanned in place), per header its line, contig start, name offset and line | byte, the
    // names, the hole counts per workgroup and the holes
    DevBuf in, stat, block, start, hdrName, bases, recLine, cStart, cName, cLine, names, holeBlock, holeStart, holeEnd, cubTmp;
    DevBuf draws; // ma_genome_build_index
};

namespace
{
template <typename T, typename O> int genome_scan( ma_genome* G, const T* in, O* out, u64 n )
{
    size_t tb = 0;
    MA_HIP( hipcub::DeviceScan::ExclusiveSum( nullptr, tb, in, out, (int)n, G->stream ) );
    if( G->cubTmp.reserve( tb + 256 ) )
        return 1;
    MA_HIP( hipcub::DeviceScan::ExclusiveSum( G->cubTmp.p, tb, in, out, (int)n, G->stream ) );
    return 0;
}
int genome_refuse( u32 refusal, u64 line, u64 byte, u32 reason, u64 bases )
{
    return fail( ma_genome_dev::refusalText( refusal, line, byte, reason, bases ) );
}
} // namespace

extern "C" {

int ma_genome_create( int device, uint64_t max_bases, ma_genome** out )
{
    if( !out || max_bases == 0 )
        return fail( "ma_genome_create: null argument or no capacity" );
    if( device < 0 ) // the calling thread's current device
        MA_HIP( hipGetDevice( &device ) );
    MA_BIND_DEVICE( device );
    std::unique_ptr<ma_genome> G( new ma_genome( ) );
    G->device = device;
    G->max_bases = max_bases;
    if( G->codes.reserve( max_bases + 64 ) || G->stat.reserve( ( TXT_WORDS + GEN_WORDS ) * 8 ) )
        return 1;
    MA_HIP( hipStreamCreateWithFlags( &G->stream, hipStreamNonBlocking ) );
    *out = G.release( );
    return 0;
}

int ma_genome_destroy( ma_genome* G )
{
    if( !G )
        return 0;
    MA_BIND_DEVICE( G->device );
    if( G->stream )
    {
        (void)hipStreamSynchronize( G->stream );
        (void)hipStreamDestroy( G->stream );
    }
    delete G;
    return 0;
}

int ma_genome_append_text( ma_genome* G, const char* text, uint64_t n_bytes, int32_t end_of_file, uint64_t* consumed )
{
    if( consumed )
        *consumed = 0;
    if( !G || ( n_bytes && !text ) )
        return fail( "ma_genome_append_text: null argument" );
    MA_BIND_DEVICE( G->device );
    const ma_genome_dev::Genome& g = G->g;
    const bool eof = end_of_file != 0;
    uint64_t n;
    u32 reason;
    const u32 atStart = ma_genome_dev::refusalAtStart( g, text, n_bytes, eof, &n, &reason );
    if( atStart != ma_genome_dev::REFUSE_NONE )
        return genome_refuse( atStart, g.uiLines, g.uiBytes, reason, 0 );
    ma_genome_dev::Chunk c;
    c.bEndOfFile = eof;
    c.uiBytes = n;
    if( n == 0 ) // nothing to parse: a chunk without a line feed, or the bare end of a file
    {
        if( ma_genome_dev::openStaysEmpty( g, 0, false, eof ) )
            return genome_refuse( ma_genome_dev::REFUSE_LINE, g.uiOpenLine, g.uiOpenByte, ma_text::ERR_FA_NO_BASES, 0 );
        if( eof )
            ma_genome_dev::commit( G->g, c );
        return 0;
    }
    c.bStartsWithHeader = text[ 0 ] == '>';
    const u64 nBlocks = ( n + TEXT_BLOCK_BYTES - 1 ) / TEXT_BLOCK_BYTES;
    if( G->in.reserve( n + 64 ) || G->block.reserve( ( nBlocks + 1 ) * 4 ) || G->names.reserve( n + 1 ) )
        return 1;
    char* const dev = G->in.as<char>( );
    unsigned long long* const stat = G->stat.as<unsigned long long>( );
    unsigned long long h[ TXT_WORDS + GEN_WORDS ];
    MA_HIP( hipMemcpyAsync( dev, text, n, hipMemcpyHostToDevice, G->stream ) );
    MA_HIP( hipMemsetAsync( stat, 0, ( TXT_WORDS + GEN_WORDS ) * 8, G->stream ) );
    MA_HIP( hipMemsetAsync( stat + TXT_LONE_CR, 0xff, 2 * 8, G->stream ) ); // TXT_LONE_CR, TXT_VIOLATION: none
    const dim3 textGrid( (unsigned)nBlocks ), textBlock( TEXT_BLOCK );
    hipLaunchKernelGGL( k_text_count, textGrid, textBlock, 0, G->stream, dev, n, G->block.as<u32>( ), stat );
    MA_HIP( hipGetLastError( ) );
    // read-back 1: the number of lines sizes the per-line scratch and launches
    MA_HIP( hipMemcpyAsync( h, stat, 8, hipMemcpyDeviceToHost, G->stream ) );
    MA_HIP( hipStreamSynchronize( G->stream ) );
    const u64 feeds = h[ TXT_FEEDS ], lines = ma_text::nLines( feeds, text[ n - 1 ] );
    // holes are counted over the chunk's new codes, 16 per lane from the 16-byte boundary at or before the genome's end: never
    // more codes than the chunk has bytes
    const u64 holeBlocks = ( n + 16 + TEXT_BLOCK_BYTES - 1 ) / TEXT_BLOCK_BYTES;
    if( G->start.reserve( ( lines + 2 ) * 4 ) || G->hdrName.reserve( ( lines + 2 ) * 8 ) || G->bases.reserve( ( lines + 2 ) * 4 ) ||
        G->recLine.reserve( ( lines + 2 ) * 4 ) || G->cStart.reserve( ( lines + 2 ) * 8 ) || G->cName.reserve( ( lines + 2 ) * 8 ) ||
        G->cLine.reserve( ( lines + 2 ) * 8 ) || G->holeBlock.reserve( ( holeBlocks + 1 ) * 8 ) )
        return 1;
    if( genome_scan( G, G->block.as<u32>( ), G->block.as<u32>( ), nBlocks ) )
        return 1;
    hipLaunchKernelGGL( k_text_lines, textGrid, textBlock, 0, G->stream, dev, n, G->block.as<u32>( ), feeds, G->start.as<u32>( ) );
    const dim3 lineGrid( (unsigned)( ( lines + 1 + 255 ) / 256 ) ), lineBlock( 256 );
    hipLaunchKernelGGL( k_text_classify, lineGrid, lineBlock, 0, G->stream, (u32)ma_text::KIND_FASTA, dev, G->start.as<u32>( ), lines, stat,
                        G->hdrName.as<u64>( ), G->bases.as<u32>( ) );
    MA_HIP( hipGetLastError( ) );
    if( genome_scan( G, G->hdrName.as<u64>( ), G->hdrName.as<u64>( ), lines + 1 ) || genome_scan( G, G->bases.as<u32>( ), G->bases.as<u32>( ), lines + 1 ) )
        return 1;
    hipLaunchKernelGGL( k_text_rec_lines, lineGrid, lineBlock, 0, G->stream, lines, G->hdrName.as<u64>( ), G->recLine.as<u32>( ) );
    GenomeChunkArgs A;
    A.text = dev;
    A.n = n, A.lines = lines;
    A.start = G->start.as<u32>( );
    A.hdrName = G->hdrName.as<u64>( );
    A.bases = G->bases.as<u32>( );
    A.recLine = G->recLine.as<u32>( );
    A.stat = stat;
    A.genomeBases = g.uiBases, A.maxBases = G->max_bases;
    A.endOfFile = eof ? 1 : 0;
    A.codes = G->codes.as<uint8_t>( );
    A.names = G->names.as<char>( );
    A.cStart = G->cStart.as<u64>( );
    A.cName = G->cName.as<u64>( );
    A.cLine = G->cLine.as<u64>( );
    hipLaunchKernelGGL( k_genome_contigs, lineGrid, lineBlock, 0, G->stream, A ); // (never more headers than lines)
    hipLaunchKernelGGL( k_genome_stat, dim3( 1 ), dim3( 1 ), 0, G->stream, A );
    hipLaunchKernelGGL( k_genome_emit, textGrid, textBlock, 0, G->stream, A );
    GenomeHoleArgs H;
    H.codes = G->codes.as<uint8_t>( );
    H.stat = stat;
    H.from = g.uiBases;
    H.cStart = G->cStart.as<u64>( );
    H.blockCnt = G->holeBlock.as<u64>( );
    H.holeStart = H.holeEnd = nullptr;
    const dim3 holeGrid( (unsigned)holeBlocks );
    hipLaunchKernelGGL( k_genome_hole_count, holeGrid, textBlock, 0, G->stream, H );
    MA_HIP( hipGetLastError( ) );
    MA_HIP( hipMemsetAsync( H.blockCnt + holeBlocks, 0, 8, G->stream ) );
    if( genome_scan( G, H.blockCnt, H.blockCnt, holeBlocks + 1 ) )
        return 1;
    hipLaunchKernelGGL( k_genome_hole_stat, dim3( 1 ), dim3( 1 ), 0, G->stream, H.blockCnt, holeBlocks, stat );
    MA_HIP( hipGetLastError( ) );
    // read-back 2: the sums and the refusal
    MA_HIP( hipMemcpyAsync( h, stat, ( TXT_WORDS + GEN_WORDS ) * 8, hipMemcpyDeviceToHost, G->stream ) );
    MA_HIP( hipStreamSynchronize( G->stream ) );
    const unsigned long long* const s = h + TXT_WORDS;
    if( ma_genome_dev::openStaysEmpty( g, s[ GEN_FIRST_BASES ], s[ GEN_CONTIGS ] > 0, eof ) )
        return genome_refuse( ma_genome_dev::REFUSE_LINE, g.uiOpenLine, g.uiOpenByte, ma_text::ERR_FA_NO_BASES, 0 );
    if( h[ TXT_VIOLATION ] != ma_text::NO_VIOLATION )
        return genome_refuse( ma_genome_dev::REFUSE_LINE, g.uiLines + ( h[ TXT_VIOLATION ] >> 8 ), g.uiBytes + s[ GEN_BYTE ],
                              (u32)( h[ TXT_VIOLATION ] & 0xffu ), 0 );
    if( !s[ GEN_EMIT ] )
        return genome_refuse( ma_genome_dev::REFUSE_CAPACITY, 0, 0, 0, g.uiBases + s[ GEN_BASES ] );
    const u64 R = s[ GEN_CONTIGS ], holes = s[ GEN_HOLES ];
    c.uiLines = lines;
    c.uiBases = s[ GEN_BASES ];
    c.uiHoleBases = s[ GEN_HOLE_BASES ];
    if( holes )
    {
        if( G->holeStart.reserve( holes * 8 ) || G->holeEnd.reserve( holes * 8 ) )
            return 1;
        H.holeStart = G->holeStart.as<u64>( ), H.holeEnd = G->holeEnd.as<u64>( );
        hipLaunchKernelGGL( k_genome_hole_emit, holeGrid, textBlock, 0, G->stream, H );
        MA_HIP( hipGetLastError( ) );
    }
    // read-back 3: the chunk's contigs and holes
    std::vector<u64> cLine( R );
    c.vStarts.resize( R );
    c.vNameOff.resize( R + 1 );
    c.sNames.resize( s[ GEN_NAME_BYTES ] );
    c.vHoleStart.resize( holes );
    c.vHoleLen.resize( holes );
    MA_HIP( hipMemcpyAsync( c.vNameOff.data( ), A.cName, ( R + 1 ) * 8, hipMemcpyDeviceToHost, G->stream ) );
    if( R )
    {
        MA_HIP( hipMemcpyAsync( c.vStarts.data( ), A.cStart, R * 8, hipMemcpyDeviceToHost, G->stream ) );
        MA_HIP( hipMemcpyAsync( cLine.data( ), A.cLine, R * 8, hipMemcpyDeviceToHost, G->stream ) );
    }
    if( !c.sNames.empty( ) )
        MA_HIP( hipMemcpyAsync( &c.sNames[ 0 ], A.names, c.sNames.size( ), hipMemcpyDeviceToHost, G->stream ) );
    if( holes )
    {
        MA_HIP( hipMemcpyAsync( c.vHoleStart.data( ), H.holeStart, holes * 8, hipMemcpyDeviceToHost, G->stream ) );
        MA_HIP( hipMemcpyAsync( c.vHoleLen.data( ), H.holeEnd, holes * 8, hipMemcpyDeviceToHost, G->stream ) );
    }
    MA_HIP( hipStreamSynchronize( G->stream ) );
    for( u64 i = 0; i < holes; i++ )
        c.vHoleLen[ i ] -= c.vHoleStart[ i ]; // (end -> length)
    c.vHdrLine.resize( R );
    c.vHdrByte.resize( R );
    for( u64 i = 0; i < R; i++ )
        c.vHdrLine[ i ] = cLine[ i ] >> 32, c.vHdrByte[ i ] = cLine[ i ] & 0xffffffffull;
    ma_genome_dev::commit( G->g, c );
    if( consumed )
        *consumed = n;
    return 0;
}

int ma_genome_counts( const ma_genome* G, uint64_t* n_contigs, uint64_t* n_bases, uint64_t* n_name_bytes, uint64_t* n_holes, uint64_t* n_hole_bases )
{
    if( !G )
        return fail( "ma_genome_counts: null genome" );
    if( n_contigs )
        *n_contigs = G->g.vStarts.size( );
    if( n_bases )
        *n_bases = G->g.uiBases;
    if( n_name_bytes )
        *n_name_bytes = G->g.sNames.size( );
    if( n_holes )
        *n_holes = G->g.vHoleStart.size( );
    if( n_hole_bases )
        *n_hole_bases = G->g.uiHoleBases;
    return 0;
}

int ma_genome_get_contigs( const ma_genome* G, uint64_t* name_off, char* names, uint64_t* starts, uint64_t* lens, uint64_t* n_holes )
{
    if( !G )
        return fail( "ma_genome_get_contigs: null genome" );
    const ma_genome_dev::Genome& g = G->g;
    const size_t nc = g.vStarts.size( );
    if( name_off )
        memcpy( name_off, g.vNameOff.data( ), ( nc + 1 ) * 8 );
    if( names && !g.sNames.empty( ) )
        memcpy( names, g.sNames.data( ), g.sNames.size( ) );
    if( starts && nc )
        memcpy( starts, g.vStarts.data( ), nc * 8 );
    if( lens && nc )
        memcpy( lens, g.vLens.data( ), nc * 8 );
    if( n_holes && nc )
        memcpy( n_holes, g.vNumHoles.data( ), nc * 8 );
    return 0;
}

int ma_genome_get_holes( const ma_genome* G, uint64_t* start, uint64_t* len )
{
    if( !G )
        return fail( "ma_genome_get_holes: null genome" );
    const size_t nh = G->g.vHoleStart.size( );
    if( start && nh )
        memcpy( start, G->g.vHoleStart.data( ), nh * 8 );
    if( len && nh )
        memcpy( len, G->g.vHoleLen.data( ), nh * 8 );
    return 0;
}

int ma_genome_get_codes( const ma_genome* G, uint64_t from, uint64_t n, uint8_t* codes )
{
    if( !G || ( n && !codes ) )
        return fail( "ma_genome_get_codes: null argument" );
    if( from > G->g.uiBases || n > G->g.uiBases - from )
        return fail( "ma_genome_get_codes: the range is not inside the genome" );
    if( n == 0 )
        return 0;
    MA_BIND_DEVICE( G->device );
    MA_HIP( hipMemcpyAsync( codes, G->codes.as<uint8_t>( ) + from, n, hipMemcpyDeviceToHost, G->stream ) );
    MA_HIP( hipStreamSynchronize( G->stream ) );
    return 0;
}

int ma_genome_build_index( ma_genome* G, uint32_t srand_seed, ma_index** out )
{
    if( !G || !out )
        return fail( "ma_genome_build_index: null argument" );
    ma_genome_dev::Genome& g = G->g;
    if( const char* why = ma_genome_dev::buildRefusal( g ) )
        return fail( why );
    if( g.vStarts.size( ) > 0x7fffffffull )
        return fail( "ma_genome_build_index: more contigs than an index holds" );
    MA_BIND_DEVICE( G->device );
    if( g.uiHoleBases )
    {
        // the draws are made here and uploaded packed; a kernel places them by the rank of each hole base
        const std::vector<uint8_t> draws = ma_genome_dev::packedDraws( srand_seed, g.uiHoleBases );
        const u64 n = g.uiBases, nBlocks = ( n + TEXT_BLOCK_BYTES - 1 ) / TEXT_BLOCK_BYTES;
        if( G->draws.reserve( draws.size( ) ) || G->holeBlock.reserve( ( nBlocks + 1 ) * 8 ) )
            return 1;
        MA_HIP( hipMemcpyAsync( G->draws.p, draws.data( ), draws.size( ), hipMemcpyHostToDevice, G->stream ) );
        const dim3 grid( (unsigned)nBlocks ), block( TEXT_BLOCK );
        hipLaunchKernelGGL( k_genome_fill_count, grid, block, 0, G->stream, G->codes.as<uint8_t>( ), n, G->holeBlock.as<u64>( ) );
        MA_HIP( hipGetLastError( ) );
        if( genome_scan( G, G->holeBlock.as<u64>( ), G->holeBlock.as<u64>( ), nBlocks ) )
            return 1;
        hipLaunchKernelGGL( k_genome_fill, grid, block, 0, G->stream, G->codes.as<uint8_t>( ), n, G->holeBlock.as<u64>( ), G->draws.as<uint8_t>( ) );
        MA_HIP( hipGetLastError( ) );
        MA_HIP( hipStreamSynchronize( G->stream ) ); // (the draws leave scope; the index is built on the default stream)
        G->draws.release( );
    }
    g.bBuilt = true; // filled: a second call would find no hole bases to place its draws in (so a build that fails below is not retried)
    for( DevBuf* d : { &G->in, &G->start, &G->hdrName, &G->bases, &G->recLine, &G->cStart, &G->cName, &G->cLine, &G->names, &G->holeStart, &G->holeEnd } )
        d->release( ); // the sort wants the memory
    ma_index* x = nullptr;
    if( ma_index_build_device( (int32_t)g.vStarts.size( ), g.vLens.data( ), G->codes.p, &x ) )
        return 1;
    if( ma_index_set_contig_names( x, g.sNames.data( ), g.vNameOff.data( ) ) ||
        ma_index_set_holes( x, g.vHoleStart.data( ), g.vHoleLen.data( ), g.vHoleStart.size( ) ) )
    {
        ma_index_destroy( x );
        return 1;
    }
    *out = x;
    return 0;
}
} // extern "C"
