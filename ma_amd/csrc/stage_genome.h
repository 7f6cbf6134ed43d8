// stage_genome.h -- the genome's FASTA text parsed on the device (ma_genome_append_text, ma_genome_build_index): what FileReader
// and the base loop of buildIndex (ma_amd/host/ma_modules.h; Pack::vAppendSequence, pack.h:586-698) make of a chunk of whole
// lines, byte-parallel.  The rules are ma_amd/host/ma_genome_dev.h and ma_text_dev.h, the code the CPU tests pin to the yardstick;
// the kernels only spread them over lanes.  Textually part of pipeline.hip, behind stage_text.h: k_text_count, k_text_lines,
// k_text_classify and k_text_rec_lines run on a chunk as they are.
//   k_genome_contigs      one lane per header line of the chunk: its contig's start in the genome, its name's place, its line and
//                         byte; the rule "a record has bases"
//   k_genome_stat         one lane: the sums, the refusal's byte offset, the open contig that stays empty, whether anything may
//                         be written
//   k_genome_emit         16 bytes per lane, 4 096 per workgroup: every base byte to its place in the genome's codes (hole bases
//                         as 4), every name byte to the chunk's names
//   k_genome_hole_count   16 codes per lane over the chunk's new codes: run starts, run ends and hole bases per workgroup
//   k_genome_hole_stat    one lane: the chunk's number of holes behind the scan of the workgroups' counts
//   k_genome_hole_emit    the same walk behind that scan: hole k's start and end
//   k_genome_fill_count / k_genome_fill   (ma_genome_build_index) hole bases per workgroup; behind the scan every hole base
//                         becomes the draw of its rank
// A lane holds its 16 bytes in four words (TextChunk); no arrays indexed at run time; plain stores.  The kernels talk to each
// other across launches only.

enum : int // the statistics block of a chunk (u64 words) behind the TXT_WORDS of the text kernels
{
    GEN_CONTIGS = 0, // header lines of the chunk
    GEN_BASES = 1, // bases of the chunk
    GEN_NAME_BYTES = 2,
    GEN_FIRST_BASES = 3, // bases before the chunk's first header
    GEN_BYTE = 4, // offset of the refused line in the chunk
    GEN_EMIT = 5, // 1: accepted and within the capacity, k_genome_emit and the hole kernels write
    GEN_HOLES = 6,
    GEN_HOLE_BASES = 7,
    GEN_WORDS = 8
};

struct GenomeChunkArgs
{
    const char* text;
    u64 n, lines;
    const u32* start;
    const u64* hdrName; // the scans
    const u32* bases;
    const u32* recLine;
    unsigned long long* stat; // TXT_WORDS + GEN_WORDS
    u64 genomeBases, maxBases; // the genome before the chunk, its capacity
    u32 endOfFile;
    uint8_t* codes; // of the whole genome
    char* names; // of the chunk
    u64* cStart; // per header line of the chunk: the contig's start in the genome (one more entry: the genome's end),
    u64* cName; //                               its name's offset in `names` (one more entry: the name bytes),
    u64* cLine; //                               its line << 32 | the line's byte offset
};

// contigs + 1 lanes
__global__ __launch_bounds__( 256 ) void k_genome_contigs( GenomeChunkArgs A )
{
    const u64 R = A.hdrName[ A.lines ] >> 32;
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 key = ma_text::NO_VIOLATION;
    if( r < R )
    {
        const u32 line = A.recLine[ r ];
        const u32 from = A.bases[ line ], to = A.bases[ r + 1 < R ? A.recLine[ r + 1 ] : A.lines ];
        A.cStart[ r ] = A.genomeBases + from;
        A.cName[ r ] = A.hdrName[ line ] & 0xffffffffull;
        A.cLine[ r ] = ( (u64)line << 32 ) | A.start[ line ];
        if( r + 1 < R || A.endOfFile ) // (a header that ends a chunk waits for the next one)
            key = ma_text::recordKey( line, from, to );
    }
    else if( r == R )
    {
        A.cStart[ r ] = A.genomeBases + A.bases[ A.lines ];
        A.cName[ r ] = A.hdrName[ A.lines ] & 0xffffffffull;
        A.cLine[ r ] = 0;
    }
    key = wave_min_u64( key );
    if( ( threadIdx.x & 63 ) == 0 && key != ma_text::NO_VIOLATION )
        atomicMin( A.stat + TXT_VIOLATION, (unsigned long long)key );
}

__global__ void k_genome_stat( GenomeChunkArgs A )
{
    unsigned long long* const g = A.stat + TXT_WORDS;
    const u64 R = A.hdrName[ A.lines ] >> 32, B = A.bases[ A.lines ], key = A.stat[ TXT_VIOLATION ];
    g[ GEN_CONTIGS ] = R;
    g[ GEN_BASES ] = B;
    g[ GEN_NAME_BYTES ] = A.hdrName[ A.lines ] & 0xffffffffull;
    g[ GEN_FIRST_BASES ] = R ? A.bases[ A.recLine[ 0 ] ] : B;
    g[ GEN_BYTE ] = key != ma_text::NO_VIOLATION ? A.start[ key >> 8 ] : 0;
    g[ GEN_EMIT ] = key == ma_text::NO_VIOLATION && A.genomeBases + B <= A.maxBases ? 1 : 0;
}

__global__ __launch_bounds__( TEXT_BLOCK ) void k_genome_emit( GenomeChunkArgs A )
{
    if( !A.stat[ TXT_WORDS + GEN_EMIT ] )
        return; // refused, or more than the genome holds: nothing is written
    const u64 base = ( (u64)blockIdx.x * TEXT_BLOCK + threadIdx.x ) * TEXT_LANE_BYTES;
    if( base >= A.n )
        return;
    // the line of the lane's first byte: the last one that starts at or before it
    u64 lo = 0, hi = A.lines - 1;
    while( lo < hi )
    {
        const u64 mid = ( lo + hi + 1 ) >> 1;
        if( A.start[ mid ] <= base )
            lo = mid;
        else
            hi = mid - 1;
    }
    u64 line = lo;
    u32 from = 0, to = 0, dstBase = 0, dstName = 0; // of `line`, loaded when the walk enters it
    ma_text::Line x;
    bool loaded = false;
    const TextChunk c = text_chunk( A.text, A.n, base );
    text_each( c, [ & ]( int k, u32 b ) {
        const u64 pos = base + k;
        if( pos >= A.n )
            return;
        if( loaded && pos >= to )
            line++, loaded = false;
        if( !loaded )
        {
            from = A.start[ line ], to = A.start[ line + 1 ];
            const u64 h0 = A.hdrName[ line ], h1 = A.hdrName[ line + 1 ];
            dstBase = A.bases[ line ];
            dstName = (u32)h0;
            x.uiLen = ma_text::content( A.text, from, to );
            x.uiBases = A.bases[ line + 1 ] - dstBase;
            x.uiName = (u32)h1 - (u32)h0;
            x.uiKind = ( h1 >> 32 ) != ( h0 >> 32 ) ? ma_text::LINE_HEADER : ma_text::LINE_BASES;
            x.uiReason = ma_text::OK;
            loaded = true;
        }
        u32 j;
        const u32 t = ma_text::byteTarget( x, (u32)( pos - from ), &j );
        if( t == ma_text::TO_CODES )
            A.codes[ A.genomeBases + dstBase + j ] = ma_text::code( (uint8_t)b ); // (a hole base: ma_genome_dev::HOLE)
        else if( t == ma_text::TO_NAMES )
            A.names[ (u64)dstName + j ] = (char)b;
    } );
}

// ---- holes ------------------------------------------------------------------------------------------------------------------
// The chunk's codes are [ from, to ) of the genome's; lane g of the grid holds the 16 codes at ( from & ~15 ) + 16 g, those
// outside [ from, to ) masked, so that the loads are aligned whatever `from` is.  The chunk is looked at ALONE: a run that the
// chunk's first base continues is joined on the host (ma_genome_dev::commit).
struct GenomeHoleArgs
{
    const uint8_t* codes;
    unsigned long long* stat; // TXT_WORDS + GEN_WORDS: reads GEN_EMIT, GEN_BASES, GEN_CONTIGS; k_genome_hole_count adds to GEN_HOLE_BASES
    u64 from;
    const u64* cStart; // the chunk's new contigs' starts, ascending
    u64* blockCnt; // per workgroup: run starts << 32 | run ends (one more entry; scanned in place)
    u64* holeStart; // k_genome_hole_emit
    u64* holeEnd;
};
struct GenomeHoleLane
{
    u32 hole; // bit k: code k is a hole base of the chunk
    ma_genome_dev::HoleMasks m;
};
__device__ __forceinline__ u32 hole_bits( const TextChunk& c )
{
    u32 hole = 0;
    text_each( c, [ & ]( int k, u32 b ) { hole |= ( ma_genome_dev::isHole( (uint8_t)b ) ? 1u : 0u ) << k; } );
    return hole;
}
__device__ __forceinline__ GenomeHoleLane genome_hole_lane( const GenomeHoleArgs& A, u64 base, u64 to )
{
    GenomeHoleLane L{ 0, { 0, 0 } };
    if( base >= to )
        return L;
    // bits of the 16 positions that lie in [ from, to ) (a position behind `to` reads as 0 in text_chunk: code A, no hole base)
    const u32 inside = base >= A.from ? 0xffffu : ( 0xffffu << (u32)( A.from - base ) ) & 0xffffu;
    L.hole = hole_bits( text_chunk( (const char*)A.codes, to, base ) ) & inside;
    const bool prev = base > A.from && ma_genome_dev::isHole( A.codes[ base - 1 ] );
    const bool next = base + 16 < to && ma_genome_dev::isHole( A.codes[ base + 16 ] );
    // contigs that start at base .. base + 16: the first one at or behind base
    u32 first = 0;
    const u64 R = A.stat[ TXT_WORDS + GEN_CONTIGS ];
    u64 lo = 0, hi = R;
    while( lo < hi )
    {
        const u64 mid = ( lo + hi ) >> 1;
        if( A.cStart[ mid ] < base )
            lo = mid + 1;
        else
            hi = mid;
    }
    for( u64 i = lo; i < R; i++ )
    {
        const u64 s = A.cStart[ i ];
        if( s > base + 16 )
            break;
        first |= 1u << (u32)( s - base );
    }
    L.m = ma_genome_dev::holeMasks( L.hole, prev, next, first );
    return L;
}

__global__ __launch_bounds__( TEXT_BLOCK ) void k_genome_hole_count( GenomeHoleArgs A )
{
    typedef hipcub::BlockReduce<u64, TEXT_BLOCK> Reduce;
    __shared__ typename Reduce::TempStorage tmp;
    u64 cnt = 0;
    u32 holeBases = 0;
    if( A.stat[ TXT_WORDS + GEN_EMIT ] )
    {
        const u64 to = A.from + A.stat[ TXT_WORDS + GEN_BASES ];
        const u64 base = ( A.from & ~15ull ) + ( (u64)blockIdx.x * TEXT_BLOCK + threadIdx.x ) * TEXT_LANE_BYTES;
        const GenomeHoleLane L = genome_hole_lane( A, base, to );
        cnt = ( (u64)__popc( L.m.uiStarts ) << 32 ) | (u64)__popc( L.m.uiEnds );
        holeBases = (u32)__popc( L.hole );
    }
    for( int m = 32; m; m >>= 1 )
        holeBases += (u32)__shfl_xor( (int)holeBases, m, 64 );
    if( ( threadIdx.x & 63 ) == 0 && holeBases )
        atomicAdd( A.stat + TXT_WORDS + GEN_HOLE_BASES, (unsigned long long)holeBases );
    const u64 sum = Reduce( tmp ).Sum( cnt );
    if( threadIdx.x == 0 )
        A.blockCnt[ blockIdx.x ] = sum;
}

// blockCnt: the exclusive sums over blocks + 1 entries
__global__ void k_genome_hole_stat( const u64* blockCnt, u64 blocks, unsigned long long* stat )
{
    stat[ TXT_WORDS + GEN_HOLES ] = blockCnt[ blocks ] >> 32; // (as many ends as starts)
}

__global__ __launch_bounds__( TEXT_BLOCK ) void k_genome_hole_emit( GenomeHoleArgs A )
{
    typedef hipcub::BlockScan<u64, TEXT_BLOCK> Scan;
    __shared__ typename Scan::TempStorage tmp;
    const u64 to = A.from + A.stat[ TXT_WORDS + GEN_BASES ];
    const u64 base = ( A.from & ~15ull ) + ( (u64)blockIdx.x * TEXT_BLOCK + threadIdx.x ) * TEXT_LANE_BYTES;
    const GenomeHoleLane L = genome_hole_lane( A, base, to );
    u64 at = 0;
    Scan( tmp ).ExclusiveSum( ( (u64)__popc( L.m.uiStarts ) << 32 ) | (u64)__popc( L.m.uiEnds ), at );
    at += A.blockCnt[ blockIdx.x ];
    u64 s = at >> 32, e = at & 0xffffffffull;
    u32 starts = L.m.uiStarts, ends = L.m.uiEnds;
    while( starts )
    {
        const u32 k = (u32)( __ffs( (int)starts ) - 1 );
        starts &= starts - 1;
        A.holeStart[ s++ ] = base + k; // the s-th run start of the chunk: k_genome_hole_count counted the same masks
    }
    while( ends )
    {
        const u32 k = (u32)( __ffs( (int)ends ) - 1 );
        ends &= ends - 1;
        A.holeEnd[ e++ ] = base + k + 1;
    }
}

// ---- the fill (ma_genome_build_index) ---------------------------------------------------------------------------------------------
// codes: n bytes, 256-byte aligned with at least 16 bytes of slack behind them
__global__ __launch_bounds__( TEXT_BLOCK ) void k_genome_fill_count( const uint8_t* codes, u64 n, u64* blockCnt )
{
    typedef hipcub::BlockReduce<u64, TEXT_BLOCK> Reduce;
    __shared__ typename Reduce::TempStorage tmp;
    const u64 base = ( (u64)blockIdx.x * TEXT_BLOCK + threadIdx.x ) * TEXT_LANE_BYTES;
    const u64 cnt = base < n ? (u64)__popc( hole_bits( text_chunk( (const char*)codes, n, base ) ) ) : 0u;
    const u64 sum = Reduce( tmp ).Sum( cnt );
    if( threadIdx.x == 0 )
        blockCnt[ blockIdx.x ] = sum;
}

// blockOff: exclusive sums of the counts; draws: ma_genome_dev::packedDraws of as many draws as the codes have hole bases
__global__ __launch_bounds__( TEXT_BLOCK ) void k_genome_fill( uint8_t* codes, u64 n, const u64* blockOff, const uint8_t* draws )
{
    typedef hipcub::BlockScan<u32, TEXT_BLOCK> Scan;
    __shared__ typename Scan::TempStorage tmp;
    const u64 base = ( (u64)blockIdx.x * TEXT_BLOCK + threadIdx.x ) * TEXT_LANE_BYTES;
    TextChunk c{ 0, 0, 0, 0 };
    if( base < n )
        c = text_chunk( (const char*)codes, n, base );
    const u32 hole = base < n ? hole_bits( c ) : 0u;
    u32 at = 0;
    Scan( tmp ).ExclusiveSum( (u32)__popc( hole ), at );
    if( !hole )
        return;
    u64 rank = blockOff[ blockIdx.x ] + at; // hole bases before this lane's
    u32 w0 = c.w0, w1 = c.w1, w2 = c.w2, w3 = c.w3;
    text_each( c, [ & ]( int k, u32 b ) {
        if( !( ( hole >> k ) & 1u ) )
            return;
        const u32 d = ma_genome_dev::drawOf( draws, rank++ ); // the rank-th hole base of the genome
        const u32 put = ( d ^ ( b & 0xffu ) ) << ( 8 * ( k & 3 ) ); // xor turns the byte into d
        if( k < 4 )
            w0 ^= put;
        else if( k < 8 )
            w1 ^= put;
        else if( k < 12 )
            w2 ^= put;
        else
            w3 ^= put;
    } );
    // (the 16 bytes lie inside the buffer's slack even where the genome ends inside them; those bytes read as 0 and stay 0)
    *reinterpret_cast<uint4*>( codes + base ) = make_uint4( w0, w1, w2, w3 );
}
