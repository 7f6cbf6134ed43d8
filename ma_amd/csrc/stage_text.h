// stage_text.h -- FASTQ / FASTA text parsed on the device (ma_batch_set_reads_text): what FileReader (ma_amd/host/ma_sam.h, the
// yardstick; fileReader.cpp:37-203) makes of a text in the strict form, for a whole batch, byte-parallel.  The rules -- character
// classes, what a line is and contributes, what is refused -- are the functions of ma_amd/host/ma_text_dev.h, the code the CPU
// tests pin to the yardstick; the kernels only spread them over lanes.  Textually part of pipeline.hip.
//   k_text_count      16 bytes per lane, 4 096 per workgroup: line feeds per workgroup and in all, the first lone '\r'
//   k_text_lines      the same walk behind a scan of the workgroups' counts: the line starts
//   k_text_classify   one lane per line: ma_text::lineOf -> header flag | name bytes, bases, the lowest violation
//   k_text_rec_lines  (behind the scans of both) record r's header line
//   k_text_records    records strided over a fixed grid: the FASTA rule "a record has bases", the longest read
//   k_text_stat       one lane: the sums, the refusal's byte offset, whether anything may be written
//   k_text_emit       16 bytes per lane again: every byte to the codes, the qualities or the names; the two offset arrays
// A long read is one long line: nothing here walks a line's bytes in one lane but the trimming of trailing junk and the search
// for the name's end, which real files end after one and a few dozen steps.  Reductions issue one atomic per wavefront (see
// k_max_qlen).  No arrays indexed at run time.  The kernels of ma_batch_set_mates_text (two texts interleaved into mate pairs)
// are at the end of the file.

enum : int // the statistics block of a parse (u64 words)
{
    TXT_FEEDS = 0, // line feeds of the text
    TXT_LONE_CR = 1, // position of the first lone '\r' (all ones: none)
    TXT_VIOLATION = 2, // lowest ma_text::key( line, reason ) (all ones: none)
    TXT_MAX_LEN = 3, // longest read
    TXT_READS = 4,
    TXT_BASES = 5,
    TXT_NAME_BYTES = 6,
    TXT_BYTE = 7, // offset of the refused line
    TXT_EMIT = 8, // 1: accepted and within the batch's capacity, k_text_emit writes
    TXT_WORDS = 16
};
static constexpr u32 TEXT_LANE_BYTES = 16, TEXT_BLOCK = 256, TEXT_BLOCK_BYTES = TEXT_LANE_BYTES * TEXT_BLOCK;

// the 16 bytes of a lane as four words; bytes beyond the text read as 0.  (The text buffer is 256-byte aligned.)
struct TextChunk
{
    u32 w0, w1, w2, w3;
    template <int K> __device__ __forceinline__ u32 byte( ) const
    {
        const u32 w = K < 4 ? w0 : K < 8 ? w1 : K < 12 ? w2 : w3;
        return ( w >> ( 8 * ( K & 3 ) ) ) & 0xffu;
    }
};
__device__ __forceinline__ TextChunk text_chunk( const char* text, u64 n, u64 base )
{
    TextChunk c{ 0, 0, 0, 0 };
    if( base + TEXT_LANE_BYTES <= n )
    {
        const uint4 v = *reinterpret_cast<const uint4*>( text + base );
        c.w0 = v.x, c.w1 = v.y, c.w2 = v.z, c.w3 = v.w;
    }
    else
    {
#pragma unroll
        for( int k = 0; k < 16; k++ )
        {
            const u32 x = base + k < n ? (u32)(uint8_t)text[ base + k ] << ( 8 * ( k & 3 ) ) : 0u;
            if( k < 4 )
                c.w0 |= x;
            else if( k < 8 )
                c.w1 |= x;
            else if( k < 12 )
                c.w2 |= x;
            else
                c.w3 |= x;
        }
    }
    return c;
}
// calls f( k, byte ) for the 16 bytes of a chunk
template <int K = 0, typename F> __device__ __forceinline__ void text_each( const TextChunk& c, F&& f )
{
    if constexpr( K < 16 )
    {
        f( K, c.byte<K>( ) );
        text_each<K + 1>( c, f );
    }
}
__device__ __forceinline__ u64 wave_min_u64( u64 v )
{
    for( int m = 32; m; m >>= 1 )
    {
        const u64 o = ( (u64)(u32)__shfl_xor( (int)( v >> 32 ), m, 64 ) << 32 ) | (u32)__shfl_xor( (int)(u32)v, m, 64 );
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__( TEXT_BLOCK ) void k_text_count( const char* text, u64 n, u32* blockCnt, unsigned long long* stat )
{
    __shared__ u32 sCnt[ TEXT_BLOCK / 64 ];
    const u64 base = ( (u64)blockIdx.x * TEXT_BLOCK + threadIdx.x ) * TEXT_LANE_BYTES;
    u32 cnt = 0;
    u64 cr = ~0ull;
    if( base < n )
    {
        const TextChunk c = text_chunk( text, n, base );
        const u32 next = base + TEXT_LANE_BYTES < n ? (u32)(uint8_t)text[ base + TEXT_LANE_BYTES ] : 0u;
        u32 feeds = 0, returns = 0; // bit k: byte k is '\n' / '\r'
        text_each( c, [ & ]( int k, u32 b ) {
            feeds |= ( b == '\n' ? 1u : 0u ) << k;
            returns |= ( b == '\r' ? 1u : 0u ) << k;
        } );
        feeds |= ( next == '\n' ? 1u : 0u ) << 16;
        cnt = (u32)__popc( feeds & 0xffffu );
        // (a byte beyond the text reads as 0, never as '\r': a '\r' found lies inside, and the text's end follows it like any other byte)
        const u32 lone = returns & ~( feeds >> 1 );
        if( lone )
            cr = base + (u32)( __ffs( (int)lone ) - 1 );
    }
    cr = wave_min_u64( cr );
    for( int m = 32; m; m >>= 1 )
        cnt += (u32)__shfl_xor( (int)cnt, m, 64 );
    if( ( threadIdx.x & 63 ) == 0 )
    {
        sCnt[ threadIdx.x >> 6 ] = cnt;
        if( cr != ~0ull )
            atomicMin( stat + TXT_LONE_CR, (unsigned long long)cr );
    }
    __syncthreads( );
    if( threadIdx.x == 0 )
    {
        u32 s = 0;
        for( u32 w = 0; w < TEXT_BLOCK / 64; w++ )
            s += sCnt[ w ];
        blockCnt[ blockIdx.x ] = s;
        if( s )
            atomicAdd( stat + TXT_FEEDS, (unsigned long long)s );
    }
}

// blockOff: exclusive sums of k_text_count's blockCnt; start: feeds + 2 words
__global__ __launch_bounds__( TEXT_BLOCK ) void k_text_lines( const char* text, u64 n, const u32* blockOff, u64 feeds, u32* start )
{
    typedef hipcub::BlockScan<u32, TEXT_BLOCK> Scan;
    __shared__ typename Scan::TempStorage tmp;
    const u64 base = ( (u64)blockIdx.x * TEXT_BLOCK + threadIdx.x ) * TEXT_LANE_BYTES;
    u32 mask = 0;
    if( base < n )
        text_each( text_chunk( text, n, base ), [ & ]( int k, u32 b ) { mask |= ( b == '\n' ? 1u : 0u ) << k; } );
    u32 at = 0;
    Scan( tmp ).ExclusiveSum( (u32)__popc( mask ), at );
    u64 line = (u64)blockOff[ blockIdx.x ] + at; // line feeds before this lane's bytes
    while( mask )
    {
        const u32 k = (u32)( __ffs( (int)mask ) - 1 );
        mask &= mask - 1;
        line++;
        if( line <= feeds ) // (always: it is the line-th feed of the text)
            start[ line ] = (u32)( base + k + 1 );
    }
    if( blockIdx.x == 0 && threadIdx.x == 0 )
    {
        start[ 0 ] = 0;
        if( text[ n - 1 ] != '\n' )
            start[ feeds + 1 ] = (u32)n;
    }
}

// one lane per line, and one more for the entry behind the last line: hdrName[ i ] = header flag << 32 | name bytes, bases[ i ]
__global__ __launch_bounds__( 256 ) void k_text_classify( u32 kind, const char* text, const u32* start, u64 lines, unsigned long long* stat,
                                                          u64* hdrName, u32* bases )
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 key = ma_text::NO_VIOLATION;
    if( i < lines )
    {
        const ma_text::Line x = ma_text::lineOf( kind, text, start, i, lines, stat[ TXT_LONE_CR ] );
        hdrName[ i ] = ( (u64)( x.uiKind == ma_text::LINE_HEADER ? 1 : 0 ) << 32 ) | x.uiName;
        bases[ i ] = x.uiBases;
        if( x.uiReason != ma_text::OK )
            key = ma_text::key( i, x.uiReason );
    }
    else if( i == lines )
    {
        hdrName[ i ] = 0;
        bases[ i ] = 0;
    }
    key = wave_min_u64( key );
    if( ( threadIdx.x & 63 ) == 0 && key != ma_text::NO_VIOLATION )
        atomicMin( stat + TXT_VIOLATION, (unsigned long long)key );
}

// hdrName: exclusive sums over lines + 1 entries: headers before line i << 32 | name bytes before it
__global__ __launch_bounds__( 256 ) void k_text_rec_lines( u64 lines, const u64* hdrName, u32* recLine )
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if( i < lines && ( hdrName[ i + 1 ] >> 32 ) != ( hdrName[ i ] >> 32 ) )
        recLine[ hdrName[ i ] >> 32 ] = (u32)i;
}

__global__ __launch_bounds__( 256 ) void k_text_records( u32 kind, u64 lines, const u64* hdrName, const u32* bases, const u32* recLine,
                                                         unsigned long long* stat )
{
    const u64 R = hdrName[ lines ] >> 32;
    u32 longest = 0;
    u64 key = ma_text::NO_VIOLATION;
    for( u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (u64)gridDim.x * blockDim.x )
    {
        const u32 line = recLine[ r ];
        const u32 from = bases[ line ], to = bases[ r + 1 < R ? recLine[ r + 1 ] : lines ];
        longest = max( longest, to - from );
        if( kind == ma_text::KIND_FASTA )
        {
            const u64 k = ma_text::recordKey( line, from, to );
            key = k < key ? k : key;
        }
    }
    key = wave_min_u64( key );
    for( int m = 32; m; m >>= 1 )
        longest = max( longest, (u32)__shfl_xor( (int)longest, m, 64 ) );
    if( ( threadIdx.x & 63 ) == 0 )
    {
        if( longest )
            atomicMax( stat + TXT_MAX_LEN, (unsigned long long)longest );
        if( key != ma_text::NO_VIOLATION )
            atomicMin( stat + TXT_VIOLATION, (unsigned long long)key );
    }
}

__global__ void k_text_stat( u64 lines, const u64* hdrName, const u32* bases, const u32* start, u64 max_reads, u64 max_bases,
                             unsigned long long* stat )
{
    const u64 R = hdrName[ lines ] >> 32, B = bases[ lines ], key = stat[ TXT_VIOLATION ];
    stat[ TXT_READS ] = R;
    stat[ TXT_BASES ] = B;
    stat[ TXT_NAME_BYTES ] = hdrName[ lines ] & 0xffffffffull;
    stat[ TXT_BYTE ] = key != ma_text::NO_VIOLATION ? start[ key >> 8 ] : 0;
    stat[ TXT_EMIT ] = key == ma_text::NO_VIOLATION && R <= max_reads && B <= max_bases ? 1 : 0;
}

struct TextEmitArgs
{
    u32 kind;
    const char* text;
    u64 n, lines;
    const u32* start;
    const u64* hdrName; // the scans
    const u32* bases;
    const unsigned long long* stat;
    u64* roff;
    uint8_t* codes;
    u64* nameOff;
    char* names;
    uint8_t* qual; // FASTQ
};
__global__ __launch_bounds__( TEXT_BLOCK ) void k_text_emit( TextEmitArgs A )
{
    if( !A.stat[ TXT_EMIT ] )
        return; // refused, or more than the batch holds: nothing is written
    const u64 base = ( (u64)blockIdx.x * TEXT_BLOCK + threadIdx.x ) * TEXT_LANE_BYTES;
    if( base >= A.n )
        return;
    if( base == 0 )
    {
        A.roff[ A.hdrName[ A.lines ] >> 32 ] = A.bases[ A.lines ];
        A.nameOff[ A.hdrName[ A.lines ] >> 32 ] = A.hdrName[ A.lines ] & 0xffffffffull;
    }
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
    u32 from = 0, to = 0, dstBase = 0, dstName = 0, dstQual = 0; // of `line`, loaded when the walk enters it
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
            x.uiKind = A.kind == ma_text::KIND_FASTQ ? (u32)( line & 3u ) : ( h1 >> 32 ) != ( h0 >> 32 ) ? ma_text::LINE_HEADER : ma_text::LINE_BASES;
            x.uiReason = ma_text::OK;
            dstQual = x.uiKind == ma_text::LINE_QUAL ? A.bases[ line - 2 ] : 0;
            if( x.uiKind == ma_text::LINE_HEADER && pos == from )
            {
                A.roff[ h0 >> 32 ] = dstBase;
                A.nameOff[ h0 >> 32 ] = dstName;
            }
            loaded = true;
        }
        u32 j;
        const u32 t = ma_text::byteTarget( x, (u32)( pos - from ), &j );
        if( t == ma_text::TO_CODES )
            A.codes[ (u64)dstBase + j ] = ma_text::code( (uint8_t)b );
        else if( t == ma_text::TO_QUAL )
            A.qual[ (u64)dstQual + j ] = (uint8_t)b;
        else if( t == ma_text::TO_NAMES )
            A.names[ (u64)dstName + j ] = (char)b;
    } );
}

// ---- mate pairs out of two texts (ma_batch_set_mates_text) ------------------------------------------------------------------------
// PairedFileReader::execute (fileReader.h:568-617) for a whole batch: both texts go through the kernels above, each on scratch of
// its own; record k of text 1 becomes read 2k, record k of text 2 read 2k + 1 (ma_text::pairHost is the serial statement).
//   k_text_mates_plan  one lane per pair: bases and name bytes of both mates into the batch's two offset arrays (scanned behind
//                      it), the longest paired read
//   k_text_mates_stat  one lane: pairs, sums, consumed bytes, the winning refusal, whether anything may be written
//   k_text_mates_emit  16 bytes per lane over one text: every byte of a paired record to its place in the interleaved arrays; a
//                      second mate reversed and complemented (NucSeq::vReverse + vSwitchAllBasePairsToComplement)
enum : int // the statistics block of a paired parse (u64 words), behind the two texts' blocks
{
    MT_PAIRS = 0,
    MT_BASES = 1, // over the paired records
    MT_NAME_BYTES = 2,
    MT_MAX_LEN = 3,
    MT_CONSUMED = 4, // two words: offset of record R of each text (the text's size if it has none)
    MT_REFUSAL = 6, // ma_text::MATES_*
    MT_TEXT = 7, // MATES_LINE: 1 or 2
    MT_VIOLATION = 8, // MATES_LINE: ma_text::key( line, reason )
    MT_BYTE = 9, // MATES_LINE: offset of the refused line
    MT_EMIT = 10, // 1: accepted and within the batch's capacity, k_text_mates_emit writes
    MT_WORDS = 16
};
// One of the two texts as the kernels above left it.  lines == 0: an empty text, or one the host refused (hostKey): no arrays.
struct TextSide
{
    const char* text;
    u64 n, lines;
    const u32* start;
    const u64* hdrName; // the scans
    const u32* bases;
    const u32* recLine;
    const unsigned long long* stat;
    u64 hostKey;
};
__device__ __forceinline__ u64 side_records( const TextSide& s )
{
    return s.lines ? s.hdrName[ s.lines ] >> 32 : 0;
}

// entries: min( max_reads, 2 x the most pairs the line counts allow ) + 1 words of roff and nameOff, all written: the lengths of
// reads 2k and 2k + 1 for k < R, 0 behind them (and everywhere when 2 R reads do not fit)
__global__ __launch_bounds__( 256 ) void k_text_mates_plan( TextSide a, TextSide b, u64 entries, u64 max_reads, u64* roff, u64* nameOff,
                                                            unsigned long long* mstat )
{
    const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 Ra = side_records( a ), Rb = side_records( b ), R = Ra < Rb ? Ra : Rb;
    u32 len0 = 0, len1 = 0, name0 = 0, name1 = 0;
    if( k < R && 2 * R <= max_reads )
    {
        const u32 la = a.recLine[ k ], lb = b.recLine[ k ];
        len0 = a.bases[ k + 1 < Ra ? a.recLine[ k + 1 ] : a.lines ] - a.bases[ la ];
        len1 = b.bases[ k + 1 < Rb ? b.recLine[ k + 1 ] : b.lines ] - b.bases[ lb ];
        name0 = (u32)a.hdrName[ la + 1 ] - (u32)a.hdrName[ la ];
        name1 = (u32)b.hdrName[ lb + 1 ] - (u32)b.hdrName[ lb ];
    }
    if( 2 * k < entries )
        roff[ 2 * k ] = len0, nameOff[ 2 * k ] = name0;
    if( 2 * k + 1 < entries )
        roff[ 2 * k + 1 ] = len1, nameOff[ 2 * k + 1 ] = name1;
    u32 longest = max( len0, len1 );
    for( int m = 32; m; m >>= 1 )
        longest = max( longest, (u32)__shfl_xor( (int)longest, m, 64 ) );
    if( ( threadIdx.x & 63 ) == 0 && longest )
        atomicMax( mstat + MT_MAX_LEN, (unsigned long long)longest );
}

// roff, nameOff: the scans of k_text_mates_plan's entries (word 0 alone, and 0, when a text is empty)
__global__ void k_text_mates_stat( TextSide a, TextSide b, u32 kindsDiffer, u64 max_reads, u64 max_bases, const u64* roff, const u64* nameOff,
                                   unsigned long long* mstat )
{
    const u64 Ra = side_records( a ), Rb = side_records( b ), R = Ra < Rb ? Ra : Rb;
    const u64 keyA = a.lines ? a.stat[ TXT_VIOLATION ] : a.hostKey, keyB = b.lines ? b.stat[ TXT_VIOLATION ] : b.hostKey;
    const bool fits = 2 * R <= max_reads;
    const u64 B = fits ? roff[ 2 * R ] : 0, N = fits ? nameOff[ 2 * R ] : 0;
    u64 refusal = ma_text::MATES_OK, text = 0, key = ma_text::NO_VIOLATION, byte = 0;
    if( keyA != ma_text::NO_VIOLATION )
        refusal = ma_text::MATES_LINE, text = 1, key = keyA, byte = a.lines ? a.start[ keyA >> 8 ] : 0;
    else if( keyB != ma_text::NO_VIOLATION )
        refusal = ma_text::MATES_LINE, text = 2, key = keyB, byte = b.lines ? b.start[ keyB >> 8 ] : 0;
    else if( kindsDiffer )
        refusal = ma_text::MATES_KIND;
    else if( !fits || B > max_bases )
        refusal = ma_text::MATES_CAPACITY;
    mstat[ MT_PAIRS ] = R;
    mstat[ MT_BASES ] = B;
    mstat[ MT_NAME_BYTES ] = N;
    mstat[ MT_CONSUMED ] = R < Ra ? a.start[ a.recLine[ R ] ] : a.n;
    mstat[ MT_CONSUMED + 1 ] = R < Rb ? b.start[ b.recLine[ R ] ] : b.n;
    mstat[ MT_REFUSAL ] = refusal;
    mstat[ MT_TEXT ] = text;
    mstat[ MT_VIOLATION ] = key;
    mstat[ MT_BYTE ] = byte;
    mstat[ MT_EMIT ] = refusal == ma_text::MATES_OK ? 1 : 0;
}

struct MatesEmitArgs
{
    u32 kind, revComp; // revComp: second mates are reversed and complemented
    TextSide s;
    const unsigned long long* mstat;
    const u64* roff; // the scans: 2 R + 1 entries each
    const u64* nameOff;
    uint8_t* codes;
    char* names;
    uint8_t* qual; // FASTQ
};
// MATE: 0 over text 1, 1 over text 2.  A base's position in its record is bases[ line ] - bases[ record's header line ] + j, so
// that a FASTA mate of several lines reverses across them.  Lanes of a reversed mate write descending addresses.
template <int MATE> __global__ __launch_bounds__( TEXT_BLOCK ) void k_text_mates_emit( MatesEmitArgs A )
{
    if( !A.mstat[ MT_EMIT ] )
        return; // refused, or more than the batch holds: nothing is written
    const u64 base = ( (u64)blockIdx.x * TEXT_BLOCK + threadIdx.x ) * TEXT_LANE_BYTES;
    if( base >= A.s.n )
        return;
    const u64 R = A.mstat[ MT_PAIRS ];
    const bool rev = MATE == 1 && A.revComp != 0;
    // the line of the lane's first byte: the last one that starts at or before it
    u64 lo = 0, hi = A.s.lines - 1;
    while( lo < hi )
    {
        const u64 mid = ( lo + hi + 1 ) >> 1;
        if( A.s.start[ mid ] <= base )
            lo = mid;
        else
            hi = mid - 1;
    }
    u64 line = lo;
    u32 from = 0, to = 0, at = 0, len = 0; // of `line`, loaded when the walk enters it; at: bases of the record before the line
    u64 dst = 0, dstName = 0;
    ma_text::Line x;
    bool loaded = false, paired = false;
    const TextChunk c = text_chunk( A.s.text, A.s.n, base );
    text_each( c, [ & ]( int k, u32 b ) {
        const u64 pos = base + k;
        if( pos >= A.s.n )
            return;
        if( loaded && pos >= to )
            line++, loaded = false;
        if( !loaded )
        {
            from = A.s.start[ line ], to = A.s.start[ line + 1 ];
            const u64 h0 = A.s.hdrName[ line ], h1 = A.s.hdrName[ line + 1 ];
            const u32 lineBases = A.s.bases[ line ];
            x.uiLen = ma_text::content( A.s.text, from, to );
            x.uiBases = A.s.bases[ line + 1 ] - lineBases;
            x.uiName = (u32)h1 - (u32)h0;
            x.uiKind = A.kind == ma_text::KIND_FASTQ ? (u32)( line & 3u ) : ( h1 >> 32 ) != ( h0 >> 32 ) ? ma_text::LINE_HEADER : ma_text::LINE_BASES;
            x.uiReason = ma_text::OK;
            // headers before the line: a header line is the record of that number, any other line belongs to the one before
            const u64 rec = ( h0 >> 32 ) - ( x.uiKind == ma_text::LINE_HEADER ? 0 : 1 );
            paired = ( x.uiKind == ma_text::LINE_HEADER || ( h0 >> 32 ) > 0 ) && rec < R;
            if( paired )
            {
                const u64 entry = 2 * rec + MATE;
                dst = A.roff[ entry ];
                len = (u32)( A.roff[ entry + 1 ] - dst );
                dstName = A.nameOff[ entry ];
                at = x.uiKind == ma_text::LINE_BASES ? lineBases - A.s.bases[ A.s.recLine[ rec ] ] : 0; // (a quality line mirrors its one bases line)
            }
            loaded = true;
        }
        if( !paired )
            return; // a record beyond the shorter text: validated, dropped
        u32 j;
        const u32 t = ma_text::byteTarget( x, (u32)( pos - from ), &j );
        const u32 p = at + j;
        if( ( t == ma_text::TO_CODES || t == ma_text::TO_QUAL ) && p >= len )
            return; // (never in a text that passed: a record's bytes lie inside the record)
        const u64 where = dst + ( rev ? len - 1 - p : p );
        if( t == ma_text::TO_CODES )
            A.codes[ where ] = rev ? ma_text::mateCode( ma_text::code( (uint8_t)b ) ) : ma_text::code( (uint8_t)b );
        else if( t == ma_text::TO_QUAL )
            A.qual[ where ] = (uint8_t)b;
        else if( t == ma_text::TO_NAMES )
            A.names[ dstName + j ] = (char)b;
    } );
}
