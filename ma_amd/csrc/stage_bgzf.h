// stage_bgzf.h -- BGZF members inflated on the device (ma_batch_set_reads_bgzf): the compressed bytes of a read file go up as they
// are and come out as the text the kernels of stage_text.h parse.  The rules -- the member form, the deflate stream, what is
// refused -- are the functions of ma_amd/host/ma_bgzf_dev.h, the code the CPU tests pin to zlib; the kernels only spread them
// over lanes.  Textually part of pipeline.hip.
//   k_bgzf_inflate  one member per lane, one wavefront per workgroup: ma_bgzf::inflate over the member's deflate bytes into its
//                   own stretch of the text.  The bit stream is 64 bits in registers, refilled by dword loads; the decode tables
//                   (the canonical form: codes per length + symbols in code order, 16-bit words) are the lane's 896 bytes of
//                   LDS, word i of lane l at [ i ][ l ]: 56 KiB per wavefront, two wavefronts per CU.  Back-references read the
//                   lane's own earlier output from global memory.  No per-lane array anywhere else.
//   k_bgzf_crc      one member per wavefront: every lane takes a 64th of the member's text, the lanes' CRC32s are folded with
//                   ma_bgzf::crcCombine in six shuffle steps.  A kernel of its own and not part of the lanes of k_bgzf_inflate:
//                   there the CRC would lengthen the one dependent chain per member that sets the kernel's time (a member is
//                   decoded by ONE lane), here 64 lanes share a member's bytes.  Also leaves the text's first and last byte for
//                   the parser's front (BGZ_FIRST, BGZ_LAST).
// A violation is ma_bgzf::key( member, reason ), the lowest wins (atomicMin, one per wavefront).

enum : int // the statistics block of an inflate (u64 words), behind the parse's TXT_WORDS
{
    BGZ_VIOLATION = 0, // lowest ma_bgzf::key( member, reason ) (all ones: none)
    BGZ_FIRST = 1, // the text's first ...
    BGZ_LAST = 2, // ... and last byte
    BGZ_WORDS = 4
};
static constexpr u32 BGZF_LANES = 64;

// a lane's decode tables in LDS
struct BgzfLdsTables
{
    uint16_t* p; // the lane's word 0
    __device__ __forceinline__ u32 get( u32 i ) const
    {
        return p[ i * BGZF_LANES ];
    }
    __device__ __forceinline__ void set( u32 i, u32 v )
    {
        p[ i * BGZF_LANES ] = (uint16_t)v;
    }
};

// text: where the first member's text goes (behind the call's head)
__global__ __launch_bounds__( BGZF_LANES ) void k_bgzf_inflate( const uint8_t* data, const ma_bgzf::Member* members, u64 nMembers, uint8_t* text,
                                                                unsigned long long* bstat )
{
    __shared__ uint16_t sTables[ ma_bgzf::T_WORDS * BGZF_LANES ];
    const u64 m = (u64)blockIdx.x * BGZF_LANES + threadIdx.x;
    u64 key = ma_bgzf::NO_VIOLATION;
    if( m < nMembers )
    {
        const ma_bgzf::Member M = members[ m ];
        const ma_bgzf::ByteSource src = { data + M.uiDeflate, M.uiDeflateBytes };
        ma_bgzf::ByteSink sink = { text + M.uiOut };
        BgzfLdsTables T = { sTables + threadIdx.x };
        const u32 reason = ma_bgzf::inflate( src, sink, T, M.uiIsize );
        if( reason != ma_bgzf::OK )
            key = ma_bgzf::key( m, reason );
    }
    key = wave_min_u64( key );
    if( threadIdx.x == 0 && key != ma_bgzf::NO_VIOLATION )
        atomicMin( bstat + BGZ_VIOLATION, (unsigned long long)key );
}

// whole: the call's text T (head + members - drop) of n bytes, for its first and last byte
__global__ __launch_bounds__( 256 ) void k_bgzf_crc( const ma_bgzf::Member* members, u64 nMembers, const uint8_t* text, const uint8_t* whole, u64 n,
                                                     unsigned long long* bstat )
{
    const u64 m = (u64)blockIdx.x * ( 256 / BGZF_LANES ) + ( threadIdx.x / BGZF_LANES ); // (the same for a whole wavefront)
    const u32 lane = threadIdx.x % BGZF_LANES;
    if( m < nMembers )
    {
        const ma_bgzf::Member M = members[ m ];
        const u32 stretch = ( M.uiIsize + BGZF_LANES - 1 ) / BGZF_LANES;
        const u32 from = min( lane * stretch, M.uiIsize ), to = min( from + stretch, M.uiIsize );
        u32 crc = ma_bgzf::crcOf( text + M.uiOut + from, to - from ), len = to - from;
        for( u32 step = 1; step < BGZF_LANES; step <<= 1 )
        {
            const u32 crcRight = (u32)__shfl_down( (int)crc, step, BGZF_LANES ), lenRight = (u32)__shfl_down( (int)len, step, BGZF_LANES );
            if( ( lane & ( 2 * step - 1 ) ) == 0 )
            {
                crc = ma_bgzf::crcCombine( crc, crcRight, lenRight );
                len += lenRight;
            }
        }
        if( lane == 0 && crc != M.uiCrc )
            atomicMin( bstat + BGZ_VIOLATION, (unsigned long long)ma_bgzf::key( m, ma_bgzf::ERR_CRC ) );
    }
    if( blockIdx.x == 0 && threadIdx.x == 0 && n > 0 )
    {
        bstat[ BGZ_FIRST ] = whole[ 0 ];
        bstat[ BGZ_LAST ] = whole[ n - 1 ];
    }
}
