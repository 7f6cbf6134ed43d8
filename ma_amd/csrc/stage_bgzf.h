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
//                   the parser's front (BGZ_FIRST, BGZ_LAST), of each text.
// ma_batch_set_mates_bgzf runs both over ONE member table, text 1's members in front of text 2's: a member's uiDeflate and uiOut
// say where its bytes are and where its text goes, so neither kernel knows of the two texts -- but for the ends k_bgzf_crc leaves.
// A violation is ma_bgzf::key( member, reason ), the lowest wins (atomicMin, one per wavefront).

enum : int // the statistics block of an inflate (u64 words), behind the parse's TXT_WORDS
{
    BGZ_VIOLATION = 0, // lowest ma_bgzf::key( member, reason ) (all ones: none)
    BGZ_FIRST = 1, // the text's first ...
    BGZ_LAST = 2, // ... and last byte; ma_batch_set_mates_bgzf's second text: BGZ_FIRST + 2, BGZ_LAST + 2
    BGZ_WORDS = 6
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

// the call's texts T (head + members - drop) of n bytes each, for their first and last bytes (a single text: n[ 1 ] = 0)
struct BgzfWhole
{
    const uint8_t* p[ 2 ];
    u64 n[ 2 ];
};
__global__ __launch_bounds__( 256 ) void k_bgzf_crc( const ma_bgzf::Member* members, u64 nMembers, const uint8_t* text, BgzfWhole whole,
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
    if( blockIdx.x == 0 && threadIdx.x < 2 ) // (no indexing of the argument by the lane: it stays in registers)
    {
        const uint8_t* const p = threadIdx.x ? whole.p[ 1 ] : whole.p[ 0 ];
        const u64 n = threadIdx.x ? whole.n[ 1 ] : whole.n[ 0 ];
        if( n > 0 )
        {
            bstat[ BGZ_FIRST + 2 * threadIdx.x ] = p[ 0 ];
            bstat[ BGZ_LAST + 2 * threadIdx.x ] = p[ n - 1 ];
        }
    }
}
