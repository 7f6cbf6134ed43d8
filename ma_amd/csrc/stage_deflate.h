// stage_deflate.h -- a text deflated on the device into BGZF members (ma_sam_bgzf_batch, ma_bgzf_deflate).  The rules -- the cuts,
// the parse, the codes, the member's bytes -- are the functions of ma_amd/host/ma_deflate_dev.h, the code the CPU tests pin to
// zlib's inflate; the kernels only spread them over the lanes of a wavefront.  Textually part of pipeline.hip.
//   k_deflate       ONE WAVEFRONT PER MEMBER (a workgroup is one wavefront; the grid strides over the members).  Per strip of 64
//                   positions every lane finds its position's match (the table's candidate and the byte before; the text is read
//                   from global memory), the greedy walk over the strip runs on wave-uniform state over the ballot of the lanes
//                   that have a match, the lanes where a token starts write it to the wavefront's token scratch and count it with
//                   LDS atomics, and the strip's positions go into the table (16-bit positions, 16 KiB of LDS; the highest
//                   position of a hash wins).  The ranks of the symbols are shared by the lanes, the code construction itself
//                   runs on lane 0.  The size of the member follows from counts and lengths; if the dynamic form is the smaller
//                   one, lane 0 writes the block header and the tokens' bits follow 64 at a time: a prefix sum over their bit
//                   counts places them in an LDS stage, whose whole bytes go to the member's slot.
//                   22.7 KiB of LDS per wavefront: 6 wavefronts per CU.  The token scratch is sized by the grid
//                   (DEFLATE_GRID_MAX wavefronts of 255 KiB), not by the members of the text.
//   k_deflate_pack  one wavefront per member, behind the scan of the members' sizes: the 18 header bytes, the deflate bytes out of
//                   the slot -- or the stored block straight from the text --, the CRC32 of the text (the 64-lane fold of
//                   k_bgzf_crc) and ISIZE, at the member's offset in the packed output.
// Every global write is bounded: a token's index by the member's text bytes (a token covers at least one), a slot's byte by the
// member's planned deflate bytes, the packed member by its planned size.  Every loop advances by at least one byte or ends.

static constexpr u32 DEFLATE_GRID_MAX = 1536; // wavefronts in flight: 256 CUs x 6
static constexpr u32 DEFLATE_SLOT = 65312; // bytes per member's slot: the dynamic form is smaller than 65 280 + 5
static constexpr u32 DEFLATE_STAGE_WORDS = 100; // 7 carried bits + 64 tokens of at most 48, and two words of slack behind
static constexpr u32 DEFLATE_STORED = 0x80000000u; // in flags[ ]: the member is a stored block

__device__ __forceinline__ u64 deflate_bits( u32 from, u32 to ) // bits from .. to - 1; from < 64, to <= 64
{
    return ( to >= 64 ? ~0ull : ( 1ull << to ) - 1ull ) & ~( ( 1ull << from ) - 1ull );
}

__global__ __launch_bounds__( 64 ) void k_deflate( const uint8_t* text, u64 n, u64 nMembers, u32* tokens, uint8_t* slots, u64* sizes, u32* flags )
{
    __shared__ uint16_t sHash[ ma_bgzf::HASH_SIZE ];
    __shared__ ma_bgzf::DeflateWork W;
    __shared__ u32 sStage[ DEFLATE_STAGE_WORDS ];
    __shared__ u32 sPlan[ 4 ];
    const u32 lane = threadIdx.x;
    u32* const myTokens = tokens + (u64)blockIdx.x * ma_bgzf::DEFLATE_CHUNK;
    for( u64 m = blockIdx.x; m < nMembers; m += gridDim.x )
    {
        const uint8_t* const T = text + m * ma_bgzf::DEFLATE_CHUNK;
        const u32 len = ma_bgzf::memberText( n, m );
        uint8_t* const slot = slots + m * DEFLATE_SLOT;
        for( u32 i = lane; i < ma_bgzf::HASH_SIZE; i += 64 )
            sHash[ i ] = (uint16_t)ma_bgzf::NO_POS;
        for( u32 i = lane; i < ma_bgzf::A_ALL; i += 64 )
            W.aCount[ i ] = 0;
        __syncthreads( );

        // ---- the parse ----
        u32 pos = 0, nTok = 0; // wave-uniform: the walk's position, the tokens so far
        for( u32 base = 0; base < len; base += ma_bgzf::STRIP )
        {
            const u32 p = base + lane;
            const bool hashable = p + 4 <= len;
            const u32 h = hashable ? ma_bgzf::hashOf( T + p ) : 0u;
            const u32 end = min( base + ma_bgzf::STRIP, len ) - base; // 1 .. 64
            if( pos < base + end ) // (else a match covers the whole strip: it only goes into the table)
            {
                u32 mlen = 0, mdist = 0;
                if( p >= pos && p < len )
                    ma_bgzf::findMatch( T, len, p, hashable ? (u32)sHash[ h ] : ma_bgzf::NO_POS, &mlen, &mdist );
                const u64 isMatch = __ballot( mlen >= ma_bgzf::MIN_MATCH );
                u64 starts = 0;
                u32 l = pos - base;
                while( l < end )
                {
                    const u64 rest = isMatch >> l;
                    if( rest == 0 )
                    {
                        starts |= deflate_bits( l, end );
                        l = end;
                        break;
                    }
                    const u32 ml = l + (u32)__ffsll( (unsigned long long)rest ) - 1u;
                    starts |= deflate_bits( l, ml + 1 );
                    l = ml + (u32)__builtin_amdgcn_readlane( (int)mlen, (int)ml );
                }
                pos = base + l;
                if( ( starts >> lane ) & 1ull )
                {
                    const u32 tok = mlen >= ma_bgzf::MIN_MATCH ? ma_bgzf::matchToken( mlen, mdist ) : (u32)T[ p ];
                    const u32 at = nTok + (u32)__popcll( starts & ( ( 1ull << lane ) - 1ull ) );
                    if( at < len )
                        myTokens[ at ] = tok;
                    if( tok < 256u )
                        atomicAdd( &W.aCount[ tok ], 1u );
                    else
                    {
                        u32 e, v;
                        atomicAdd( &W.aCount[ ma_bgzf::lengthSymbol( mlen, &e, &v ) ], 1u );
                        atomicAdd( &W.aCount[ ma_bgzf::A_DIST + ma_bgzf::distSymbol( mdist, &e, &v ) ], 1u );
                    }
                }
                nTok += (u32)__popcll( starts );
            }
            __syncthreads( ); // the strip's reads of the table are done
            bool pending = hashable;
            while( __ballot( pending ) != 0 ) // at least the winner of a round leaves it
            {
                if( pending )
                    sHash[ h ] = (uint16_t)p;
                __syncthreads( );
                if( pending && (u32)sHash[ h ] >= p )
                    pending = false; // it is there, or a later position of the strip is
                __syncthreads( );
            }
        }
        nTok = min( nTok, len );
        if( lane == 0 )
            W.aCount[ ma_bgzf::END_OF_BLOCK ] = 1;
        __syncthreads( );

        // ---- the codes: planSerial( ) with the ranks shared by the lanes ----
        for( u32 s = lane; s < ma_bgzf::N_LITLEN; s += 64 )
            if( W.aCount[ ma_bgzf::A_LITLEN + s ] != 0 )
                W.aOrder[ ma_bgzf::rankOf( W, ma_bgzf::A_LITLEN, ma_bgzf::N_LITLEN, s ) ] = (uint16_t)s;
        __syncthreads( );
        u32 aTrue[ 3 ] = { 0, 0, 0 };
        if( lane == 0 )
        {
            ma_bgzf::lengthsOf( W, ma_bgzf::A_LITLEN, ma_bgzf::N_LITLEN, ma_bgzf::usedOf( W, ma_bgzf::A_LITLEN, ma_bgzf::N_LITLEN ), 15 );
            ma_bgzf::codesOf( W, ma_bgzf::A_LITLEN, ma_bgzf::N_LITLEN );
            aTrue[ 0 ] = W.aCount[ ma_bgzf::A_DIST ], aTrue[ 1 ] = W.aCount[ ma_bgzf::A_DIST + 1 ], aTrue[ 2 ] = W.aCount[ ma_bgzf::A_DIST + 2 ];
            ma_bgzf::padAlphabet( W, ma_bgzf::A_DIST, ma_bgzf::N_DIST );
        }
        __syncthreads( );
        if( lane < ma_bgzf::N_DIST && W.aCount[ ma_bgzf::A_DIST + lane ] != 0 )
            W.aOrder[ ma_bgzf::rankOf( W, ma_bgzf::A_DIST, ma_bgzf::N_DIST, lane ) ] = (uint16_t)lane;
        __syncthreads( );
        if( lane == 0 )
        {
            ma_bgzf::lengthsOf( W, ma_bgzf::A_DIST, ma_bgzf::N_DIST, ma_bgzf::usedOf( W, ma_bgzf::A_DIST, ma_bgzf::N_DIST ), 15 );
            ma_bgzf::codesOf( W, ma_bgzf::A_DIST, ma_bgzf::N_DIST );
            W.aCount[ ma_bgzf::A_DIST ] = aTrue[ 0 ], W.aCount[ ma_bgzf::A_DIST + 1 ] = aTrue[ 1 ], W.aCount[ ma_bgzf::A_DIST + 2 ] = aTrue[ 2 ];
            ma_bgzf::planHeader( W );
            ma_bgzf::padAlphabet( W, ma_bgzf::A_CODELEN, ma_bgzf::N_CODELEN );
        }
        __syncthreads( );
        if( lane < ma_bgzf::N_CODELEN && W.aCount[ ma_bgzf::A_CODELEN + lane ] != 0 )
            W.aOrder[ ma_bgzf::rankOf( W, ma_bgzf::A_CODELEN, ma_bgzf::N_CODELEN, lane ) ] = (uint16_t)lane;
        __syncthreads( );
        if( lane == 0 )
        {
            ma_bgzf::lengthsOf( W, ma_bgzf::A_CODELEN, ma_bgzf::N_CODELEN, ma_bgzf::usedOf( W, ma_bgzf::A_CODELEN, ma_bgzf::N_CODELEN ), 7 );
            ma_bgzf::codesOf( W, ma_bgzf::A_CODELEN, ma_bgzf::N_CODELEN );
            ma_bgzf::planHeader( W );
            bool stored;
            const u32 deflateBytes = ma_bgzf::deflateBytesOf( len, ma_bgzf::planBits( W ), &stored );
            sizes[ m ] = ma_bgzf::MEMBER_FRAME + deflateBytes;
            flags[ m ] = deflateBytes | ( stored ? DEFLATE_STORED : 0u );
            sPlan[ 0 ] = stored ? 0u : deflateBytes;
            if( !stored ) // the block header; the tokens go on behind its last whole byte
            {
                ma_bgzf::BitWriter B = { slot, deflateBytes, 0, 0, 0 };
                ma_bgzf::writeHeader( W, B );
                sPlan[ 1 ] = B.uiBytes, sPlan[ 2 ] = (u32)B.uiAcc, sPlan[ 3 ] = B.uiCnt;
            }
        }
        __syncthreads( );

        // ---- the bits ----
        const u32 cap = sPlan[ 0 ]; // 0: stored, k_deflate_pack copies the text
        if( cap != 0 )
        {
            u32 bytes = sPlan[ 1 ], carry = sPlan[ 2 ] & 0xffu, cb = sPlan[ 3 ]; // whole bytes written, the bits behind them, their number
            for( u32 t0 = 0; t0 < nTok; t0 += 64 )
            {
                for( u32 i = lane; i < DEFLATE_STAGE_WORDS; i += 64 )
                    sStage[ i ] = i == 0 ? carry : 0u;
                __syncthreads( );
                u64 v = 0;
                u32 nb = 0;
                if( t0 + lane < nTok )
                    v = ma_bgzf::tokenBits( W, myTokens[ t0 + lane ], &nb );
                u32 incl = nb;
                for( u32 d = 1; d < 64; d <<= 1 )
                {
                    const u32 o = (u32)__shfl_up( (int)incl, d, 64 );
                    if( lane >= d )
                        incl += o;
                }
                const u32 total = cb + (u32)__shfl( (int)incl, 63, 64 );
                if( nb != 0 )
                {
                    const u32 off = cb + incl - nb, w = off >> 5, sh = off & 31u;
                    const u64 lo = v << sh;
                    const u32 hi = sh != 0 ? (u32)( v >> ( 64u - sh ) ) : 0u;
                    atomicOr( &sStage[ w ], (u32)lo );
                    if( ( lo >> 32 ) != 0 )
                        atomicOr( &sStage[ w + 1 ], (u32)( lo >> 32 ) );
                    if( hi != 0 )
                        atomicOr( &sStage[ w + 2 ], hi );
                }
                __syncthreads( );
                const u32 whole = total >> 3;
                for( u32 k = lane; k < whole; k += 64 )
                    if( bytes + k < cap )
                        slot[ bytes + k ] = (uint8_t)( sStage[ k >> 2 ] >> ( 8u * ( k & 3u ) ) );
                carry = ( sStage[ whole >> 2 ] >> ( 8u * ( whole & 3u ) ) ) & 0xffu;
                bytes += whole;
                cb = total & 7u;
                __syncthreads( );
            }
            if( lane == 0 )
            {
                ma_bgzf::BitWriter B = { slot, cap, bytes, carry, cb };
                B.put( W.aCode[ ma_bgzf::END_OF_BLOCK ], W.aLength[ ma_bgzf::END_OF_BLOCK ] );
                B.finish( );
            }
        }
        __syncthreads( ); // (the next member starts by clearing what lane 0 may still read)
    }
}

// off: the exclusive sums of k_deflate's sizes (nMembers + 1 entries); out: off[ nMembers ] bytes
__global__ __launch_bounds__( 256 ) void k_deflate_pack( const uint8_t* text, u64 n, u64 nMembers, const uint8_t* slots, const u64* off, const u32* flags,
                                                         uint8_t* out )
{
    const u64 m = (u64)blockIdx.x * 4 + ( threadIdx.x / 64 ); // (the same for a whole wavefront)
    const u32 lane = threadIdx.x % 64;
    if( m >= nMembers )
        return;
    const uint8_t* const T = text + m * ma_bgzf::DEFLATE_CHUNK;
    const u32 len = ma_bgzf::memberText( n, m );
    const u32 deflateBytes = flags[ m ] & ~DEFLATE_STORED;
    const bool stored = ( flags[ m ] & DEFLATE_STORED ) != 0;
    const u32 size = (u32)( off[ m + 1 ] - off[ m ] );
    if( size != ma_bgzf::MEMBER_FRAME + deflateBytes || ( stored && deflateBytes != len + 5u ) )
        return; // (cannot be: the sizes are k_deflate's)
    uint8_t* const p = out + off[ m ];
    if( lane == 0 )
        ma_bgzf::writeMemberHead( p, size );
    uint8_t* const stream = p + ma_bgzf::MEMBER_HEAD;
    if( stored )
    {
        if( lane == 0 )
            ma_bgzf::writeStoredHead( stream, len );
        for( u32 i = lane; i < len; i += 64 )
            stream[ 5 + i ] = T[ i ];
    }
    else
    {
        const uint8_t* const slot = slots + m * DEFLATE_SLOT;
        for( u32 i = lane; i < deflateBytes; i += 64 )
            stream[ i ] = slot[ i ];
    }
    const u32 stretch = ( len + 63 ) / 64;
    const u32 from = min( lane * stretch, len ), to = min( from + stretch, len );
    u32 crc = ma_bgzf::crcOf( T + from, to - from ), bytes = to - from;
    for( u32 step = 1; step < 64; step <<= 1 )
    {
        const u32 crcRight = (u32)__shfl_down( (int)crc, step, 64 ), bytesRight = (u32)__shfl_down( (int)bytes, step, 64 );
        if( ( lane & ( 2 * step - 1 ) ) == 0 )
        {
            crc = ma_bgzf::crcCombine( crc, crcRight, bytesRight );
            bytes += bytesRight;
        }
    }
    if( lane == 0 )
        ma_bgzf::writeMemberTail( stream + deflateBytes, crc, len );
}
