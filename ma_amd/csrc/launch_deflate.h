// launch_deflate.h -- ma_sam_bgzf_batch, the downloads of its members, and the primitive ma_bgzf_deflate.  Textually part of
// pipeline.hip; the kernels are in stage_deflate.h, the rules in ma_amd/host/ma_deflate_dev.h.
//
// One sequence for both (deflate_front / deflate_rest): k_deflate over the text's members -- it leaves each member's size and, for
// a dynamic member, its deflate bytes in the member's slot --, a scan of the sizes into the members' offsets, the wait with the
// ONE read-back of the compressed size, and k_deflate_pack into the packed output with nobody waiting.  The gets and downloads
// are two plain copies through the batch's one download slot.
namespace
{
int deflate_front( hipStream_t st, const uint8_t* text, u64 n, DeflateBufs& S, DeflateMembers& O, unsigned long long* hBytes )
{
    const u64 members = ma_bgzf::deflateMembers( n );
    const u32 grid = (u32)std::min<u64>( members, DEFLATE_GRID_MAX );
    if( S.tokens.reserve( (u64)grid * ma_bgzf::DEFLATE_CHUNK * 4 ) || S.slots.reserve( members * DEFLATE_SLOT ) || S.sizes.reserve( ( members + 1 ) * 8 ) ||
        S.flags.reserve( members * 4 ) || O.off.reserve( ( members + 1 ) * 8 ) )
        return 1;
    MA_HIP( hipMemsetAsync( S.sizes.as<u64>( ) + members, 0, 8, st ) );
    hipLaunchKernelGGL( k_deflate, dim3( grid ), dim3( 64 ), 0, st, text, n, members, S.tokens.as<u32>( ), S.slots.as<uint8_t>( ), S.sizes.as<u64>( ),
                        S.flags.as<u32>( ) );
    MA_HIP( hipGetLastError( ) );
    size_t tb = 0;
    MA_HIP( hipcub::DeviceScan::ExclusiveSum( nullptr, tb, S.sizes.as<u64>( ), O.off.as<u64>( ), (int)( members + 1 ), st ) );
    if( S.cub.reserve( tb + 256 ) )
        return 1;
    MA_HIP( hipcub::DeviceScan::ExclusiveSum( S.cub.p, tb, S.sizes.as<u64>( ), O.off.as<u64>( ), (int)( members + 1 ), st ) );
    MA_HIP( hipMemcpyAsync( hBytes, O.off.as<u64>( ) + members, 8, hipMemcpyDeviceToHost, st ) );
    return 0;
}

// behind the wait: *hBytes is the size of the output
int deflate_rest( hipStream_t st, const uint8_t* text, u64 n, DeflateBufs& S, DeflateMembers& O, u64 bytes )
{
    const u64 members = ma_bgzf::deflateMembers( n );
    if( bytes < members * ( ma_bgzf::MEMBER_FRAME + 1 ) || bytes > ma_bgzf::deflateBound( n ) )
        return fail( "deflate: the members' sizes do not add up (" + std::to_string( bytes ) + " bytes for " + std::to_string( n ) + ")" );
    if( O.bytes.reserve( bytes + 64 ) )
        return 1;
    hipLaunchKernelGGL( k_deflate_pack, dim3( (unsigned)( ( members + 3 ) / 4 ) ), dim3( 256 ), 0, st, text, n, members, S.slots.as<uint8_t>( ),
                        O.off.as<u64>( ), S.flags.as<u32>( ), O.bytes.as<uint8_t>( ) );
    MA_HIP( hipGetLastError( ) );
    return 0;
}

// the text the call names, or the message
int sam_bgzf_state( ma_batch* b, int32_t pair, const char* who, bool needMembers, SamTextState** s )
{
    if( !b )
        return fail( std::string( who ) + ": null batch" );
    *s = pair ? &b->pairSam : &b->sam;
    if( !b->st.has( ( *s )->id ) )
        return fail( std::string( who ) + ": no SAM text to deflate (run " + ( pair ? "ma_pair_sam_batch" : "ma_sam_batch" ) + " first)" );
    if( needMembers && !b->st.has( ma_state::membersOf( ( *s )->id ) ) )
        return fail( std::string( who ) + ": run ma_sam_bgzf_batch first (making the SAM text again drops the members)" );
    return 0;
}

int get_sam_bgzf( ma_batch* b, int32_t pair, uint64_t* member_off, void* bytes, bool async )
{
    SamTextState* s;
    const char* const who = async ? "ma_batch_start_sam_bgzf_download" : "ma_batch_get_sam_bgzf";
    if( sam_bgzf_state( b, pair, who, true, &s ) )
        return 1;
    MA_BIND_DEVICE( b->device );
    if( download_begin( b, async, "ma_batch_start_sam_bgzf_download" ) )
        return 1;
    const ma_state::TextCounts& c = b->st.text( s->id );
    if( c.zMembers == 0 )
    {
        if( member_off )
            member_off[ 0 ] = 0;
        return 0;
    }
    hipStream_t cs;
    if( download_stream( b, async, &cs ) )
        return 1;
    if( member_off )
        MA_HIP( hipMemcpyAsync( member_off, s->z.off.p, ( c.zMembers + 1 ) * 8, hipMemcpyDeviceToHost, cs ) );
    if( bytes )
        MA_HIP( hipMemcpyAsync( bytes, s->z.bytes.p, c.zBytes, hipMemcpyDeviceToHost, cs ) );
    return download_end( b, async, cs );
}
} // namespace

extern "C" {

int ma_sam_bgzf_batch( ma_batch* b, int32_t pair )
{
    SamTextState* s;
    if( sam_bgzf_state( b, pair, "ma_sam_bgzf_batch", false, &s ) )
        return 1;
    MA_BIND_DEVICE( b->device );
    if( download_wait( b ) ) // the members of the last call may still be on their way down
        return 1;
    b->st.drop( ma_state::membersOf( s->id ) );
    ma_state::TextCounts& c = b->st.text( s->id );
    if( c.bytes )
    {
        unsigned long long total = 0;
        if( b->timing )
            (void)hipEventRecord( b->ev[ 14 ], b->stream );
        if( deflate_front( b->stream, s->text.as<uint8_t>( ), c.bytes, b->zScratch, s->z, &total ) )
            return 1;
        if( batch_wait( b ) )
            return 1;
        if( deflate_rest( b->stream, s->text.as<uint8_t>( ), c.bytes, b->zScratch, s->z, total ) )
            return 1;
        if( b->timing )
        {
            (void)hipEventRecord( b->ev[ 15 ], b->stream );
            float ms = 0;
            if( hipEventSynchronize( b->ev[ 15 ] ) == hipSuccess && hipEventElapsedTime( &ms, b->ev[ 14 ], b->ev[ 15 ] ) == hipSuccess )
                b->kms[ 7 ] = ms;
        }
        c.zMembers = ma_bgzf::deflateMembers( c.bytes );
        c.zBytes = total;
    }
    b->st.finish( ma_state::membersOf( s->id ) );
    return 0;
}

int ma_batch_sam_bgzf_counts( ma_batch* b, int32_t pair, uint64_t* n_members, uint64_t* n_bytes )
{
    SamTextState* s;
    if( sam_bgzf_state( b, pair, "ma_batch_sam_bgzf_counts", true, &s ) )
        return 1;
    if( n_members )
        *n_members = b->st.text( s->id ).zMembers;
    if( n_bytes )
        *n_bytes = b->st.text( s->id ).zBytes;
    return 0;
}

int ma_batch_get_sam_bgzf( ma_batch* b, int32_t pair, uint64_t* member_off, void* bytes )
{
    return get_sam_bgzf( b, pair, member_off, bytes, false );
}

int ma_batch_start_sam_bgzf_download( ma_batch* b, int32_t pair, uint64_t* member_off, void* bytes )
{
    return get_sam_bgzf( b, pair, member_off, bytes, true );
}

int ma_bgzf_deflate( const ma_index* x, const void* text, uint64_t n_bytes, uint64_t* n_members, uint64_t* n_out, uint64_t* member_off, void* out,
                     uint64_t cap )
{
    if( !x || ( n_bytes && !text ) )
        return fail( "ma_bgzf_deflate: null argument" );
    MA_BIND_DEVICE( x->device );
    const u64 members = ma_bgzf::deflateMembers( n_bytes );
    unsigned long long total = 0;
    DeflateBufs S;
    DeflateMembers O;
    DevBuf in;
    if( n_bytes )
    {
        if( in.reserve( n_bytes + 64 ) )
            return 1;
        MA_HIP( hipMemcpyAsync( in.p, text, n_bytes, hipMemcpyHostToDevice, nullptr ) );
        if( deflate_front( nullptr, in.as<uint8_t>( ), n_bytes, S, O, &total ) )
            return 1;
        MA_HIP( hipStreamSynchronize( nullptr ) );
    }
    if( n_members )
        *n_members = members;
    if( n_out )
        *n_out = total;
    if( !out )
        return 0;
    if( cap < total )
        return fail( "ma_bgzf_deflate: the members take " + std::to_string( total ) + " bytes, cap is " + std::to_string( cap ) );
    if( member_off )
        member_off[ 0 ] = 0;
    if( n_bytes == 0 )
        return 0;
    if( deflate_rest( nullptr, in.as<uint8_t>( ), n_bytes, S, O, total ) )
        return 1;
    if( member_off )
        MA_HIP( hipMemcpyAsync( member_off, O.off.p, ( members + 1 ) * 8, hipMemcpyDeviceToHost, nullptr ) );
    MA_HIP( hipMemcpyAsync( out, O.bytes.p, total, hipMemcpyDeviceToHost, nullptr ) );
    MA_HIP( hipStreamSynchronize( nullptr ) );
    return 0;
}
} // extern "C"
