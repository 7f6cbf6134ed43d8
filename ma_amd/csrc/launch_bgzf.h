// launch_bgzf.h -- ma_batch_set_reads_bgzf: BGZF members inflated on the device into the text buffer of ma_batch_set_reads_text,
// then that call's parse.  Textually part of pipeline.hip; the kernels are in stage_bgzf.h, the rules in
// ma_amd/host/ma_bgzf_dev.h, the parse's front and rest in launch_text.h.
//
// The host walks the member headers (it decodes nothing), refuses at the first bad one, and builds the member table; data, table
// and head go up, k_bgzf_inflate and k_bgzf_crc run, and k_text_count runs right behind them -- it needs neither the kind of the
// text nor its last byte.  TWO read-backs:
//   1  the line feeds, the inflate's lowest violation, the text's first and last byte -- in one copy; the first byte gives the
//      kind, the last one the number of lines that sizes the per-line work
//   2  reads / bases / name bytes / longest read / the text's refusal (text_single_rest, as ma_batch_set_reads_text's second)
// Everything is enqueued on the batch's own stream.
// The walk, the upload and the launch of the two kernels are functions of their own: ma_batch_set_mates_bgzf
// (launch_mates_bgzf.h) runs them over the members of two texts.

static int bgzf_refuse( u64 member, u64 byte, u32 reason )
{
    char msg[ 320 ];
    ma_bgzf::message( msg, sizeof( msg ), member, byte, reason );
    return fail( msg );
}

// The member table of ONE chain of members, headers only, appended to `table`: a member's deflate bytes are at dataAt + its
// offset in `data` (where the chain goes in b->bgzIn), its text goes to outAt + the running sum of ISIZE (uiIn stays the offset
// in `data`: what a refusal names).  OK and the chain's inflated bytes, or the first bad header's reason and offset.
static u32 bgzf_walk( const uint8_t* data, u64 n_bytes, u64 dataAt, u64 outAt, std::vector<ma_bgzf::Member>& table, u64* inflated, u64* badAt )
{
    *inflated = 0;
    for( u64 at = 0; at < n_bytes; )
    {
        ma_bgzf::Member m;
        const u32 reason = ma_bgzf::header( data, n_bytes, at, &m );
        if( reason != ma_bgzf::OK )
        {
            *badAt = at;
            return reason;
        }
        m.uiDeflate += dataAt;
        m.uiOut = outAt + *inflated;
        *inflated += m.uiIsize;
        at += m.uiBytes;
        table.push_back( m );
    }
    return ma_bgzf::OK;
}

// The table goes up and k_bgzf_inflate and k_bgzf_crc run over ALL its members (at least one), whose bytes are in b->bgzIn
// already: ONE launch each, however many chains the table holds.  text: what the members' uiOut count from; whole: the call's
// text(s) for the ends; bstat: BGZ_WORDS words.  The two events around the kernels are ma_batch_kernel_ms [6] (bgzf_time).
static int bgzf_inflate( ma_batch* b, const std::vector<ma_bgzf::Member>& table, char* text, const BgzfWhole& whole, unsigned long long* bstat )
{
    const u64 nMembers = table.size( );
    if( b->bgzMembers.reserve( nMembers * sizeof( ma_bgzf::Member ) ) )
        return 1;
    MA_HIP( hipMemcpyAsync( b->bgzMembers.p, table.data( ), nMembers * sizeof( ma_bgzf::Member ), hipMemcpyHostToDevice, b->stream ) );
    MA_HIP( hipMemsetAsync( bstat, 0, BGZ_WORDS * 8, b->stream ) );
    MA_HIP( hipMemsetAsync( bstat + BGZ_VIOLATION, 0xff, 8, b->stream ) );
    if( b->timing )
        (void)hipEventRecord( b->ev[ 12 ], b->stream );
    hipLaunchKernelGGL( k_bgzf_inflate, dim3( (unsigned)( ( nMembers + BGZF_LANES - 1 ) / BGZF_LANES ) ), dim3( BGZF_LANES ), 0, b->stream,
                        b->bgzIn.as<uint8_t>( ), b->bgzMembers.as<ma_bgzf::Member>( ), nMembers, reinterpret_cast<uint8_t*>( text ), bstat );
    hipLaunchKernelGGL( k_bgzf_crc, dim3( (unsigned)( ( nMembers + 3 ) / 4 ) ), dim3( 256 ), 0, b->stream, b->bgzMembers.as<ma_bgzf::Member>( ),
                        nMembers, reinterpret_cast<const uint8_t*>( text ), whole, bstat );
    MA_HIP( hipGetLastError( ) );
    if( b->timing )
        (void)hipEventRecord( b->ev[ 13 ], b->stream );
    return 0;
}
// behind the wait that follows bgzf_inflate
static void bgzf_time( ma_batch* b )
{
    float ms = 0;
    if( b->timing && hipEventElapsedTime( &ms, b->ev[ 12 ], b->ev[ 13 ] ) == hipSuccess )
        b->kms[ 6 ] = ms;
}

extern "C" {

int ma_batch_set_reads_bgzf( ma_batch* b, const char* head, uint64_t n_head, const void* members, uint64_t n_bytes, uint64_t n_drop,
                             uint64_t* n_reads )
{
    if( !b || ( n_head && !head ) || ( n_bytes && !members ) )
        return fail( "ma_batch_set_reads_bgzf: null argument" );
    MA_BIND_DEVICE( b->device );
    if( n_reads )
        *n_reads = 0;
    if( text_no_reads( b ) )
        return 1;
    // the member table: headers only
    const uint8_t* const data = static_cast<const uint8_t*>( members );
    std::vector<ma_bgzf::Member> table;
    u64 inflated = 0, badAt = 0;
    const u32 bad = bgzf_walk( data, n_bytes, 0, n_head, table, &inflated, &badAt );
    if( bad != ma_bgzf::OK )
        return batch_wait( b ) || bgzf_refuse( table.size( ), badAt, bad );
    if( n_drop > inflated )
        return batch_wait( b ) || fail( "ma_batch_set_reads_bgzf: n_drop is larger than the inflated part of the text" );
    const u64 n = n_head + inflated - n_drop;
    if( n > ma_text::MAX_TEXT_BYTES )
        return batch_wait( b ) || text_refuse( 0, 0, ma_text::ERR_TOO_LARGE, "ma_batch_set_reads_bgzf: text" );
    if( n_head && head[ 0 ] != '@' && head[ 0 ] != '>' )
        return batch_wait( b ) || text_refuse( 0, 0, ma_text::ERR_KIND, "ma_batch_set_reads_bgzf: text" );
    if( b->txtNameOff.reserve( ( b->max_reads + 1 ) * 8 ) )
        return 1;
    MA_HIP( hipMemsetAsync( b->txtNameOff.p, 0, 8, b->stream ) );
    if( b->txtIn.reserve( n_head + inflated + 64 ) || b->txtStat.reserve( ( TXT_WORDS + BGZ_WORDS ) * 8 ) )
        return 1;
    unsigned long long* const stat = b->txtStat.as<unsigned long long>( );
    unsigned long long* const bstat = stat + TXT_WORDS;
    unsigned long long h[ TXT_WORDS + BGZ_WORDS ];
    char* const text = b->txtIn.as<char>( );
    if( n_head )
        MA_HIP( hipMemcpyAsync( text, head, n_head, hipMemcpyHostToDevice, b->stream ) );
    const u64 nMembers = table.size( );
    if( nMembers )
    {
        if( b->bgzIn.reserve( n_bytes + 64 ) )
            return 1;
        MA_HIP( hipMemcpyAsync( b->bgzIn.p, data, n_bytes, hipMemcpyHostToDevice, b->stream ) );
        const BgzfWhole whole = { { reinterpret_cast<const uint8_t*>( text ), nullptr }, { n, 0 } };
        if( bgzf_inflate( b, table, text, whole, bstat ) )
            return 1;
    }
    TextFront t{ nullptr, n, text, stat, &b->txtOne };
    if( n && text_front_count( b, t ) )
        return 1;
    if( nMembers )
    {
        // read-back 1: the line feeds, the inflate's violation, the first and the last byte
        MA_HIP( hipMemcpyAsync( h, stat, ( TXT_WORDS + BGZ_WORDS ) * 8, hipMemcpyDeviceToHost, b->stream ) );
        if( batch_wait( b ) )
            return 1;
        bgzf_time( b );
        const unsigned long long* const hb = h + TXT_WORDS;
        if( hb[ BGZ_VIOLATION ] != ma_bgzf::NO_VIOLATION )
        {
            const u64 member = hb[ BGZ_VIOLATION ] >> 8;
            return bgzf_refuse( member, table[ member ].uiIn, (u32)( hb[ BGZ_VIOLATION ] & 0xffu ) );
        }
        t.first = n ? (char)hb[ BGZ_FIRST ] : '\0', t.last = n ? (char)hb[ BGZ_LAST ] : '\0';
    }
    else if( n ) // the head alone: the host has both bytes, but the line feeds are on the device
    {
        MA_HIP( hipMemcpyAsync( h, stat, 8, hipMemcpyDeviceToHost, b->stream ) );
        if( batch_wait( b ) )
            return 1;
        t.first = head[ 0 ], t.last = head[ n - 1 ];
    }
    if( n == 0 )
        return text_empty( b );
    if( t.first != '@' && t.first != '>' )
        return text_refuse( 0, 0, ma_text::ERR_KIND, "ma_batch_set_reads_bgzf: text" );
    t.kind = text_kind( t.first );
    t.feeds = h[ TXT_FEEDS ];
    // (a refused text, or more than the batch holds: nothing is written, the batch stays as text_no_reads left it)
    return text_single_rest( b, t, h, "ma_batch_set_reads_bgzf", "ma_batch_set_reads_bgzf: text", n_reads );
}
} // extern "C"
