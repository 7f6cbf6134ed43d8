// launch_mates_bgzf.h -- ma_batch_set_mates_bgzf and ma_batch_get_mates_rest: the two BGZF-compressed read files of a paired-end
// run inflated on the device, then ma_batch_set_mates_text's parse.  Textually part of pipeline.hip; the rules and the order of
// the refusals are in ma_amd/host/ma_mates_bgzf_dev.h, the walk and the inflate in launch_bgzf.h, the parse in launch_text.h.
//
// The host walks the headers of both chains into ONE member table, text 1's members in front of text 2's, and both chains are
// inflated by ONE k_bgzf_inflate launch (and one k_bgzf_crc): a member is decoded by one lane and a launch lasts as long as its
// slowest lane, so two launches one after the other would cost twice what one over both tables costs.  A violation's key is
// its index in the joint table, so the lowest one is text 1's if text 1 has any.  Text 2 goes behind text 1 in txtIn at a
// 256-byte aligned offset -- behind ALL that text 1's members inflate to, the bytes the call drops included, because both
// texts are written at the same time.  k_text_count of each text runs right behind the inflate.  TWO read-backs:
//   1  the line feeds of both texts, the inflate's lowest violation, the first and last byte of both texts -- in one copy
//   2  the mates statistics (text_mates_rest, as ma_batch_set_mates_text's second)
// Both texts stay in txtIn until the batch gets other reads: ma_batch_get_mates_rest copies what lies beyond the last pair.

static int mates_bgzf_refuse( u32 text, u64 member, u64 byte, u32 reason )
{
    char msg[ 320 ];
    ma_bgzf::messageMates( msg, sizeof( msg ), text, member, byte, reason );
    return fail( msg );
}
static int mates_bgzf_refuse_drop( u32 text )
{
    char msg[ 160 ];
    ma_bgzf::messageMatesDrop( msg, sizeof( msg ), text );
    return fail( msg );
}

extern "C" {

int ma_batch_set_mates_bgzf( ma_batch* b, const ma_bgzf_text side[ 2 ], int32_t rev_comp_mates, uint64_t* n_pairs, uint64_t text_bytes[ 2 ],
                             uint64_t consumed[ 2 ] )
{
    static const char* const WHO = "ma_batch_set_mates_bgzf";
    if( !b || !side || ( side[ 0 ].n_head && !side[ 0 ].head ) || ( side[ 0 ].n_bytes && !side[ 0 ].members ) || ( side[ 1 ].n_head && !side[ 1 ].head ) ||
        ( side[ 1 ].n_bytes && !side[ 1 ].members ) )
        return fail( "ma_batch_set_mates_bgzf: null argument" );
    MA_BIND_DEVICE( b->device );
    if( n_pairs )
        *n_pairs = 0;
    if( consumed )
        consumed[ 0 ] = consumed[ 1 ] = 0;
    if( text_bytes )
        text_bytes[ 0 ] = text_bytes[ 1 ] = 0;
    if( text_no_reads( b ) )
        return 1;
    // the joint member table, headers only: where a text starts in txtIn (at) and a chain in bgzIn (dataAt)
    const uint8_t* const data[ 2 ] = { static_cast<const uint8_t*>( side[ 0 ].members ), static_cast<const uint8_t*>( side[ 1 ].members ) };
    const u64 dataAt[ 2 ] = { 0, ( side[ 0 ].n_bytes + 63 ) & ~(u64)63 };
    std::vector<ma_bgzf::Member> table;
    u64 at[ 2 ] = { 0, 0 }, inflated[ 2 ], first[ 2 ]; // first: a chain's first member in the table
    for( int i = 0; i < 2; i++ )
    {
        u64 badAt = 0;
        first[ i ] = table.size( );
        at[ i ] = i ? ( side[ 0 ].n_head + inflated[ 0 ] + 255 ) & ~(u64)255 : 0;
        const u32 bad = bgzf_walk( data[ i ], side[ i ].n_bytes, dataAt[ i ], at[ i ] + side[ i ].n_head, table, &inflated[ i ], &badAt );
        if( bad != ma_bgzf::OK )
            return batch_wait( b ) || mates_bgzf_refuse( i + 1, table.size( ) - first[ i ], badAt, bad );
    }
    // a drop that is too large is refused BEHIND the members' verdict: that text is inflated and checked, and not parsed
    const bool dropBad[ 2 ] = { side[ 0 ].n_drop > inflated[ 0 ], side[ 1 ].n_drop > inflated[ 1 ] };
    u64 n[ 2 ];
    for( int i = 0; i < 2; i++ )
        n[ i ] = dropBad[ i ] ? 0 : side[ i ].n_head + inflated[ i ] - side[ i ].n_drop;
    for( int i = 0; i < 2; i++ )
        if( n[ i ] > ma_text::MAX_TEXT_BYTES )
            return batch_wait( b ) || mates_refuse( WHO, ma_text::MATES_LINE, i + 1, 0, 0, ma_text::ERR_TOO_LARGE );
    const u64 nMembers = table.size( ), nStat = 2 * TXT_WORDS + MT_WORDS + BGZ_WORDS;
    if( b->txtNameOff.reserve( ( b->max_reads + 1 ) * 8 ) || b->txtIn.reserve( at[ 1 ] + side[ 1 ].n_head + inflated[ 1 ] + 64 ) ||
        b->txtStat.reserve( nStat * 8 ) )
        return 1;
    MA_HIP( hipMemsetAsync( b->txtNameOff.p, 0, 8, b->stream ) );
    unsigned long long* const stat = b->txtStat.as<unsigned long long>( );
    unsigned long long* const bstat = stat + 2 * TXT_WORDS + MT_WORDS;
    MA_HIP( hipMemsetAsync( stat, 0, nStat * 8, b->stream ) );
    char* const text = b->txtIn.as<char>( );
    for( int i = 0; i < 2; i++ )
        if( side[ i ].n_head )
            MA_HIP( hipMemcpyAsync( text + at[ i ], side[ i ].head, side[ i ].n_head, hipMemcpyHostToDevice, b->stream ) );
    if( nMembers )
    {
        if( b->bgzIn.reserve( dataAt[ 1 ] + side[ 1 ].n_bytes + 64 ) )
            return 1;
        for( int i = 0; i < 2; i++ )
            if( side[ i ].n_bytes )
                MA_HIP( hipMemcpyAsync( b->bgzIn.as<uint8_t>( ) + dataAt[ i ], data[ i ], side[ i ].n_bytes, hipMemcpyHostToDevice, b->stream ) );
        const BgzfWhole whole = { { reinterpret_cast<const uint8_t*>( text ), reinterpret_cast<const uint8_t*>( text + at[ 1 ] ) }, { n[ 0 ], n[ 1 ] } };
        if( bgzf_inflate( b, table, text, whole, bstat ) )
            return 1;
    }
    TextFront t[ 2 ] = { { nullptr, n[ 0 ], text, stat, &b->txtOne }, { nullptr, n[ 1 ], text + at[ 1 ], stat + TXT_WORDS, &b->txtMate } };
    for( int i = 0; i < 2; i++ )
    {
        t[ i ].kind = 0, t[ i ].nBlocks = t[ i ].feeds = t[ i ].lines = 0;
        t[ i ].first = t[ i ].last = '\0';
        if( n[ i ] && text_front_count( b, t[ i ] ) )
            return 1;
    }
    unsigned long long h[ 2 * TXT_WORDS + MT_WORDS + BGZ_WORDS ];
    if( nMembers || n[ 0 ] || n[ 1 ] )
    {
        // read-back 1: the line feeds of both texts, the inflate's violation, the first and last byte of both texts
        MA_HIP( hipMemcpyAsync( h, stat, nStat * 8, hipMemcpyDeviceToHost, b->stream ) );
        if( batch_wait( b ) )
            return 1;
    }
    if( nMembers )
    {
        bgzf_time( b );
        const unsigned long long* const hb = h + 2 * TXT_WORDS + MT_WORDS;
        if( hb[ BGZ_VIOLATION ] != ma_bgzf::NO_VIOLATION )
        {
            const u64 member = hb[ BGZ_VIOLATION ] >> 8;
            const int i = member >= first[ 1 ] ? 1 : 0;
            return mates_bgzf_refuse( i + 1, member - first[ i ], table[ member ].uiIn, (u32)( hb[ BGZ_VIOLATION ] & 0xffu ) );
        }
        for( int i = 0; i < 2; i++ )
            if( n[ i ] )
                t[ i ].first = (char)hb[ BGZ_FIRST + 2 * i ], t[ i ].last = (char)hb[ BGZ_LAST + 2 * i ];
    }
    else // heads alone: the host has the bytes
        for( int i = 0; i < 2; i++ )
            if( n[ i ] )
                t[ i ].first = side[ i ].head[ 0 ], t[ i ].last = side[ i ].head[ n[ i ] - 1 ];
    for( int i = 0; i < 2; i++ )
        if( dropBad[ i ] )
            return mates_bgzf_refuse_drop( i + 1 );
    // from here on ma_batch_set_mates_text on ( T_1, T_2 ): a text of neither kind is not parsed -- text 1's refuses the call
    // at once, text 2's after text 1 was validated
    u64 hostKey[ 2 ];
    for( int i = 0; i < 2; i++ )
        hostKey[ i ] = n[ i ] && t[ i ].first != '@' && t[ i ].first != '>' ? ma_text::key( 0, ma_text::ERR_KIND ) : ma_text::NO_VIOLATION;
    if( hostKey[ 0 ] != ma_text::NO_VIOLATION )
        return mates_refuse( WHO, ma_text::MATES_LINE, 1, 0, 0, ma_text::ERR_KIND );
    const bool parsed[ 2 ] = { n[ 0 ] > 0, n[ 1 ] > 0 && hostKey[ 1 ] == ma_text::NO_VIOLATION };
    for( int i = 0; i < 2; i++ )
        if( parsed[ i ] )
            t[ i ].kind = text_kind( t[ i ].first );
    uint64_t pairs = 0, used[ 2 ] = { 0, 0 };
    const int refused = text_mates_rest( b, t, parsed, hostKey, h, rev_comp_mates, WHO, &pairs, used );
    if( n_pairs )
        *n_pairs = pairs; // (after "batch capacity exceeded": what a caller sizes the next batch object by)
    if( refused )
        return 1;
    const u64 restAt[ 2 ] = { at[ 0 ] + used[ 0 ], at[ 1 ] + used[ 1 ] }, restBytes[ 2 ] = { n[ 0 ] - used[ 0 ], n[ 1 ] - used[ 1 ] };
    b->st.keepMatesRest( restAt, restBytes );
    for( int i = 0; i < 2; i++ )
    {
        if( consumed )
            consumed[ i ] = used[ i ];
        if( text_bytes )
            text_bytes[ i ] = n[ i ];
    }
    return 0;
}

int ma_batch_get_mates_rest( ma_batch* b, int32_t which, uint64_t* n_bytes, char* out )
{
    if( !b || ( which != 0 && which != 1 ) )
        return fail( "ma_batch_get_mates_rest: null batch, or which is neither 0 nor 1" );
    if( !b->st.matesRest )
        return fail( "ma_batch_get_mates_rest: run ma_batch_set_mates_bgzf first" );
    if( n_bytes )
        *n_bytes = b->st.restBytes[ which ];
    if( !out || !b->st.restBytes[ which ] )
        return 0;
    MA_BIND_DEVICE( b->device );
    MA_HIP( hipMemcpyAsync( out, b->txtIn.as<char>( ) + b->st.restAt[ which ], b->st.restBytes[ which ], hipMemcpyDeviceToHost, b->stream ) );
    return batch_wait( b );
}
} // extern "C"
