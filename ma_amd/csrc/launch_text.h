// launch_text.h -- ma_batch_set_reads_text, ma_batch_set_mates_text and the getters of a batch's reads and read text.  Textually
// part of pipeline.hip; the kernels are in stage_text.h, the rules in ma_amd/host/ma_text_dev.h.

// the batch holds no reads and no text (what a failed ma_batch_set_reads_text leaves, and what it starts from)
static int text_no_reads( ma_batch* b )
{
    b->n_reads = b->n_bases = 0;
    b->max_qlen = 0;
    batch_own_reads( b );
    b->st.newReads( );
    MA_HIP( hipMemsetAsync( b->roff.p, 0, 8, b->stream ) );
    return 0;
}

// an empty text (behind text_no_reads and the first name offset): no reads, with names -- none
static int text_empty( ma_batch* b )
{
    if( batch_wait( b ) )
        return 1;
    b->st.finish( ma_state::NAMES );
    return 0;
}

// who: the words in front of "line <L> ..." ("ma_batch_set_reads_text", "ma_batch_set_reads_bgzf: text")
static int text_refuse( u64 line, u64 byte, u32 reason, const char* who = "ma_batch_set_reads_text" )
{
    char msg[ 256 ];
    ma_text::messageOf( msg, sizeof( msg ), who, line, byte, reason );
    return fail( msg );
}
// who: the call's name ("ma_batch_set_mates_text", "ma_batch_set_mates_bgzf")
static int mates_refuse( const char* who, u32 refusal, u32 text, u64 line, u64 byte, u32 reason )
{
    char msg[ 256 ];
    ma_text::messageMatesOf( msg, sizeof( msg ), who, refusal, text, line, byte, reason );
    return fail( msg );
}

// what the host sees of a text without parsing it: NO_VIOLATION, or the refusal at line 0
static u64 text_host_key( const char* text, u64 n )
{
    if( n > ma_text::MAX_TEXT_BYTES )
        return ma_text::key( 0, ma_text::ERR_TOO_LARGE );
    if( n && text[ 0 ] != '@' && text[ 0 ] != '>' )
        return ma_text::key( 0, ma_text::ERR_KIND );
    return ma_text::NO_VIOLATION;
}

// The front of a parse, k_text_count .. k_text_records, of ONE text of n > 0 bytes on scratch of its own: both entry points run
// it, ma_batch_set_mates_text once per text.  text_front_count uploads and counts, the caller reads the line feeds back
// (stat[ TXT_FEEDS ]) and sets `feeds`, text_front_lines does the per-line work.  A text that is on the device already
// (ma_batch_set_reads_bgzf inflates it there) has no `host`: nothing is uploaded, and the caller sets `first`, `last` and `kind`
// behind the read-back that brings the two bytes with the line feeds.
struct TextFront
{
    const char* host; // NULL: the text is in `dev` already
    u64 n;
    char* dev; // 256-byte aligned, inside b->txtIn
    unsigned long long* stat; // TXT_WORDS words inside b->txtStat
    ma_batch::TextScratch* scratch;
    u32 kind;
    u64 nBlocks, feeds, lines;
    char first, last; // the text's first and last byte
};
static u32 text_kind( char first )
{
    return first == '@' ? ma_text::KIND_FASTQ : ma_text::KIND_FASTA;
}
static int text_front_count( ma_batch* b, TextFront& t )
{
    t.nBlocks = ( t.n + TEXT_BLOCK_BYTES - 1 ) / TEXT_BLOCK_BYTES;
    if( t.scratch->block.reserve( ( t.nBlocks + 1 ) * 4 ) )
        return 1;
    if( t.host )
    {
        t.first = t.host[ 0 ], t.last = t.host[ t.n - 1 ];
        t.kind = text_kind( t.first );
        MA_HIP( hipMemcpyAsync( t.dev, t.host, t.n, hipMemcpyHostToDevice, b->stream ) );
    }
    MA_HIP( hipMemsetAsync( t.stat, 0, TXT_WORDS * 8, b->stream ) );
    MA_HIP( hipMemsetAsync( t.stat + TXT_LONE_CR, 0xff, 2 * 8, b->stream ) ); // TXT_LONE_CR, TXT_VIOLATION: none
    hipLaunchKernelGGL( k_text_count, dim3( (unsigned)t.nBlocks ), dim3( TEXT_BLOCK ), 0, b->stream, t.dev, t.n, t.scratch->block.as<u32>( ), t.stat );
    MA_HIP( hipGetLastError( ) );
    return 0;
}
static TextSide text_side( const TextFront& t, u64 hostKey )
{
    TextSide s;
    s.text = t.dev;
    s.n = t.n, s.lines = t.lines;
    s.start = t.scratch->start.as<u32>( );
    s.hdrName = t.scratch->hdrName.as<u64>( );
    s.bases = t.scratch->bases.as<u32>( );
    s.recLine = t.scratch->recLine.as<u32>( );
    s.stat = t.stat;
    s.hostKey = hostKey;
    return s;
}
static int text_front_lines( ma_batch* b, TextFront& t )
{
    ma_batch::TextScratch& S = *t.scratch;
    t.lines = ma_text::nLines( t.feeds, t.last );
    const u64 lines = t.lines;
    if( S.start.reserve( ( lines + 2 ) * 4 ) || S.hdrName.reserve( ( lines + 2 ) * 8 ) || S.bases.reserve( ( lines + 2 ) * 4 ) ||
        S.recLine.reserve( ( lines + 2 ) * 4 ) )
        return 1;
    if( scan_exclusive<u32>( b, S.block.as<u32>( ), S.block.as<u32>( ), t.nBlocks ) )
        return 1;
    const dim3 textGrid( (unsigned)t.nBlocks ), textBlock( TEXT_BLOCK );
    hipLaunchKernelGGL( k_text_lines, textGrid, textBlock, 0, b->stream, t.dev, t.n, S.block.as<u32>( ), t.feeds, S.start.as<u32>( ) );
    const dim3 lineGrid( (unsigned)( ( lines + 1 + 255 ) / 256 ) ), lineBlock( 256 );
    hipLaunchKernelGGL( k_text_classify, lineGrid, lineBlock, 0, b->stream, t.kind, t.dev, S.start.as<u32>( ), lines, t.stat, S.hdrName.as<u64>( ),
                        S.bases.as<u32>( ) );
    MA_HIP( hipGetLastError( ) );
    if( scan_exclusive<u64>( b, S.hdrName.as<u64>( ), S.hdrName.as<u64>( ), lines + 1 ) ||
        scan_exclusive<u32>( b, S.bases.as<u32>( ), S.bases.as<u32>( ), lines + 1 ) )
        return 1;
    hipLaunchKernelGGL( k_text_rec_lines, lineGrid, lineBlock, 0, b->stream, lines, S.hdrName.as<u64>( ), S.recLine.as<u32>( ) );
    hipLaunchKernelGGL( k_text_records, dim3( (unsigned)std::min<u64>( 256, ( lines + 255 ) / 256 ) ), lineBlock, 0, b->stream, t.kind, lines,
                        S.hdrName.as<u64>( ), S.bases.as<u32>( ), S.recLine.as<u32>( ), t.stat );
    MA_HIP( hipGetLastError( ) );
    return 0;
}

// The rest of a single text's parse behind the read-back of its line feeds (t.feeds is set): the per-line kernels, k_text_stat,
// k_text_emit, the read-back of the statistics into h (TXT_WORDS words) and the batch's new state.  who / whoText: the call's
// name, and the words in front of "line <L> ..." in a refusal.
static int text_single_rest( ma_batch* b, TextFront& t, unsigned long long* h, const char* who, const char* whoText, uint64_t* n_reads )
{
    const u64 n = t.n;
    unsigned long long* const stat = t.stat;
    if( b->txtNames.reserve( n + 1 ) || ( t.kind == ma_text::KIND_FASTQ && b->txtQual.reserve( b->max_bases + 1 ) ) || text_front_lines( b, t ) )
        return 1;
    const TextSide s = text_side( t, ma_text::NO_VIOLATION );
    hipLaunchKernelGGL( k_text_stat, dim3( 1 ), dim3( 1 ), 0, b->stream, t.lines, s.hdrName, s.bases, s.start, b->max_reads, b->max_bases, stat );
    TextEmitArgs A;
    A.kind = t.kind;
    A.text = t.dev;
    A.n = n, A.lines = t.lines;
    A.start = s.start;
    A.hdrName = s.hdrName;
    A.bases = s.bases;
    A.stat = stat;
    A.roff = b->roff.as<u64>( );
    A.codes = b->reads.as<uint8_t>( );
    A.nameOff = b->txtNameOff.as<u64>( );
    A.names = b->txtNames.as<char>( );
    A.qual = t.kind == ma_text::KIND_FASTQ ? b->txtQual.as<uint8_t>( ) : nullptr;
    hipLaunchKernelGGL( k_text_emit, dim3( (unsigned)t.nBlocks ), dim3( TEXT_BLOCK ), 0, b->stream, A );
    MA_HIP( hipGetLastError( ) );
    // the last read-back: reads, bases, name bytes, the longest read, the refusal
    MA_HIP( hipMemcpyAsync( h, stat, TXT_WORDS * 8, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    if( h[ TXT_VIOLATION ] != ma_text::NO_VIOLATION )
        return text_refuse( h[ TXT_VIOLATION ] >> 8, h[ TXT_BYTE ], (u32)( h[ TXT_VIOLATION ] & 0xffu ), whoText );
    if( !h[ TXT_EMIT ] )
    {
        if( n_reads )
            *n_reads = h[ TXT_READS ]; // (what a caller sizes the next batch object by)
        return fail( std::string( who ) + ": batch capacity exceeded" );
    }
    b->n_reads = h[ TXT_READS ];
    b->n_bases = h[ TXT_BASES ];
    b->max_qlen = (u32)h[ TXT_MAX_LEN ];
    b->st.nameBytes = h[ TXT_NAME_BYTES ];
    b->st.hasQual = t.kind == ma_text::KIND_FASTQ;
    b->st.finish( ma_state::NAMES );
    if( n_reads )
        *n_reads = b->n_reads;
    return 0;
}

static int text_mates_rest( ma_batch* b, TextFront t[ 2 ], const bool parsed[ 2 ], const u64 hostKey[ 2 ], unsigned long long* h, int32_t rev_comp_mates,
                            const char* who, uint64_t* n_pairs, uint64_t consumed[ 2 ] ); // (behind ma_batch_set_mates_text)

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
    const u64 hostKey = text_host_key( text, n );
    if( hostKey != ma_text::NO_VIOLATION )
        return batch_wait( b ) || text_refuse( 0, 0, (u32)( hostKey & 0xffu ) );
    if( b->txtNameOff.reserve( ( b->max_reads + 1 ) * 8 ) )
        return 1;
    MA_HIP( hipMemsetAsync( b->txtNameOff.p, 0, 8, b->stream ) );
    if( n == 0 )
        return text_empty( b );
    if( b->txtIn.reserve( n + 64 ) || b->txtStat.reserve( TXT_WORDS * 8 ) )
        return 1;
    unsigned long long* const stat = b->txtStat.as<unsigned long long>( );
    unsigned long long h[ TXT_WORDS ];
    TextFront t{ text, n, b->txtIn.as<char>( ), stat, &b->txtOne };
    if( text_front_count( b, t ) )
        return 1;
    // read-back 1: the number of lines sizes the per-line scratch and launches
    MA_HIP( hipMemcpyAsync( h, stat, 8, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    t.feeds = h[ TXT_FEEDS ];
    return text_single_rest( b, t, h, "ma_batch_set_reads_text", "ma_batch_set_reads_text", n_reads );
}

int ma_batch_set_mates_text( ma_batch* b, const char* text1, uint64_t n1, const char* text2, uint64_t n2, int32_t rev_comp_mates,
                             uint64_t* n_pairs, uint64_t consumed[ 2 ] )
{
    if( !b || ( n1 && !text1 ) || ( n2 && !text2 ) )
        return fail( "ma_batch_set_mates_text: null argument" );
    MA_BIND_DEVICE( b->device );
    if( n_pairs )
        *n_pairs = 0;
    if( consumed )
        consumed[ 0 ] = consumed[ 1 ] = 0;
    if( text_no_reads( b ) )
        return 1;
    // A text the host refuses at its first byte, or an empty one, is not parsed: it has no records, so there are no pairs, but
    // the other text is validated all the same (a violation in text 1 wins over text 2's)
    const u64 hostKey[ 2 ] = { text_host_key( text1, n1 ), text_host_key( text2, n2 ) };
    if( hostKey[ 0 ] != ma_text::NO_VIOLATION )
        return batch_wait( b ) || mates_refuse( "ma_batch_set_mates_text", ma_text::MATES_LINE, 1, 0, 0, (u32)( hostKey[ 0 ] & 0xffu ) );
    const bool parsed[ 2 ] = { n1 > 0, n2 > 0 && hostKey[ 1 ] == ma_text::NO_VIOLATION };
    const u64 at2 = ( n1 + 255 ) & ~(u64)255; // text 2 behind text 1 in the one upload buffer
    if( b->txtNameOff.reserve( ( b->max_reads + 1 ) * 8 ) || b->txtIn.reserve( at2 + ( parsed[ 1 ] ? n2 : 0 ) + 64 ) ||
        b->txtStat.reserve( ( 2 * TXT_WORDS + MT_WORDS ) * 8 ) )
        return 1;
    MA_HIP( hipMemsetAsync( b->txtNameOff.p, 0, 8, b->stream ) );
    unsigned long long* const stat = b->txtStat.as<unsigned long long>( );
    unsigned long long* const mstat = stat + 2 * TXT_WORDS;
    MA_HIP( hipMemsetAsync( stat, 0, ( 2 * TXT_WORDS + MT_WORDS ) * 8, b->stream ) );
    TextFront t[ 2 ] = { { text1, n1, b->txtIn.as<char>( ), stat, &b->txtOne }, { text2, n2, b->txtIn.as<char>( ) + at2, stat + TXT_WORDS, &b->txtMate } };
    for( int i = 0; i < 2; i++ )
    {
        t[ i ].kind = 0, t[ i ].nBlocks = t[ i ].feeds = t[ i ].lines = 0;
        if( parsed[ i ] && text_front_count( b, t[ i ] ) )
            return 1;
    }
    unsigned long long h[ 2 * TXT_WORDS + MT_WORDS ];
    if( parsed[ 0 ] || parsed[ 1 ] )
    {
        // read-back 1: the line feeds of both texts, in one copy
        MA_HIP( hipMemcpyAsync( h, stat, ( TXT_WORDS + 1 ) * 8, hipMemcpyDeviceToHost, b->stream ) );
        if( batch_wait( b ) )
            return 1;
    }
    return text_mates_rest( b, t, parsed, hostKey, h, rev_comp_mates, "ma_batch_set_mates_text", n_pairs, consumed );
}
} // extern "C"

// The rest of a parse of two texts behind the read-back of their line feeds into h (h[ i * TXT_WORDS + TXT_FEEDS ]; kind, first
// and last of a parsed text are set): the per-line kernels of each text, k_text_mates_plan / _stat / _emit, the read-back of the
// mates statistics into h and the batch's new state.  parsed / hostKey: as ma_batch_set_mates_text decides them; the statistics
// are the 2 * TXT_WORDS + MT_WORDS words at the front of b->txtStat; who: the call's name in a refusal.  The TXT_* words of a
// text that is NOT parsed are not read here or by the mates kernels (its hostKey or its emptiness speaks for it), and they
// differ by caller: all zero from ma_batch_set_mates_text, which never counts such a text, and k_text_count's from
// ma_batch_set_mates_bgzf, which counts every text before it knows the first byte.
static int text_mates_rest( ma_batch* b, TextFront t[ 2 ], const bool parsed[ 2 ], const u64 hostKey[ 2 ], unsigned long long* h, int32_t rev_comp_mates,
                            const char* who, uint64_t* n_pairs, uint64_t consumed[ 2 ] )
{
    unsigned long long* const mstat = b->txtStat.as<unsigned long long>( ) + 2 * TXT_WORDS;
    const u64 n1 = t[ 0 ].n, n2 = t[ 1 ].n;
    u64 most = ~0ull; // pairs at most: a FASTQ record has four lines, a FASTA record two or more
    for( int i = 0; i < 2; i++ )
    {
        if( !parsed[ i ] )
        {
            most = 0;
            continue;
        }
        t[ i ].feeds = h[ i * TXT_WORDS + TXT_FEEDS ];
        if( text_front_lines( b, t[ i ] ) )
            return 1;
        most = std::min<u64>( most, t[ i ].kind == ma_text::KIND_FASTQ ? ( t[ i ].lines + 3 ) / 4 : ( t[ i ].lines + 1 ) / 2 );
    }
    const bool fastq = parsed[ 0 ] && parsed[ 1 ] && t[ 0 ].kind == ma_text::KIND_FASTQ && t[ 1 ].kind == ma_text::KIND_FASTQ;
    const u32 kindsDiffer = parsed[ 0 ] && parsed[ 1 ] && t[ 0 ].kind != t[ 1 ].kind ? 1 : 0;
    if( b->txtNames.reserve( n1 + n2 + 1 ) || ( fastq && b->txtQual.reserve( b->max_bases + 1 ) ) )
        return 1;
    const TextSide side[ 2 ] = { text_side( t[ 0 ], hostKey[ 0 ] ), text_side( t[ 1 ], hostKey[ 1 ] ) };
    u64* const roff = b->roff.as<u64>( );
    u64* const nameOff = b->txtNameOff.as<u64>( );
    if( most > 0 )
    {
        // lengths of the interleaved reads, 0 behind the last pair; never more entries than the batch's arrays hold
        const u64 entries = std::min<u64>( b->max_reads, 2 * most ) + 1;
        hipLaunchKernelGGL( k_text_mates_plan, dim3( (unsigned)( ( ( entries + 1 ) / 2 + 255 ) / 256 ) ), dim3( 256 ), 0, b->stream, side[ 0 ], side[ 1 ],
                            entries, b->max_reads, roff, nameOff, mstat );
        MA_HIP( hipGetLastError( ) );
        if( scan_exclusive<u64>( b, roff, roff, entries ) || scan_exclusive<u64>( b, nameOff, nameOff, entries ) )
            return 1;
    }
    hipLaunchKernelGGL( k_text_mates_stat, dim3( 1 ), dim3( 1 ), 0, b->stream, side[ 0 ], side[ 1 ], kindsDiffer, b->max_reads, b->max_bases, roff,
                        nameOff, mstat );
    if( most > 0 && !kindsDiffer )
    {
        MatesEmitArgs A;
        A.kind = t[ 0 ].kind;
        A.revComp = rev_comp_mates != 0 ? 1 : 0;
        A.mstat = mstat;
        A.roff = roff;
        A.nameOff = nameOff;
        A.codes = b->reads.as<uint8_t>( );
        A.names = b->txtNames.as<char>( );
        A.qual = fastq ? b->txtQual.as<uint8_t>( ) : nullptr;
        A.s = side[ 0 ];
        hipLaunchKernelGGL( k_text_mates_emit<0>, dim3( (unsigned)t[ 0 ].nBlocks ), dim3( TEXT_BLOCK ), 0, b->stream, A );
        A.s = side[ 1 ];
        hipLaunchKernelGGL( k_text_mates_emit<1>, dim3( (unsigned)t[ 1 ].nBlocks ), dim3( TEXT_BLOCK ), 0, b->stream, A );
    }
    MA_HIP( hipGetLastError( ) );
    // read-back 2: pairs, sums, the longest read, the consumed bytes, the refusal
    MA_HIP( hipMemcpyAsync( h, mstat, MT_WORDS * 8, hipMemcpyDeviceToHost, b->stream ) );
    if( batch_wait( b ) )
        return 1;
    if( h[ MT_REFUSAL ] != ma_text::MATES_OK )
    {
        if( text_no_reads( b ) || batch_wait( b ) ) // (the offset arrays hold the plan's sums)
            return 1;
        if( h[ MT_REFUSAL ] == ma_text::MATES_CAPACITY && n_pairs )
            *n_pairs = h[ MT_PAIRS ]; // (what a caller sizes the next batch object by)
        return mates_refuse( who, (u32)h[ MT_REFUSAL ], (u32)h[ MT_TEXT ], h[ MT_VIOLATION ] >> 8, h[ MT_BYTE ], (u32)( h[ MT_VIOLATION ] & 0xffu ) );
    }
    b->n_reads = 2 * h[ MT_PAIRS ];
    b->n_bases = h[ MT_BASES ];
    b->max_qlen = (u32)h[ MT_MAX_LEN ];
    b->st.nameBytes = h[ MT_NAME_BYTES ];
    b->st.hasQual = fastq;
    b->st.finish( ma_state::NAMES );
    if( n_pairs )
        *n_pairs = h[ MT_PAIRS ];
    if( consumed )
        consumed[ 0 ] = h[ MT_CONSUMED ], consumed[ 1 ] = h[ MT_CONSUMED + 1 ];
    return 0;
}

extern "C" {

int ma_batch_read_counts( ma_batch* b, uint64_t* n_reads, uint64_t* n_bases, uint64_t* n_name_bytes, int32_t* has_qual )
{
    if( !b )
        return fail( "ma_batch_read_counts: null batch" );
    if( n_reads )
        *n_reads = b->d_roff ? b->n_reads : 0;
    if( n_bases )
        *n_bases = b->d_roff ? b->n_bases : 0;
    if( n_name_bytes )
        *n_name_bytes = b->st.has( ma_state::NAMES ) ? b->st.nameBytes : 0;
    if( has_qual )
        *has_qual = b->st.has( ma_state::NAMES ) && b->st.hasQual ? 1 : 0;
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
    if( !b || !b->d_roff || !b->st.has( ma_state::NAMES ) )
        return fail( "ma_batch_get_read_text: the reads have no names (ma_batch_set_read_text or ma_batch_set_reads_text)" );
    if( qual && !b->st.hasQual )
        return fail( "ma_batch_get_read_text: the reads have no qualities" );
    MA_BIND_DEVICE( b->device );
    if( name_off )
        MA_HIP( hipMemcpyAsync( name_off, b->txtNameOff.p, ( b->n_reads + 1 ) * 8, hipMemcpyDeviceToHost, b->stream ) );
    if( names && b->st.nameBytes )
        MA_HIP( hipMemcpyAsync( names, b->txtNames.p, b->st.nameBytes, hipMemcpyDeviceToHost, b->stream ) );
    if( qual && b->n_bases )
        MA_HIP( hipMemcpyAsync( qual, b->txtQual.p, b->n_bases, hipMemcpyDeviceToHost, b->stream ) );
    return batch_wait( b );
}
} // extern "C"
