// stage_sam.h -- the single-end SAM records of a batch as text, formatted on the device: the bytes FileWriter::execute
// (ma_amd/host/ma_sam.h, the yardstick) makes of the downloaded MappingQuality records, i.e. those of the reference's
// FileWriter::execute (fileWriter.cpp:11-158).  The record layout is ma_sam::formatRead of ma_amd/host/ma_sam_dev.h, the code
// the CPU tests pin to the goldens; the kernels only supply its sinks.  Textually part of pipeline.hip.
//   k_sam_size   one lane per read: formatRead over the counting sink -> the read's byte count (scanned into offsets by the
//                launcher) and the errors (a record that ends beyond its read)
//   k_sam_write  per wavefront, for its 64 reads: (1) one lane per read writes the short columns -- QNAME .. TLEN, the cigar,
//                the tabs, a CG tag -- and notes where SEQ goes; (2) all 64 lanes walk the records of the 64 reads together and
//                copy SEQ (code -> letter, reverse-complemented on the reverse strand) and QUAL with lanes striding over
//                bytes: coalesced stores for the ~80 % of a short read's record that these two columns are.
// Both kernels are templates over Tags: with MA_SAM_NGMLR_TAGS the read's lane also writes the tags (ma_sam::putNgmlrTags: MD SV
// AS NM XI XE XR CV SA QS QE) in phase (1), behind the place it leaves for QUAL, reading the reference's bases from the index's
// pac and the runs of N from the index's holes (ma_index_set_holes); phase (2) is the same.  The instantiations without tags
// hold the code they held before there were tags.
// No arrays indexed at run time, decimal numbers by digit count (ma_sam::WriteSink::number).

// the MappingQuality list of one read as a list of ma_sam_dev.h
struct SamDevList
{
    const AlnHeader* hdr; // of the read's first harmonized set
    const u32* order; // MappingQuality order of the read
    const u64* pool;
    u32 n;
    __device__ __forceinline__ u32 size( ) const
    {
        return n;
    }
    __device__ __forceinline__ ma_sam::Rec rec( u32 k ) const
    {
        const AlnHeader& h = hdr[ order[ k ] ];
        return ma_sam::Rec{ h.begin_ref, h.end_ref, h.begin_q, h.end_q, h.n_ops, h.secondary, h.supplementary, h.mapq, h.score };
    }
    __device__ __forceinline__ u64 opType( u32 k, u32 j ) const
    {
        return op_type( pool[ hdr[ order[ k ] ].ops_off + j ] );
    }
    __device__ __forceinline__ u64 opLen( u32 k, u32 j ) const
    {
        return op_len( pool[ hdr[ order[ k ] ].ops_off + j ] );
    }
};

enum : int // the statistics of a SAM text, of this stage and of stage_pair_sam.h
{
    SAM_STAT_BYTES = 0, // bytes of the batch's text (the launcher copies the scan's last offset here)
    SAM_STAT_ERRORS = 1, // records that end beyond their read (paired: their mate)
    SAM_STAT_FIRST = 2, // the first of them in the batch's order, as the stage's count sink writes it (with tags: the slot times
                        // 4 plus the error's kind less one, so that the first kind of the first record is kept)
    SAM_STAT_COUNT = 4
};

struct SamKernelArgs
{
    ma_sam::Contigs contigs;
    u32 options;
    u32 n_reads;
    const u64* hset_off;
    const u64* roff;
    const uint8_t* reads;
    const AlnHeader* hdr;
    const u64* pool;
    const u32* mq_order;
    const u32* mq_cnt;
    const char* names; // QNAME strings, CSR
    const u64* name_off;
    const uint8_t* qual; // one character per base in the reads' CSR, or null
    u64* cnt; // per read: bytes of its records
    const u64* off; // their exclusive scan (k_sam_write)
    u64* seq_pos; // per slot hset_off[ r ] + k: where SEQ of record k starts in the text, ~0 for a record that is not printed
    char* text;
    unsigned long long* stat;
    ma_sam::Ref ref; // the tags' reference bases and holes: the index's pac, its holes, the forward strand's size
};

__device__ __forceinline__ SamDevList sam_list( const SamKernelArgs& A, u32 r )
{
    const u32 c = A.mq_cnt[ r ]; // (0 for every read of a batch without harmonized sets: hset_off is not read then)
    const u64 b = c ? A.hset_off[ r ] : 0;
    return SamDevList{ A.hdr + b, A.mq_order + b, A.pool, c };
}
__device__ __forceinline__ ma_sam::Read sam_read( const SamKernelArgs& A, u32 r )
{
    const u64 o = A.roff[ r ], no = A.name_off[ r ];
    return ma_sam::Read{ A.names + no, A.name_off[ r + 1 ] - no, A.reads + o, A.qual ? A.qual + o : nullptr, A.roff[ r + 1 ] - o };
}

// the counting sink, with the errors going to the batch's statistics: the records that end beyond their read, and as
// SAM_STAT_FIRST the first of them in read order, the slot hset_off[ read ] + index in the read's list
struct SamCountSink : ma_sam::CountSink
{
    unsigned long long* stat;
    u64 slot0;
    __device__ __forceinline__ void error( u32, i64, u32 k )
    {
        atomicAdd( &stat[ SAM_STAT_ERRORS ], 1ull );
        atomicMin( &stat[ SAM_STAT_FIRST ], (unsigned long long)( slot0 + k ) );
    }
};

// the same for records with tags, which can fail in four ways: slot and kind go into SAM_STAT_FIRST together
struct SamTagCountSink : ma_sam::CountSink
{
    unsigned long long* stat;
    u64 slot0;
    __device__ __forceinline__ void error( u32 kind, i64, u32 k )
    {
        atomicAdd( &stat[ SAM_STAT_ERRORS ], 1ull );
        atomicMin( &stat[ SAM_STAT_FIRST ], (unsigned long long)( ( ( slot0 + k ) << 2 ) | ( kind - 1 ) ) );
    }
};

template <bool Tags> __global__ void __launch_bounds__( 256 ) k_sam_size( SamKernelArgs A )
{
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if( r >= A.n_reads )
        return;
    const SamDevList l = sam_list( A, r );
    if constexpr( Tags )
    {
        SamTagCountSink s;
        s.stat = A.stat;
        s.slot0 = l.n ? A.hset_off[ r ] : 0;
        ma_sam::formatRead( s, A.options, A.contigs, sam_read( A, r ), l, A.ref );
        A.cnt[ r ] = s.n;
    }
    else
    {
        SamCountSink s;
        s.stat = A.stat;
        s.slot0 = l.n ? A.hset_off[ r ] : 0;
        ma_sam::formatRead( s, A.options, A.contigs, sam_read( A, r ), l );
        A.cnt[ r ] = s.n;
    }
}

// the short columns: everything but the bytes of SEQ and QUAL, whose places are noted for the wavefront
struct SamColumnSink : ma_sam::WriteSink
{
    u64* seq_pos; // of the read's first slot
    u64 unmapped_seq; // where SEQ of the unmapped record starts (relative to the read's text), ~0: no such record
    __device__ __forceinline__ void seq( const ma_sam::Read&, u64 uiFrom, u64 uiTo, bool, u32 k )
    {
        if( k == ma_sam::UNMAPPED )
            unmapped_seq = n;
        else
            seq_pos[ k ] = n;
        n += uiTo - uiFrom;
    }
    __device__ __forceinline__ void qual( const ma_sam::Read&, u64 uiFrom, u64 uiTo, u32 )
    {
        n += uiTo - uiFrom;
    }
};

// SEQ and QUAL of one record by the whole wavefront (all arguments wave-uniform): text[ pos .. ) = the letters of
// codes[ from, to ), reverse-complemented when rev; behind it and a tab, qual[ qfrom, qto )
__device__ __forceinline__ void sam_copy_record( char* text, u64 pos, const uint8_t* codes, const uint8_t* qual, u64 from, u64 to, bool rev,
                                                 u64 qfrom, u64 qto, u32 lane )
{
    const u64 ns = to - from;
    if( rev )
        for( u64 i = lane; i < ns; i += 64 )
            text[ pos + i ] = ma_sam::complementChar( codes[ to - 1 - i ] );
    else
        for( u64 i = lane; i < ns; i += 64 )
            text[ pos + i ] = ma_sam::baseChar( codes[ from + i ] );
    if( qual && qfrom < qto )
        for( u64 i = lane; i < qto - qfrom; i += 64 )
            text[ pos + ns + 1 + i ] = (char)qual[ qfrom + i ];
}

__device__ __forceinline__ u64 sam_bcast( u64 v, u32 src )
{
    return ( (u64)(u32)__shfl( (int)( v >> 32 ), (int)src, 64 ) << 32 ) | (u32)__shfl( (int)(u32)v, (int)src, 64 );
}

template <bool Tags> __global__ void __launch_bounds__( 256 ) k_sam_write( SamKernelArgs A )
{
    const u32 lane = threadIdx.x & 63;
    const u32 r0 = blockIdx.x * 256 + ( threadIdx.x & ~63u ); // first read of this wavefront
    const u32 r = r0 + lane;
    // (1) one lane per read
    u64 out = 0, unm = ~0ull;
    u32 c = 0;
    if( r < A.n_reads )
    {
        const SamDevList l = sam_list( A, r );
        out = A.off[ r ];
        c = l.n;
        SamColumnSink s;
        s.p = A.text + out;
        s.n = 0;
        s.seq_pos = A.seq_pos + ( c ? A.hset_off[ r ] : 0 );
        s.unmapped_seq = ~0ull;
        for( u32 k = 0; k < c; k++ )
            s.seq_pos[ k ] = ~0ull;
        if constexpr( Tags )
            ma_sam::formatRead( s, A.options, A.contigs, sam_read( A, r ), l, A.ref );
        else
            ma_sam::formatRead( s, A.options, A.contigs, sam_read( A, r ), l );
        unm = s.unmapped_seq;
    }
    // seq_pos was written by other lanes of this wavefront.  The fence orders the stores before the loads below; that the
    // loads SEE them rests on the wavefront running in lockstep and on both going through the CU's vector L1 (global_store /
    // global_load).  A.seq_pos must therefore never become `const __restrict__` (nor be read through a pointer that is): the
    // compiler could then fetch it with scalar loads, whose cache does not see the vector stores of this kernel.
    __threadfence_block( );
    // (2) the wavefront walks the reads of its lanes; everything below is the same in all 64 lanes
    const u32 nw = r0 < A.n_reads ? ( A.n_reads - r0 < 64 ? A.n_reads - r0 : 64 ) : 0;
    const bool soft = ( A.options & ma_sam::SOFT_CLIP ) != 0;
    for( u32 t = 0; t < nw; t++ )
    {
        const u32 rt = r0 + t;
        const u64 outT = sam_bcast( out, t ), unmT = sam_bcast( unm, t );
        const u32 cT = (u32)__shfl( (int)c, (int)t, 64 );
        const u64 ro = A.roff[ rt ], len = A.roff[ rt + 1 ] - ro;
        const uint8_t* codes = A.reads + ro;
        const uint8_t* qual = A.qual ? A.qual + ro : nullptr;
        if( unmT != ~0ull )
            sam_copy_record( A.text + outT, unmT, codes, qual, 0, len, false, 0, len, lane );
        if( cT == 0 )
            continue;
        const u64 b = A.hset_off[ rt ];
        const u64 F = A.contigs.forwardSize( );
        for( u32 k = 0; k < cT; k++ )
        {
            const u64 pos = A.seq_pos[ b + k ];
            if( pos == ~0ull )
                continue;
            const AlnHeader& h = A.hdr[ b + A.mq_order[ b + k ] ];
            // what putRecord of ma_sam_dev.h handed to seq( ) / qual( ): both ranges clamped to the read
            const u64 from = soft ? 0 : h.begin_q, to = soft ? len : ( h.end_q < len ? h.end_q : len );
            const u64 qto = h.end_q < len ? h.end_q : len;
            sam_copy_record( A.text + outT, pos, codes, qual, from, to, h.begin_ref >= F, h.begin_q, qto, lane );
        }
    }
}

// ---- diagnostics: the tags' XI (kind 0: num / den) or CV (kind 1: 100 * num / den) arithmetic and "%f" formatter as the
// kernels run them (ma_sam::putRatio), one pair per lane into a 0-padded slot of 16 bytes.  A text that would not fit its slot
// (a quotient of 10^8 and more) leaves the slot empty.
__global__ void __launch_bounds__( 256 ) k_ngmlr_float_probe( int kind, const u64* num, const u64* den, u64 n, char* out )
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if( i >= n )
        return;
    ma_sam::CountSink c;
    ma_sam::detail::putRatio( c, kind != 0, num[ i ], den[ i ] );
    ma_sam::WriteSink w{ out + 16 * i };
    if( c.n <= 15 )
        ma_sam::detail::putRatio( w, kind != 0, num[ i ], den[ i ] );
    for( u64 j = w.n; j < 16; j++ )
        out[ 16 * i + j ] = 0;
}
