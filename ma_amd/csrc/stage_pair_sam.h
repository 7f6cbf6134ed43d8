// stage_pair_sam.h -- the paired-end SAM records of a batch as text, formatted on the device: the bytes PairedFileWriter::execute
// (ma_amd/host/ma_sam.h, the yardstick) makes of the downloaded pair records, i.e. those of the reference's
// PairedFileWriter::execute (fileWriter.cpp:158-383).  The record layout is ma_sam::formatPair of ma_amd/host/ma_sam_dev.h, the code the CPU tests pin to
// the goldens; the kernels only supply its pair list and its sinks.  Nothing is packed: the records are read where k_finish
// left them, through the picks of k_pair_pick, with the overrides k_pair_pack would apply.  Textually part of pipeline.hip.
//   k_pair_sam_size   one lane per pair: formatPair over the counting sink -> the pair's byte count (scanned into offsets by
//                     the launcher) and the errors (a record that ends beyond its own mate)
//   k_pair_sam_write  per wavefront, for its 64 pairs, in the two phases of k_sam_write (stage_sam.h): (1) one lane per pair
//                     writes the short columns and notes where SEQ goes; (2) all 64 lanes copy SEQ and QUAL of every record
//                     of the 64 pairs together.
// No arrays indexed at run time.

// the records of one pair in the order of ma_batch_get_pairs, as a pair list of ma_sam_dev.h
struct PairSamDevList
{
    const AlnHeader* hdr; // PICKED: of the first mate's first harmonized set; a whole list: of that mate's
    const AlnHeader* hdr2; // PICKED: of the second mate's
    const u32* order; // MappingQuality order, as hdr
    const u32* order2;
    const u64* pool;
    u32 n; // records
    u32 i, j; // PICKED: the picked records of the two lists
    bool picked, first; // a whole list: of the first mate
    bool set_mapq;
    double mapq;
    __device__ __forceinline__ u32 size( ) const
    {
        return n;
    }
    // index into the mate's MappingQuality order / whether record k is the second mate's of a picked pair
    __device__ __forceinline__ const AlnHeader& at( u32 k ) const
    {
        const bool second = picked && k != 0;
        const AlnHeader* h = second ? hdr2 : hdr;
        const u32* o = second ? order2 : order;
        return h[ o[ picked ? ( k ? j : i ) : k ] ];
    }
    __device__ __forceinline__ ma_sam::Rec rec( u32 k ) const
    {
        const AlnHeader& h = at( k );
        return ma_sam::Rec{ h.begin_ref,
                            h.end_ref,
                            h.begin_q,
                            h.end_q,
                            h.n_ops,
                            picked ? 0u : (u32)h.secondary,
                            picked ? 0u : (u32)h.supplementary,
                            picked && set_mapq ? mapq : h.mapq };
    }
    __device__ __forceinline__ u64 opType( u32 k, u32 o ) const
    {
        return op_type( pool[ at( k ).ops_off + o ] );
    }
    __device__ __forceinline__ u64 opLen( u32 k, u32 o ) const
    {
        return op_len( pool[ at( k ).ops_off + o ] );
    }
    __device__ __forceinline__ i32 mate( u32 k ) const // as pair_emit's callers (stage_pair.h)
    {
        return picked ? ( k ? 0 : 1 ) : ( first ? 1 : 0 );
    }
    __device__ __forceinline__ i32 other( u32 k ) const
    {
        return picked ? ( k ? 0 : 1 ) : -1;
    }
};

struct PairSamKernelArgs
{
    ma_sam::Contigs contigs;
    u32 options;
    u32 n_pairs;
    u32 picks_valid; // 0: a batch without harmonized sets -- ma_pair_batch launched nothing, every pair is "both unaligned"
    const u64* hset_off;
    const u64* roff;
    const uint8_t* reads;
    const AlnHeader* hdr;
    const u64* pool;
    const u32* mq_order;
    const u32* mq_cnt;
    const ma_pair::Pick* pick;
    const char* names; // QNAME strings, CSR
    const u64* name_off;
    const uint8_t* qual; // one character per base in the reads' CSR, or null
    u64* cnt; // per pair: bytes of its records
    const u64* off; // their exclusive scan (k_pair_sam_write)
    u64* seq_pos; // per header slot hset_off[ read ] + index in the read's MappingQuality order: where SEQ of that record starts
                  // in the pair's text, ~0 for a record that is not printed
    char* text;
    unsigned long long* stat;
};

// slot0 / slot1: the seq_pos slots of record 0 (records k: slot0 + k for a whole list) and of record 1 of a picked pair
__device__ __forceinline__ PairSamDevList pair_sam_list( const PairSamKernelArgs& A, u32 k, u64& slot0, u64& slot1 )
{
    PairSamDevList l;
    l.hdr = l.hdr2 = A.hdr;
    l.order = l.order2 = A.mq_order;
    l.pool = A.pool;
    l.n = l.i = l.j = 0;
    l.picked = l.first = l.set_mapq = false;
    l.mapq = 0.0;
    slot0 = slot1 = 0;
    if( !A.picks_valid )
        return l;
    const ma_pair::Pick p = A.pick[ k ];
    const u64 b1 = A.hset_off[ 2 * k ], b2 = A.hset_off[ 2 * k + 1 ];
    const u32 c1 = A.mq_cnt[ 2 * k ], c2 = A.mq_cnt[ 2 * k + 1 ];
    if( p.kind == ma_pair::PICKED && p.i < c1 && p.j < c2 )
    {
        l.hdr = A.hdr + b1, l.order = A.mq_order + b1;
        l.hdr2 = A.hdr + b2, l.order2 = A.mq_order + b2;
        l.n = 2, l.i = p.i, l.j = p.j;
        l.picked = true;
        l.set_mapq = p.set_mapq != 0;
        l.mapq = p.mapq;
        slot0 = b1 + p.i, slot1 = b2 + p.j;
    }
    else if( p.kind == ma_pair::FIRST_LIST || p.kind == ma_pair::SECOND_LIST )
    {
        l.first = p.kind == ma_pair::FIRST_LIST;
        const u64 b = l.first ? b1 : b2;
        l.hdr = A.hdr + b, l.order = A.mq_order + b;
        l.n = l.first ? c1 : c2;
        slot0 = b;
    }
    return l;
}
__device__ __forceinline__ ma_sam::Read pair_sam_read( const PairSamKernelArgs& A, u32 r )
{
    const u64 o = A.roff[ r ], no = A.name_off[ r ], len = A.roff[ r + 1 ] - o;
    // an empty mate has no quality string (the host layer's NucSeq::xQuality is empty then): its QUAL is "*" as without qualities
    return ma_sam::Read{ A.names + no, A.name_off[ r + 1 ] - no, A.reads + o, A.qual && len ? A.qual + o : nullptr, len };
}

// the counting sink, with the errors going to the batch's statistics (SAM_STAT_* of stage_sam.h): the records that end beyond
// their mate, and as SAM_STAT_FIRST the first of them in pair order, pair << 32 | index in the pair's records
struct PairSamCountSink : ma_sam::CountSink
{
    unsigned long long* stat;
    u64 pair;
    __device__ __forceinline__ void error( u32, i64, u32 k )
    {
        atomicAdd( &stat[ SAM_STAT_ERRORS ], 1ull );
        atomicMin( &stat[ SAM_STAT_FIRST ], (unsigned long long)( ( pair << 32 ) | k ) );
    }
};

__global__ void __launch_bounds__( 256 ) k_pair_sam_size( PairSamKernelArgs A )
{
    const u32 k = blockIdx.x * 256 + threadIdx.x;
    if( k >= A.n_pairs )
        return;
    u64 s0, s1;
    const PairSamDevList l = pair_sam_list( A, k, s0, s1 );
    PairSamCountSink s;
    s.stat = A.stat;
    s.pair = k;
    ma_sam::formatPair( s, A.options, A.contigs, pair_sam_read( A, 2 * k ), pair_sam_read( A, 2 * k + 1 ), l );
    A.cnt[ k ] = s.n;
}

// the short columns: everything but the bytes of SEQ and QUAL, whose places are noted for the wavefront
struct PairSamColumnSink : ma_sam::WriteSink
{
    u64* seq_pos;
    u64 slot0, slot1;
    bool picked;
    u64 unmapped_seq1, unmapped_seq2; // where SEQ of the first / second mate's unaligned record starts (relative to the pair's
                                      // text), ~0: no such record, or one of an empty mate (nothing to copy)
    u32 unmapped_qual; // bit 0 / 1: QUAL of the first / second mate's unaligned record is printed (behind its SEQ)
    __device__ __forceinline__ void seq( const ma_sam::Read&, u64 uiFrom, u64 uiTo, bool, u32 k )
    {
        if( k == ma_sam::UNMAPPED_FIRST )
            unmapped_seq1 = n;
        else if( k == ma_sam::UNMAPPED_SECOND )
            unmapped_seq2 = n;
        else
            seq_pos[ picked ? ( k ? slot1 : slot0 ) : slot0 + k ] = n;
        n += uiTo - uiFrom;
    }
    __device__ __forceinline__ void qual( const ma_sam::Read&, u64 uiFrom, u64 uiTo, u32 k )
    {
        if( k == ma_sam::UNMAPPED_FIRST )
            unmapped_qual |= 1u;
        else if( k == ma_sam::UNMAPPED_SECOND )
            unmapped_qual |= 2u;
        n += uiTo - uiFrom;
    }
};

__global__ void __launch_bounds__( 256 ) k_pair_sam_write( PairSamKernelArgs A )
{
    const u32 lane = threadIdx.x & 63;
    const u32 k0 = blockIdx.x * 256 + ( threadIdx.x & ~63u ); // first pair of this wavefront
    const u32 k = k0 + lane;
    // (1) one lane per pair
    u64 out = 0, unm1 = ~0ull, unm2 = ~0ull;
    u32 unmq = 0;
    if( k < A.n_pairs )
    {
        PairSamColumnSink s;
        const PairSamDevList l = pair_sam_list( A, k, s.slot0, s.slot1 );
        out = A.off[ k ];
        s.p = A.text + out;
        s.n = 0;
        s.seq_pos = A.seq_pos;
        s.picked = l.picked;
        s.unmapped_seq1 = s.unmapped_seq2 = ~0ull;
        s.unmapped_qual = 0;
        for( u32 r = 0; r < l.n; r++ )
            A.seq_pos[ l.picked ? ( r ? s.slot1 : s.slot0 ) : s.slot0 + r ] = ~0ull;
        ma_sam::formatPair( s, A.options, A.contigs, pair_sam_read( A, 2 * k ), pair_sam_read( A, 2 * k + 1 ), l );
        unm1 = s.unmapped_seq1, unm2 = s.unmapped_seq2;
        unmq = s.unmapped_qual;
    }
    // seq_pos was written by other lanes of this wavefront: see k_sam_write (stage_sam.h) for what the loads below rest on.
    // A.seq_pos must never become `const __restrict__` (nor be read through a pointer that is).
    __threadfence_block( );
    // (2) the wavefront walks the pairs of its lanes; everything below is the same in all 64 lanes
    const u32 nw = k0 < A.n_pairs ? ( A.n_pairs - k0 < 64 ? A.n_pairs - k0 : 64 ) : 0;
    const bool soft = ( A.options & ma_sam::SOFT_CLIP ) != 0;
    const u64 F = A.contigs.forwardSize( );
    for( u32 t = 0; t < nw; t++ )
    {
        const u32 kt = k0 + t;
        const u64 outT = sam_bcast( out, t ), unm1T = sam_bcast( unm1, t ), unm2T = sam_bcast( unm2, t );
        const u64 ro1 = A.roff[ 2 * kt ], ro2 = A.roff[ 2 * kt + 1 ], len1 = ro2 - ro1, len2 = A.roff[ 2 * kt + 2 ] - ro2;
        // the unaligned records: whether QUAL is printed behind SEQ -- only in a pair without any record, and the other mate
        // may be empty there -- is what phase 1 saw (the "*" of the one-mate-unaligned record was written there)
        const u32 unmqT = (u32)__shfl( (int)unmq, (int)t, 64 );
        if( unm1T != ~0ull )
            sam_copy_record( A.text + outT, unm1T, A.reads + ro1, ( unmqT & 1u ) ? A.qual + ro1 : nullptr, 0, len1, false, 0, len1, lane );
        if( unm2T != ~0ull )
            sam_copy_record( A.text + outT, unm2T, A.reads + ro2, ( unmqT & 2u ) ? A.qual + ro2 : nullptr, 0, len2, false, 0, len2, lane );
        u64 s0, s1;
        const PairSamDevList l = pair_sam_list( A, kt, s0, s1 );
        for( u32 r = 0; r < l.n; r++ )
        {
            const u64 pos = A.seq_pos[ l.picked ? ( r ? s1 : s0 ) : s0 + r ];
            if( pos == ~0ull )
                continue;
            const AlnHeader& h = l.at( r );
            // what putRecord of ma_sam_dev.h handed to seq( ) / qual( ): both ranges clamped to the record's OWN mate
            const bool firstMate = l.mate( r ) != 0;
            const u64 ro = firstMate ? ro1 : ro2, len = firstMate ? len1 : len2;
            const u64 from = soft ? 0 : h.begin_q, to = soft ? len : ( h.end_q < len ? h.end_q : len );
            const u64 qto = h.end_q < len ? h.end_q : len;
            sam_copy_record( A.text + outT, pos, A.reads + ro, A.qual ? A.qual + ro : nullptr, from, to, h.begin_ref >= F, h.begin_q, qto, lane );
        }
    }
}
