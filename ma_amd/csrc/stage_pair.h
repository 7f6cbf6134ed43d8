// stage_pair.h -- PairedReads::execute (pairedReads.cpp:14-131) on the device: reads 2k and 2k+1 of a batch are the mates of
// pair k; one lane per pair picks one alignment of each mate out of the two MappingQuality lists k_finish left
// (k_pair_pick), then the picked records are packed in the layout of the C ABI (k_pair_pack).  The pick itself -- rate(),
// scan(), confidence() -- is the code of ma_amd/host/ma_pair_flat.h, the same the host runs.  Textually part of pipeline.hip.
//
// A pair needs its candidates in memory only when several of them share the best (key, proper): then the reference's
// result is whatever libstdc++'s unstable std::sort over ALL candidates puts first, and the lane sorts them in LDS
// (ss::sort_upto32).  PAIR_TIE_CAP candidates of 16 bytes per lane are 32 KB per block of 64 lanes; a tied pair with more
// is left to the host (k_pair_pick lists it, ma_pair_batch finishes it with the same header: gather -> pick -> apply).
enum : u32
{
    PAIR_TIE_CAP = 32
};

struct PairParams
{
    ma_pair::Params P;
    u32 n_pairs;
};

// the MappingQuality list of one read as a list of ma_pair_flat.h
struct PairDevList
{
    const AlnHeader* hdr; // of the read's first harmonized set
    const u32* order; // MappingQuality order of the read
    const u64* pool;
    u32 n;
    __device__ __forceinline__ u32 size( ) const
    {
        return n;
    }
    __device__ __forceinline__ const AlnHeader& at( u32 k ) const
    {
        return hdr[ order[ k ] ];
    }
    __device__ __forceinline__ i64 score( u32 k ) const
    {
        return at( k ).score;
    }
    __device__ __forceinline__ u64 begin( u32 k ) const
    {
        return at( k ).begin_ref;
    }
    __device__ __forceinline__ bool nonzero( u32 k ) const // Alignment::length() != 0: the sum of the op lengths
    {
        const AlnHeader& h = at( k );
        for( u32 o = 0; o < h.n_ops; o++ )
            if( op_len( pool[ h.ops_off + o ] ) != 0 )
                return true;
        return false;
    }
    __device__ __forceinline__ u32 seeds( u32 k ) const
    {
        const AlnHeader& h = at( k );
        u32 c = 0;
        for( u32 o = 0; o < h.n_ops; o++ )
            c += op_type( pool[ h.ops_off + o ] ) == MT_SEED ? 1u : 0u;
        return c;
    }
    __device__ __forceinline__ u64 opsOf( u32 k ) const
    {
        return at( k ).n_ops;
    }
};

struct PairKernelArgs
{
    PairParams pp;
    const u64* hset_off;
    const u64* roff;
    const AlnHeader* hdr;
    const u64* pool;
    const u32* mq_order;
    const u32* mq_cnt;
    ma_pair::Pick* pick; // per pair
    u64* cnt; // per pair: records, ops of the records (the sizes k_pair_pack's offsets are scanned from)
    u64* nops;
    u32* over; // pairs left to the host, in no particular order (CTR_PAIR_OVER of them)
    unsigned long long* ctr;
};

__device__ __forceinline__ PairDevList pair_list( const PairKernelArgs& A, u32 r )
{
    const u64 b = A.hset_off[ r ];
    return PairDevList{ A.hdr + b, A.mq_order + b, A.pool, A.mq_cnt[ r ] };
}
// records and ops a pick stands for
__device__ __forceinline__ void pair_sizes( const ma_pair::Pick& p, const PairDevList& a, const PairDevList& b, u64& c, u64& o )
{
    c = o = 0;
    if( p.kind == ma_pair::PICKED )
        c = 2, o = a.opsOf( p.i ) + b.opsOf( p.j );
    else if( p.kind == ma_pair::FIRST_LIST || p.kind == ma_pair::SECOND_LIST )
    {
        const PairDevList l = p.kind == ma_pair::FIRST_LIST ? a : b; // (a copy: a reference would pin both lists in memory)
        c = l.n;
        for( u32 k = 0; k < l.n; k++ )
            o += l.opsOf( k );
    }
}

__global__ void __launch_bounds__( 64 ) k_pair_pick( PairKernelArgs A )
{
    __shared__ ma_pair::Cand tie[ 64 ][ PAIR_TIE_CAP ];
    const u32 k = blockIdx.x * 64 + threadIdx.x;
    u64 c = 0, o = 0;
    if( k < A.pp.n_pairs )
    {
        const PairDevList a = pair_list( A, 2 * k ), b = pair_list( A, 2 * k + 1 );
        const u64 l1 = A.roff[ 2 * k + 1 ] - A.roff[ 2 * k ], l2 = A.roff[ 2 * k + 2 ] - A.roff[ 2 * k + 1 ];
        ma_pair::Scan s;
        ma_pair::Pick p = ma_pair::pickUntied( a, b, A.pp.P, l1, l2, s );
        if( p.kind == ma_pair::TIED_UNSORTED && s.nCand <= PAIR_TIE_CAP )
        {
            ma_pair::Cand* v = tie[ threadIdx.x ];
            ma_pair::fill( a, b, A.pp.P, v );
            ss::sort_upto32( v, (i64)s.nCand, ma_pair::Before( ) );
            p = ma_pair::confidence( a, b, A.pp.P, v[ 0 ], v[ 0 ].key, s.nCand, l1, l2 );
        }
        if( p.kind == ma_pair::TIED_UNSORTED )
            A.over[ atomicAdd( &A.ctr[ CTR_PAIR_OVER ], 1ull ) ] = k; // (at most n_pairs entries)
        else if( p.kind == ma_pair::NO_CANDIDATE )
            atomicAdd( &A.ctr[ CTR_PAIR_ERR ], 1ull );
        pair_sizes( p, a, b, c, o );
        A.pick[ k ] = p;
        A.cnt[ k ] = c;
        A.nops[ k ] = o;
    }
    const u64 cw = wave_sum_u64( c ), ow = wave_sum_u64( o );
    if( threadIdx.x == 0 && cw )
    {
        atomicAdd( &A.ctr[ CTR_PAIR_RECS ], (unsigned long long)cw );
        atomicAdd( &A.ctr[ CTR_PAIR_OPS ], (unsigned long long)ow );
    }
}

// ---- the pairs left to the host: what ma_pair_flat.h's pick reads of every alignment of both lists, one lane per pair
struct PairCompact
{
    i64 score;
    u64 begin;
    u32 nonzero, seeds;
};
__global__ void k_pair_gather( PairKernelArgs A, u32 n_over, const u64* out_off, PairCompact* out )
{
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if( t >= n_over )
        return;
    const u32 k = A.over[ t ];
    u64 w = out_off[ t ];
    for( u32 m = 0; m < 2; m++ )
    {
        const PairDevList l = pair_list( A, 2 * k + m );
        for( u32 i = 0; i < l.n; i++ )
            out[ w++ ] = PairCompact{ l.score( i ), l.begin( i ), l.nonzero( i ) ? 1u : 0u, l.seeds( i ) };
    }
}
__global__ void k_pair_apply( PairKernelArgs A, u32 n_over, const ma_pair::Pick* picks )
{
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if( t >= n_over )
        return;
    const u32 k = A.over[ t ];
    const ma_pair::Pick p = picks[ t ];
    u64 c, o;
    pair_sizes( p, pair_list( A, 2 * k ), pair_list( A, 2 * k + 1 ), c, o );
    A.pick[ k ] = p;
    A.cnt[ k ] = c;
    A.nops[ k ] = o;
    atomicAdd( &A.ctr[ CTR_PAIR_RECS ], (unsigned long long)c );
    atomicAdd( &A.ctr[ CTR_PAIR_OPS ], (unsigned long long)o );
}

// ---- the records of every pair in the layout of the C ABI (cf. k_aln_pack): pair k's records at alns[ rec_off[ k ] .. ),
// their ops as (type, length) pairs from ops_off[ k ] on; mate = the dump's bFirst, other = the partner's index in the pair
__device__ __forceinline__ void pair_emit( const AlnHeader& h, const u64* pool, u64 slot, u64& po, bool picked, const ma_pair::Pick& p,
                                           i32 mateV, i32 otherV, ma_alignment* alns, u64* ops, i32* mate, i32* other )
{
    ma_alignment a;
    a.begin_ref = (i64)h.begin_ref;
    a.end_ref = (i64)h.end_ref;
    a.begin_q = (i64)h.begin_q;
    a.end_q = (i64)h.end_q;
    a.score = h.score;
    a.soc_index = h.soc_index;
    a.n_ops = h.n_ops;
    a.ops_off = po;
    a.secondary = picked ? 0 : h.secondary;
    a.supplementary = picked ? 0 : h.supplementary;
    a.mapq = picked && p.set_mapq ? p.mapq : h.mapq;
    alns[ slot ] = a;
    mate[ slot ] = mateV;
    other[ slot ] = otherV;
    for( u32 j = 0; j < h.n_ops; j++ )
    {
        const u64 o = pool[ h.ops_off + j ];
        ops[ 2 * ( po + j ) ] = op_type( o );
        ops[ 2 * ( po + j ) + 1 ] = op_len( o );
    }
    po += h.n_ops;
}
__global__ void k_pair_pack( PairKernelArgs A, const u64* rec_off, const u64* ops_off, ma_alignment* alns, u64* ops, i32* mate,
                             i32* other )
{
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if( k >= A.pp.n_pairs )
        return;
    const ma_pair::Pick p = A.pick[ k ];
    const PairDevList a = pair_list( A, 2 * k ), b = pair_list( A, 2 * k + 1 );
    const u64 ro = rec_off[ k ];
    u64 po = ops_off[ k ];
    if( p.kind == ma_pair::PICKED )
    {
        pair_emit( a.at( p.i ), A.pool, ro, po, true, p, 1, 1, alns, ops, mate, other );
        pair_emit( b.at( p.j ), A.pool, ro + 1, po, true, p, 0, 0, alns, ops, mate, other );
    }
    else if( p.kind == ma_pair::FIRST_LIST || p.kind == ma_pair::SECOND_LIST )
    {
        const bool first = p.kind == ma_pair::FIRST_LIST;
        const PairDevList l = first ? a : b;
        for( u32 i = 0; i < l.n; i++ )
            pair_emit( l.at( i ), A.pool, ro + i, po, false, p, first ? 1 : 0, -1, alns, ops, mate, other );
    }
}
