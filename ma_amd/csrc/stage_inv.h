// stage_inv.h -- "Detect Small Inversions" (SmallInversions::execute, smallInversions.h:22-221) for a whole batch on the
// device: what the host module ma_amd::SmallInversions (ma_amd/host/ma_modules.h, the yardstick) makes of the MappingQuality
// lists.  The record logic is ma_inv::scanDrops / stretchJob / assemble / place of ma_amd/host/ma_inv_dev.h, the code the CPU
// tests pin to the reference's dumps; the kernels supply the lists, the bookkeeping and the bounds.  Textually part of pipeline.hip.
//   k_inv_scan      one lane per (read, record of its MappingQuality list).  Pass one counts the record's drop stretches, the
//                   bytes of their windows and the ops their records can need, and checks them against the read and the text;
//                   a scan over the block and one atomic per block and quantity give the block's candidates their places; pass
//                   two walks the record again and writes each candidate -- (read, record, stretch), its ma_ksw_job, its
//                   window's bases from the index's packed text -- in list order.  Nothing is written beyond the capacities the
//                   launcher passes; the totals tell it when they were too small.
//   k_inv_assemble  one lane per candidate: cigar -> ops behind the end of the batch's ops pool through aln_append (nw.h),
//                   the score filter, the record's header.  Candidates are few (5 of 276 lists of the f4 golden) and an M run
//                   is a few hundred bases at most: a lane per candidate keeps the append chain where it is serial anyway.
//   k_inv_merge     one lane per read: the final list -- every parent's header in MappingQuality order, each kept inversion
//                   directly behind its parent, several under one parent in stretch order (pRet of smallInversions.h:185-207).
// No arrays indexed at run time; every walk is bounded by n_ops, every index by the read's length or the text's size.

enum : int // the statistics of one ma_inversions_batch
{
    INV_STAT_CAND = 0, // drop stretches found
    INV_STAT_WIN = 1, // bytes of their windows
    INV_STAT_OPS = 2, // words of ops their records can need
    INV_STAT_ERRORS = 3, // stretches that end beyond their read or whose window is not inside one strand of the text
    INV_STAT_FIRST = 4, // the first of them: slot << 2 | ma_inv::ERR_*
    INV_STAT_JOBS = 5, // candidates with both sides non-empty
    INV_STAT_RECS = 6, // inversion records kept ...
    INV_STAT_REC_OPS = 7, // ... and their ops
    INV_STAT_SYMBOL = 8, // cigars with a symbol that is none of M I D
    INV_STAT_FLAGS = 9, // MA_ERR_* of the assembly (ops overflow: cannot happen within the bound)
    INV_STAT_COUNT = 16
};

struct InvCand
{
    u32 read, rec; // rec: index in the read's MappingQuality list
    ma_inv::Stretch s;
    u64 win_begin; // of its window on the doubled text
    u64 ops_off; // of its ops region, relative to the first one
    u32 ops_cap, kept;
};

struct InvKernelArgs
{
    IndexView X;
    ma_inv::Params P;
    NwParams NP;
    u32 n_reads;
    u64 n_slots;
    // the MappingQuality lists
    const u64* off;
    const AlnHeader* hdr;
    const u32* order;
    const u32* cnt;
    const u64* roff;
    const uint8_t* reads;
    u64* pool; // the ops pool; the inversions' ops go behind pool_used
    u64 pool_used;
    // candidates: per slot their number and the first one's index; per candidate its record, job, shape and window
    u32* slot_cnt;
    u64* slot_first;
    InvCand* cand;
    ma_ksw_job* jobs;
    i32* shapes; // qlen, tlen, w per candidate
    uint8_t* win;
    u64 cand_cap, win_cap, n_cand;
    unsigned long long* stat;
    // the DP results
    const ma_ez* ez;
    const u64* cig_off;
    const u32* cig_pool;
    // the final lists
    AlnHeader* inv_hdr; // per candidate
    u32* fin_cnt;
    const u64* fin_off;
    AlnHeader* fin_hdr;
    u32* fin_order;
};

// the slot's read: the last r with off[ r ] <= slot (reads without records share their offset with the next read)
__device__ __forceinline__ u32 inv_read_of_slot( const u64* off, u32 n_reads, u64 slot )
{
    u32 lo = 0, hi = n_reads; // off[ lo ] <= slot < off[ hi ]
    while( hi - lo > 1 )
    {
        const u32 mid = lo + ( hi - lo ) / 2;
        if( off[ mid ] <= slot )
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__( 256 ) k_inv_scan( InvKernelArgs A )
{
    typedef hipcub::BlockScan<unsigned long long, 256> Scan;
    __shared__ typename Scan::TempStorage tmp;
    __shared__ unsigned long long base[ 3 ];
    const u64 slot = (u64)blockIdx.x * 256 + threadIdx.x;
    u32 r = 0, k = 0;
    bool live = false;
    if( slot < A.n_slots )
    {
        r = inv_read_of_slot( A.off, A.n_reads, slot );
        k = (u32)( slot - A.off[ r ] );
        live = k < A.cnt[ r ];
    }
    const u64 b = live ? A.off[ r ] : 0;
    const SamDevList l{ A.hdr + b, A.order + b, A.pool, live ? A.cnt[ r ] : 0u };
    const u64 readLen = live ? A.roff[ r + 1 ] - A.roff[ r ] : 0;
    // pass one
    unsigned long long nCand = 0, nWin = 0, nOps = 0;
    u32 nJobs = 0, nBad = 0, firstBad = 0;
    if( live )
        ma_inv::scanDrops( A.P, l, k, [ & ]( const ma_inv::Stretch& s ) {
            ma_inv::Job j;
            const u32 e = ma_inv::stretchJob( A.P, s, readLen, A.X.n, A.X.F, j );
            if( e != ma_inv::OK )
            {
                if( nBad++ == 0 )
                    firstBad = e;
                return;
            }
            nCand++;
            nWin += (u64)j.tlen;
            nOps += ma_inv::opsBound( j );
            nJobs += j.hasDp( ) ? 1u : 0u;
        } );
    if( nBad )
    {
        atomicAdd( &A.stat[ INV_STAT_ERRORS ], (unsigned long long)nBad );
        atomicMin( &A.stat[ INV_STAT_FIRST ], (unsigned long long)( slot << 2 | firstBad ) );
        nCand = nWin = nOps = 0; // (the call fails: nothing of this record is written)
        nJobs = 0;
    }
    if( nJobs )
        atomicAdd( &A.stat[ INV_STAT_JOBS ], (unsigned long long)nJobs );
    // the block's candidates, window bytes and ops in list order; one atomic per block and quantity
    unsigned long long candAt, winAt, opsAt, total[ 3 ];
    Scan( tmp ).ExclusiveSum( nCand, candAt, total[ 0 ] );
    __syncthreads( );
    Scan( tmp ).ExclusiveSum( nWin, winAt, total[ 1 ] );
    __syncthreads( );
    Scan( tmp ).ExclusiveSum( nOps, opsAt, total[ 2 ] );
    if( threadIdx.x == 0 )
    {
        base[ 0 ] = total[ 0 ] ? atomicAdd( &A.stat[ INV_STAT_CAND ], total[ 0 ] ) : 0;
        base[ 1 ] = total[ 1 ] ? atomicAdd( &A.stat[ INV_STAT_WIN ], total[ 1 ] ) : 0;
        base[ 2 ] = total[ 2 ] ? atomicAdd( &A.stat[ INV_STAT_OPS ], total[ 2 ] ) : 0;
    }
    __syncthreads( );
    if( slot >= A.n_slots )
        return;
    candAt += base[ 0 ];
    winAt += base[ 1 ];
    opsAt += base[ 2 ];
    A.slot_cnt[ slot ] = (u32)nCand;
    A.slot_first[ slot ] = candAt;
    if( nCand == 0 )
        return;
    // pass two
    ma_inv::scanDrops( A.P, l, k, [ & ]( const ma_inv::Stretch& s ) {
        ma_inv::Job j;
        if( ma_inv::stretchJob( A.P, s, readLen, A.X.n, A.X.F, j ) != ma_inv::OK )
            return;
        const u64 c = candAt++, w = winAt, o = opsAt;
        winAt += (u64)j.tlen;
        opsAt += ma_inv::opsBound( j );
        if( c >= A.cand_cap || w + (u64)j.tlen > A.win_cap )
            return; // (the launcher sees the totals, grows and launches again)
        InvCand x;
        x.read = r;
        x.rec = k;
        x.s = s;
        x.win_begin = j.winBegin;
        x.ops_off = o;
        x.ops_cap = (u32)ma_inv::opsBound( j );
        x.kept = 0;
        A.cand[ c ] = x;
        ma_ksw_job kj;
        kj.qlen = j.qlen;
        kj.tlen = j.tlen;
        kj.w = j.w;
        kj.zdrop = j.zdrop;
        kj.flag = j.flag;
        kj.reserved = 0;
        kj.q_off = A.roff[ r ] + s.startQ; // into the batch's reads
        kj.t_off = w;
        A.jobs[ c ] = kj;
        A.shapes[ 3 * c ] = j.qlen;
        A.shapes[ 3 * c + 1 ] = j.tlen;
        A.shapes[ 3 * c + 2 ] = j.w;
        for( i32 i = 0; i < j.tlen; i++ ) // the bytes ma_pack_extract hands the host module (text_base: vExtractSubsection)
            A.win[ w + (u64)i ] = (uint8_t)text_base( A.X, j.winBegin + (u64)i );
    } );
}

// Alignment::append for ma_inv::assemble
struct InvBuilder
{
    const NwParams& P;
    AlnBuilder& A;
    __device__ __forceinline__ void append( u32 type, u64 size )
    {
        aln_append( P, A, type, size );
    }
};

__global__ void __launch_bounds__( 64 ) k_inv_assemble( InvKernelArgs A )
{
    const u64 c = (u64)blockIdx.x * 64 + threadIdx.x;
    if( c >= A.n_cand )
        return;
    const InvCand x = A.cand[ c ];
    const ma_ksw_job kj = A.jobs[ c ];
    ma_inv::Job j;
    j.winBegin = x.win_begin;
    j.winEnd = x.win_begin + (u64)kj.tlen;
    j.qlen = kj.qlen;
    j.tlen = kj.tlen;
    j.w = kj.w;
    j.zdrop = kj.zdrop;
    j.flag = kj.flag;
    AlnHeader h;
    h.begin_ref = h.end_ref = h.begin_q = h.end_q = 0;
    h.score = 0;
    h.length = 0;
    h.ops_off = A.pool_used + x.ops_off;
    h.n_ops = 0;
    h.ops_cap = x.ops_cap;
    h.soc_index = 0;
    h.secondary = h.supplementary = 0;
    h.mapq = 0;
    u32 err = 0;
    AlnBuilder ab;
    ab.h = &h;
    ab.ops = A.pool + h.ops_off;
    ab.err = &err;
    InvBuilder B{ A.NP, ab };
    // (a job without DP has no result record of its own: its cigar is empty)
    const u32 nCigar = j.hasDp( ) ? (u32)A.ez[ c ].n_cigar : 0u;
    const u32* cig = A.cig_pool + ( j.hasDp( ) ? A.cig_off[ c ] : 0 );
    const uint8_t* q = A.reads + kj.q_off;
    const uint8_t* t = A.win + kj.t_off;
    const u32 qlen = (u32)kj.qlen, tlen = (u32)kj.tlen;
    bool walked = true; // the cigar of a qlen x tlen job stays inside both: anything else is refused, not followed
    const bool ok = ma_inv::assemble(
        nCigar, [ & ]( u32 i ) { return cig[ i ]; },
        [ & ]( u64 i ) -> u32 {
            walked = walked && i < qlen;
            return i < qlen ? q[ i ] : 4u;
        },
        [ & ]( u64 i ) -> u32 {
            walked = walked && i < tlen;
            return i < tlen ? t[ i ] : 5u;
        },
        B );
    aln_flush( ab );
    if( !ok || !walked )
        atomicAdd( &A.stat[ INV_STAT_SYMBOL ], 1ull );
    if( err )
        atomicOr( &A.stat[ INV_STAT_FLAGS ], (unsigned long long)err );
    const bool keep = ok && walked && !err && ma_inv::kept( A.P, h.score );
    if( keep )
    {
        const u64 b = A.off[ x.read ];
        ma_inv::place( h, A.hdr[ b + A.order[ b + x.rec ] ], x.s, j );
        atomicAdd( &A.fin_cnt[ x.read ], 1u );
        atomicAdd( &A.stat[ INV_STAT_RECS ], 1ull );
        atomicAdd( &A.stat[ INV_STAT_REC_OPS ], (unsigned long long)h.n_ops );
    }
    A.inv_hdr[ c ] = h;
    A.cand[ c ].kept = keep ? 1u : 0u;
}

__global__ void __launch_bounds__( 256 ) k_inv_merge( InvKernelArgs A )
{
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if( r >= A.n_reads )
        return;
    const u32 n = A.cnt[ r ];
    const u64 b = n ? A.off[ r ] : 0, first = A.fin_off[ r ];
    u64 at = first;
    for( u32 k = 0; k < n; k++ )
    {
        A.fin_hdr[ at++ ] = A.hdr[ b + A.order[ b + k ] ];
        const u32 nc = A.slot_cnt[ b + k ];
        const u64 c0 = A.slot_first[ b + k ];
        for( u32 i = 0; i < nc; i++ )
            if( A.cand[ c0 + i ].kept )
                A.fin_hdr[ at++ ] = A.inv_hdr[ c0 + i ];
    }
    for( u64 i = first; i < at; i++ ) // (the lists' order array: they are in their order already)
        A.fin_order[ i ] = (u32)( i - first );
}
