// seeding.h -- BinarySeeding (binarySeeding.h:55-452, binarySeeding.cpp:32-178) as a per-read state
// machine that performs exactly one FMIndex::extend_backward per step, so that the 64 reads of a
// wavefront advance in lockstep through one shared "load two occ blocks + popcount" code path
// regardless of which extension phase each read is in.  (Template flag TXT, k_seed on reads in LDS: a maxSpan run whose
// interval is down to one row goes on by comparing the read with the packed text, 32 bases per step -- "text mode" below.)
#pragma once
#include "fm_device.h"

namespace ma
{
struct SeedParams
{
    u32 technique; // 0 maxSpan, 1 SMEMs, 2 MEMs (mems_from below; the state machine serves 0 and 1)
    u32 min_seed_len; // MEMs only: xMinSeedLength (binarySeeding.h:568)
    u32 min_amb, max_amb;
    u32 min_seed_size_drop;
    u32 disable_heuristics;
    double rel_min_seed_size_amount;
    u64 genome_size_disable;
    const uint8_t* window_begin = nullptr; // device kernels whose reads stay in HBM: the reads array, for seed_qbyte's 16-byte window
    const uint8_t* window_end = nullptr; // (null: off)
    u32 smem_compact = 0; // SMEM pending lists hold 16-byte entries (smem_put / smem_get): reads < 2^22 bases, text < 2^35
    u32 smem_merge = 0; // SMEM backward phase: an entry whose interval equals that of the entry pushed before it is not kept (seed_apply)
};

// Scratch a read needs while it is being seeded (lives in HBM, one slot per resident lane).
struct SeedScratch
{
    ma_segment* stage; // staged output segments of the read in flight (capacity seg_cap)
    u32 seg_cap;
    ma_segment* smem_a; // SMEM pending lists (capacity smem_cap each)
    ma_segment* smem_b;
    u32 smem_cap;
    u32 drop_div; // SeedParams::min_seed_size_drop (seed_emit keeps the running sum seed_finish needs)
    u32* stack; // 2 * MA_SEED_STACK words: interval stack of procesInterval (kept out of SeedLane so that the lane
                // state stays in registers; a dynamically indexed member would put the whole struct in scratch memory)
    // Round 6: the HEADS of the two SMEM lists in LDS (16-byte entries only; kernels whose reads stay in HBM).  A backward list holds one
    // to three entries once equal intervals are merged, the forward list about a dozen: with the first lds_n entries of each list in
    // LDS a backward step neither reads nor writes a list entry in HBM (50 kb x 10 k reads, SMEM tasks: 1.42 TB of fabric traffic per
    // step for 0.35 TB of occ blocks before).  Entry e of list w (0 = smem_a, 1 = smem_b) of this lane: lds[ 2 (w lds_n + e) lds_stride ].
    // lds_n <= smem_cap: an entry past the capacity is never written (the batch goes to the fallback), so none may be read from LDS.
    u64* lds = nullptr;
    u32 lds_n = 0, lds_stride = 0;
};

enum SeedPhase : u32
{
    PH_NEW_CENTER = 0,
    PH_P1_RIGHT = 1,
    PH_P1_LEFT = 2,
    PH_P2_LEFT = 3,
    PH_P2_RIGHT = 4,
    PH_SMEM_FWD = 5,
    PH_SMEM_BWD = 6,
    PH_DONE = 7
};

#define MA_SEED_STACK 40

struct SeedLane
{
    // read
    const uint8_t* q;
    u32 qlen;
    // interval stack of procesInterval (binarySeeding.cpp:32-84): left parts recurse, right parts iterate
    // (entries live in SeedScratch::stack)
    u32 sp;
    u32 aS, aN; // area currently processed
    // extension state
    u32 phase;
    u32 center, i, start, end;
    u32 s1_start, s1_end; // first (right-then-left) segment of the center, for the duplicate test
    i64 ik[ 3 ];
    // K-mer table entry of the centre's LEFT run (second pass), looked up together with the right run's (seed_center): the
    // two gathers share one memory round trip.  eL1 == 0: none
    u64 eL0, eL1;
    // reads in HBM: the bases around the centre the transitions need -- q[c-K], q[c-1], q[c], q[c+1], q[c+K], 3 bits each,
    // bit 15 = valid -- out of the block seed_center loaded (otherwise every transition is a memory round trip of its own)
    u32 cb;
    // SMEM state
    u32 nPrev, nCurr, jPrev; // list sizes / cursor
    u32 curQStart, curQSize; // prev[jPrev] of the extension in flight (its interval is in ik): read once, in seed_prepare
    u32 bHaveOne, retS, retE;
    u32 flip; // which of smem_a/smem_b is "prev"
    i64 lastK, lastS; // interval of the entry pushed last onto curr: the twin test of smem_merge
    u64 first0, first1; // the entry pushed FIRST onto curr (16-byte form): what the next position starts with (seed_try)
    u64 nxt0, nxt1; // prev[ jPrev ] of the NEXT backward step (16-byte entries only), requested one step ahead: the entry
    u32 nxtOk; //      arrives while this step's occ blocks are on their way, instead of in a round trip of its own
    // output
    u32 nseg;
    u32 err;
    u64 drop_sum; // sum over emitted segments of q_size / min_seed_size_drop (numSeedsLarger, segment.h:278-289)
    // counters
    u32 steps, blocks;
    // task mode (one lane per AREA instead of per read, pipeline.hip k_seed_tasks): after the area's centre has been
    // extended the lane stops and reports the two remaining areas instead of walking them itself
    u32 task_mode;
    u32 childS[ 2 ], childN[ 2 ]; // [0] left of the covered interval, [1] right of it; N == 0: none
    // 16 read bytes in registers for reads that stay in HBM (seed_qbyte): a lane walks its read base by base, and one
    // byte load per step is one 64-byte fabric request per step once the line has left L2 -- a third of the requests
    // k_seed issued on 10 kb reads (431 GB of fetches for 299 GB of occ blocks)
    u32 qwinLo;
    u32 qw0, qw1, qw2, qw3;
};

// base i of the lane's read.  P.window_begin / window_end (wave-uniform; null = off: the read is in LDS, or host code)
// delimit the reads array: the 16 bytes are taken aligned, or flush with an end of the array where an aligned block
// would leave it.
MA_HD void seed_qwin_load( SeedLane& L, const SeedParams& P, u32 i )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    const uintptr_t a = (uintptr_t)( L.q + i );
    uintptr_t base = a & ~(uintptr_t)15;
    uint4 v;
    if( base + 16 > (uintptr_t)P.window_end || base < (uintptr_t)P.window_begin )
    {
        // first / last bytes of the reads array: flush with its end, byte loads
        if( base + 16 > (uintptr_t)P.window_end )
            base = (uintptr_t)P.window_end - 16;
        if( base < (uintptr_t)P.window_begin )
            base = (uintptr_t)P.window_begin;
        __builtin_memcpy( &v, (const void*)base, 16 );
    }
    else
        v = *(const uint4*)base; // one global_load_dwordx4
    L.qw0 = v.x, L.qw1 = v.y, L.qw2 = v.z, L.qw3 = v.w;
    L.qwinLo = i - (u32)( a - base );
#endif
}
template <bool WIN> MA_HD u32 seed_qbyte( SeedLane& L, const SeedParams& P, u32 i )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    if( WIN && P.window_end )
    {
        if( i - L.qwinLo >= 16u )
            seed_qwin_load( L, P, i );
        const u32 d = i - L.qwinLo;
        // selects of VALUES: without the empty asm the compiler folds them into one load through a selected address, and that address
        // keeps the whole lane state of k_seed_tasks* in scratch memory (90 scratch stores in its loop, 0.76 TB of writes per step)
        u32 w0 = L.qw0, w1 = L.qw1, w2 = L.qw2, w3 = L.qw3;
        asm( "" : "+v"( w0 ), "+v"( w1 ), "+v"( w2 ), "+v"( w3 ) );
        const u32 lo = d & 8u ? w2 : w0, hi = d & 8u ? w3 : w1;
        return ( ( d & 4u ? hi : lo ) >> ( 8u * ( d & 3u ) ) ) & 0xffu;
    }
#endif
    return L.q[ i ];
}

MA_HD u32 comp_base( u32 c ) // NucSeq::nucleotideComplement (nucSeq.h:524-532)
{
    return c < 4 ? 3 - c : 5;
}

// Entries of the SMEM pending lists (binarySeeding.h:296-433).  The lists live in HBM, one pair per resident lane, and
// their traffic is as large as that of the occ blocks (Illumina preset: 99 GB of reads and 94 GB of writes per 1 M reads
// beside 105 GB of occ blocks).  A 40-byte record straddles 64-byte lines; packed into 16 bytes -- three 35-bit interval
// fields and ONE 22-bit query field -- an entry is one aligned dwordx4 and four of them share a line.
// The start of the match is not stored: all entries of one list share it.  The forward phase pushes (center, ...)
// (binarySeeding.h:296-337), a backward position i pushes (i, ...) (:380-413), so the entries a backward position i reads were
// pushed at i + 1 (or by the forward phase with center = i + 1) and the caller names the start when it unpacks (`qs`);
// the 40-byte form keeps its own copy, and the host emulation checks that both agree.  (Round 4 stored two 11-bit query
// fields, which kept reads of 2048 bases and more -- the Nanopore preset's -- on the 40-byte records.)
#define MA_SMEM_QZ_BITS 22
MA_HD void smem_pack( u32 qz, i64 a, i64 b, i64 c, u64& w0, u64& w1 )
{
    w0 = (u64)a | ( ( (u64)c & 0x1fffffffull ) << 35 );
    w1 = (u64)b | ( ( (u64)c >> 29 ) << 35 ) | ( (u64)qz << 41 );
}
MA_HD ma_segment smem_unpack( u64 w0, u64 w1, u32 qs )
{
    ma_segment s;
    s.sa_start = (i64)( w0 & 0x7ffffffffull );
    s.sa_start_rc = (i64)( w1 & 0x7ffffffffull );
    s.sa_size = (i64)( ( w0 >> 35 ) | ( ( ( w1 >> 35 ) & 0x3full ) << 29 ) );
    s.q_start = (i64)qs;
    s.q_size = (i64)( ( w1 >> 41 ) & ( ( 1ull << MA_SMEM_QZ_BITS ) - 1 ) );
    return s;
}
MA_HD void smem_put( const SeedParams& P, ma_segment* list, u32 idx, u32 qs, u32 qz, i64 a, i64 b, i64 c )
{
    if( P.smem_compact )
    {
        u64* w = (u64*)list + 2 * (u64)idx;
        u64 w0, w1;
        smem_pack( qz, a, b, c, w0, w1 );
#if defined( __HIP_DEVICE_COMPILE__ )
        *(ulonglong2*)w = make_ulonglong2( w0, w1 );
#else
        w[ 0 ] = w0, w[ 1 ] = w1;
#endif
    }
    else
    {
        ma_segment s;
        s.q_start = qs, s.q_size = qz, s.sa_start = a, s.sa_start_rc = b, s.sa_size = c;
        list[ idx ] = s;
    }
}
// qs: the start all entries of this list share (see above)
MA_HD ma_segment smem_get( const SeedParams& P, const ma_segment* list, u32 idx, u32 qs )
{
    if( P.smem_compact )
    {
        const u64* w = (const u64*)list + 2 * (u64)idx;
#if defined( __HIP_DEVICE_COMPILE__ )
        const ulonglong2 v = *(const ulonglong2*)w;
        const u64 w0 = v.x, w1 = v.y;
#else
        const u64 w0 = w[ 0 ], w1 = w[ 1 ];
#endif
        return smem_unpack( w0, w1, qs );
    }
#if !defined( __HIP_DEVICE_COMPILE__ )
    if( (u64)list[ idx ].q_start != (u64)qs )
        abort( ); // host emulation only: the shared start the compact form relies on
#endif
    return list[ idx ];
}

// request entry idx of a list of 16-byte entries into the lane's prefetch registers
MA_HD void smem_prefetch( SeedLane& L, const ma_segment* list, u32 idx );
// the same three by list NUMBER (0 = smem_a, 1 = smem_b): the first S.lds_n entries of a list live in LDS (SeedScratch::lds)
MA_HD void smem_put_w( const SeedParams& P, const SeedScratch& S, u32 w, u32 idx, u32 qs, u32 qz, i64 a, i64 b, i64 c )
{
    if( P.smem_compact && idx < S.lds_n )
    {
        u64 w0, w1;
        smem_pack( qz, a, b, c, w0, w1 );
        u64* p = S.lds + 2 * (u64)( ( w * S.lds_n + idx ) * S.lds_stride );
#if defined( __HIP_DEVICE_COMPILE__ )
        *(ulonglong2*)p = make_ulonglong2( w0, w1 );
#else
        p[ 0 ] = w0, p[ 1 ] = w1;
#endif
        return;
    }
    smem_put( P, w ? S.smem_b : S.smem_a, idx, qs, qz, a, b, c );
}
MA_HD ma_segment smem_get_w( const SeedParams& P, const SeedScratch& S, u32 w, u32 idx, u32 qs )
{
    if( P.smem_compact && idx < S.lds_n )
    {
        const u64* p = S.lds + 2 * (u64)( ( w * S.lds_n + idx ) * S.lds_stride );
#if defined( __HIP_DEVICE_COMPILE__ )
        const ulonglong2 v = *(const ulonglong2*)p;
        return smem_unpack( v.x, v.y, qs );
#else
        return smem_unpack( p[ 0 ], p[ 1 ], qs );
#endif
    }
    return smem_get( P, w ? S.smem_b : S.smem_a, idx, qs );
}
MA_HD void seed_emit( SeedLane& L, const SeedScratch& S, u32 start, u32 size, i64 a, i64 b, i64 c )
{
    if( L.nseg < S.seg_cap )
    {
        ma_segment s;
        s.q_start = start;
        s.q_size = size;
        s.sa_start = a;
        s.sa_start_rc = b;
        s.sa_size = c;
        S.stage[ L.nseg ] = s;
        if( S.drop_div )
            L.drop_sum += (u64)size / (u64)S.drop_div;
    }
    else
        L.err |= MA_ERR_SEG_OVERFLOW;
    L.nseg++;
}

MA_HD void smem_prefetch( SeedLane& L, const ma_segment* list, u32 idx )
{
    const u64* w = (const u64*)list + 2 * (u64)idx;
#if defined( __HIP_DEVICE_COMPILE__ )
    const ulonglong2 v = *(const ulonglong2*)w;
    L.nxt0 = v.x, L.nxt1 = v.y;
#else
    L.nxt0 = w[ 0 ], L.nxt1 = w[ 1 ];
#endif
    L.nxtOk = 1;
}
MA_HD void smem_prefetch_w( SeedLane& L, const SeedScratch& S, u32 w, u32 idx ) // (16-byte entries only, like smem_prefetch)
{
    if( idx < S.lds_n )
    {
        const u64* p = S.lds + 2 * (u64)( ( w * S.lds_n + idx ) * S.lds_stride );
#if defined( __HIP_DEVICE_COMPILE__ )
        const ulonglong2 v = *(const ulonglong2*)p;
        L.nxt0 = v.x, L.nxt1 = v.y;
#else
        L.nxt0 = p[ 0 ], L.nxt1 = p[ 1 ];
#endif
        L.nxtOk = 1;
        return;
    }
    smem_prefetch( L, w ? S.smem_b : S.smem_a, idx );
}
MA_HD void seed_begin_read( SeedLane& L, const uint8_t* q, u32 qlen )
{
    L.nxtOk = 0;
    L.q = q;
    L.qlen = qlen;
    L.qwinLo = 0x80000000u; // empty
    L.sp = 0;
    L.aS = 0;
    L.aN = qlen;
    L.nseg = 0;
    L.drop_sum = 0;
    L.err = 0;
    L.steps = L.blocks = 0;
    L.task_mode = 0;
    L.phase = qlen == 0 ? PH_DONE : PH_NEW_CENTER;
}
// task mode: the lane extends the centre of [aS, aS + aN) of the read and stops
MA_HD void seed_begin_area( SeedLane& L, const uint8_t* q, u32 qlen, u32 aS, u32 aN )
{
    seed_begin_read( L, q, qlen );
    L.task_mode = 1;
    L.aS = aS;
    L.aN = aN;
    L.childN[ 0 ] = L.childN[ 1 ] = 0;
    L.childS[ 0 ] = L.childS[ 1 ] = 0;
    L.phase = aN == 0 ? PH_DONE : PH_NEW_CENTER;
}

// After an extension around `center` covered [cS, cS+cN] (reference convention), split the area
// (binarySeeding.cpp:58-82): recurse left first, continue right afterwards.
MA_HD void seed_after_center( SeedLane& L, const SeedScratch& S, u32 cS, u32 cN )
{
    const u32 cE = cS + cN, aE = L.aS + L.aN;
    const bool hasLeft = cS != 0 && L.aS + 1 < cS;
    const bool hasRight = aE > cE + 1;
    if( L.task_mode )
    {
        L.childS[ 0 ] = L.aS, L.childN[ 0 ] = hasLeft ? cS - L.aS : 0;
        L.childS[ 1 ] = cE, L.childN[ 1 ] = hasRight ? aE - cE : 0;
        L.phase = PH_DONE;
        return;
    }
    if( hasLeft )
    {
        if( hasRight )
        {
            if( L.sp < MA_SEED_STACK )
            {
                S.stack[ 2 * L.sp ] = cE;
                S.stack[ 2 * L.sp + 1 ] = aE - cE;
                L.sp++;
            }
            else
                L.err |= MA_ERR_STACK_OVERFLOW;
        }
        L.aN = cS - L.aS; // [aS, cS)
        L.phase = PH_NEW_CENTER;
    }
    else if( hasRight )
    {
        L.aS = cE;
        L.aN = aE - cE;
        L.phase = PH_NEW_CENTER;
    }
    else if( L.sp > 0 )
    {
        L.sp--;
        L.aS = S.stack[ 2 * L.sp ];
        L.aN = S.stack[ 2 * L.sp + 1 ];
        L.phase = PH_NEW_CENTER;
    }
    else
        L.phase = PH_DONE;
}

// The first K-1 extension steps of a run that starts at the centre with a single-base interval come from the K-mer table of
// the index: the right run (PH_P1_RIGHT) of the bases q[centre .. centre+K-1] complemented, the left run (PH_P2_LEFT) of
// q[centre], q[centre-1], ..  An entry is valid for a run when its interval is still larger than min_amb: interval sizes only
// shrink along a run, so none of the skipped steps would have met the stop rule (binarySeeding.h:109-112).
MA_HD bool kmer_decode( const SeedParams& P, u64 x, u64 y, i64 ik[ 3 ] )
{
    const i64 size = (i64)( ( x >> 35 ) | ( ( ( y >> 35 ) & 0x3full ) << 29 ) );
    if( size <= (i64)P.min_amb )
        return false;
    ik[ 0 ] = (i64)( x & 0x7ffffffffull );
    ik[ 1 ] = (i64)( y & 0x7ffffffffull );
    ik[ 2 ] = size;
    return true;
}
// 2-bit codes of up to 16 bases held one per byte (x: bases 0..7, y: 8..15) -> base j at bits 2j, 2j+1
MA_HD u32 kmer_gather( u64 x, u64 y )
{
    auto g = []( u64 v ) -> u32 {
        v = ( v | ( v >> 6 ) ) & 0x000f000f000f000full;
        v = ( v | ( v >> 12 ) ) & 0x000000ff000000ffull;
        return (u32)( ( v | ( v >> 24 ) ) & 0xffffull );
    };
    return g( x ) | g( y ) << 16;
}
MA_HD u32 kmer_key_right( u32 le, u32 K ) // first base of the span most significant, complemented
{
    u32 r = 0;
#if defined( __HIP_DEVICE_COMPILE__ )
    r = __brev( le ) >> ( 32u - 2u * K );
#else
    for( u32 j = 0; j < 32; j++ )
        r |= ( ( le >> j ) & 1u ) << ( 31u - j );
    r >>= 32u - 2u * K;
#endif
    r = ( ( r & 0xaaaaaaaau ) >> 1 ) | ( ( r & 0x55555555u ) << 1 );
    return r ^ (u32)( ( 1ull << ( 2u * K ) ) - 1ull );
}

// Start of a centre: its base (returned), and -- when the index has a K-mer table -- the table entries of BOTH runs that
// start at the centre: eR (returned through eRx / eRy, 0 = none) and the lane's eL.  Reads in HBM (WIN): ONE load of the 48
// bytes around the centre serves the base, both keys and the bases the later transitions of this centre start with (L.cb);
// step by step the same costs a window load for the centre, K byte loads per key and a window load per transition, each a
// memory round trip of its own that the whole wavefront waits for.
template <bool WIN, bool JUMP, bool SM = true, bool MS = true> MA_HD u32 seed_center( SeedLane& L, const SeedParams& P, const IndexView& X, u64& eRx, u64& eRy )
{
    const u32 K = JUMP && MS && ( !SM || P.technique == 0 ) ? X.kmer_k : 0, c = L.center;
    eRx = eRy = 0;
    if( MS )
    {
        L.eL0 = L.eL1 = 0;
        L.cb = 0;
    }
    bool vR = K != 0 && c + K <= L.qlen, vL = K != 0 && c + 1 >= K;
    u32 keyR = 0, keyL = 0, qc;
#if defined( __HIP_DEVICE_COMPILE__ )
    const uintptr_t a0 = (uintptr_t)( L.q + c ) - K; // q[c-K] (possibly in front of the read)
    const uintptr_t base = a0 & ~(uintptr_t)15;
    if( WIN && K != 0 && P.window_end && base >= (uintptr_t)P.window_begin && base + 48 <= (uintptr_t)P.window_end )
    {
        const uint4 b0 = ( (const uint4*)base )[ 0 ], b1 = ( (const uint4*)base )[ 1 ], b2 = ( (const uint4*)base )[ 2 ];
        const u64 w0 = b0.x | (u64)b0.y << 32, w1 = b0.z | (u64)b0.w << 32, w2 = b1.x | (u64)b1.y << 32, w3 = b1.z | (u64)b1.w << 32,
                  w4 = b2.x | (u64)b2.y << 32, w5 = b2.z | (u64)b2.w << 32;
        const u32 d0 = (u32)( a0 - base ), sh = 8u * ( d0 & 7u );
        const bool t = ( d0 & 8u ) != 0;
        auto fun = [ & ]( u64 lo, u64 hi ) -> u64 { return sh ? ( lo >> sh ) | ( hi << ( 64u - sh ) ) : lo; };
        // v[j]: bytes 8j .. 8j+7 of the view that starts at q[c-K]
        const u64 v0 = fun( t ? w1 : w0, t ? w2 : w1 ), v1 = fun( t ? w2 : w1, t ? w3 : w2 ), v2 = fun( t ? w3 : w2, t ? w4 : w3 ),
                  v3 = fun( t ? w4 : w3, t ? w5 : w4 );
        auto at = [ & ]( u32 j ) -> u32 { // j is wave-uniform
            const u64 v = j < 8 ? v0 : j < 16 ? v1 : j < 24 ? v2 : v3;
            return (u32)( v >> ( 8u * ( j & 7u ) ) ) & 0xffu;
        };
        auto span = [ & ]( u32 j, u64& x, u64& y ) { // K bytes from byte j on
            const u32 s8 = 8u * ( j & 7u );
            const u64 p = j < 8 ? v0 : j < 16 ? v1 : v2, q = j < 8 ? v1 : j < 16 ? v2 : v3, r = j < 8 ? v2 : j < 16 ? v3 : 0ull;
            x = s8 ? ( p >> s8 ) | ( q << ( 64u - s8 ) ) : p;
            y = s8 ? ( q >> s8 ) | ( r << ( 64u - s8 ) ) : q;
            if( K < 8 )
                x &= ( 1ull << ( 8u * K ) ) - 1ull;
            y = K > 8 ? y & ( ( 1ull << ( 8u * ( K - 8u ) ) ) - 1ull ) : 0ull; // K <= 14
        };
        qc = at( K );
        const u32 qm1 = at( K - 1 ), qp1 = at( K + 1 ), qmK = at( 0 ), qpK = at( 2 * K );
        if( ( ( qc | qm1 | qp1 | qmK | qpK ) & ~7u ) == 0 )
            L.cb = qmK | qm1 << 3 | qc << 6 | qp1 << 9 | qpK << 12 | 0x8000u;
        u64 x, y;
        span( K, x, y );
        vR = vR && ( ( x | y ) & 0xfcfcfcfcfcfcfcfcull ) == 0;
        keyR = kmer_key_right( kmer_gather( x, y ), K );
        span( 1, x, y );
        vL = vL && ( ( x | y ) & 0xfcfcfcfcfcfcfcfcull ) == 0;
        keyL = kmer_gather( x, y ); // q[c] = last base of the span most significant
    }
    else
#endif
    {
        qc = seed_qbyte<WIN>( L, P, c );
        if( qc >= 4 )
            return qc;
        u32 bad = 0;
        for( u32 j = 0; vR && j < K; j++ )
        {
            const u32 b = L.q[ c + j ];
            bad |= b >> 2;
            keyR = ( keyR << 2 ) | ( ( 3u - b ) & 3u );
        }
        vR = vR && !bad;
        bad = 0;
        for( u32 j = 0; vL && j < K; j++ )
        {
            const u32 b = L.q[ c - j ];
            bad |= b >> 2;
            keyL = ( keyL << 2 ) | ( b & 3u );
        }
        vL = vL && !bad;
    }
    if( qc >= 4 )
        return qc;
#if defined( __HIP_DEVICE_COMPILE__ )
    if( K != 0 )
    {
        // both gathers in flight before either entry is looked at
        ulonglong2 eR = make_ulonglong2( 0, 0 ), eL = make_ulonglong2( 0, 0 );
        if( vR )
            eR = ( (const ulonglong2*)X.kmer_tab )[ keyR ];
        if( vL )
            eL = ( (const ulonglong2*)X.kmer_tab )[ keyL ];
        eRx = eR.x, eRy = eR.y;
        L.eL0 = eL.x, L.eL1 = eL.y;
    }
#endif
    return qc;
}
// base i of the read out of the centre's cached bases when it is one of them
template <bool WIN> MA_HD u32 seed_qbyte_c( SeedLane& L, const SeedParams& P, const IndexView& X, u32 i )
{
    if( WIN && ( L.cb & 0x8000u ) )
    {
        const u32 K = X.kmer_k;
        const i32 d = (i32)( i - L.center );
        if( d == -1 )
            return ( L.cb >> 3 ) & 7u;
        if( d == 1 )
            return ( L.cb >> 9 ) & 7u;
        if( d == 0 )
            return ( L.cb >> 6 ) & 7u;
        if( d == -(i32)K )
            return L.cb & 7u;
        if( d == (i32)K )
            return ( L.cb >> 12 ) & 7u;
    }
    return seed_qbyte<WIN>( L, P, i );
}

MA_HD bool seed_stop( const SeedParams& P, const i64 ok[ 3 ], const i64 ik[ 3 ] ) // binarySeeding.h:109-112
{
    if( ok[ 2 ] <= 0 )
        return true;
    return ok[ 2 ] <= (i64)P.min_amb && ik[ 2 ] <= (i64)P.max_amb;
}

// ---- text mode of the maxSpan runs (template flag TXT) ---------------------------------------------------------------------
// Once the interval of a run has shrunk to ONE row, every further extend_backward answers a single question: does the next base
// of the read equal the next base of the reference at the one locus the row stands for?  For a 6.2 Gnt text that is the case after
// 17-20 bases, so about 230 of the 270 occ blocks a unique 150 bp read gathers are spent on it, one random 64-byte line per base.
// The packed text answers it for 32 bases with one line.  A lane whose interval reaches size 1 while its run goes on
//   1. locates the row: p = bwt_sa( ik[ 0 ] ), one LF step per trip through the block load of the lanes that still extend,
//      then the SA sample (the walk is not new work: a segment that becomes a seed paid it in k_lf_walk);
//   2. compares: up to 32 read bases per trip against the pack, XOR of 2-bit codes and a count of the equal prefix.
// The position stays known over the direction switch (binarySeeding.h:118-120), so the second run of a pass compares too.
//
// Why the result is the same.  The BWT is that of the doubled text T2 = T . revcomp( T ) of length n, which text_base( ) defines
// (index_build.hip sorts the suffixes of exactly that text, TextView::at == text_base; the reference's builder reads the same pack,
// and a base the FASTA gave as N is a plain nucleotide in the pack and therefore in both).  bwt_sa returns positions in T2 --
// k_seed_final folds r >= n / 2 -- and T2 is its own reverse complement: pattern P stands at p iff revcomp( P ) stands at n - p - |P|.
//  * Left step.  ik[ 0 ] = k is the row of the suffix at p = SA[ k ], ik[ 2 ] == 1.  extend_backward by c counts the rows of
//    [ k, k + 1 ) whose BWT character is c: size 1 iff the character in front of the suffix is c, i.e. iff p > 0 and
//    text_base( p - 1 ) == c; the new row is that of the suffix at p - 1.  At p == 0 (row `primary`, whose BWT character is '$')
//    every base fails.
//  * Right step by read base b.  The machine extends the interval of the reverse complement, which stands at n - p - len, by
//    comp_base( b ): size 1 iff n - p - len > 0 and text_base( n - p - len - 1 ) == 3 - b, and the mirror of that position is
//    p + len: iff p + len < n and text_base( p + len ) == b.  The end of the text fails like its start.
//  * A read base >= 4 gives size 0 in extend_backward and counts as a mismatch here.
//  * The junction of the strands at F and the borders of contigs are no special case in the BWT, and none here: matches across
//    them are found by both and dealt with downstream (bridging seeds) as before.
//  * The stop rule (seed_stop): with min_amb >= 1 an interval of size 1 stops the run at once, so the mode is entered only for
//    min_amb == 0, where a run stops iff the extension is empty.
// State: ik[ 2 ] == 1 and ik[ 1 ] < 0 (a row is never negative).  Locating: ik[ 0 ] = the row reached, -1 - ik[ 1 ] = LF steps so far.
// Comparing: ik[ 1 ] == MA_TM_CMP, ik[ 0 ] = p, the position in T2 of q[ start .. end ].  A lane enters the mode only with an extension
// of the same run pending, so a run never ends -- and never turns -- while its row is being located.
// A segment emitted in this state carries sa_start = -1 - p, sa_start_rc = -1, sa_size = 1: extraction takes the position as
// given (stage_extract.h), and seed_materialise recomputes the rows where someone asks for the record.
#define MA_TM_CMP ( (i64)( 1ull << 63 ) )
template <bool TXT> MA_HD void seed_text_enter( SeedLane& L, const SeedParams& P )
{
    if( !TXT || P.min_amb != 0 || L.ik[ 2 ] != 1 )
        return;
    const bool right = L.phase == PH_P1_RIGHT || L.phase == PH_P2_RIGHT;
    if( right ? L.i < L.qlen : L.i != 0xffffffffu )
        L.ik[ 1 ] = -1;
}
// rows of a segment that carries a position: the bi-interval is a function of the pattern, found by plain backward search
MA_HD void seed_materialise( const IndexView& X, const uint8_t* q, ma_segment& s )
{
    if( s.sa_start >= 0 )
        return;
    i64 ik[ 3 ];
    init_interval( X, q[ s.q_start + s.q_size ], ik );
    for( i64 i = s.q_start + s.q_size - 1; i >= s.q_start; i-- )
    {
        i64 ok[ 3 ];
        u32 nb;
        extend_backward( X, ik, q[ i ], ok, nb );
        ik[ 0 ] = ok[ 0 ], ik[ 1 ] = ok[ 1 ], ik[ 2 ] = ok[ 2 ];
    }
    s.sa_start = ik[ 0 ], s.sa_start_rc = ik[ 1 ], s.sa_size = ik[ 2 ];
}
MA_HD u64 rev2_64( u64 v ) // the 32 2-bit groups of v in reverse order
{
    v = ( ( v >> 2 ) & 0x3333333333333333ull ) | ( ( v & 0x3333333333333333ull ) << 2 );
    v = ( ( v >> 4 ) & 0x0f0f0f0f0f0f0f0full ) | ( ( v & 0x0f0f0f0f0f0f0f0full ) << 4 );
    return __builtin_bswap64( v );
}
MA_HD u64 low2m( u32 m ) // the low 2 m bits, m <= 32
{
    return m >= 32 ? ~0ull : ( 1ull << ( 2u * m ) ) - 1ull;
}
// 2-bit codes of the read's bases [ a, a + m ), m <= 32: base a + j at bits 2j, 2j + 1 of w; bit 2j of bad set where it is no nucleotide.
// FAST: five 8-byte groups instead of m byte loads; q is 4-byte aligned and readable up to the next multiple of 8 past a + m (the LDS
// copy of k_seed: its stride covers the read's length rounded up to 8)
template <bool FAST> MA_HD void text_read_pack( const uint8_t* q, u32 a, u32 m, u64& w, u64& bad )
{
    if( FAST )
    {
        auto g = []( u64 v ) -> u64 {
            v = ( v | ( v >> 6 ) ) & 0x000f000f000f000full;
            v = ( v | ( v >> 12 ) ) & 0x000000ff000000ffull;
            return ( v | ( v >> 24 ) ) & 0xffffull;
        };
        const u32 g0 = a & ~7u;
        u64 v[ 5 ];
#pragma unroll
        for( u32 t = 0; t < 5; t++ )
        {
            v[ t ] = 0;
            if( g0 + 8 * t < a + m )
            {
                const u32* p = (const u32*)__builtin_assume_aligned( q + g0 + 8 * t, 4 );
                v[ t ] = (u64)p[ 0 ] | (u64)p[ 1 ] << 32;
            }
        }
        u64 c[ 5 ], n[ 5 ];
#pragma unroll
        for( u32 t = 0; t < 5; t++ )
        {
            c[ t ] = g( v[ t ] & 0x0303030303030303ull );
            const u64 hi = ( v[ t ] >> 2 ) & 0x3f3f3f3f3f3f3f3full; // a byte's bits 2..7: non-zero = no nucleotide
            n[ t ] = g( ( ( hi + 0x3f3f3f3f3f3f3f3full ) >> 6 ) & 0x0101010101010101ull );
        }
        const u64 cl = c[ 0 ] | c[ 1 ] << 16 | c[ 2 ] << 32 | c[ 3 ] << 48, nl = n[ 0 ] | n[ 1 ] << 16 | n[ 2 ] << 32 | n[ 3 ] << 48;
        const u32 s = 2u * ( a & 7u );
        w = ( s ? ( cl >> s ) | ( c[ 4 ] << ( 64u - s ) ) : cl ) & low2m( m );
        bad = ( s ? ( nl >> s ) | ( n[ 4 ] << ( 64u - s ) ) : nl ) & low2m( m );
        return;
    }
    w = bad = 0;
    for( u32 j = 0; j < m; j++ )
    {
        const u32 b = q[ a + j ];
        w |= (u64)( b & 3u ) << ( 2u * j );
        bad |= (u64)( b >= 4 ? 1u : 0u ) << ( 2u * j );
    }
}
// The pack's forward bases [ g, g + m ), m <= 32, base g + j at bits 2j, 2j + 1.  FAST: out of the two aligned 8-byte words w0, w1 that
// text_pac_request loaded (the pack is 8-byte aligned and readable 16 bytes past its last base: ma_index_create pads it)
MA_HD u64 text_pac_word( u64 g )
{
    return ( g >> 2 ) & ~7ull;
}
template <bool FAST> MA_HD void text_pac_request( const IndexView& X, u64 g, u64& w0, u64& w1 )
{
    w0 = w1 = 0;
    if( FAST )
    {
        const u64* p = (const u64*)__builtin_assume_aligned( X.pac + text_pac_word( g ), 8 );
        w0 = p[ 0 ], w1 = p[ 1 ];
    }
}
template <bool FAST> MA_HD u64 text_pac_pack( const IndexView& X, u64 g, u32 m, u64 w0, u64 w1 )
{
    if( FAST )
    {
        // a byte holds its four bases most significant first: reverse the groups of every byte
        auto r = []( u64 v ) -> u64 {
            v = ( ( v >> 2 ) & 0x3333333333333333ull ) | ( ( v & 0x3333333333333333ull ) << 2 );
            return ( ( v >> 4 ) & 0x0f0f0f0f0f0f0f0full ) | ( ( v & 0x0f0f0f0f0f0f0f0full ) << 4 );
        };
        w0 = r( w0 ), w1 = r( w1 );
        const u32 s = 2u * (u32)( g - 4ull * text_pac_word( g ) ); // 0 .. 62
        return ( s ? ( w0 >> s ) | ( w1 << ( 64u - s ) ) : w0 ) & low2m( m );
    }
    u64 w = 0;
    for( u32 j = 0; j < m; j++ )
        w |= (u64)fwd_base( X, g + j ) << ( 2u * j );
    return w;
}

// Can the lane extend right away, i.e. without any phase transition?  (The kernel batches the transitions of a
// wavefront: a lane whose transition is due idles for a few steps until enough lanes wait, so that the divergent
// bookkeeping of seed_prepare is executed once for many lanes instead of on every step for one or two.)
// SM = false: the kernel serves maxSpan only (P.technique == 0): the SMEM states and their lane registers are compiled out;
// MS = false: SMEMs only (P.technique == 1), the same for the maxSpan states
template <bool WIN = false, bool SM = true, bool MS = true> MA_HD bool seed_try( SeedLane& L, const SeedParams& P, u32& c, const SeedScratch* S = nullptr )
{
    if( SM && L.phase == PH_SMEM_BWD )
    {
        // the next entry of the list was requested a step ago (seed_prepare / here): take it, request the one after it
        if( S != nullptr && L.nxtOk && L.jPrev < L.nPrev )
        {
            const ma_segment s = smem_unpack( L.nxt0, L.nxt1, L.i + 1 );
            L.ik[ 0 ] = s.sa_start, L.ik[ 1 ] = s.sa_start_rc, L.ik[ 2 ] = s.sa_size;
            L.curQStart = (u32)s.q_start, L.curQSize = (u32)s.q_size;
            if( L.jPrev + 1 < L.nPrev )
                smem_prefetch_w( L, *S, L.flip, L.jPrev + 1 );
            else
                L.nxtOk = 0;
            c = seed_qbyte<WIN>( L, P, L.i );
            return true;
        }
        // End of a backward position (the bookkeeping of seed_prepare's PH_SMEM_BWD) without leaving the fast path: the next
        // position starts with the entry that was pushed FIRST onto the list just written, which is still in registers -- no
        // list read, no batching with other lanes' transitions; the second entry is requested for the step after this one.
        // (16-byte entries only.)  The entry was pushed at position L.i, which is the start it carries.
        if( S != nullptr && P.smem_compact && L.jPrev == L.nPrev && L.nCurr >= 1 && L.i != 0 )
        {
            L.flip ^= 1;
            L.nPrev = L.nCurr;
            L.nCurr = 0;
            L.jPrev = 0;
            L.bHaveOne = 0;
            L.retS = L.i;
            const ma_segment s = smem_unpack( L.first0, L.first1, L.i );
            L.ik[ 0 ] = s.sa_start, L.ik[ 1 ] = s.sa_start_rc, L.ik[ 2 ] = s.sa_size;
            L.curQStart = (u32)s.q_start, L.curQSize = (u32)s.q_size;
            if( L.nPrev > 1 )
                smem_prefetch_w( L, *S, L.flip, 1 );
            else
                L.nxtOk = 0;
            L.i--;
            c = seed_qbyte<WIN>( L, P, L.i );
            return true;
        }
        return false;
    }
    const bool right = ( MS && ( L.phase == PH_P1_RIGHT || L.phase == PH_P2_RIGHT ) ) || ( SM && L.phase == PH_SMEM_FWD );
    const bool left = MS && ( L.phase == PH_P1_LEFT || L.phase == PH_P2_LEFT );
    const bool ok = right ? L.i < L.qlen : ( left && L.i != 0xffffffffu );
    if( ok )
    {
        const u32 b = seed_qbyte<WIN>( L, P, L.i );
        c = right ? comp_base( b ) : b;
    }
    return ok;
}

// The base of THIS step has been taken out of the 16-byte window (seed_try / seed_prepare returned true); when the run's next
// base lies outside of it, the next block is requested now, ahead of this step's occ blocks: it arrives while the lane waits
// for those anyway.  (Loaded on demand at the top of the next step, some lane of the wavefront needs a block on nearly every
// trip, and every trip became two memory round trips in a row: 7.2 k of 13.7 k cycles per trip of the 10 kb workload.)
template <bool WIN> MA_HD void seed_prefetch( SeedLane& L, const SeedParams& P )
{
#if defined( __HIP_DEVICE_COMPILE__ )
    if( WIN && P.window_end )
    {
        const bool right = L.phase == PH_P1_RIGHT || L.phase == PH_P2_RIGHT || L.phase == PH_SMEM_FWD;
        const bool left = L.phase == PH_P1_LEFT || L.phase == PH_P2_LEFT;
        const u32 nxt = right ? L.i + 1 : L.i - 1; // L.i == 0 going left: wraps, and fails the test below
        if( ( right || left ) && nxt < L.qlen && nxt - L.qwinLo >= 16u )
            seed_qwin_load( L, P, nxt );
    }
#endif
}

// ---- transitions (no index access) ----------------------------------------------------------
// Runs cheap bookkeeping until the lane either needs an extension (returns true and sets c) or is done.
// JUMP: use the K-mer table of the index (only the kernel whose register budget has room for it: inlined into the
// read-per-lane kernel it costs a wave of occupancy, 117 -> 138 VGPRs, which eats the gain)
// TXT: the text mode of the maxSpan runs (above)
template <bool WIN = false, bool JUMP = false, bool SM = true, bool MS = true, bool TXT = false> MA_HD bool seed_prepare( SeedLane& L, const SeedParams& P, const SeedScratch& S, const IndexView& X, u32& c )
{
    while( true )
    {
        switch( L.phase )
        {
            case PH_DONE:
                return false;
            case PH_NEW_CENTER:
            {
                L.center = L.aS + L.aN / 2;
                u64 eRx, eRy;
                const u32 qc = seed_center<WIN, JUMP, SM, MS>( L, P, X, eRx, eRy );
                if( qc >= 4 )
                { // N covers one position (binarySeeding.h:70-72 / 275-277)
                    seed_after_center( L, S, L.center, 1 );
                    break;
                }
                init_interval( X, 3 - qc, L.ik );
                if( MS && ( !SM || P.technique == 0 ) )
                {
                    if( L.ik[ 2 ] == 0 )
                    {
                        seed_after_center( L, S, L.center, 1 );
                        break;
                    }
                    L.start = L.end = L.center; // (start: what the left run begins with; the text mode reads the match's extent on the way)
                    L.i = L.center + 1;
                    L.phase = PH_P1_RIGHT;
                    if( JUMP && kmer_decode( P, eRx, eRy, L.ik ) )
                    {
                        L.end = L.center + X.kmer_k - 1;
                        L.i = L.center + X.kmer_k;
                        seed_text_enter<TXT>( L, P );
                    }
                }
                else if( SM )
                {
                    L.nCurr = 0;
                    L.retS = L.retE = L.center;
                    L.i = L.center + 1;
                    L.flip = 0;
                    L.phase = PH_SMEM_FWD;
                }
                else
                    L.phase = PH_DONE;
                break;
            }
            case PH_P1_RIGHT:
                if( !MS )
                    return false;
                if( L.i < L.qlen )
                {
                    c = comp_base( seed_qbyte_c<WIN>( L, P, X, L.i ) );
                    return true;
                }
                // end of query: switch direction (binarySeeding.h:118-120); a lane in text mode keeps its position
                if( !TXT || L.ik[ 1 ] >= 0 )
                    mswap( L.ik[ 0 ], L.ik[ 1 ] );
                L.start = L.center;
                if( L.center > 0 )
                {
                    L.i = L.center - 1;
                    L.phase = PH_P1_LEFT;
                    break;
                }
                L.phase = PH_P1_LEFT;
                L.i = 0xffffffffu; // sentinel: left loop skipped
                break;
            case PH_P1_LEFT:
                if( !MS )
                    return false;
                if( L.i != 0xffffffffu )
                {
                    c = seed_qbyte_c<WIN>( L, P, X, L.i );
                    return true;
                }
                // record first segment and start the second pass (binarySeeding.h:152-163)
                if( TXT && L.ik[ 1 ] < 0 )
                    seed_emit( L, S, L.start, L.end - L.start, -1 - L.ik[ 0 ], -1, 1 );
                else
                    seed_emit( L, S, L.start, L.end - L.start, L.ik[ 0 ], L.ik[ 1 ], L.ik[ 2 ] );
                L.s1_start = L.start;
                L.s1_end = L.end;
                init_interval( X, seed_qbyte_c<WIN>( L, P, X, L.center ), L.ik );
                L.start = L.end = L.center;
                L.phase = PH_P2_LEFT;
                L.i = L.center > 0 ? L.center - 1 : 0xffffffffu;
                if( JUMP && kmer_decode( P, L.eL0, L.eL1, L.ik ) )
                {
                    L.start = L.center - ( X.kmer_k - 1 );
                    L.i = L.start > 0 ? L.start - 1 : 0xffffffffu;
                    seed_text_enter<TXT>( L, P );
                }
                break;
            case PH_P2_LEFT:
                if( !MS )
                    return false;
                if( L.i != 0xffffffffu )
                {
                    c = seed_qbyte_c<WIN>( L, P, X, L.i );
                    return true;
                }
                if( !TXT || L.ik[ 1 ] >= 0 )
                    mswap( L.ik[ 0 ], L.ik[ 1 ] );
                L.end = L.center;
                L.i = L.center + 1;
                L.phase = PH_P2_RIGHT;
                break;
            case PH_P2_RIGHT:
                if( !MS )
                    return false;
                if( L.i < L.qlen )
                {
                    c = comp_base( seed_qbyte_c<WIN>( L, P, X, L.i ) );
                    return true;
                }
                {
                    // finish the center (binarySeeding.h:226-251)
                    if( L.s1_start == L.start && L.s1_end == L.end )
                        seed_after_center( L, S, L.s1_start, L.s1_end - L.s1_start );
                    else
                    {
                        if( TXT && L.ik[ 1 ] < 0 )
                            seed_emit( L, S, L.start, L.end - L.start, -1 - L.ik[ 0 ], -1, 1 );
                        else
                            seed_emit( L, S, L.start, L.end - L.start, L.ik[ 1 ], L.ik[ 0 ], L.ik[ 2 ] );
                        const u32 s = L.start < L.s1_start ? L.start : L.s1_start;
                        const u32 e = L.end > L.s1_end ? L.end : L.s1_end;
                        seed_after_center( L, S, s, e - s );
                    }
                }
                break;
            case PH_SMEM_FWD:
                if( !SM )
                    return false;
                if( L.i < L.qlen )
                {
                    c = comp_base( seed_qbyte<WIN>( L, P, L.i ) );
                    return true;
                }
                // forward phase over: reverse the list (binarySeeding.h:343) and go backwards
                {
                    for( u32 a = 0, b = L.nCurr; a + 1 < b; a++, b-- )
                    {
                        const ma_segment t = smem_get_w( P, S, 0, a, L.center ), u = smem_get_w( P, S, 0, b - 1, L.center );
                        smem_put_w( P, S, 0, a, (u32)u.q_start, (u32)u.q_size, u.sa_start, u.sa_start_rc, u.sa_size );
                        smem_put_w( P, S, 0, b - 1, (u32)t.q_start, (u32)t.q_size, t.sa_start, t.sa_start_rc, t.sa_size );
                    }
                    L.nPrev = L.nCurr;
                    L.nCurr = 0;
                    L.flip = 0; // prev = smem_a, curr = smem_b
                    L.jPrev = 0;
                    L.nxtOk = 0;
                    L.bHaveOne = 0;
                    if( L.center != 0 && L.nPrev > 0 )
                    {
                        L.i = L.center - 1;
                        L.phase = PH_SMEM_BWD;
                    }
                    else
                    {
                        // cannot extend backwards at all (binarySeeding.h:354, 437-448)
                        if( L.nPrev > 0 )
                        {
                            const ma_segment f = smem_get_w( P, S, 0, 0, L.center );
                            seed_emit( L, S, (u32)f.q_start, (u32)f.q_size, f.sa_start, f.sa_start_rc, f.sa_size );
                        }
                        seed_after_center( L, S, L.retS, L.retE - L.retS );
                    }
                }
                break;
            case PH_SMEM_BWD:
            {
                if( !SM )
                    return false;
                if( L.jPrev < L.nPrev )
                {
                    const ma_segment s = L.nxtOk ? smem_unpack( L.nxt0, L.nxt1, L.i + 1 ) : smem_get_w( P, S, L.flip, L.jPrev, L.i + 1 );
                    if( P.smem_compact && L.jPrev + 1 < L.nPrev )
                        smem_prefetch_w( L, S, L.flip, L.jPrev + 1 );
                    else
                        L.nxtOk = 0;
                    L.ik[ 0 ] = s.sa_start;
                    L.ik[ 1 ] = s.sa_start_rc;
                    L.ik[ 2 ] = s.sa_size;
                    L.curQStart = (u32)s.q_start;
                    L.curQSize = (u32)s.q_size;
                    c = seed_qbyte<WIN>( L, P, L.i );
                    return true;
                }
                // end of one backward position: swap lists (binarySeeding.h:416-433)
                L.nxtOk = 0;
                L.flip ^= 1;
                L.nPrev = L.nCurr;
                L.nCurr = 0;
                L.jPrev = 0;
                L.bHaveOne = 0;
                bool fin = false;
                if( L.nPrev == 0 )
                    fin = true;
                else
                {
                    L.retS = L.i;
                    if( L.i == 0 )
                        fin = true;
                    else
                        L.i--;
                }
                if( fin )
                {
                    if( L.nPrev > 0 )
                    {
                        const ma_segment f = smem_get_w( P, S, L.flip, 0, L.i );
                        seed_emit( L, S, (u32)f.q_start, (u32)f.q_size, f.sa_start, f.sa_start_rc, f.sa_size );
                    }
                    seed_after_center( L, S, L.retS, L.retE - L.retS );
                }
                break;
            }
            default:
                return false;
        }
    }
}

// ---- apply the result of the extension requested by seed_prepare --------------------------------
template <bool SM = true, bool MS = true, bool TXT = false> MA_HD void seed_apply( SeedLane& L, const SeedParams& P, const SeedScratch& S, const i64 ok[ 3 ] )
{
    switch( L.phase )
    {
        case PH_P1_RIGHT:
        case PH_P2_RIGHT:
            if( !MS )
                break;
            if( seed_stop( P, ok, L.ik ) )
                L.i = L.qlen; // leave the loop; seed_prepare performs the transition
            else
            {
                L.end = L.i;
                L.ik[ 0 ] = ok[ 0 ], L.ik[ 1 ] = ok[ 1 ], L.ik[ 2 ] = ok[ 2 ];
                L.i++;
                seed_text_enter<TXT>( L, P );
            }
            break;
        case PH_P1_LEFT:
        case PH_P2_LEFT:
            if( !MS )
                break;
            if( seed_stop( P, ok, L.ik ) )
                L.i = 0xffffffffu;
            else
            {
                L.start = L.i;
                L.ik[ 0 ] = ok[ 0 ], L.ik[ 1 ] = ok[ 1 ], L.ik[ 2 ] = ok[ 2 ];
                L.i = L.i == 0 ? 0xffffffffu : L.i - 1;
                seed_text_enter<TXT>( L, P );
            }
            break;
        case PH_SMEM_FWD:
        { // binarySeeding.h:296-337
            if( !SM )
                break;
            auto push = [ & ]( u32 st, u32 sz, i64 a, i64 b, i64 c ) {
                if( L.nCurr < S.smem_cap )
                    smem_put_w( P, S, 0, L.nCurr, st, sz, a, b, c );
                else
                    L.err |= MA_ERR_SMEM_OVERFLOW;
                L.nCurr++;
            };
            if( ok[ 2 ] != L.ik[ 2 ] )
                push( L.center, L.i - L.center - 1, L.ik[ 1 ], L.ik[ 0 ], L.ik[ 2 ] );
            if( L.i == L.qlen - 1 && ok[ 2 ] != 0 )
                push( L.center, L.i - L.center, ok[ 1 ], ok[ 0 ], ok[ 2 ] );
            if( ok[ 2 ] == 0 || ( ok[ 2 ] <= (i64)P.min_amb && L.ik[ 2 ] <= (i64)P.max_amb ) )
                L.i = L.qlen; // break
            else
            {
                L.ik[ 0 ] = ok[ 0 ], L.ik[ 1 ] = ok[ 1 ], L.ik[ 2 ] = ok[ 2 ];
                L.retE = L.i;
                L.i++;
            }
            break;
        }
        case PH_SMEM_BWD:
        { // binarySeeding.h:380-413
            if( !SM )
                break;
            ma_segment s; // = prev[ L.jPrev ], kept in the lane state by seed_prepare (saves a memory round trip per step)
            s.q_start = L.curQStart, s.q_size = L.curQSize, s.sa_start = L.ik[ 0 ], s.sa_start_rc = L.ik[ 1 ], s.sa_size = L.ik[ 2 ];
            if( ok[ 2 ] <= (i64)P.min_amb && !L.bHaveOne )
            {
                seed_emit( L, S, (u32)s.q_start, (u32)s.q_size, s.sa_start, s.sa_start_rc, s.sa_size );
                L.bHaveOne = 1;
            }
            else if( ok[ 2 ] > (i64)P.min_amb || ( ok[ 2 ] > 0 && (u64)s.q_size >= (u64)P.max_amb ) )
            {
                // Twins.  The list is ordered by decreasing match length; after a few backward steps most of its entries
                // have shrunk to the SAME interval (for a unique read: all ~13 of them, the one locus) and differ only in
                // length.  extend_backward reads start and size only, so twins fail or survive together on every later
                // position, stay neighbours, and the later one is never emitted: when they fail the earlier one has set
                // bHaveOne (or found it set), and with uiMinAmbiguity == 0 a failed entry has size 0 and is not pushed
                // either (binarySeeding.h:380-413); at the start of the query only the front of the list is emitted
                // (:437-448).  Dropping the later twin here changes no emitted segment and no list's emptiness -- and
                // takes the backward phase of a 150 bp read from ~13 extensions per position to ~1 (a run-time switch:
                // with uiMinAmbiguity > 0 a failed twin of sufficient length IS pushed, so the lists stay as they are).
                const bool twin = P.smem_merge && L.nCurr > 0 && L.lastK == ok[ 0 ] && L.lastS == ok[ 2 ];
                if( !twin )
                {
                    if( L.nCurr < S.smem_cap )
                        smem_put_w( P, S, L.flip ^ 1u, L.nCurr, L.i, (u32)s.q_size + 1, ok[ 0 ], ok[ 1 ], ok[ 2 ] );
                    else
                        L.err |= MA_ERR_SMEM_OVERFLOW;
                    if( L.nCurr == 0 )
                        smem_pack( (u32)s.q_size + 1, ok[ 0 ], ok[ 1 ], ok[ 2 ], L.first0, L.first1 );
                    L.nCurr++;
                    L.lastK = ok[ 0 ], L.lastS = ok[ 2 ];
                }
            }
            L.jPrev++;
            break;
        }
        default:
            break;
    }
}

// BinarySeeding::execute's post filter (binarySeeding.cpp:172-175, numSeedsLarger segment.h:278-289):
// returns the number of segments to keep (0 = drop all)
MA_HD u32 seed_finish( const SeedLane& L, const SeedParams& P, const SeedScratch& S, const IndexView& X )
{
    u32 n = L.nseg < S.seg_cap ? L.nseg : S.seg_cap;
    if( !P.disable_heuristics && P.min_seed_size_drop != 0 )
    {
        const u64 sum = L.drop_sum; // == sum of stage[k].q_size / min_seed_size_drop over the n kept segments
        if( (double)sum < P.rel_min_seed_size_amount * (double)L.qlen && P.genome_size_disable < X.n )
            n = 0;
    }
    return n;
}

// memExtension (binarySeeding.h:460-537) for ONE start position i of a read: extend rightwards from q[i]; whenever rows
// drop out of the interval (and the match is longer than the minimal seed length and not too ambiguous), the dropped rows
// are maximal to the right, and those of them that cannot be extended to the left by q[i-1] are reported -- per row when
// only some of them can.  SINK::emit( q_start, q_size, sa_start, sa_size ) receives the segments in the reference's order;
// the intervals of dropped rows carry -1 as start of the reverse-complement interval (fMIndex.h:123-150), which
// extend_backward's start and size do not depend on.  Every position is independent: one lane per (read, position).
template <typename SINK>
MA_HD void mems_from( const IndexView& X, const SeedParams& P, const uint8_t* q, u32 qlen, u32 i, SINK& sink, u64& steps, u64& blocks )
{
    if( q[ i ] >= 4 )
        return;
    const i64 minAmb = (i64)P.min_amb, maxAmb = (i64)P.max_amb;
    i64 ik[ 3 ];
    init_interval( X, 3u - q[ i ], ik );
    u32 nb;
    for( u32 j = i + 1; j <= qlen && ik[ 2 ] > minAmb; j++ )
    {
        i64 ok[ 3 ] = { 0, -1, 0 };
        if( j < qlen && q[ j ] < 4 )
        {
            extend_backward( X, ik, 3u - q[ j ], ok, nb );
            steps++, blocks += nb;
        }
        if( j - i - 1 > P.min_seed_len && ok[ 2 ] < ik[ 2 ] && ik[ 2 ] < maxAmb )
        {
            // ik.revComp( ) minus ok.revComp( ): at most two runs of rows (do_for_difference)
            const i64 aS = ik[ 1 ], aE = ik[ 1 ] + ik[ 2 ], bS = ok[ 1 ], bE = ok[ 1 ] + ok[ 2 ];
            const i64 uiY = mmin( bS, aE ), uiX = mmax( bE, aS );
            for( int part = 0; part < 2; part++ )
            {
                const i64 dS = part == 0 ? aS : uiX, dN = part == 0 ? uiY - aS : aE - uiX;
                if( dN <= 0 )
                    continue; // start( ) < uiY / uiX < end( ) do not hold
                i64 xe[ 3 ] = { 0, -1, 0 };
                if( i > 0 )
                {
                    const i64 xd[ 3 ] = { dS, -1, dN };
                    extend_backward( X, xd, q[ i - 1 ], xe, nb );
                    steps++, blocks += nb;
                }
                if( xe[ 2 ] == 0 )
                    sink.emit( i, j - i - 1, dS, dN );
                else if( xe[ 2 ] < dN )
                {
                    i64 kLast = dS;
                    for( i64 k = dS; k <= dS + dN; k++ )
                    {
                        bool cut = k == dS + dN;
                        if( !cut )
                        {
                            const i64 xr[ 3 ] = { k, -1, 1 };
                            i64 xo[ 3 ];
                            extend_backward( X, xr, q[ i - 1 ], xo, nb );
                            steps++, blocks += nb;
                            cut = xo[ 2 ] != 0;
                        }
                        if( cut )
                        {
                            if( k > kLast )
                                sink.emit( i, j - i - 1, kLast, k - kLast );
                            kLast = k + 1;
                        }
                    }
                }
            }
        }
        ik[ 0 ] = ok[ 0 ], ik[ 1 ] = ok[ 1 ], ik[ 2 ] = ok[ 2 ];
    }
}

// One trip of a lane that seed_try / seed_prepare found ready to extend by c: an FM step -- or, TXT, whatever the lane's text mode
// is at: an LF step of the locate walk, the SA sample at its end, or a compare of up to 32 bases.  All loads are requested before
// any result is looked at, so the lanes of a wavefront share one memory round trip whichever of the four they do.
// steps counts the extend_backward calls, blocks every 64-byte line asked for (occ, LF, SA sample and text).
// FAST: see text_read_pack / text_pac_request
template <bool TXT, bool SM, bool MS, bool FAST> MA_HD void seed_step( SeedLane& L, const SeedParams& P, const SeedScratch& S, const IndexView& X, u32 c )
{
    i64 ok[ 3 ];
    u32 nb;
    if( !TXT )
    {
        extend_backward( X, L.ik, c, ok, nb );
        L.steps++;
        L.blocks += nb;
        seed_apply<SM, MS>( L, P, S, ok );
        return;
    }
    const bool fm = L.ik[ 1 ] >= 0, cmp = L.ik[ 1 ] == MA_TM_CMP;
    const bool smp = !fm && !cmp && ( L.ik[ 0 ] & ( ( (i64)1 << X.sa_shift ) - 1 ) ) == 0, lf = !fm && !cmp && !smp;
    const bool right = L.phase == PH_P1_RIGHT || L.phase == PH_P2_RIGHT;
    const u32 len = L.end - L.start + 1;
    // ---- requests
    ExtendReq R;
    R.hasK = R.hasL = false;
    R.kk = R.ll = 0;
    nb = 0;
    if( fm && c < 4 )
        extend_request( X, L.ik, R, nb );
    else if( lf && L.ik[ 0 ] != X.primary )
    {
        R.kk = L.ik[ 0 ] - ( L.ik[ 0 ] > X.primary );
        R.hasK = true;
        load_block( X.bwt, (u64)R.kk >> 7, R.bk );
        nb = 1;
    }
    i64 sv = 0;
    if( smp )
    {
        sv = sa_sample( X, L.ik[ 0 ] );
        nb = 1;
    }
    // compare: m bases, the read's from a on, the pack's from g on; rev: the locus lies on the reverse strand (the pack's bases
    // run against the read's and are complemented); top: the first base compared is the chunk's last
    u32 m = 0, a = 0;
    u64 g = 0, w0 = 0, w1 = 0;
    bool rev = false;
    if( cmp )
    {
        const u64 p = (u64)L.ik[ 0 ];
        if( right )
        {
            const u64 pos = p + len;
            rev = pos >= X.F;
            const u64 avail = pos >= X.n ? 0 : ( rev ? X.n - pos : X.F - pos );
            m = (u32)mmin<u64>( mmin<u64>( 32, L.qlen - L.i ), avail );
            a = L.i;
            g = rev ? X.n - pos - m : pos;
        }
        else
        {
            rev = p > X.F;
            const u64 avail = rev ? p - X.F : p;
            m = (u32)mmin<u64>( mmin<u64>( 32, (u64)L.i + 1 ), avail );
            a = L.i + 1 - m;
            g = rev ? X.n - p : p - m;
        }
        if( m )
        {
            text_pac_request<FAST>( X, g, w0, w1 );
            nb = 1 + ( ( text_pac_word( g ) & 63 ) == 56 ? 1 : 0 );
        }
    }
    L.blocks += nb;
    // ---- results
    if( fm )
    {
        if( c < 4 )
            extend_result( X, L.ik, c, R, ok );
        else
            ok[ 0 ] = ok[ 1 ] = ok[ 2 ] = 0;
        L.steps++;
        seed_apply<SM, MS, TXT>( L, P, S, ok );
    }
    else if( lf )
    {
        L.ik[ 0 ] = R.hasK ? inv_psi_in_block<true>( X, R.bk, R.kk ) : 0;
        L.ik[ 1 ]--;
    }
    else if( smp )
    {
        const i64 r = ( -1 - L.ik[ 1 ] ) + sv; // bwt_sa: where the pattern of ik[ 0 ] stands -- the reverse complement's in a right run
        L.ik[ 0 ] = right ? (i64)X.n - r - (i64)len : r;
        L.ik[ 1 ] = MA_TM_CMP;
    }
    else
    {
        u32 eq = 0;
        if( m )
        {
            u64 w, bad;
            text_read_pack<FAST>( L.q, a, m, w, bad );
            u64 t = text_pac_pack<FAST>( X, g, m, w0, w1 );
            if( rev )
            {
                w = rev2_64( w ) >> ( 64u - 2u * m );
                bad = rev2_64( bad ) >> ( 64u - 2u * m );
                t ^= low2m( m );
            }
            const u64 x = ( w ^ t ) | bad;
            const bool top = right == rev;
            eq = x == 0 ? m : top ? m - 1 - (u32)( 63 - __builtin_clzll( x ) ) / 2 : (u32)__builtin_ctzll( x ) / 2;
        }
        if( right )
        {
            L.end += eq;
            L.i = eq == m && m ? L.i + eq : L.qlen; // a mismatch, or the text's end: the run is over
        }
        else
        {
            L.ik[ 0 ] -= eq;
            L.start -= eq;
            L.i = eq == m && m ? L.i - eq : 0xffffffffu; // (i + 1 == eq: the read's start, the same value)
        }
    }
}

// Whole read on one lane (used by the host emulation and as the loop body of the kernel).
template <bool TXT = false, bool FAST = false> MA_HD void seed_read_serial( SeedLane& L, const SeedParams& P, const SeedScratch& S, const IndexView& X )
{
    u32 c;
    while( seed_prepare<false, false, true, true, TXT>( L, P, S, X, c ) )
        seed_step<TXT, true, true, FAST>( L, P, S, X, c );
}
} // namespace ma
