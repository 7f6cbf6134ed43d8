// ma_pair_flat.h -- PairedReads::execute (pairedReads.cpp:14-131) on FLAT records: the pick of one alignment per mate out of
// the two MappingQuality lists of a pair, restated once for three users:
//   - the device stage (ma_amd/csrc/stage_pair.h) runs scan() / rate() / confidence() of this header inside its kernel;
//   - libma_amd.so finishes the pairs the kernel hands back (tied best key among more candidates than it sorts on chip) with
//     pick() on compact per-alignment fields;
//   - host callers and the CPU tests run pickFlat() on ma_alignment arrays (tests/test_pairs_host.py pins it to the goldens
//     the compiled reference wrote and to PairedReads::execute of ma_modules.h).
// No reference headers, no containers: include/ma_amd.h only.
//
// What the reference does per pair: every (i, j) with both alignments of non-zero length is a candidate with key
// score_i + score_j; mates on opposite strands whose begins lie mean +- 3 std apart are a PROPER pair, key =
// (int64)(key * bonus).  Highest key wins, proper before improper among equal keys; among several candidates of the best
// (key, proper) the reference takes what libstdc++'s unstable std::sort over ALL candidates puts first.  The two picked
// records lose secondary / supplementary; a proper winner among more than one candidate sets both mapping qualities.
#pragma once
#if !defined( MA_AMD_H ) // (libma_amd.so includes it by its own path)
#include "ma_amd.h"
#endif

#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#if defined( __HIPCC__ )
#define MA_PAIR_HD __host__ __device__ __forceinline__
#else
#define MA_PAIR_HD inline
#endif

namespace ma_pair
{
struct Params
{
    uint64_t mean; // (size_t)xMeanPairedReadDistance: truncated before it is compared
    double std, bonus; // xStdPairedReadDistance, xPairedBonus
    int32_t match;
    uint64_t n; // Pack::uiUnpackedSizeForwardPlusReverse
};
inline Params params( const ma_params& P, uint64_t uiRefLenFwdRev )
{
    return Params{ (uint64_t)P.mean_paired_dist, P.std_paired_dist, P.paired_bonus, P.match, uiRefLenFwdRev };
}

struct Cand // 16 bytes: the kernel sorts up to 32 of them per lane in LDS
{
    int64_t key;
    uint32_t i; // index in the first mate's list
    uint32_t jp; // index in the second mate's list | proper << 31
    MA_PAIR_HD bool proper( ) const
    {
        return ( jp >> 31 ) != 0;
    }
    MA_PAIR_HD uint32_t j( ) const
    {
        return jp & 0x7fffffffu;
    }
    // the reference's sort order (pairedReads.cpp:97-105)
    MA_PAIR_HD bool before( const Cand& o ) const
    {
        return key != o.key ? key > o.key : ( proper( ) && !o.proper( ) );
    }
    MA_PAIR_HD bool sameKey( const Cand& o ) const
    {
        return key == o.key && proper( ) == o.proper( );
    }
};
struct Before
{
    MA_PAIR_HD bool operator( )( const Cand& a, const Cand& b ) const
    {
        return a.before( b );
    }
};

enum : uint32_t
{
    NONE = 0, // both lists empty: no records
    SECOND_LIST = 1, // first mate's list empty: the second mate's whole list
    FIRST_LIST = 2, // second mate's list empty: the first mate's whole list
    PICKED = 3, // records i of the first and j of the second mate
    NO_CANDIDATE = 4, // both lists non-empty, every candidate of length 0: the call fails
    TIED_UNSORTED = 5 // scan() only: several candidates share the best key, the caller has to sort
};
struct Pick
{
    uint32_t kind, i, j, set_mapq;
    double mapq; // both records' mapping quality when set_mapq
};

// A list is anything with: uint32_t size(); int64_t score(k); uint64_t begin(k); bool nonzero(k) [length() != 0];
// uint32_t seeds(k) [Alignment::getNumSeeds: ops of type seed].
template <typename LA, typename LB> MA_PAIR_HD Cand rate( const LA& a, uint32_t i, const LB& b, uint32_t j, const Params& P )
{
    Cand c{ a.score( i ) + b.score( j ), i, j };
    const uint64_t uiF = P.n / 2, uiB1 = a.begin( i ), uiB2 = b.begin( j );
    if( ( uiB1 >= uiF ) == ( uiB2 >= uiF ) )
        return c; // same strand
    const uint64_t uiMirrored = P.n - ( uiB2 + 1 );
    const double fDist = (double)( uiB1 > uiMirrored ? uiB1 - uiMirrored : uiMirrored - uiB1 );
    const double fLo = (double)P.mean - P.std * 3, fHi = (double)P.mean + P.std * 3;
    if( fDist >= fLo && fDist <= fHi )
    {
        c.key = (int64_t)( c.key * P.bonus );
        c.jp |= 0x80000000u;
    }
    return c;
}

struct Scan
{
    Cand best;
    uint64_t nCand; // candidates in all
    uint32_t nTied; // ... of them with the best (key, proper)
    int64_t second; // highest key among the others (when the best is unique and nCand > 1)
};
// One pass over the candidates in the reference's order (i outer, j inner)
template <typename LA, typename LB> MA_PAIR_HD Scan scan( const LA& a, const LB& b, const Params& P )
{
    Scan s{ Cand{ 0, 0, 0 }, 0, 0, INT64_MIN };
    const uint32_t n1 = a.size( ), n2 = b.size( );
    for( uint32_t i = 0; i < n1; i++ )
    {
        if( !a.nonzero( i ) )
            continue;
        for( uint32_t j = 0; j < n2; j++ )
        {
            if( !b.nonzero( j ) )
                continue;
            const Cand c = rate( a, i, b, j, P );
            if( s.nCand == 0 )
                s.best = c, s.nTied = 1;
            else if( c.before( s.best ) )
            {
                s.second = s.best.key; // the former best is one of the others now, and no other key was higher
                s.best = c, s.nTied = 1;
            }
            else
            {
                if( c.sameKey( s.best ) )
                    s.nTied++;
                s.second = c.key > s.second ? c.key : s.second;
            }
            s.nCand++;
        }
    }
    return s;
}
// All candidates in that order into v (room for scan().nCand of them)
template <typename LA, typename LB> MA_PAIR_HD void fill( const LA& a, const LB& b, const Params& P, Cand* v )
{
    const uint32_t n1 = a.size( ), n2 = b.size( );
    uint64_t w = 0;
    for( uint32_t i = 0; i < n1; i++ )
        for( uint32_t j = 0; j < n2; j++ )
            if( a.nonzero( i ) && b.nonzero( j ) )
                v[ w++ ] = rate( a, i, b, j, P );
}

// The pair's mapping quality (pairedReads.cpp:113-126): single precision, widened at the end
template <typename LA, typename LB>
MA_PAIR_HD Pick confidence( const LA& a, const LB& b, const Params& P, const Cand& win, int64_t iRunnerUp, uint64_t nCand,
                            uint64_t uiQLen1, uint64_t uiQLen2 )
{
    Pick p{ PICKED, win.i, win.j( ), 0, 0.0 };
    if( !win.proper( ) || nCand <= 1 )
        return p;
    float fConfidence = ( (float)( win.key - iRunnerUp ) ) / win.key;
    if( a.seeds( p.i ) <= 1 && b.seeds( p.j ) <= 1 )
        fConfidence /= 2;
    const bool bStrongA = (double)a.score( p.i ) >= (double)( (uint64_t)P.match * uiQLen1 ) * 0.8 && a.size( ) >= 3;
    const bool bStrongB = (double)b.score( p.j ) >= (double)( (uint64_t)P.match * uiQLen2 ) * 0.8 && b.size( ) >= 3;
    if( bStrongA || bStrongB )
        fConfidence *= 2;
    p.set_mapq = 1;
    p.mapq = fConfidence > 1 ? 1 : fConfidence;
    return p;
}

// Everything but the sort of the tied case: kind TIED_UNSORTED tells the caller to fill(), sort with Before and call
// confidence( v[ 0 ], v[ 0 ].key ) itself.
template <typename LA, typename LB>
MA_PAIR_HD Pick pickUntied( const LA& a, const LB& b, const Params& P, uint64_t uiQLen1, uint64_t uiQLen2, Scan& s )
{
    s = Scan{ Cand{ 0, 0, 0 }, 0, 0, INT64_MIN };
    if( a.size( ) == 0 )
        return Pick{ b.size( ) == 0 ? (uint32_t)NONE : (uint32_t)SECOND_LIST, 0, 0, 0, 0.0 };
    if( b.size( ) == 0 )
        return Pick{ FIRST_LIST, 0, 0, 0, 0.0 };
    s = scan( a, b, P );
    if( s.nCand == 0 )
        return Pick{ NO_CANDIDATE, 0, 0, 0, 0.0 };
    if( s.nTied > 1 )
        return Pick{ TIED_UNSORTED, 0, 0, 0, 0.0 };
    return confidence( a, b, P, s.best, s.second, s.nCand, uiQLen1, uiQLen2 );
}

inline const char* noCandidateText( )
{
    return "PairedReads: no alignment of non-zero length to pair";
}

// The whole pick on the host; the tied case goes through the real std::sort like the reference's.
template <typename LA, typename LB> inline Pick pick( const LA& a, const LB& b, const Params& P, uint64_t uiQLen1, uint64_t uiQLen2 )
{
    Scan s;
    Pick p = pickUntied( a, b, P, uiQLen1, uiQLen2, s );
    if( p.kind != TIED_UNSORTED )
        return p;
    std::vector<Cand> v( s.nCand );
    fill( a, b, P, v.data( ) );
    std::sort( v.begin( ), v.end( ), Before( ) );
    return confidence( a, b, P, v[ 0 ], v[ 0 ].key, s.nCand, uiQLen1, uiQLen2 );
}

// A MappingQuality list as the C ABI returns it (ma_batch_get_mapq_alignments): records + (type, length) pairs
struct FlatList
{
    const ma_alignment* a;
    uint32_t n;
    const uint64_t* ops;
    uint32_t size( ) const
    {
        return n;
    }
    int64_t score( uint32_t k ) const
    {
        return a[ k ].score;
    }
    uint64_t begin( uint32_t k ) const
    {
        return (uint64_t)a[ k ].begin_ref;
    }
    bool nonzero( uint32_t k ) const
    {
        for( uint32_t o = 0; o < a[ k ].n_ops; o++ )
            if( ops[ 2 * ( a[ k ].ops_off + o ) + 1 ] != 0 )
                return true;
        return false;
    }
    uint32_t seeds( uint32_t k ) const
    {
        uint32_t c = 0;
        for( uint32_t o = 0; o < a[ k ].n_ops; o++ )
            c += ops[ 2 * ( a[ k ].ops_off + o ) ] == 0 ? 1 : 0; // MatchType::seed
        return c;
    }
};
inline Pick pickFlat( const ma_alignment* a1, uint32_t n1, const ma_alignment* a2, uint32_t n2, const uint64_t* ops, uint64_t uiQLen1,
                      uint64_t uiQLen2, const Params& P )
{
    return pick( FlatList{ a1, n1, ops }, FlatList{ a2, n2, ops }, P, uiQLen1, uiQLen2 );
}
// Records of the pair in the order PairedReads::execute returns them, with its changes applied (ops_off still counts in
// `ops`); mate[k] = 1: record of the first mate, other[k] = index of the partner's record within the pair or -1.  Returns
// the number of records; out / mate / other need room for max( n1, n2, 2 ).  A NO_CANDIDATE pick yields none.
inline uint32_t records( const Pick& p, const ma_alignment* a1, uint32_t n1, const ma_alignment* a2, uint32_t n2, ma_alignment* out,
                         int32_t* mate, int32_t* other )
{
    if( p.kind == FIRST_LIST || p.kind == SECOND_LIST )
    {
        const ma_alignment* src = p.kind == FIRST_LIST ? a1 : a2;
        const uint32_t n = p.kind == FIRST_LIST ? n1 : n2;
        for( uint32_t k = 0; k < n; k++ )
            out[ k ] = src[ k ], mate[ k ] = p.kind == FIRST_LIST ? 1 : 0, other[ k ] = -1;
        return n;
    }
    if( p.kind != PICKED )
        return 0;
    out[ 0 ] = a1[ p.i ], out[ 1 ] = a2[ p.j ];
    for( int k = 0; k < 2; k++ )
    {
        out[ k ].secondary = out[ k ].supplementary = 0;
        if( p.set_mapq )
            out[ k ].mapq = p.mapq;
        mate[ k ] = 1 - k, other[ k ] = 1 - k;
    }
    return 2;
}
} // namespace ma_pair
