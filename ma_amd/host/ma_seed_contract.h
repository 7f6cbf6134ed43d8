// ma_seed_contract.h -- what ma_chain_batch relies on in seeds and strips handed in (ma_batch_set_seeds, ma_batch_set_soc_heap;
// include/ma_amd.h states the contract), checked on the host before anything is uploaded.  libma_amd.so (ma_amd/csrc/pipeline.hip)
// calls these two functions; tests/emul/seed_contract_test.cpp drives them clause by clause.  Plain C++: no HIP.
//
// Why each clause: the chain stage indexes the contig table by r_start (seq_id_for_position), computes n - r_start - 1 for a
// reverse-strand seed, casts every field to u64 and sums len without a bound, and carves its scratch by the seed offsets; the
// sweep trusts delta as given, and a delta that is not ExtractSeeds' puts a seed into a strip of another contig.
//
// A seed is handed in as ExtractSeeds leaves it (segment.h:89-113, stripOfConsideration.h:41-53, 97-112): a match at position p of
// the doubled text (forward strand . reverse complement, n = 2 F) with p < F has r_start = p, on_forward = 1; one with p >= F is
// mirrored, r_start = n - 1 - p, on_forward = 0.  Either way r_start is a forward position.  The reference's extraction checks
// neither contig borders nor the strand junction -- a match of the seeding may run over both, and such seeds reach
// StripOfConsiderationSeeds::execute --, so the contract bounds a seed by the doubled text only: p + len <= n.
#pragma once
#include "../../include/ma_amd.h"
#include <stdint.h>
#include <string>

namespace ma_contract
{
// "" if the seeds keep the contract, else the message (without the function's name) naming the read and the seed.
// roff: the reads' offsets (n_reads + 1); cstart: the contigs' forward start positions, ascending, cstart[0] == 0; F: forward length.
inline std::string seeds_violation( const uint64_t* seed_off, const ma_seed* seeds, uint64_t n_reads, const uint64_t* roff,
                                    const uint64_t* cstart, uint64_t n_contigs, uint64_t F )
{
    if( seed_off[ 0 ] != 0 )
        return "seed_off does not start at 0";
    for( uint64_t r = 0; r < n_reads; r++ )
        if( seed_off[ r + 1 ] < seed_off[ r ] )
            return "seed_off decreases at read " + std::to_string( r );
    if( seed_off[ n_reads ] > 0xffffffffull )
        return "more than 2^32 - 1 seeds";
    const uint64_t n = 2 * F;
    for( uint64_t r = 0; r < n_reads; r++ )
    {
        const uint64_t qlen = roff[ r + 1 ] - roff[ r ];
        for( uint64_t k = seed_off[ r ]; k < seed_off[ r + 1 ]; k++ )
        {
            const ma_seed& x = seeds[ k ];
            const std::string where = " (read " + std::to_string( r ) + ", seed " + std::to_string( k - seed_off[ r ] ) + ")";
            if( x.q_start < 0 || x.len < 0 || x.r_start < 0 || x.delta < 0 )
                return "negative field" + where;
            if( x.len < 1 )
                return "empty seed" + where;
            if( (uint64_t)x.q_start > qlen || (uint64_t)x.len > qlen - (uint64_t)x.q_start )
                return "seed ends beyond its read of " + std::to_string( qlen ) + " bases" + where;
            if( x.on_forward > 1 )
                return "on_forward is neither 0 nor 1" + where;
            if( (uint64_t)x.r_start >= F )
                return "r_start outside the forward text of " + std::to_string( F ) + " bases" + where;
            // the match on the doubled text: [r_start, r_start + len) forward, [n - 1 - r_start, n - 1 - r_start + len) mirrored
            if( x.on_forward ? (uint64_t)x.len > n - (uint64_t)x.r_start : (uint64_t)x.len > (uint64_t)x.r_start + 1 )
                return "seed ends beyond the doubled text of " + std::to_string( n ) + " bases" + where;
            // ExtractSeeds::setDeltaOfSeed with rectangular strips: r + (qlen - q) + (qlen + 1) * contig of r
            uint64_t lo = 0, hi = n_contigs; // the last contig that starts at or before r_start
            while( hi - lo > 1 )
            {
                const uint64_t mid = lo + ( hi - lo ) / 2;
                if( cstart[ mid ] <= (uint64_t)x.r_start )
                    lo = mid;
                else
                    hi = mid;
            }
            const uint64_t want = (uint64_t)x.r_start + ( qlen - (uint64_t)x.q_start ) + ( qlen + 1 ) * lo;
            if( (uint64_t)x.delta != want )
                return "delta is " + std::to_string( x.delta ) + ", ExtractSeeds computes " + std::to_string( want ) + where;
        }
    }
    return "";
}

// the strips of ma_batch_set_soc_heap against the seed counts (seed_off as checked above)
inline std::string socs_violation( const uint64_t* soc_off, const ma_soc* socs, const uint64_t* seed_off, uint64_t n_reads )
{
    if( soc_off[ 0 ] != 0 )
        return "soc_off does not start at 0";
    for( uint64_t r = 0; r < n_reads; r++ )
        if( soc_off[ r + 1 ] < soc_off[ r ] )
            return "soc_off decreases at read " + std::to_string( r );
    for( uint64_t r = 0; r < n_reads; r++ )
    {
        if( seed_off[ r + 1 ] < seed_off[ r ] )
            return "seed_off decreases at read " + std::to_string( r );
        const uint64_t nSeeds = seed_off[ r + 1 ] - seed_off[ r ];
        if( soc_off[ r + 1 ] - soc_off[ r ] > nSeeds )
            return "more strips than seeds (read " + std::to_string( r ) + ")";
        for( uint64_t k = soc_off[ r ]; k < soc_off[ r + 1 ]; k++ )
        {
            const ma_soc& s = socs[ k ];
            const std::string where = " (read " + std::to_string( r ) + ", strip " + std::to_string( k - soc_off[ r ] ) + ")";
            if( s.begin > s.end || s.end > nSeeds )
                return "strip outside the read's " + std::to_string( nSeeds ) + " seeds" + where;
            if( s.n_seeds != s.end - s.begin )
                return "n_seeds is not end - begin" + where;
        }
    }
    return "";
}
} // namespace ma_contract
