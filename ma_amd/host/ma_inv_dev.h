// ma_inv_dev.h -- the logic of "Detect Small Inversions" (SmallInversions, libs/ma/inc/ma/module/smallInversions.h:22-221) over
// FLAT records, written once for the host and the device:
//   scanDrops   forAllDropPos (smallInversions.h:53-116): the stretches between seeds of one alignment in which the running
//               score falls "Z Drop Inversions" below its maximum
//   stretchJob  the reverse-strand window of a stretch and its kswcpp call (smallInversions.h:118-133, 207)
//   assemble    cigar -> alignment (smallInversions.h:140-172) and the score filter (194-203); place( ) finishes the record
// Its users: the kernels of ma_amd/csrc/stage_inv.h (k_inv_scan, k_inv_assemble), and tests/emul/inv_dev_test.cpp, which runs
// the same functions on the host and pins them to the dumps the compiled reference wrote (tests/golden/inv.*) and to the host
// module's restatement SmallInversions::DropScan (ma_modules.h), the yardstick.  No containers, no arrays indexed at run time:
// include/ma_amd.h only.  The reference's quirks are kept as they are and listed HERE:
//   a stretch is reported only AT a seed op -- a drop behind the last seed is never reported;
//   the stretch before the first seed starts at the record's begin;
//   the score of a seed op is that of a match op;
//   the drop is max - current - max( dq, dr ) * extend, measured against the best prefix of the stretch, in int arithmetic;
//   it is compared with >= zdrop_inversion;
//   with disable_heuristics a stretch with an empty side yields an empty record.
#pragma once
#if !defined( MA_AMD_H ) // (libma_amd.so includes it by its own path)
#include "ma_amd.h"
#endif

#include <stdint.h>

#if defined( __HIPCC__ )
#define MA_INV_HD __host__ __device__ __forceinline__
#else
#define MA_INV_HD inline
#endif

namespace ma_inv
{
enum : uint32_t // MatchType (alignment.h:22-29), the op types of the flat records
{
    OP_SEED = 0,
    OP_MATCH = 1,
    OP_MISMATCH = 2,
    OP_INSERTION = 3,
    OP_DELETION = 4
};
enum : uint32_t // why a stretch cannot be served (stretchJob)
{
    OK = 0,
    ERR_BEYOND_READ = 1, // it ends beyond its read
    ERR_OUTSIDE_TEXT = 2, // its window is not inside the doubled text
    ERR_BRIDGING = 3 // its window lies on both strands (Pack::vExtractSubsection refuses it, pack.h:1147-1236)
};

// what the module reads of the parameters
struct Params
{
    int32_t match, mismatch, gap, extend;
    int32_t zdrop_inversion, zdrop, bandwidth_ext, harm_score_min, disable_heuristics;
};
MA_INV_HD Params params( const ma_params& rP )
{
    return Params{ rP.match, rP.mismatch, rP.gap, rP.extend, rP.zdrop_inversion, rP.zdrop, rP.bandwidth_ext, rP.harm_score_min,
                   rP.disable_heuristics };
}

// a stretch between two seeds: [startQ, endQ) on the query, [startR, endR) on the doubled text
struct Stretch
{
    uint64_t startQ, startR, endQ, endR;
};

// forAllDropPos over record k of a list with rec( k ) (begin_ref, begin_q, n_ops), opType( k, j ), opLen( k, j ); emit( Stretch )
// is called once per stretch, in the order of the walk.  The walk is n_ops steps.
template <typename List, typename Emit> MA_INV_HD void scanDrops( const Params& rP, const List& rList, uint32_t k, Emit&& emit )
{
    const auto xRec = rList.rec( k );
    uint64_t uiQ = xRec.begin_q, uiR = xRec.begin_ref; // current position
    uint64_t uiFromQ = uiQ, uiFromR = uiR; // where the open stretch began (end of the last seed)
    uint64_t uiBestQ = uiQ, uiBestR = uiR; // position of the best prefix of the stretch
    const int iNone = -2147483647 - 1;
    int iScore = 0, iBest = iNone, iDrop = 0;
    for( uint32_t j = 0; j < xRec.n_ops; j++ )
    {
        const uint64_t uiType = rList.opType( k, j ), uiLen = rList.opLen( k, j );
        if( uiType == OP_SEED )
        {
            if( iDrop >= rP.zdrop_inversion )
                emit( Stretch{ uiFromQ, uiFromR, uiQ, uiR } );
            // the stretch restarts behind the seed that is about to be consumed
            uiFromQ = uiQ + uiLen;
            uiFromR = uiR + uiLen;
            iScore = iDrop = 0;
            iBest = iNone;
        }
        if( uiType == OP_SEED || uiType == OP_MATCH )
            iScore += rP.match * (int)uiLen;
        else if( uiType == OP_MISMATCH )
            iScore -= rP.mismatch * (int)uiLen;
        else
            iScore -= rP.gap + rP.extend * (int)uiLen;
        uiQ += uiType != OP_DELETION ? uiLen : 0;
        uiR += uiType != OP_INSERTION ? uiLen : 0;
        if( iScore >= iBest )
        {
            iBest = iScore;
            uiBestQ = uiQ;
            uiBestR = uiR;
            continue;
        }
        const uint64_t uiDq = uiQ - uiBestQ, uiDr = uiR - uiBestR;
        const int iAway = (int)( uiDq > uiDr ? uiDq : uiDr );
        const int iNow = iBest - iScore - iAway * rP.extend;
        iDrop = iDrop > iNow ? iDrop : iNow;
    }
}

// The kswcpp call of a stretch (smallInversions.h:118-133): the query [startQ, endQ) against the window
// [uiN - ( endR + 1 ), uiN - ( startR + 1 )) of the doubled text -- Pack::uiPositionToReverseStrand of both ends (pack.h:924-927) --
// with uiN = forward + reverse size, uiF = forward size.  q_off / t_off are the caller's.  A side may be empty: no DP then and an
// empty cigar (kswcpp_core.h:362-364).
struct Job
{
    uint64_t winBegin, winEnd;
    int32_t qlen, tlen, w, zdrop, flag;
    MA_INV_HD bool hasDp( ) const
    {
        return qlen > 0 && tlen > 0;
    }
};
MA_INV_HD uint32_t stretchJob( const Params& rP, const Stretch& rS, uint64_t uiReadLength, uint64_t uiN, uint64_t uiF, Job& rJob )
{
    if( rS.endQ < rS.startQ || rS.endQ > uiReadLength )
        return ERR_BEYOND_READ;
    if( rS.endR < rS.startR || rS.endR >= uiN )
        return ERR_OUTSIDE_TEXT;
    rJob.winBegin = uiN - ( rS.endR + 1 );
    rJob.winEnd = uiN - ( rS.startR + 1 );
    if( rJob.winBegin < rJob.winEnd && ( rJob.winBegin >= uiF ) != ( rJob.winEnd - 1 >= uiF ) )
        return ERR_BRIDGING;
    if( rS.endQ - rS.startQ > 0x7fffffffull || rJob.winEnd - rJob.winBegin > 0x7fffffffull )
        return ERR_OUTSIDE_TEXT;
    rJob.qlen = (int32_t)( rS.endQ - rS.startQ );
    rJob.tlen = (int32_t)( rJob.winEnd - rJob.winBegin );
    rJob.w = rP.bandwidth_ext;
    rJob.zdrop = rP.zdrop;
    rJob.flag = 0;
    return OK;
}
// words of ops an assembled record can need at most
MA_INV_HD uint64_t opsBound( const Job& rJob )
{
    return (uint64_t)rJob.qlen + (uint64_t)rJob.tlen + 2;
}

// smallInversions.h:140-172: the cigar's M runs split base by base into match / mismatch, I and D runs as they are, appended to a
// builder with append( type, length ) -- Alignment::append, so that runs merge and the score is Alignment's.  cigar( i ) is word i,
// query( i ) the code of query position startQ + i, window( i ) the code at window offset i.  false: a symbol that is none of M I D.
template <typename Cigar, typename Query, typename Window, typename Builder>
MA_INV_HD bool assemble( uint32_t uiCigarWords, const Cigar& cigar, const Query& query, const Window& window, Builder& rBuilder )
{
    uint64_t qPos = 0, rPos = 0;
    for( uint32_t c = 0; c < uiCigarWords; c++ )
    {
        const uint32_t uiWord = cigar( c ), uiSymbol = uiWord & 0xf, uiAmount = uiWord >> 4;
        if( uiSymbol == 0 )
        {
            for( uint32_t uiPos = 0; uiPos < uiAmount; uiPos++ )
                rBuilder.append( query( qPos + uiPos ) == window( rPos + uiPos ) ? OP_MATCH : OP_MISMATCH, 1 );
            qPos += uiAmount;
            rPos += uiAmount;
        }
        else if( uiSymbol == 1 )
        {
            rBuilder.append( OP_INSERTION, uiAmount );
            qPos += uiAmount;
        }
        else if( uiSymbol == 2 )
        {
            rBuilder.append( OP_DELETION, uiAmount );
            rPos += uiAmount;
        }
        else
            return false;
    }
    return true;
}
// smallInversions.h:194: is the assembled alignment reported?
MA_INV_HD bool kept( const Params& rP, int64_t iScore )
{
    return rP.disable_heuristics != 0 || iScore > (int64_t)( rP.harm_score_min * rP.match );
}
// smallInversions.h:196-203: a kept record (anything with begin_q, end_q, begin_ref, end_ref, secondary, supplementary, mapq,
// soc_index; assembled from 0 / 0) takes its place on the query and the text and its parent's strip
template <typename Record, typename Parent> MA_INV_HD void place( Record& rRec, const Parent& rParent, const Stretch& rS, const Job& rJob )
{
    rRec.begin_q += rS.startQ;
    rRec.end_q += rS.startQ;
    rRec.begin_ref += rJob.winBegin;
    rRec.end_ref += rJob.winBegin;
    rRec.supplementary = 1;
    rRec.secondary = 0;
    rRec.mapq = 0;
    rRec.soc_index = rParent.soc_index;
}
} // namespace ma_inv
