// TEST INFRASTRUCTURE ONLY (part of ma_oracle.cpp).
// NeedlemanWunsch (needlemanWunsch.h:111-134, needlemanWunsch.cpp:24-877), Alignment::append /
// removeDangeling / larger (alignment.cpp:10-98,240-296, alignment.h:819-886), MappingQuality
// (mappingQuality.cpp:11-131, alignment.h:659-735).
namespace
{
// Alignment::append (alignment.cpp:10-98)
static void alnAppend( const ma_or_params& P, Aln& A, int type, u64 size )
{
    if( size == 0 )
        return;
    if( type == MT_SEED || type == MT_MATCH )
    {
        A.score += (i64)( (u64)P.match * size );
        A.eRef += size;
        A.eQ += size;
    }
    else if( type == MT_MISS )
    {
        A.score -= (i64)( (u64)P.mismatch * size );
        A.eRef += size;
        A.eQ += size;
    }
    else
    {
        if( type == MT_INS )
            A.eQ += size;
        else
            A.eRef += size;
        if( A.data.size( ) != 0 && A.data.back( ).first == type )
        {
            size += A.data.back( ).second;
            A.length -= A.data.back( ).second;
            if( (u64)P.extend * A.data.back( ).second + (u64)P.gap < (u64)P.sv_penalty )
                A.score += (i64)( (u64)P.extend * A.data.back( ).second + (u64)P.gap );
            else
                A.score += (i64)(u64)P.sv_penalty;
            A.data.pop_back( );
        }
        if( (u64)P.extend * size + (u64)P.gap < (u64)P.sv_penalty )
            A.score -= (i64)( (u64)P.extend * size + (u64)P.gap );
        else
            A.score -= (i64)(u64)P.sv_penalty;
    }
    if( A.data.size( ) != 0 && A.data.back( ).first == type )
        A.data.back( ).second += size;
    else
        A.data.push_back( std::make_pair( type, size ) );
    A.length += size;
}

// Alignment::removeDangeling (alignment.cpp:240-296)
static void alnRemoveDangling( const ma_or_params& P, Aln& A )
{
    if( A.data.empty( ) )
        return;
    auto refund = [ & ]( u64 len ) {
        if( (u64)P.gap + (u64)P.extend * len < (u64)P.sv_penalty )
            A.score += (i64)( (u64)P.gap + (u64)P.extend * len );
        else
            A.score += (i64)(u64)P.sv_penalty;
    };
    while( A.data.front( ).first == MT_DEL || A.data.front( ).first == MT_INS )
    {
        if( A.data.front( ).first == MT_DEL )
            A.bRef += A.data.front( ).second;
        else
            A.bQ += A.data.front( ).second;
        refund( A.data.front( ).second );
        A.length -= A.data.front( ).second;
        A.data.erase( A.data.begin( ), A.data.begin( ) + 1 );
    }
    while( A.data.back( ).first == MT_DEL || A.data.back( ).first == MT_INS )
    {
        if( A.data.back( ).first == MT_DEL )
            A.eRef -= A.data.back( ).second;
        else
            A.eQ -= A.data.back( ).second;
        refund( A.data.back( ).second );
        A.length -= A.data.back( ).second;
        A.data.pop_back( );
    }
}

struct NwCtx
{
    const Ctx& c;
    std::vector<uint8_t>& Q; // query codes (temporarily reversed in place like the reference does)
    std::vector<uint8_t>& R; // extracted reference window
};

inline void appendMatchRun( const NwCtx& n, Aln& A, u64 qPos, u64 rPos, uint32_t amount )
{
    for( uint32_t k = 0; k < amount; k++ )
        alnAppend( n.c.P, A, n.Q[ k + qPos ] == n.R[ k + rPos ] ? MT_MATCH : MT_MISS, 1 );
}

// ksw_ext (needlemanWunsch.cpp:24-55)
inline void kswExt( const NwCtx& n, u64 fromQ, u64 toQ, u64 fromR, u64 toR, bool bRef, Ez& ez )
{
    kswDispatch( (int)( toQ - fromQ ), n.Q.data( ) + fromQ, (int)( toR - fromR ), n.R.data( ) + fromR, n.c.P,
                 n.c.P.bandwidth_ext, (int)(size_t)n.c.P.zdrop,
                 bRef ? ( KSW_EZ_EXTZ_ONLY | KSW_EZ_RIGHT | KSW_EZ_REV_CIGAR ) : KSW_EZ_EXTZ_ONLY, ez );
}

// NeedlemanWunsch::ksw (needlemanWunsch.cpp:82-169) with ksw_simplified (57-79)
static void nwKsw( const NwCtx& n, u64 fromQ, u64 toQ, u64 fromR, u64 toR, Aln& A )
{
    if( toR <= fromR )
        if( toQ <= fromQ )
            return;
    if( toQ <= fromQ )
    {
        alnAppend( n.c.P, A, MT_DEL, toR - fromR );
        return;
    }
    if( toR <= fromR )
    {
        alnAppend( n.c.P, A, MT_INS, toQ - fromQ );
        return;
    }
    Ez ez;
    int qlen = (int)( toQ - fromQ ), tlen = (int)( toR - fromR );
    int w = n.c.P.min_bandwidth_gap;
    if( std::abs( tlen - qlen ) + 10 > w )
        w = std::abs( tlen - qlen ) + 10;
    kswDispatch( qlen, n.Q.data( ) + fromQ, tlen, n.R.data( ) + fromR, n.c.P, w, -1, 0, ez );
    u64 qPos = fromQ, rPos = fromR;
    for( uint32_t cg : ez.cigar )
    {
        uint32_t sym = cg & 0xf, amount = cg >> 4;
        switch( sym )
        {
            case 0:
                appendMatchRun( n, A, qPos, rPos, amount );
                qPos += amount;
                rPos += amount;
                break;
            case 1:
                alnAppend( n.c.P, A, MT_INS, amount );
                qPos += amount;
                break;
            case 2:
                alnAppend( n.c.P, A, MT_DEL, amount );
                rPos += amount;
                break;
        }
    }
    // (sic) leftover query as deletion, leftover reference as insertion (needlemanWunsch.cpp:167-168)
    alnAppend( n.c.P, A, MT_DEL, toQ - qPos );
    alnAppend( n.c.P, A, MT_INS, toR - rPos );
}

// NeedlemanWunsch::ksw_dual_ext (needlemanWunsch.cpp:239-497)
static void nwDualExt( const NwCtx& n, u64 fromQ, u64 toQ, u64 fromR, u64 toR, Aln& A )
{
    const ma_or_params& P = n.c.P;
    Ez ezL, ezR;
    kswExt( n, fromQ, toQ, fromR, toR, false, ezL );
    std::reverse( n.Q.begin( ) + fromQ, n.Q.begin( ) + toQ );
    std::reverse( n.R.begin( ) + fromR, n.R.begin( ) + toR );
    kswExt( n, fromQ, toQ, fromR, toR, true, ezR );
    std::reverse( n.Q.begin( ) + fromQ, n.Q.begin( ) + toQ );
    std::reverse( n.R.begin( ) + fromR, n.R.begin( ) + toR );

    u64 qCenter = ( fromQ + (u64)(i64)ezL.max_q + ( toQ - (u64)(i64)ezR.max_q - 1 ) ) / 2;
    qCenter = std::max( fromQ, std::min( toQ, qCenter ) );
    u64 rCenter = ( fromR + (u64)(i64)ezL.max_t + ( toR - (u64)(i64)ezR.max_t - 1 ) ) / 2;
    rCenter = std::max( fromR, std::min( toR, rCenter ) );

    u64 qPos = fromQ, rPos = fromR;
    if( rPos != rCenter && qPos != qCenter )
        for( size_t i = 0; i < ezL.cigar.size( ); ++i )
        {
            uint32_t sym = ezL.cigar[ i ] & 0xf, amount = ezL.cigar[ i ] >> 4;
            switch( sym )
            {
                case 0:
                    if( qPos + amount > qCenter )
                        amount = (uint32_t)( qCenter - qPos );
                    if( rPos + amount > rCenter )
                        amount = (uint32_t)( rCenter - rPos );
                    appendMatchRun( n, A, qPos, rPos, amount );
                    qPos += amount;
                    rPos += amount;
                    break;
                case 1:
                    if( qPos + amount > qCenter )
                        amount = (uint32_t)( qCenter - qPos );
                    alnAppend( P, A, MT_INS, amount );
                    qPos += amount;
                    break;
                case 2:
                    if( rPos + amount > rCenter )
                        amount = (uint32_t)( rCenter - rPos );
                    alnAppend( P, A, MT_DEL, amount );
                    rPos += amount;
                    break;
            }
            if( rPos == rCenter )
                break;
            if( qPos == qCenter )
                break;
        }
    u64 rPosRight = toR - (u64)(i64)ezR.max_t - 1;
    u64 qPosRight = toQ - (u64)(i64)ezR.max_q - 1;
    uint32_t notUnrolled = 0;
    int lastType = MT_SEED;
    size_t i = 0;
    for( ; i < ezR.cigar.size( ); ++i )
    {
        if( rPosRight >= rCenter && qPosRight >= qCenter )
            break;
        uint32_t sym = ezR.cigar[ i ] & 0xf, amount = ezR.cigar[ i ] >> 4;
        switch( sym )
        {
            case 0:
                if( rPosRight + amount >= rCenter && qPosRight + amount >= qCenter )
                {
                    if( rPosRight < rCenter && ( qPosRight >= qCenter || rCenter - rPosRight > qCenter - qPosRight ) )
                    {
                        notUnrolled = amount - (uint32_t)( rCenter - rPosRight );
                        amount = (uint32_t)( rCenter - rPosRight );
                    }
                    else
                    {
                        notUnrolled = amount - (uint32_t)( qCenter - qPosRight );
                        amount = (uint32_t)( qCenter - qPosRight );
                    }
                }
                qPosRight += amount;
                rPosRight += amount;
                lastType = MT_MATCH;
                break;
            case 1:
                if( qPosRight + amount > qCenter && rPosRight >= rCenter )
                {
                    notUnrolled = amount - (uint32_t)( qCenter - qPosRight );
                    amount = (uint32_t)( qCenter - qPosRight );
                }
                qPosRight += amount;
                lastType = MT_INS;
                break;
            case 2:
                if( rPosRight + amount > rCenter && qPosRight >= qCenter )
                {
                    notUnrolled = amount - (uint32_t)( rCenter - rPosRight );
                    amount = (uint32_t)( rCenter - rPosRight );
                }
                rPosRight += amount;
                lastType = MT_DEL;
                break;
        }
    }
    // gap between both extensions (needlemanWunsch.cpp:400-430); int8 q/e promoted, u64 arithmetic,
    // note the (sic) precedence q + e * qPosRight - qPos
    const u64 kq = (u64)(i64)(int8_t)P.gap, ke = (u64)(i64)(int8_t)P.extend;
    u64 mmPen = ( qPosRight - qPos ) >= ( rPosRight - rPos ) ? ( qPosRight - qPos ) - ( rPosRight - rPos )
                                                           : ( rPosRight - rPos ) - ( qPosRight - qPos );
    mmPen *= (u64)P.mismatch;
    size_t uiM = std::min( ( qPosRight - qPos ), ( rPosRight - rPos ) );
    if( uiM > 0 )
        mmPen += kq + ke * uiM;
    u64 gapPen = 0;
    if( qPosRight - qPos > 0 )
        gapPen += kq + ke * qPosRight - qPos;
    if( rPosRight - rPos > 0 )
        gapPen += kq + ke * rPosRight - rPos;
    if( mmPen < gapPen )
        while( qPos < qPosRight && rPos < rPosRight )
        {
            alnAppend( P, A, n.Q[ qPos ] == n.R[ rPos ] ? MT_MATCH : MT_MISS, 1 );
            qPos++;
            rPos++;
        }
    alnAppend( P, A, MT_INS, qPosRight - qPos );
    alnAppend( P, A, MT_DEL, rPosRight - rPos );
    if( lastType == MT_MATCH )
        appendMatchRun( n, A, qPosRight, rPosRight, notUnrolled );
    else
        alnAppend( P, A, lastType, notUnrolled );
    switch( lastType )
    {
        case MT_MATCH:
            qPosRight += notUnrolled;
            rPosRight += notUnrolled;
            break;
        case MT_INS:
            qPosRight += notUnrolled;
            break;
        case MT_DEL:
            rPosRight += notUnrolled;
            break;
        default:
            break;
    }
    for( ; i < ezR.cigar.size( ); ++i )
    {
        uint32_t sym = ezR.cigar[ i ] & 0xf, amount = ezR.cigar[ i ] >> 4;
        switch( sym )
        {
            case 0:
                appendMatchRun( n, A, qPosRight, rPosRight, amount );
                qPosRight += amount;
                rPosRight += amount;
                break;
            case 1:
                alnAppend( P, A, MT_INS, amount );
                qPosRight += amount;
                break;
            case 2:
                alnAppend( P, A, MT_DEL, amount );
                rPosRight += amount;
                break;
        }
    }
}

// NeedlemanWunsch::dynPrg (needlemanWunsch.cpp:499-622)
static void dynPrg( const NwCtx& n, u64 fromQ, u64 toQ, u64 fromR, u64 toR, Aln& A, bool bLocalBeginning,
                    bool bLocalEnd )
{
    const ma_or_params& P = n.c.P;
    if( toR <= fromR )
        if( toQ <= fromQ )
            return;
    if( toQ <= fromQ )
    {
        alnAppend( P, A, MT_DEL, toR - fromR );
        return;
    }
    if( toR <= fromR )
    {
        alnAppend( P, A, MT_INS, toQ - fromQ );
        return;
    }
    if( !bLocalBeginning && !bLocalEnd )
    {
        if( toQ - fromQ > (u64)P.max_gap_area || toR - fromR > (u64)P.max_gap_area )
            nwDualExt( n, fromQ, toQ, fromR, toR, A );
        else
            nwKsw( n, fromQ, toQ, fromR, toR, A );
        return;
    }
    const bool bReverse = bLocalBeginning;
    Ez ez;
    if( bReverse )
    {
        std::reverse( n.Q.begin( ) + fromQ, n.Q.begin( ) + toQ );
        std::reverse( n.R.begin( ) + fromR, n.R.begin( ) + toR );
    }
    kswExt( n, fromQ, toQ, fromR, toR, bReverse, ez );
    if( bReverse )
    {
        std::reverse( n.Q.begin( ) + fromQ, n.Q.begin( ) + toQ );
        std::reverse( n.R.begin( ) + fromR, n.R.begin( ) + toR );
    }
    u64 qPos = fromQ, rPos = fromR;
    if( bReverse )
    {
        rPos = toR - (u64)(i64)ez.max_t - 1;
        qPos = toQ - (u64)(i64)ez.max_q - 1;
    }
    for( uint32_t cg : ez.cigar )
    {
        uint32_t sym = cg & 0xf, amount = cg >> 4;
        switch( sym )
        {
            case 0:
                appendMatchRun( n, A, qPos, rPos, amount );
                qPos += amount;
                rPos += amount;
                break;
            case 1:
                alnAppend( P, A, MT_INS, amount );
                qPos += amount;
                break;
            case 2:
                alnAppend( P, A, MT_DEL, amount );
                rPos += amount;
                break;
        }
    }
    if( bReverse )
    {
        u64 byR = toR - (u64)(i64)ez.max_t - 1, byQ = toQ - (u64)(i64)ez.max_q - 1;
        A.bRef += byR;
        A.eRef += byR;
        A.bQ += byQ;
        A.eQ += byQ;
    }
}

// NeedlemanWunsch::execute_one (needlemanWunsch.cpp:625-877), bLocal == false
static Aln executeOne( const Ctx& c, const SeedSet& set, std::vector<uint8_t>& Q )
{
    const ma_or_index& x = c.x;
    const ma_or_params& P = c.P;
    Aln ret;
    ret.socIndex = set.socIndex;
    const std::vector<Seed>& S = set.v;
    if( S.empty( ) )
        return ret;
    const u64 qlen = Q.size( );
    u64 beginRef = S.front( ).r, endRef = S.back( ).endRef( );
    u64 endQuery = S.back( ).end( ), beginQuery = S.front( ).q;
    for( const Seed& s : S )
    {
        if( endRef < s.endRef( ) )
            endRef = s.endRef( );
        if( beginRef > s.r )
            beginRef = s.r;
        if( endQuery < s.end( ) )
            endQuery = s.end( );
        if( beginQuery > s.end( ) )
            beginQuery = s.q;
    }
    if( beginRef >= endRef || bridging( x, beginRef, endRef - beginRef + 1 ) )
        return ret;
    {
        i64 oldContig = seqIdOrRev( x, beginRef );
        beginRef -= (u64)P.padding;
        if( beginRef > endRef )
            beginRef = 0;
        endRef += (u64)P.padding;
        if( endRef >= x.n )
            endRef = x.n - 1;
        endQuery = qlen;
        beginQuery = 0;
        if( seqIdOrRev( x, beginRef ) != oldContig )
            beginRef = startOfSeqOrRev( x, oldContig );
        if( seqIdOrRev( x, endRef ) != oldContig )
            endRef = endOfSeqOrRev( x, oldContig ) - 1;
    }
    ret.bRef = ret.eRef = beginRef;
    ret.bQ = ret.eQ = beginQuery;
    std::vector<uint8_t> R( endRef - beginRef );
    for( u64 p = beginRef; p < endRef; p++ )
        R[ p - beginRef ] = x.textBase( p );
    NwCtx n{ c, Q, R };
    dynPrg( n, 0, S.front( ).q, 0, S.front( ).r - beginRef, ret, true, false );
    u64 endLastQ = S.front( ).end( );
    u64 endLastR = S.front( ).endRef( ) - beginRef;
    alnAppend( P, ret, MT_SEED, S.front( ).len );
    bool bSkip = true;
    for( const Seed& s : S )
    {
        if( bSkip )
        {
            bSkip = false;
            continue;
        }
        if( s.len == 0 )
            continue;
        u64 ovQ = endLastQ - s.q;
        if( s.q > endLastQ )
            ovQ = 0;
        u64 ovR = endLastR - ( s.r - beginRef );
        if( s.r > endLastR + beginRef )
            ovR = 0;
        u64 len = s.len;
        u64 overlap = std::max( ovQ, ovR );
        if( len > overlap )
        {
            dynPrg( n, endLastQ, s.q, endLastR, s.r - beginRef, ret, false, false );
            if( ovQ > ovR )
                alnAppend( P, ret, MT_DEL, ovQ - ovR );
            if( ovR > ovQ )
                alnAppend( P, ret, MT_INS, ovR - ovQ );
            alnAppend( P, ret, MT_SEED, len - overlap );
            if( s.end( ) > endLastQ )
                endLastQ = s.end( );
            if( s.endRef( ) > endLastR + beginRef )
                endLastR = s.endRef( ) - beginRef;
        }
    }
    dynPrg( n, endLastQ, endQuery - 1, endLastR, endRef - beginRef - 1, ret, false, true );
    alnRemoveDangling( P, ret );
    return ret;
}

// Alignment::larger (alignment.h:819-845)
inline bool alnLarger( const Aln& a, const Aln& b )
{
    size_t uiA = 0, uiB = 0;
    if( b.secondary )
        uiB = 2;
    if( b.supplementary )
        uiB = 1;
    if( a.secondary )
        uiA = 2;
    if( a.supplementary )
        uiA = 1;
    if( uiA != uiB )
        return uiA < uiB;
    if( a.score == b.score )
        return a.socIndex < b.socIndex;
    return a.score > b.score;
}

// the final sort of NeedlemanWunsch::execute (needlemanWunsch.h:131-132)
static void nwSort( std::vector<Aln>& out )
{
    // the reference sorts shared_ptrs; sorting indices reproduces the same permutation
    std::vector<size_t> idx( out.size( ) );
    for( size_t i = 0; i < idx.size( ); i++ )
        idx[ i ] = i;
    std::sort( idx.begin( ), idx.end( ), [ & ]( size_t a, size_t b ) { return alnLarger( out[ a ], out[ b ] ); } );
    std::vector<Aln> tmp;
    for( size_t i : idx )
        tmp.push_back( std::move( out[ i ] ) );
    out.swap( tmp );
}

// NeedlemanWunsch::execute (needlemanWunsch.h:111-134)
static void nwExecute( const Ctx& c, const std::vector<SeedSet>& sets, const uint8_t* q, u64 qlen, std::vector<Aln>& out )
{
    out.clear( );
    std::vector<uint8_t> Q( q, q + qlen );
    for( const SeedSet& s : sets )
        out.push_back( executeOne( c, s, Q ) );
    nwSort( out );
}

// Alignment::overlap (alignment.h:659-735)
static double alnOverlap( const Aln& a, const Aln& o )
{
    u64 uiS = std::max( a.bQ, o.bQ ), uiE = std::min( a.eQ, o.eQ );
    if( uiS >= uiE )
        return 0;
    u64 ov = 0;
    size_t i = 0, j = 0;
    u64 qp = a.bQ, qo = o.bQ;
    while( qp + a.data[ i ].second < uiS )
    {
        if( a.data[ i ].first != MT_DEL )
            qp += a.data[ i ].second;
        i++;
    }
    while( qo + o.data[ j ].second < uiS )
    {
        if( o.data[ j ].first != MT_DEL )
            qo += o.data[ j ].second;
        j++;
    }
    while( qp < uiE && qo < uiE && i < a.data.size( ) && j < o.data.size( ) )
    {
        u64 ql = 0, qlo = 0;
        if( a.data[ i ].first != MT_DEL )
            ql = a.data[ i ].second;
        if( o.data[ j ].first != MT_DEL )
            qlo = o.data[ j ].second;
        u64 s_in = std::max( std::max( qp, qo ), uiS );
        u64 e_in = std::min( std::min( qp + ql, qo + qlo ), uiE );
        u64 cur = 0;
        if( s_in < e_in )
            cur = e_in - s_in;
        if( a.data[ i ].first != MT_INS && o.data[ j ].first != MT_INS )
            ov += cur;
        if( qp + ql < qo + qlo )
        {
            qp += ql;
            i++;
        }
        else
        {
            qo += qlo;
            j++;
        }
    }
    u64 sz = std::min( a.eQ - a.bQ, o.eQ - o.bQ );
    return ov / static_cast<double>( sz );
}

// MappingQuality::execute (mappingQuality.cpp:11-131)
static void mappingQuality( const Ctx& c, u64 qlen, std::vector<Aln>& alns, std::vector<Aln>& out )
{
    const ma_or_params& P = c.P;
    out.clear( );
    auto sortIdx = [ & ]( auto cmp ) {
        std::vector<size_t> idx( alns.size( ) );
        for( size_t i = 0; i < idx.size( ); i++ )
            idx[ i ] = i;
        std::sort( idx.begin( ), idx.end( ), [ & ]( size_t a, size_t b ) { return cmp( alns[ a ], alns[ b ] ); } );
        std::vector<Aln> tmp;
        for( size_t i : idx )
            tmp.push_back( std::move( alns[ i ] ) );
        alns.swap( tmp );
    };
    sortIdx( []( const Aln& a, const Aln& b ) { return a.score > b.score; } );
    if( alns.size( ) == 0 )
        return;
    Aln& first = alns[ 0 ];
    first.secondary = false;
    size_t nSupp = 0;
    for( size_t i = 1; i < alns.size( ); i++ )
    {
        alns[ i ].mapq = 0.0;
        if( nSupp < (size_t)P.max_supplementary && alnOverlap( alns[ i ], first ) < P.max_overlap_supplementary )
        {
            alns[ i ].supplementary = true;
            alns[ i ].secondary = false;
            nSupp++;
        }
        else
        {
            alns[ i ].supplementary = false;
            alns[ i ].secondary = true;
        }
    }
    if( alns.size( ) - nSupp >= 2 )
    {
        size_t i = 1;
        const Aln* second = nullptr;
        while( second == nullptr || second->supplementary )
        {
            second = &alns[ i ];
            i++;
        }
        if( first.score == 0 )
            first.mapq = 0;
        else
            first.mapq = static_cast<double>( first.score - second->score ) / static_cast<double>( first.score );
    }
    else
        first.mapq = first.score / (double)( (u64)P.match * qlen );
    size_t nSeeds = 0;
    for( auto& d : first.data )
        if( d.first == MT_SEED )
            nSeeds++;
    if( nSeeds <= 1 )
        first.mapq /= 2;
    if( first.score >= (u64)P.match * qlen * 0.8 && alns.size( ) >= 3 )
        first.mapq *= 2;
    if( first.mapq > 1 )
        first.mapq = 1;
    if( nSupp > 0 )
    {
        for( size_t i = 1; i < alns.size( ); i++ )
            if( alns[ i ].supplementary )
                alns[ i ].mapq = alns[ 0 ].mapq;
        sortIdx( []( const Aln& a, const Aln& b ) { return alnLarger( a, b ); } );
    }
    out = alns;
    if( P.report_n_best != 0 && out.size( ) > (size_t)P.report_n_best + nSupp )
        out.erase( out.begin( ) + P.report_n_best + nSupp, out.end( ) );
    out.erase( std::remove_if( out.begin( ), out.end( ),
                               [ & ]( const Aln& a ) { return a.score < (long)(size_t)P.min_alignment_score; } ),
               out.end( ) );
}
} // namespace
