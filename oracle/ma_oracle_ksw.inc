// TEST INFRASTRUCTURE ONLY (part of ma_oracle.cpp).
// kswcpp banded two-piece affine DP, int8 difference recurrences on 16-lane blocks
// (libs/kswcpp/inc/kswcpp_core.h:14-841, kswcpp.h:21-129, sse_xx.h, kswcpp_sse_xx.cpp:23-66).
// Scalar restatement of the SSE4.1 path: every 16-lane block [st,en] the reference touches is
// computed lane by lane with wrapping int8 arithmetic, so out-of-band lanes carry the same stale
// state.  Bytes the reference reads beyond its zero-filled scratch (up to 15 B past qr's padded
// end) are modelled as zero (kswcpp_mem.h:146-161: only the requested size is cleared).
namespace
{
#define KSW_EZ_RIGHT 0x02
#define KSW_EZ_EXTZ_ONLY 0x40
#define KSW_EZ_REV_CIGAR 0x80

struct Ez // kswcpp_extz_t (kswcpp.h:31-41)
{
    uint32_t max = 0;
    int zdropped = 0;
    int max_q = -1, max_t = -1, mqe = INT32_MIN, mqe_t = -1, mte = INT32_MIN, mte_q = -1, score = INT32_MIN;
    int reach_end = 0;
    std::vector<uint32_t> cigar;
};

inline void ezReset( Ez& ez ) // ksw_reset_extz (kswcpp_core.h:14-20)
{
    ez.max_q = ez.max_t = ez.mqe_t = ez.mte_q = -1;
    ez.max = 0;
    ez.score = ez.mqe = ez.mte = INT32_MIN;
    ez.cigar.clear( );
    ez.zdropped = 0;
    ez.reach_end = 0;
}

// ksw_apply_zdrop (kswcpp_core.h:22-44), is_rot == 1; ez->max is a 31-bit unsigned bit-field
inline int applyZdrop( Ez& ez, int32_t H, int a, int b, int zdrop, int8_t e )
{
    int r = a, t = b;
    if( H > (int32_t)ez.max )
    {
        ez.max = (uint32_t)H & 0x7fffffffu;
        ez.max_t = t;
        ez.max_q = r - t;
    }
    else if( t >= ez.max_t && r - t >= ez.max_q )
    {
        int tl = t - ez.max_t, ql = ( r - t ) - ez.max_q, l;
        l = tl > ql ? tl - ql : ql - tl;
        if( zdrop >= 0 && (int32_t)( ez.max - H ) > zdrop + l * e )
        {
            ez.zdropped = 1;
            return 1;
        }
    }
    return 0;
}

inline void pushCigar( std::vector<uint32_t>& c, uint32_t op, int len ) // ksw_push_cigar (46-65)
{
    if( c.empty( ) || op != ( c.back( ) & 0xf ) )
        c.push_back( (uint32_t)len << 4 | op );
    else
        c.back( ) += (uint32_t)len << 4;
}

// ksw_backtrack__ (kswcpp_core.h:76-150) with is_rot = 1, min_intron_len = 0
static void backtrack( int is_rev, const std::vector<uint8_t>& p, const std::vector<int>& off,
                       const std::vector<int>& off_end, i64 n_col, int i0, int j0, std::vector<uint32_t>& cigar )
{
    cigar.clear( );
    i64 i = i0, j = j0, r, state = 0;
    uint32_t tmp;
    while( i >= 0 && j >= 0 )
    {
        int force_state = -1;
        r = i + j;
        if( i < off[ r ] )
            force_state = 2;
        if( i > off_end[ r ] )
            force_state = 1;
        tmp = force_state < 0 ? p[ r * n_col + i - off[ r ] ] : 0;
        if( state == 0 )
            state = tmp & 7;
        else if( !( tmp >> ( state + 2 ) & 1 ) )
            state = 0;
        if( state == 0 )
            state = tmp & 7;
        if( force_state >= 0 )
            state = force_state;
        if( state == 0 )
            pushCigar( cigar, 0, 1 ), --i, --j;
        else if( state == 1 || state == 3 )
            pushCigar( cigar, 2, 1 ), --i;
        else
            pushCigar( cigar, 1, 1 ), --j;
    }
    if( i >= 0 )
        pushCigar( cigar, 2, (int)( i + 1 ) );
    if( j >= 0 )
        pushCigar( cigar, 1, (int)( j + 1 ) );
    if( !is_rev )
        std::reverse( cigar.begin( ), cigar.end( ) );
}

// DP cell update of one diagonal over the aligned lanes (kswcpp_core.h:653-766); branch-free per lane so
// that the compiler can vectorise it with the same 16 x int8 SSE lanes the reference uses
template <bool LEFT>
static inline void kswLanes( const int nl, const int8_t* __restrict s, const int8_t* __restrict oxx,
                             const int8_t* __restrict ovv, const int8_t* __restrict ox22, int8_t* __restrict u,
                             int8_t* __restrict v, int8_t* __restrict x, int8_t* __restrict y, int8_t* __restrict x2,
                             int8_t* __restrict y2, uint8_t* __restrict pr, const int8_t sc_mch, const int8_t q,
                             const int8_t e, const int8_t q2, const int8_t e2 )
{
    const int8_t qe = (int8_t)( q + e ), qe2 = (int8_t)( q2 + e2 );
#pragma GCC ivdep
    for( int j = 0; j < nl; j++ )
    {
        int8_t z = s[ j ];
        const int8_t xt1 = oxx[ j ], vt1 = ovv[ j ], x2t1 = ox22[ j ];
        const int8_t ut = u[ j ];
        int8_t a = (int8_t)( xt1 + vt1 );
        int8_t b = (int8_t)( y[ j ] + ut );
        int8_t a2 = (int8_t)( x2t1 + vt1 );
        int8_t b2 = (int8_t)( y2[ j ] + ut );
        uint8_t d;
        if( LEFT )
        {
            d = a > z ? 1 : 0;
            z = z > a ? z : a;
            d = b > z ? 2 : d;
            z = z > b ? z : b;
            d = a2 > z ? 3 : d;
            z = z > a2 ? z : a2;
            d = b2 > z ? 4 : d;
            z = z > b2 ? z : b2;
        }
        else
        {
            d = z > a ? 0 : 1; // (z > a).andnot(1)
            z = z > a ? z : a;
            d = z > b ? d : 2; // 2.blendv(d, z > b)
            z = z > b ? z : b;
            d = z > a2 ? d : 3;
            z = z > a2 ? z : a2;
            // dangling else at kswcpp_core.h:693-699: state 4 is never recorded with CIGAR + right-align
            z = z > b2 ? z : b2;
        }
        z = z < sc_mch ? z : sc_mch;
        u[ j ] = (int8_t)( z - vt1 );
        v[ j ] = (int8_t)( z - ut );
        int8_t tmp = (int8_t)( z - q );
        a = (int8_t)( a - tmp );
        b = (int8_t)( b - tmp );
        tmp = (int8_t)( z - q2 );
        a2 = (int8_t)( a2 - tmp );
        b2 = (int8_t)( b2 - tmp );
        if( LEFT )
        {
            x[ j ] = (int8_t)( ( a > 0 ? a : 0 ) - qe );
            d |= a > 0 ? 0x08 : 0;
            y[ j ] = (int8_t)( ( b > 0 ? b : 0 ) - qe );
            d |= b > 0 ? 0x10 : 0;
            x2[ j ] = (int8_t)( ( a2 > 0 ? a2 : 0 ) - qe2 );
            d |= a2 > 0 ? 0x20 : 0;
            y2[ j ] = (int8_t)( ( b2 > 0 ? b2 : 0 ) - qe2 );
            d |= b2 > 0 ? 0x40 : 0;
        }
        else
        {
            x[ j ] = (int8_t)( ( 0 > a ? 0 : a ) - qe );
            d |= 0 > a ? 0 : 0x08;
            y[ j ] = (int8_t)( ( 0 > b ? 0 : b ) - qe );
            d |= 0 > b ? 0 : 0x10;
            x2[ j ] = (int8_t)( ( 0 > a2 ? 0 : a2 ) - qe2 );
            d |= 0 > a2 ? 0 : 0x20;
            y2[ j ] = (int8_t)( ( 0 > b2 ? 0 : b2 ) - qe2 );
            d |= 0 > b2 ? 0 : 0x40;
        }
        pr[ j ] = d;
    }
}

// kswcpp_inner_core (kswcpp_core.h:308-841) for one H-score width; HBITS = 16 or 32 selects the
// int16/int32 H array and the 8-/4-lane calcMaxScore (kswcpp_core.h:156-299)
template <typename TH, int HL> static void kswCore( int qlen, const uint8_t* query, int tlen, const uint8_t* target,
                                                   const ma_or_params& P, int w, int zdrop, int flag, Ez& ez )
{
    ezReset( ez );
    if( qlen <= 0 || tlen <= 0 )
        return;
    int8_t q = (int8_t)P.gap, e = (int8_t)P.extend, q2 = (int8_t)P.gap2, e2 = (int8_t)P.extend2;
    const int8_t sc_mch = (int8_t)( P.match < 0 ? -P.match : P.match ); // KswCppParam ctor (kswcpp.h:66-80)
    const int8_t sc_mis = (int8_t)( P.mismatch > 0 ? -P.mismatch : P.mismatch );
    i64 t;
    const i64 qe = q + e;
    if( q2 + e2 < q + e )
    {
        std::swap( q, q2 );
        std::swap( e, e2 );
    }
    if( w < 0 )
        w = tlen > qlen ? tlen : qlen;
    const i64 wl = w, wr = w;
    const int tlen_ = ( tlen + 15 ) / 16;
    i64 n_col_ = qlen < tlen ? qlen : tlen;
    n_col_ = ( ( n_col_ < w + 1 ? n_col_ : w + 1 ) + 15 ) / 16 + 1;
    const int qlen_ = ( qlen + 15 ) / 16;
    {
        // mat: match, mismatch, and 0 for the wildcard row/column (kswcpp.h:83-93)
        i64 max_sc = sc_mch, min_sc = sc_mis;
        max_sc = max_sc > 0 ? max_sc : 0;
        min_sc = min_sc < 0 ? min_sc : 0;
        if( -min_sc > 2 * ( q + e ) )
            return;
    }
    i64 long_thres = e != e2 ? ( q2 - q ) / ( e - e2 ) - 1 : 0;
    if( q2 + e2 + long_thres * e2 > q + e + long_thres * e )
        ++long_thres;
    const i64 long_diff = long_thres * ( e - e2 ) - ( q2 - q ) - e2;

    // one scratch buffer u|v|x|y|x2|y2|s|sf|qr (kswcpp_core.h:434-444), zero filled, + 16 zero bytes slack
    const size_t L = (size_t)tlen_ * 16;
    // per-thread scratch reused across calls like the reference's AlignedMemoryManager (kswcpp_mem.h:111-211)
    static thread_local std::vector<uint8_t> mem;
    mem.assign( L * 8 + (size_t)qlen_ * 16 + 32, 0 );
    int8_t* u8 = (int8_t*)&mem[ 0 ];
    int8_t* v8 = u8 + L;
    int8_t* x8 = v8 + L;
    int8_t* y8 = x8 + L;
    int8_t* x28 = y8 + L;
    int8_t* y28 = x28 + L;
    int8_t* s8 = y28 + L;
    uint8_t* sf = (uint8_t*)( s8 + L );
    uint8_t* qr = sf + L;
    memset( u8, (uint8_t)( -q - e ), L );
    memset( v8, (uint8_t)( -q - e ), L );
    memset( x8, (uint8_t)( -q - e ), L );
    memset( y8, (uint8_t)( -q - e ), L );
    memset( x28, (uint8_t)( -q2 - e2 ), L );
    memset( y28, (uint8_t)( -q2 - e2 ), L );
    static thread_local std::vector<TH> H;
    H.assign( L, std::numeric_limits<TH>::min( ) );
    // direction matrix: malloc'ed, not cleared, by the reference (kswcpp_mem.h:319-333)
    static thread_local std::vector<uint8_t> p;
    {
        const size_t need = (size_t)( ( (i64)qlen + tlen - 1 ) * n_col_ + 1 ) * 16;
        if( p.size( ) < need )
            p.resize( need );
    }
    static thread_local std::vector<int> off, off_end;
    if( off.size( ) < (size_t)( qlen + tlen - 1 ) )
    {
        off.resize( qlen + tlen - 1 );
        off_end.resize( qlen + tlen - 1 );
    }
    for( t = 0; t < qlen; ++t )
        qr[ t ] = query[ qlen - 1 - t ];
    memcpy( sf, target, tlen );
    const bool left = !( flag & KSW_EZ_RIGHT );

    static thread_local std::vector<int8_t> oxx, ovv, ox22; // old x / v / x2 of the active window (+1 carry-in)
    i64 last_st = -1, last_en = -1;
    for( i64 r = 0; r < (i64)qlen + tlen - 1; ++r )
    {
        int st = 0, en = tlen - 1, st0, en0;
        int8_t x1, x21, v1;
        if( st < r - qlen + 1 )
            st = (int)( r - qlen + 1 );
        if( en > r )
            en = (int)r;
        if( st < ( ( r - wr + 1 ) >> 1 ) )
            st = (int)( ( r - wr + 1 ) >> 1 );
        if( en > ( ( r + wl ) >> 1 ) )
            en = (int)( ( r + wl ) >> 1 );
        if( st > en )
        {
            ez.zdropped = 1;
            break;
        }
        st0 = st;
        en0 = en;
        st = ( st / 16 ) * 16;
        en = ( en + 16 ) / 16 * 16 - 1;
        if( st > 0 )
        {
            if( st - 1 >= last_st && st - 1 <= last_en )
                x1 = x8[ st - 1 ], x21 = x28[ st - 1 ], v1 = v8[ st - 1 ];
            else
                x1 = (int8_t)( -q - e ), x21 = (int8_t)( -q2 - e2 ), v1 = (int8_t)( -q - e );
        }
        else
        {
            x1 = (int8_t)( -q - e );
            x21 = (int8_t)( -q2 - e2 );
            v1 = (int8_t)( r == 0 ? -q - e : r < long_thres ? -e : r == long_thres ? long_diff : -e2 );
        }
        if( en >= r )
        {
            y8[ r ] = (int8_t)( -q - e );
            y28[ r ] = (int8_t)( -q2 - e2 );
            u8[ r ] = (int8_t)( r == 0 ? -q - e : r < long_thres ? -e : r == long_thres ? long_diff : -e2 );
        }
        // score profile from the UNALIGNED st0 in steps of 16 (kswcpp_core.h:598-615); may run past
        // s into sf and read past sf into qr exactly like the unaligned SSE loads/stores do
        {
            const uint8_t* qrr = qr + ( qlen - 1 - r );
            for( t = st0; t <= en0; t += 16 )
            {
                int8_t tmp[ 16 ];
                for( int j = 0; j < 16; j++ )
                {
                    uint8_t sq = sf[ t + j ], sq2 = qrr[ t + j ];
                    int8_t val = sq == sq2 ? sc_mch : sc_mis;
                    if( sq == 4 || sq2 == 4 )
                        val = (int8_t)( -e2 );
                    tmp[ j ] = val;
                }
                memcpy( s8 + t, tmp, 16 ); // store after all 16 loads (a store may alias sf[0..14])
            }
        }
        off[ r ] = st;
        off_end[ r ] = en;
        uint8_t* pr = &p[ (size_t)( ( r * n_col_ ) - st / 16 ) * 16 ];
        // lanes [st,en]: lane t reads OLD x[t-1], v[t-1] (shiftl<1>|carry) (kswcpp_core.h:653-766)
        {
            const int nl = en - st + 1;
            cnt( 4, (u64)nl );
            oxx.resize( nl + 1 );
            ovv.resize( nl + 1 );
            ox22.resize( nl + 1 );
            oxx[ 0 ] = x1;
            ovv[ 0 ] = v1;
            ox22[ 0 ] = x21;
            for( int j = 0; j < nl; j++ )
            {
                oxx[ j + 1 ] = x8[ st + j ];
                ovv[ j + 1 ] = v8[ st + j ];
                ox22[ j + 1 ] = x28[ st + j ];
            }
            if( left )
                kswLanes<true>( nl, s8 + st, oxx.data( ), ovv.data( ), ox22.data( ), u8 + st, v8 + st, x8 + st, y8 + st,
                                x28 + st, y28 + st, pr + st, sc_mch, q, e, q2, e2 );
            else
                kswLanes<false>( nl, s8 + st, oxx.data( ), ovv.data( ), ox22.data( ), u8 + st, v8 + st, x8 + st, y8 + st,
                                 x28 + st, y28 + st, pr + st, sc_mch, q, e, q2, e2 );
        }
        // calcMaxScore (kswcpp_core.h:156-299), exact-max branch
        {
            TH max_H, max_t;
            if( r > 0 )
            {
                const i64 en1 = st0 + ( ( en0 - st0 ) / HL ) * HL;
                max_H = H[ en0 ] = (TH)( en0 > 0 ? H[ en0 - 1 ] + u8[ en0 ] : H[ en0 ] + v8[ en0 ] );
                max_t = (TH)en0;
                TH vH[ HL ], vT[ HL ];
                for( int j = 0; j < HL; j++ )
                    vH[ j ] = max_H, vT[ j ] = max_t;
                TH tt;
                for( tt = (TH)st0; tt < (TH)en1; tt = (TH)( tt + HL ) )
                    for( int j = 0; j < HL; j++ )
                    {
                        TH h = (TH)( H[ tt + j ] + (TH)v8[ tt + j ] );
                        H[ tt + j ] = h;
                        if( h > vH[ j ] )
                            vH[ j ] = h, vT[ j ] = tt;
                    }
                max_H = vH[ 0 ];
                max_t = vT[ 0 ];
                for( int j = 1; j < HL; j++ )
                {
                    max_H = vH[ j ] > max_H ? vH[ j ] : max_H; // independent horizontal maxima
                    max_t = vT[ j ] > max_t ? vT[ j ] : max_t;
                }
                for( ; tt < (TH)en0; ++tt )
                {
                    H[ tt ] = (TH)( H[ tt ] + (TH)v8[ tt ] );
                    if( H[ tt ] > max_H )
                        max_H = H[ tt ], max_t = tt;
                }
            }
            else
            {
                H[ 0 ] = (TH)( v8[ 0 ] - qe );
                max_H = H[ 0 ];
                max_t = 0;
            }
            if( en0 == tlen - 1 && H[ en0 ] > ez.mte )
                ez.mte = H[ en0 ], ez.mte_q = (int)( r - en ); // aligned en (kswcpp_core.h:774)
            if( r - st0 == qlen - 1 && H[ st0 ] > ez.mqe )
                ez.mqe = H[ st0 ], ez.mqe_t = st0;
            if( applyZdrop( ez, max_H, (int)r, max_t, zdrop, e2 ) )
                break;
            if( r == qlen + tlen - 2 && en0 == tlen - 1 )
                ez.score = H[ tlen - 1 ];
        }
        last_st = st;
        last_en = en;
    }
    // backtrack target selection (kswcpp_core.h:796-835)
    const int rev_cigar = !!( flag & KSW_EZ_REV_CIGAR );
    const i64 ncol = n_col_ * 16;
    if( !ez.zdropped && !( flag & KSW_EZ_EXTZ_ONLY ) )
        backtrack( rev_cigar, p, off, off_end, ncol, tlen - 1, qlen - 1, ez.cigar );
    else if( !ez.zdropped && ( flag & KSW_EZ_EXTZ_ONLY ) && ez.mqe > (int)ez.max )
    {
        ez.reach_end = 1;
        backtrack( rev_cigar, p, off, off_end, ncol, ez.mqe_t, qlen - 1, ez.cigar );
    }
    else if( ez.max_t >= 0 && ez.max_q >= 0 )
        backtrack( rev_cigar, p, off, off_end, ncol, ez.max_t, ez.max_q, ez.cigar );
}

// kswcpp_sse_xx_instr_set (kswcpp_sse_xx.cpp:23-66): int16 H unless max(qlen,tlen)*24 overflows int16
static void kswDispatch( int qlen, const uint8_t* q, int tlen, const uint8_t* t, const ma_or_params& P, int w,
                         int zdrop, int flag, Ez& ez )
{
    cnt( 5 );
    if( tlsCalls )
        tlsCalls->push_back( KswCall{ qlen, tlen, w, zdrop, flag } );
    int minScr = std::min( { P.mismatch > 0 ? -P.mismatch : P.mismatch, -P.gap, -P.extend, -P.gap2, -P.extend2 } );
    int maxSc = P.match < 0 ? -P.match : P.match;
    i64 sz = std::max( qlen, tlen );
    auto risk = [ & ]( i64 lo, i64 hi ) { return sz * (int8_t)minScr < lo || sz * (int8_t)maxSc > hi; };
    if( !risk( INT16_MIN, INT16_MAX ) )
        kswCore<int16_t, 8>( qlen, q, tlen, t, P, w, zdrop, flag, ez );
    else if( !risk( INT32_MIN, INT32_MAX ) )
        kswCore<int32_t, 4>( qlen, q, tlen, t, P, w, zdrop, flag, ez );
    else
        ezReset( ez );
}
} // namespace
