// TEST INFRASTRUCTURE ONLY (part of ma_oracle.cpp): C API, batch driver, text dump.
namespace
{
struct ReadResult
{
    std::vector<Seg> segs;
    std::vector<Seed> seeds; // after ExtractSeeds (before the SoC sort)
    std::vector<SeedSet> harm;
    std::vector<Aln> alns; // NeedlemanWunsch::execute order
    std::vector<Aln> mq; // after MappingQuality
};

static void alignRead( const Ctx& c, const uint8_t* q, u64 qlen, ReadResult& R, std::vector<SeedSet>* socDump )
{
    seedRead( c, q, qlen, R.segs );
    extractSeeds( c, R.segs, qlen, R.seeds );
    std::vector<Seed> work = R.seeds;
    SoCQueue Q;
    if( socDump )
    {
        std::vector<Seed> w2 = R.seeds;
        SoCQueue Q2;
        socSweep( c, w2, qlen, Q2 );
        while( !Q2.empty( ) )
        {
            SoCOrder sc = Q2.vMaxima.front( ).sc;
            SeedSet s = Q2.pop( );
            Seed tag; // smuggle the score / ambiguity of the SoC in a pseudo seed at the back
            tag.q = sc.accLen;
            tag.amb = sc.amb;
            s.v.push_back( tag );
            socDump->push_back( s );
        }
    }
    socSweep( c, work, qlen, Q );
    harmonize( c, Q, qlen, R.harm );
    nwExecute( c, R.harm, q, qlen, R.alns );
    std::vector<Aln> tmp = R.alns;
    mappingQuality( c, qlen, tmp, R.mq );
}

inline void dumpSeedLine( FILE* f, const char* tag, const Seed& s )
{
    fprintf( f, "%s %llu %llu %llu %u %d %llu\n", tag, (unsigned long long)s.q, (unsigned long long)s.len,
             (unsigned long long)s.r, s.amb, (int)s.fwd, (unsigned long long)s.delta );
}
} // namespace

struct ma_or_result
{
    std::vector<u64> segOff, seedOff, hsetOff, hseedOff, alnOff, mqOff;
    std::vector<ma_or_alignment> mq; // MappingQuality::execute output per read (no ops)
    std::vector<ma_or_segment> segs;
    std::vector<ma_or_seed> seeds, hseeds;
    std::vector<uint32_t> hsetSoc;
    std::vector<ma_or_alignment> alns;
    std::vector<u64> ops;
    u64 counters[ 8 ] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    u64 nAligned = 0;
};

extern "C" {

ma_or_index* ma_or_index_build( int32_t n_contigs, const uint64_t* contig_lens, const uint8_t* codes )
{
    ma_or_index* x = new ma_or_index( );
    u64 F = 0;
    for( int i = 0; i < n_contigs; i++ )
    {
        x->cstart.push_back( F );
        x->clen.push_back( contig_lens[ i ] );
        F += contig_lens[ i ];
    }
    x->F = F;
    x->pac.assign( ( F + 3 ) / 4, 0 );
    for( u64 p = 0; p < F; p++ )
        x->pac[ p >> 2 ] |= (uint8_t)( ( codes[ p ] & 3 ) << ( ( ~p & 3 ) << 1 ) );
    std::vector<uint8_t> t( 2 * F );
    for( u64 p = 0; p < F; p++ )
    {
        t[ p ] = codes[ p ] & 3;
        t[ 2 * F - 1 - p ] = 3 - ( codes[ p ] & 3 );
    }
    buildFromText( *x, t );
    return x;
}

ma_or_index* ma_or_index_from_parts( const uint32_t* bwt_words, uint64_t n_words, const int64_t* sa, uint64_t n_sa,
                                     const uint64_t L2[ 5 ], int64_t primary, uint64_t ref_len, const uint8_t* pac,
                                     int32_t n_contigs, const uint64_t* contig_starts, const uint64_t* contig_lens )
{
    ma_or_index* x = new ma_or_index( );
    x->n = ref_len;
    x->F = ref_len / 2;
    x->primary = primary;
    for( int i = 0; i < 5; i++ )
        x->L2[ i ] = L2[ i ];
    x->bwt.assign( bwt_words, bwt_words + n_words );
    x->sa.assign( sa, sa + n_sa );
    x->pac.assign( pac, pac + ( x->F + 3 ) / 4 );
    x->cstart.assign( contig_starts, contig_starts + n_contigs );
    x->clen.assign( contig_lens, contig_lens + n_contigs );
    return x;
}

void ma_or_index_free( ma_or_index* x )
{
    delete x;
}

int ma_or_index_store( const ma_or_index* x, const char* prefix )
{
    std::string p( prefix );
    FILE* f = fopen( ( p + ".bwt" ).c_str( ), "wb" );
    if( !f )
        return -1;
    fwrite( &x->primary, 8, 1, f ); // vSaveBWT (fMIndex.h:515-526)
    fwrite( &x->L2[ 1 ], 8, 4, f );
    fwrite( x->bwt.data( ), 4, x->bwt.size( ), f );
    fclose( f );
    f = fopen( ( p + ".sa" ).c_str( ), "wb" );
    if( !f )
        return -1;
    int32_t intv = 32;
    fwrite( &x->primary, 8, 1, f ); // vSaveSuffixArray (fMIndex.h:530-549)
    fwrite( &x->L2[ 1 ], 8, 4, f );
    fwrite( &intv, 4, 1, f );
    fwrite( &x->n, 8, 1, f );
    fwrite( x->sa.data( ) + 1, 8, x->sa.size( ) - 1, f );
    fclose( f );
    f = fopen( ( p + ".pac" ).c_str( ), "wb" );
    if( !f )
        return -1;
    // vStorePack (pack.h:181-228): packed bytes, then (if F%4==0 an extra 0 byte) and a count byte F%4
    fwrite( x->pac.data( ), 1, x->pac.size( ), f );
    if( x->F % 4 == 0 )
    {
        uint8_t z = 0;
        fwrite( &z, 1, 1, f );
    }
    uint8_t c = (uint8_t)( x->F % 4 );
    fwrite( &c, 1, 1, f );
    fclose( f );
    return 0;
}

uint64_t ma_or_index_n_words( const ma_or_index* x )
{
    return x->bwt.size( );
}
uint64_t ma_or_index_n_sa( const ma_or_index* x )
{
    return x->sa.size( );
}
const uint32_t* ma_or_index_bwt( const ma_or_index* x )
{
    return x->bwt.data( );
}
const int64_t* ma_or_index_sa( const ma_or_index* x )
{
    return x->sa.data( );
}
const uint8_t* ma_or_index_pac( const ma_or_index* x )
{
    return x->pac.data( );
}
void ma_or_index_meta( const ma_or_index* x, uint64_t L2_out[ 5 ], int64_t* primary, uint64_t* ref_len )
{
    for( int i = 0; i < 5; i++ )
        L2_out[ i ] = x->L2[ i ];
    *primary = x->primary;
    *ref_len = x->n;
}

void ma_or_extend_backward( const ma_or_index* x, const int64_t ik[ 3 ], uint8_t c, int64_t ok[ 3 ] )
{
    extendBackward( *x, ik, c, ok );
}
int64_t ma_or_bwt_sa( const ma_or_index* x, int64_t row )
{
    return bwtSa( *x, row );
}

int ma_or_ksw( int32_t qlen, const uint8_t* q, int32_t tlen, const uint8_t* t, int32_t w, int32_t zdrop, int32_t flag,
               const ma_or_params* p, ma_or_ez* out, uint32_t* cigar, int32_t cigar_cap )
{
    Ez ez;
    kswDispatch( qlen, q, tlen, t, *p, w, zdrop, flag, ez );
    out->max = (int32_t)ez.max;
    out->zdropped = ez.zdropped;
    out->max_q = ez.max_q;
    out->max_t = ez.max_t;
    out->mqe = ez.mqe;
    out->mqe_t = ez.mqe_t;
    out->mte = ez.mte;
    out->mte_q = ez.mte_q;
    out->score = ez.score;
    out->reach_end = ez.reach_end;
    out->n_cigar = (int32_t)ez.cigar.size( );
    if( (int32_t)ez.cigar.size( ) > cigar_cap )
        return -1;
    for( size_t i = 0; i < ez.cigar.size( ); i++ )
        cigar[ i ] = ez.cigar[ i ];
    return (int)ez.cigar.size( );
}

static ma_or_seed toSeedRec( const Seed& s )
{
    ma_or_seed r;
    r.q_start = (i64)s.q;
    r.len = (i64)s.len;
    r.r_start = (i64)s.r;
    r.delta = (i64)s.delta;
    r.ambiguity = s.amb;
    r.on_forward = s.fwd ? 1 : 0;
    return r;
}

ma_or_result* ma_or_align_batch( const ma_or_index* x, const ma_or_params* P, const uint8_t* reads,
                                 const uint64_t* off, uint64_t n, int32_t n_threads )
{
    if( n_threads < 1 )
        n_threads = 1;
    std::vector<ReadResult> RR( n );
    std::vector<Counters> C( n_threads );
    std::atomic<u64> next( 0 );
    auto worker = [ & ]( int tid ) {
        tlsCnt = &C[ tid ];
        Ctx c{ *x, *P };
        while( true )
        {
            u64 i0 = next.fetch_add( 64 );
            if( i0 >= n )
                break;
            for( u64 i = i0; i < std::min( n, i0 + 64 ); i++ )
                alignRead( c, reads + off[ i ], off[ i + 1 ] - off[ i ], RR[ i ], nullptr );
        }
        tlsCnt = nullptr;
    };
    if( n_threads == 1 )
        worker( 0 );
    else
    {
        std::vector<std::thread> th;
        for( int t = 0; t < n_threads; t++ )
            th.emplace_back( worker, t );
        for( auto& t : th )
            t.join( );
    }
    ma_or_result* res = new ma_or_result( );
    for( auto& c : C )
        for( int i = 0; i < 8; i++ )
            res->counters[ i ] += c.v[ i ];
    res->segOff.push_back( 0 );
    res->seedOff.push_back( 0 );
    res->hsetOff.push_back( 0 );
    res->hseedOff.push_back( 0 );
    res->alnOff.push_back( 0 );
    res->mqOff.push_back( 0 );
    for( u64 i = 0; i < n; i++ )
    {
        ReadResult& R = RR[ i ];
        for( const Seg& s : R.segs )
            res->segs.push_back( ma_or_segment{ (i64)s.start, (i64)s.size, s.sa[ 0 ], s.sa[ 1 ], s.sa[ 2 ] } );
        res->segOff.push_back( res->segs.size( ) );
        for( const Seed& s : R.seeds )
            res->seeds.push_back( toSeedRec( s ) );
        res->seedOff.push_back( res->seeds.size( ) );
        for( const SeedSet& h : R.harm )
        {
            for( const Seed& s : h.v )
                res->hseeds.push_back( toSeedRec( s ) );
            res->hseedOff.push_back( res->hseeds.size( ) );
            res->hsetSoc.push_back( h.socIndex );
        }
        res->hsetOff.push_back( res->hsetSoc.size( ) );
        for( const Aln& a : R.alns )
        {
            ma_or_alignment r;
            r.begin_ref = (i64)a.bRef;
            r.end_ref = (i64)a.eRef;
            r.begin_q = (i64)a.bQ;
            r.end_q = (i64)a.eQ;
            r.score = a.score;
            r.soc_index = a.socIndex;
            r.n_ops = (uint32_t)a.data.size( );
            r.ops_off = res->ops.size( ) / 2;
            r.secondary = r.supplementary = 0;
            r.mapq = 0;
            for( auto& d : a.data )
            {
                res->ops.push_back( (u64)d.first );
                res->ops.push_back( d.second );
            }
            res->alns.push_back( r );
        }
        res->alnOff.push_back( res->alns.size( ) );
        for( const Aln& a : R.mq )
        {
            ma_or_alignment r;
            r.begin_ref = (i64)a.bRef;
            r.end_ref = (i64)a.eRef;
            r.begin_q = (i64)a.bQ;
            r.end_q = (i64)a.eQ;
            r.score = a.score;
            r.soc_index = a.socIndex;
            r.n_ops = (uint32_t)a.data.size( );
            r.ops_off = 0;
            r.secondary = a.secondary ? 1 : 0;
            r.supplementary = a.supplementary ? 1 : 0;
            r.mapq = a.mapq;
            res->mq.push_back( r );
        }
        res->mqOff.push_back( res->mq.size( ) );
        if( !R.mq.empty( ) )
            res->nAligned++;
    }
    return res;
}

void ma_or_result_free( ma_or_result* r )
{
    delete r;
}
const uint64_t* ma_or_res_seg_off( const ma_or_result* r )
{
    return r->segOff.data( );
}
const ma_or_segment* ma_or_res_segs( const ma_or_result* r )
{
    return r->segs.data( );
}
const uint64_t* ma_or_res_seed_off( const ma_or_result* r )
{
    return r->seedOff.data( );
}
const ma_or_seed* ma_or_res_seeds( const ma_or_result* r )
{
    return r->seeds.data( );
}
const uint64_t* ma_or_res_hset_off( const ma_or_result* r )
{
    return r->hsetOff.data( );
}
const uint64_t* ma_or_res_hseed_off( const ma_or_result* r )
{
    return r->hseedOff.data( );
}
const uint32_t* ma_or_res_hset_soc( const ma_or_result* r )
{
    return r->hsetSoc.data( );
}
const ma_or_seed* ma_or_res_hseeds( const ma_or_result* r )
{
    return r->hseeds.data( );
}
const uint64_t* ma_or_res_aln_off( const ma_or_result* r )
{
    return r->alnOff.data( );
}
const uint64_t* ma_or_res_mq_off( const ma_or_result* r )
{
    return r->mqOff.data( );
}
const ma_or_alignment* ma_or_res_mq( const ma_or_result* r )
{
    return r->mq.data( );
}
const ma_or_alignment* ma_or_res_alns( const ma_or_result* r )
{
    return r->alns.data( );
}
const uint64_t* ma_or_res_ops( const ma_or_result* r )
{
    return r->ops.data( );
}
uint64_t ma_or_res_n_ops( const ma_or_result* r )
{
    return r->ops.size( ) / 2;
}
void ma_or_res_counters( const ma_or_result* r, uint64_t out[ 8 ] )
{
    for( int i = 0; i < 8; i++ )
        out[ i ] = r->counters[ i ];
}
uint64_t ma_or_res_n_aligned( const ma_or_result* r )
{
    return r->nAligned;
}

// ---- the chain stage alone, from given seeds (tests of the product's sorts on chosen input orders) ----
struct ma_or_chain_result
{
    std::vector<u64> seedOff, socOff, hsetOff, hseedOff;
    std::vector<ma_or_seed> sorted, hseeds;
    std::vector<ma_or_soc> heap, pops;
    std::vector<uint32_t> hsetSoc;
};

static ma_or_soc toSocRec( const SoCEntry& e )
{
    ma_or_soc r;
    r.acc_len = e.sc.accLen;
    r.ambiguity = e.sc.amb;
    r.n_seeds = e.sc.cnt;
    r.begin = (uint32_t)e.b;
    r.end = (uint32_t)e.e;
    return r;
}

ma_or_chain_result* ma_or_chain_seeds( const ma_or_index* x, const ma_or_params* P, const uint64_t* read_lens,
                                       const uint64_t* seed_off, const ma_or_seed* seeds, uint64_t n )
{
    ma_or_chain_result* res = new ma_or_chain_result( );
    Ctx c{ *x, *P };
    res->seedOff.push_back( 0 );
    res->socOff.push_back( 0 );
    res->hsetOff.push_back( 0 );
    res->hseedOff.push_back( 0 );
    for( u64 i = 0; i < n; i++ )
    {
        std::vector<Seed> work;
        for( u64 k = seed_off[ i ]; k < seed_off[ i + 1 ]; k++ )
        {
            Seed s;
            s.q = (u64)seeds[ k ].q_start;
            s.len = (u64)seeds[ k ].len;
            s.r = (u64)seeds[ k ].r_start;
            s.delta = (u64)seeds[ k ].delta;
            s.amb = seeds[ k ].ambiguity;
            s.fwd = seeds[ k ].on_forward != 0;
            work.push_back( s );
        }
        SoCQueue Q;
        socSweep( c, work, read_lens[ i ], Q ); // std::sort by delta, the windows, make_heap, std::sort by reference position
        for( const Seed& s : work )
            res->sorted.push_back( toSeedRec( s ) );
        res->seedOff.push_back( res->sorted.size( ) );
        for( const SoCEntry& e : Q.vMaxima )
            res->heap.push_back( toSocRec( e ) );
        {
            std::vector<SoCEntry> h = Q.vMaxima; // pop order (SoCPriorityQueue::pop, soc.h:240-284) on a copy of the array
            while( !h.empty( ) )
            {
                res->pops.push_back( toSocRec( h.front( ) ) );
                std::pop_heap( h.begin( ), h.end( ), SoCQueue::heapOrder );
                h.pop_back( );
            }
        }
        res->socOff.push_back( res->heap.size( ) );
        std::vector<SeedSet> harm;
        harmonize( c, Q, read_lens[ i ], harm );
        for( const SeedSet& h : harm )
        {
            for( const Seed& s : h.v )
                res->hseeds.push_back( toSeedRec( s ) );
            res->hseedOff.push_back( res->hseeds.size( ) );
            res->hsetSoc.push_back( h.socIndex );
        }
        res->hsetOff.push_back( res->hsetSoc.size( ) );
    }
    return res;
}
void ma_or_chain_result_free( ma_or_chain_result* r )
{
    delete r;
}
const void* ma_or_chain_res_array( const ma_or_chain_result* r, int32_t which, uint64_t* count )
{
#define MA_OR_ARR( v )                                                                                                 \
    {                                                                                                                  \
        *count = r->v.size( );                                                                                         \
        return r->v.data( );                                                                                           \
    }
    switch( which )
    {
        case MA_OR_CHAIN_SEED_OFF: MA_OR_ARR( seedOff )
        case MA_OR_CHAIN_SORTED_SEEDS: MA_OR_ARR( sorted )
        case MA_OR_CHAIN_SOC_OFF: MA_OR_ARR( socOff )
        case MA_OR_CHAIN_SOC_HEAP: MA_OR_ARR( heap )
        case MA_OR_CHAIN_SOC_POPS: MA_OR_ARR( pops )
        case MA_OR_CHAIN_HSET_OFF: MA_OR_ARR( hsetOff )
        case MA_OR_CHAIN_HSEED_OFF: MA_OR_ARR( hseedOff )
        case MA_OR_CHAIN_HSET_SOC: MA_OR_ARR( hsetSoc )
        case MA_OR_CHAIN_HSEEDS: MA_OR_ARR( hseeds )
    }
#undef MA_OR_ARR
    *count = 0;
    return nullptr;
}

// ---- the NeedlemanWunsch + MappingQuality stage alone, from given harmonized sets (tests of the product's walk on chosen sets) ----
struct ma_or_nw_result
{
    std::vector<u64> alnOff, mqOff, ops, mqOps, jobOff, nAligned;
    std::vector<ma_or_alignment> alns, mq;
    std::vector<ma_or_ksw_call> jobs;
};

static ma_or_alignment toAlnRec( const Aln& a, std::vector<u64>& ops, bool flags )
{
    ma_or_alignment r;
    r.begin_ref = (i64)a.bRef;
    r.end_ref = (i64)a.eRef;
    r.begin_q = (i64)a.bQ;
    r.end_q = (i64)a.eQ;
    r.score = a.score;
    r.soc_index = a.socIndex;
    r.n_ops = (uint32_t)a.data.size( );
    r.ops_off = ops.size( ) / 2;
    r.secondary = flags && a.secondary ? 1 : 0;
    r.supplementary = flags && a.supplementary ? 1 : 0;
    r.mapq = flags ? a.mapq : 0;
    for( auto& d : a.data )
    {
        ops.push_back( (u64)d.first );
        ops.push_back( d.second );
    }
    return r;
}

ma_or_nw_result* ma_or_nw_sets( const ma_or_index* x, const ma_or_params* P, const uint8_t* reads, const uint64_t* read_off,
                                uint64_t n, const uint64_t* hset_off, const uint64_t* hseed_off, const uint32_t* hset_soc,
                                const ma_or_seed* hseeds )
{
    ma_or_nw_result* res = new ma_or_nw_result( );
    Ctx c{ *x, *P };
    res->alnOff.push_back( 0 );
    res->mqOff.push_back( 0 );
    res->jobOff.push_back( 0 );
    res->nAligned.push_back( 0 );
    std::vector<KswCall> calls;
    for( u64 i = 0; i < n; i++ )
    {
        const u64 qlen = read_off[ i + 1 ] - read_off[ i ];
        std::vector<uint8_t> Q( reads + read_off[ i ], reads + read_off[ i + 1 ] );
        std::vector<Aln> alns;
        for( u64 s = hset_off[ i ]; s < hset_off[ i + 1 ]; s++ )
        {
            SeedSet set;
            set.socIndex = hset_soc[ s ];
            for( u64 k = hseed_off[ s ]; k < hseed_off[ s + 1 ]; k++ )
            {
                Seed sd;
                sd.q = (u64)hseeds[ k ].q_start;
                sd.len = (u64)hseeds[ k ].len;
                sd.r = (u64)hseeds[ k ].r_start;
                sd.delta = (u64)hseeds[ k ].delta;
                sd.amb = hseeds[ k ].ambiguity;
                sd.fwd = hseeds[ k ].on_forward != 0;
                set.v.push_back( sd );
            }
            calls.clear( );
            tlsCalls = &calls; // the kswcpp calls of this set, in call order
            alns.push_back( executeOne( c, set, Q ) );
            tlsCalls = nullptr;
            for( const KswCall& k : calls )
                res->jobs.push_back( ma_or_ksw_call{ k.qlen, k.tlen, k.w, k.zdrop, k.flag } );
            res->jobOff.push_back( res->jobs.size( ) );
        }
        nwSort( alns ); // NeedlemanWunsch::execute's final sort (needlemanWunsch.h:131-132)
        for( const Aln& a : alns )
            res->alns.push_back( toAlnRec( a, res->ops, false ) );
        res->alnOff.push_back( res->alns.size( ) );
        std::vector<Aln> tmp = alns, mq;
        mappingQuality( c, qlen, tmp, mq );
        for( const Aln& a : mq )
            res->mq.push_back( toAlnRec( a, res->mqOps, true ) );
        res->mqOff.push_back( res->mq.size( ) );
        if( !mq.empty( ) )
            res->nAligned[ 0 ]++;
    }
    return res;
}
void ma_or_nw_result_free( ma_or_nw_result* r )
{
    delete r;
}
const void* ma_or_nw_res_array( const ma_or_nw_result* r, int32_t which, uint64_t* count )
{
#define MA_OR_ARR( v )                                                                                                 \
    {                                                                                                                  \
        *count = r->v.size( );                                                                                         \
        return r->v.data( );                                                                                           \
    }
    switch( which )
    {
        case MA_OR_NW_ALN_OFF: MA_OR_ARR( alnOff )
        case MA_OR_NW_ALNS: MA_OR_ARR( alns )
        case MA_OR_NW_OPS: MA_OR_ARR( ops )
        case MA_OR_NW_MQ_OFF: MA_OR_ARR( mqOff )
        case MA_OR_NW_MQ: MA_OR_ARR( mq )
        case MA_OR_NW_MQ_OPS: MA_OR_ARR( mqOps )
        case MA_OR_NW_JOB_OFF: MA_OR_ARR( jobOff )
        case MA_OR_NW_JOBS: MA_OR_ARR( jobs )
        case MA_OR_NW_N_ALIGNED: MA_OR_ARR( nAligned )
    }
#undef MA_OR_ARR
    *count = 0;
    return nullptr;
}

int ma_or_dump_pipe( const ma_or_index* x, const ma_or_params* P, const uint8_t* reads, const uint64_t* off,
                     uint64_t n, const char* out_path )
{
    FILE* f = fopen( out_path, "w" );
    if( !f )
        return -1;
    Ctx c{ *x, *P };
    for( u64 i = 0; i < n; i++ )
    {
        ReadResult R;
        std::vector<SeedSet> soc;
        u64 qlen = off[ i + 1 ] - off[ i ];
        alignRead( c, reads + off[ i ], qlen, R, &soc );
        fprintf( f, "R %llu %llu\n", (unsigned long long)i, (unsigned long long)qlen );
        fprintf( f, "SEG %zu\n", R.segs.size( ) );
        for( const Seg& s : R.segs )
            fprintf( f, "s %llu %llu %lld %lld %lld\n", (unsigned long long)s.start, (unsigned long long)s.size,
                     (long long)s.sa[ 0 ], (long long)s.sa[ 1 ], (long long)s.sa[ 2 ] );
        fprintf( f, "SEED %zu\n", R.seeds.size( ) );
        for( const Seed& s : R.seeds )
            dumpSeedLine( f, "d", s );
        fprintf( f, "SOC %zu\n", soc.size( ) );
        for( SeedSet& s : soc )
        {
            Seed tag = s.v.back( );
            s.v.pop_back( );
            fprintf( f, "c %u %llu %u %zu\n", s.socIndex, (unsigned long long)tag.q, tag.amb, s.v.size( ) );
            for( const Seed& e : s.v )
                dumpSeedLine( f, "e", e );
        }
        fprintf( f, "HARM %zu\n", R.harm.size( ) );
        for( const SeedSet& h : R.harm )
        {
            fprintf( f, "h %u %zu\n", h.socIndex, h.v.size( ) );
            for( const Seed& e : h.v )
                dumpSeedLine( f, "g", e );
        }
        fprintf( f, "ALN %zu\n", R.alns.size( ) );
        for( const Aln& a : R.alns )
        {
            fprintf( f, "a %llu %llu %llu %llu %lld %u %zu", (unsigned long long)a.bRef, (unsigned long long)a.eRef,
                     (unsigned long long)a.bQ, (unsigned long long)a.eQ, (long long)a.score, a.socIndex,
                     a.data.size( ) );
            for( auto& d : a.data )
                fprintf( f, " %d:%llu", d.first, (unsigned long long)d.second );
            fprintf( f, "\n" );
        }
        fprintf( f, "MQ %zu\n", R.mq.size( ) );
        for( const Aln& a : R.mq )
            fprintf( f, "m %llu %llu %llu %llu %lld %d %d %.17g\n", (unsigned long long)a.bRef,
                     (unsigned long long)a.eRef, (unsigned long long)a.bQ, (unsigned long long)a.eQ,
                     (long long)a.score, (int)a.secondary, (int)a.supplementary, a.mapq );
    }
    fclose( f );
    return 0;
}

static void dumpF4Line( FILE* f, const char* tag, const Aln& a )
{
    fprintf( f, "%s %d %d %llu %llu %llu %llu %lld %u %d %d %.17g %zu", tag, (int)a.first, a.other, (unsigned long long)a.bRef,
             (unsigned long long)a.eRef, (unsigned long long)a.bQ, (unsigned long long)a.eQ, (long long)a.score, a.socIndex,
             (int)a.secondary, (int)a.supplementary, a.mapq, a.data.size( ) );
    for( auto& d : a.data )
        fprintf( f, " %d:%llu", d.first, (unsigned long long)d.second );
    fprintf( f, "\n" );
}

int ma_or_dump_f4( const ma_or_index* x, const ma_or_params* P, const uint8_t* reads, const uint64_t* off, uint64_t n,
                   const char* path )
{
    FILE* f = fopen( path, "w" );
    if( !f )
        return -1;
    Ctx c{ *x, *P };
    auto finalList = [ & ]( u64 i, std::vector<Aln>& fin ) {
        ReadResult R;
        alignRead( c, reads + off[ i ], off[ i + 1 ] - off[ i ], R, nullptr );
        if( P->search_inversions )
            smallInversions( c, reads + off[ i ], R.mq, fin );
        else
            fin = R.mq;
    };
    if( !P->use_paired_reads )
        for( u64 i = 0; i < n; i++ )
        {
            std::vector<Aln> fin;
            finalList( i, fin );
            fprintf( f, "R %llu %llu\nFIN 0 %zu\n", (unsigned long long)i, (unsigned long long)( off[ i + 1 ] - off[ i ] ),
                     fin.size( ) );
            for( const Aln& a : fin )
                dumpF4Line( f, "f", a );
        }
    else
        for( u64 k = 0; 2 * k + 1 < n; k++ )
        {
            std::vector<Aln> fin[ 2 ], pair;
            finalList( 2 * k, fin[ 0 ] );
            finalList( 2 * k + 1, fin[ 1 ] );
            const u64 l1 = off[ 2 * k + 1 ] - off[ 2 * k ], l2 = off[ 2 * k + 2 ] - off[ 2 * k + 1 ];
            pairedReads( c, l1, l2, fin[ 0 ], fin[ 1 ], pair );
            fprintf( f, "P %llu %llu %llu\n", (unsigned long long)k, (unsigned long long)l1, (unsigned long long)l2 );
            for( int m = 0; m < 2; m++ )
            {
                fprintf( f, "FIN %d %zu\n", m, fin[ m ].size( ) );
                for( const Aln& a : fin[ m ] )
                    dumpF4Line( f, "f", a );
            }
            fprintf( f, "PAIR %zu\n", pair.size( ) );
            for( const Aln& a : pair )
                dumpF4Line( f, "p", a );
        }
    fclose( f );
    return 0;
}

} // extern "C"
