// CPU test of what Engine (ma_amd/host/ma_engine.h) asks of the C ABI: every symbol the engine reaches is a stub here that prints
// one line -- its name and its value arguments (counts, byte sizes, option bits, flags; of a pointer only whether it is null) --
// and returns fixed small answers.  The scenarios run on ONE engine, so capacities and the recycled result carry over from one to
// the next; after each the scalar fields of the result are printed.  No GPU, no libma_amd.so, and never a time: the output is
// compared byte for byte with tests/golden/engine_calls.txt (tests/test_engine_calls.py), which pins the calls, their order and
// their arguments across changes of the header.  The engine's MA_ENGINE_TRACE line goes to stderr (last scenario).
#include "../../ma_amd/host/ma_engine.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static const char* P( const void* p )
{
    return p ? "ptr" : "null";
}
#define U( x ) ( (unsigned long long)( x ) )

// what the stubs answer
static const uint64_t N_SEG = 5, N_SEED = 7, N_HSET = 3, N_HSEED = 9, N_ALN = 4, N_OPS = 6, N_ALIGNED = 2, N_SOCS = 2;
static const uint64_t N_PAIR_RECS = 3, N_PAIR_OPS = 5, N_PAIRS_ON_HOST = 1, SAM_BYTES = 13, PAIR_SAM_BYTES = 11;
static const uint64_t TEXT_READS = 3, TEXT_PAIRS = 2;
static uint64_t g_reads = 0; // reads of the batch as the last setter left them
static int g_refuse = 0; // the next setter call of a text form fails ...
static uint64_t g_refuseCount = 0; // ... and reports this many reads (pairs)
static int g_batches = 0; // live device batches

extern "C" {
const char* ma_last_error( void )
{
    return "stub: the last call failed";
}
int ma_host_alloc( uint64_t bytes, void** out )
{
    return ( *out = malloc( bytes ) ) == nullptr;
}
int ma_host_free( void* p )
{
    free( p );
    return 0;
}
int ma_stream_create( const ma_index* x, void** out )
{
    printf( "ma_stream_create index=%s\n", P( x ) );
    *out = (void*)0x51;
    return 0;
}
int ma_stream_destroy( const ma_index* x, void* s )
{
    printf( "ma_stream_destroy index=%s stream=%s\n", P( x ), P( s ) );
    return 0;
}
int ma_batch_create( const ma_index* x, const ma_params* p, uint64_t max_reads, uint64_t max_bases, ma_batch** out )
{
    printf( "ma_batch_create index=%s params=%s max_reads=%llu max_bases=%llu\n", P( x ), P( p ), U( max_reads ), U( max_bases ) );
    *out = (ma_batch*)malloc( 8 );
    g_batches++;
    g_reads = 0;
    return 0;
}
int ma_batch_destroy( ma_batch* b )
{
    printf( "ma_batch_destroy batch=%s\n", P( b ) );
    free( b );
    g_batches--;
    return 0;
}
int ma_batch_set_stream( ma_batch* b, void* s )
{
    printf( "ma_batch_set_stream batch=%s stream=%s\n", P( b ), P( s ) );
    return 0;
}
int ma_batch_set_blocking_sync( ma_batch* b, int on )
{
    printf( "ma_batch_set_blocking_sync batch=%s on=%d\n", P( b ), on );
    return 0;
}
int ma_batch_set_reads( ma_batch* b, const uint8_t* codes, const uint64_t* off, uint64_t n )
{
    printf( "ma_batch_set_reads batch=%s codes=%s offsets=%s n=%llu bases=%llu\n", P( b ), P( codes ), P( off ), U( n ), U( off[ n ] ) );
    g_reads = n;
    return 0;
}
int ma_batch_set_read_text( ma_batch* b, const char* names, const uint64_t* name_off, const uint8_t* qual )
{
    printf( "ma_batch_set_read_text batch=%s names=%s name_off=%s name_bytes=%llu qual=%s\n", P( b ), P( names ), P( name_off ),
            U( name_off[ g_reads ] ), P( qual ) );
    return 0;
}
static int text_answer( uint64_t* n, uint64_t fits, uint64_t per )
{
    if( g_refuse )
    {
        g_refuse = 0;
        *n = g_refuseCount;
        printf( "  -> refused, reports %llu\n", U( g_refuseCount ) );
        return 1;
    }
    *n = fits;
    g_reads = per * fits;
    return 0;
}
int ma_batch_set_reads_text( ma_batch* b, const char* text, uint64_t n_bytes, uint64_t* n_reads )
{
    printf( "ma_batch_set_reads_text batch=%s text=%s n_bytes=%llu n_reads=%s\n", P( b ), P( text ), U( n_bytes ), P( n_reads ) );
    return text_answer( n_reads, TEXT_READS, 1 );
}
int ma_batch_set_reads_bgzf( ma_batch* b, const char* head, uint64_t n_head, const void* members, uint64_t n_bytes, uint64_t n_drop,
                             uint64_t* n_reads )
{
    printf( "ma_batch_set_reads_bgzf batch=%s head=%s n_head=%llu members=%s n_bytes=%llu n_drop=%llu n_reads=%s\n", P( b ), P( head ),
            U( n_head ), P( members ), U( n_bytes ), U( n_drop ), P( n_reads ) );
    return text_answer( n_reads, TEXT_READS, 1 );
}
int ma_batch_set_mates_text( ma_batch* b, const char* text1, uint64_t n1, const char* text2, uint64_t n2, int32_t rev_comp_mates,
                             uint64_t* n_pairs, uint64_t consumed[ 2 ] )
{
    printf( "ma_batch_set_mates_text batch=%s text1=%s n1=%llu text2=%s n2=%llu rev_comp_mates=%d n_pairs=%s consumed=%s\n", P( b ),
            P( text1 ), U( n1 ), P( text2 ), U( n2 ), (int)rev_comp_mates, P( n_pairs ), P( consumed ) );
    consumed[ 0 ] = n1, consumed[ 1 ] = n2;
    return text_answer( n_pairs, TEXT_PAIRS, 2 );
}
int ma_align_batch( ma_batch* b )
{
    printf( "ma_align_batch batch=%s\n", P( b ) );
    return 0;
}
int ma_inversions_batch( ma_batch* b )
{
    printf( "ma_inversions_batch batch=%s\n", P( b ) );
    return 0;
}
int ma_batch_sync( ma_batch* b )
{
    printf( "ma_batch_sync batch=%s\n", P( b ) );
    return 0;
}
int ma_batch_host_ms( ma_batch* b, float out[ 8 ] )
{
    printf( "ma_batch_host_ms batch=%s out=%s\n", P( b ), P( out ) );
    for( int i = 0; i < 8; i++ )
        out[ i ] = 0.5f * (float)( i + 1 );
    return 0;
}
int ma_batch_counts( ma_batch* b, uint64_t* n_segments, uint64_t* n_seeds, uint64_t* n_hsets, uint64_t* n_hseeds, uint64_t* n_alignments,
                     uint64_t* n_ops, uint64_t* n_aligned_reads )
{
    printf( "ma_batch_counts batch=%s segments=%s seeds=%s hsets=%s hseeds=%s alignments=%s ops=%s aligned_reads=%s\n", P( b ),
            P( n_segments ), P( n_seeds ), P( n_hsets ), P( n_hseeds ), P( n_alignments ), P( n_ops ), P( n_aligned_reads ) );
    uint64_t* const out[ 7 ] = { n_segments, n_seeds, n_hsets, n_hseeds, n_alignments, n_ops, n_aligned_reads };
    const uint64_t val[ 7 ] = { N_SEG, N_SEED, N_HSET, N_HSEED, N_ALN, N_OPS, N_ALIGNED };
    for( int i = 0; i < 7; i++ )
        if( out[ i ] )
            *out[ i ] = val[ i ];
    return 0;
}
// (the getters fill what the library would: an array the engine made too small is a finding of the sanitizer build)
static void csr( uint64_t* off, uint64_t n, uint64_t total )
{
    for( uint64_t i = 0; i < n; i++ )
        off[ i ] = std::min<uint64_t>( i, total );
    off[ n ] = total;
}
int ma_batch_get_segments( ma_batch* b, uint64_t* seg_off, ma_segment* segs )
{
    printf( "ma_batch_get_segments batch=%s seg_off=%s segs=%s\n", P( b ), P( seg_off ), P( segs ) );
    csr( seg_off, g_reads, N_SEG );
    memset( segs, 0, N_SEG * sizeof( ma_segment ) );
    return 0;
}
int ma_batch_get_seeds( ma_batch* b, uint64_t* seed_off, ma_seed* seeds )
{
    printf( "ma_batch_get_seeds batch=%s seed_off=%s seeds=%s\n", P( b ), P( seed_off ), P( seeds ) );
    csr( seed_off, g_reads, N_SEED );
    memset( seeds, 0, N_SEED * sizeof( ma_seed ) );
    return 0;
}
int ma_batch_get_hsets( ma_batch* b, uint64_t* hset_off, uint64_t* hseed_off, uint32_t* hset_soc, ma_seed* hseeds )
{
    printf( "ma_batch_get_hsets batch=%s hset_off=%s hseed_off=%s hset_soc=%s hseeds=%s\n", P( b ), P( hset_off ), P( hseed_off ),
            P( hset_soc ), P( hseeds ) );
    csr( hset_off, g_reads, N_HSET );
    csr( hseed_off, N_HSET, N_HSEED );
    memset( hset_soc, 0, N_HSET * 4 );
    memset( hseeds, 0, N_HSEED * sizeof( ma_seed ) );
    return 0;
}
int ma_batch_get_soc_heap( ma_batch* b, uint64_t* n_socs, uint64_t* soc_off, ma_soc* socs, uint64_t* seed_off, ma_seed* sorted_seeds )
{
    printf( "ma_batch_get_soc_heap batch=%s n_socs=%s soc_off=%s socs=%s seed_off=%s sorted_seeds=%s\n", P( b ), P( n_socs ), P( soc_off ),
            P( socs ), P( seed_off ), P( sorted_seeds ) );
    *n_socs = N_SOCS;
    if( soc_off )
        csr( soc_off, g_reads, N_SOCS );
    if( socs )
        memset( socs, 0, N_SOCS * sizeof( ma_soc ) );
    if( seed_off )
        csr( seed_off, g_reads, N_SEED );
    if( sorted_seeds )
        memset( sorted_seeds, 0, N_SEED * sizeof( ma_seed ) );
    return 0;
}
static void records( uint64_t* off, uint64_t n, ma_alignment* alns, uint64_t* ops, uint64_t nAln, uint64_t nOps )
{
    csr( off, n, nAln );
    memset( alns, 0, nAln * sizeof( ma_alignment ) );
    memset( ops, 0, 2 * nOps * 8 );
    alns[ nAln - 1 ].ops_off = nOps - 2; // the last record: where the engine reads the number of ops from
    alns[ nAln - 1 ].n_ops = 2;
}
int ma_batch_get_alignments( ma_batch* b, uint64_t* aln_off, ma_alignment* alns, uint64_t* ops )
{
    printf( "ma_batch_get_alignments batch=%s aln_off=%s alns=%s ops=%s\n", P( b ), P( aln_off ), P( alns ), P( ops ) );
    records( aln_off, g_reads, alns, ops, N_ALN, N_OPS );
    return 0;
}
int ma_batch_get_mapq_alignments( ma_batch* b, uint64_t* aln_off, ma_alignment* alns, uint64_t* ops )
{
    printf( "ma_batch_get_mapq_alignments batch=%s aln_off=%s alns=%s ops=%s\n", P( b ), P( aln_off ), P( alns ), P( ops ) );
    records( aln_off, g_reads, alns, ops, N_ALN, N_OPS );
    return 0;
}
int ma_pair_batch( ma_batch* b )
{
    printf( "ma_pair_batch batch=%s\n", P( b ) );
    return 0;
}
int ma_batch_pair_counts( ma_batch* b, uint64_t* n_pairs, uint64_t* n_records, uint64_t* n_ops, uint64_t* n_host_pairs )
{
    printf( "ma_batch_pair_counts batch=%s n_pairs=%s n_records=%s n_ops=%s n_host_pairs=%s\n", P( b ), P( n_pairs ), P( n_records ),
            P( n_ops ), P( n_host_pairs ) );
    if( n_pairs )
        *n_pairs = g_reads / 2;
    if( n_records )
        *n_records = N_PAIR_RECS;
    if( n_ops )
        *n_ops = N_PAIR_OPS;
    if( n_host_pairs )
        *n_host_pairs = N_PAIRS_ON_HOST;
    return 0;
}
int ma_batch_get_pairs( ma_batch* b, uint64_t* pair_off, ma_alignment* alns, uint64_t* ops, int32_t* mate, int32_t* other )
{
    printf( "ma_batch_get_pairs batch=%s pair_off=%s alns=%s ops=%s mate=%s other=%s\n", P( b ), P( pair_off ), P( alns ), P( ops ),
            P( mate ), P( other ) );
    records( pair_off, g_reads / 2, alns, ops, N_PAIR_RECS, N_PAIR_OPS );
    memset( mate, 0, N_PAIR_RECS * 4 );
    memset( other, 0, N_PAIR_RECS * 4 );
    return 0;
}
int ma_sam_batch( ma_batch* b, uint32_t options )
{
    printf( "ma_sam_batch batch=%s options=%u\n", P( b ), options );
    return 0;
}
int ma_batch_sam_counts( ma_batch* b, uint64_t* n_bytes )
{
    printf( "ma_batch_sam_counts batch=%s n_bytes=%s\n", P( b ), P( n_bytes ) );
    *n_bytes = SAM_BYTES;
    return 0;
}
int ma_batch_get_sam( ma_batch* b, uint64_t* rec_off, char* text )
{
    printf( "ma_batch_get_sam batch=%s rec_off=%s text=%s\n", P( b ), P( rec_off ), P( text ) );
    csr( rec_off, g_reads, SAM_BYTES );
    memset( text, 'x', SAM_BYTES );
    return 0;
}
int ma_pair_sam_batch( ma_batch* b, uint32_t options )
{
    printf( "ma_pair_sam_batch batch=%s options=%u\n", P( b ), options );
    return 0;
}
int ma_batch_pair_sam_counts( ma_batch* b, uint64_t* n_pairs, uint64_t* n_bytes )
{
    printf( "ma_batch_pair_sam_counts batch=%s n_pairs=%s n_bytes=%s\n", P( b ), P( n_pairs ), P( n_bytes ) );
    if( n_pairs )
        *n_pairs = g_reads / 2;
    *n_bytes = PAIR_SAM_BYTES;
    return 0;
}
int ma_batch_get_pair_sam( ma_batch* b, uint64_t* pair_off, char* text )
{
    printf( "ma_batch_get_pair_sam batch=%s pair_off=%s text=%s\n", P( b ), P( pair_off ), P( text ) );
    csr( pair_off, g_reads / 2, PAIR_SAM_BYTES );
    memset( text, 'x', PAIR_SAM_BYTES );
    return 0;
}
} // extern "C"

using namespace ma_amd::engine;

static void show( const BatchResult& R )
{
    printf( "result: uiReads=%zu bStages=%d bSocQueues=%d bPairs=%d bSam=%d uiSamOptions=%u uiSamBytes=%llu uiMqAlignments=%llu uiMqOps=%llu "
            "uiPairRecords=%llu uiPairOps=%llu uiPairsOnHost=%llu uiAlignedReads=%llu\n",
            R.uiReads, (int)R.bStages, (int)R.bSocQueues, (int)R.bPairs, (int)R.bSam, R.uiSamOptions, U( R.uiSamBytes ), U( R.uiMqAlignments ),
            U( R.uiMqOps ), U( R.uiPairRecords ), U( R.uiPairOps ), U( R.uiPairsOnHost ), U( R.uiAlignedReads ) );
    // the offset arrays a consumer walks whatever the form of the result: their last entries (a recycled result must not keep old ones)
    printf( "        vMqOff[n]=%llu", U( R.vMqOff[ R.uiReads ] ) );
    if( R.bPairs )
        printf( " vPairOff[n/2]=%llu", U( R.vPairOff[ R.uiReads / 2 ] ) );
    if( R.bSam )
        printf( " vSamOff[last]=%llu", U( R.vSamOff[ R.bPairs ? R.uiReads / 2 : R.uiReads ] ) );
    printf( "\n" );
}
static void title( const char* s )
{
    printf( "== %s\n", s );
}

int main( )
{
    // four reads of 1..4 bases, their names, qualities for all of them
    const std::vector<std::vector<uint8_t>> vCodes = { { 0 }, { 1, 2 }, { 3, 0, 1 }, { 2, 2, 3, 4 } };
    const char* aNames[ 4 ] = { "a", "bb", "ccc", "dddd" };
    const uint8_t aQual[ 4 ] = { 'I', 'J', 'K', 'L' };
    std::vector<ReadRef> vFour, vThree;
    for( const auto& rC : vCodes )
        vFour.emplace_back( rC );
    vThree.assign( vFour.begin( ), vFour.begin( ) + 3 );
    std::vector<ReadText> vAll( 4 ), vNone( 4 ), vMix( 4 );
    for( size_t i = 0; i < 4; i++ )
    {
        vAll[ i ].pName = vNone[ i ].pName = vMix[ i ].pName = aNames[ i ];
        vAll[ i ].uiNameLen = vNone[ i ].uiNameLen = vMix[ i ].uiNameLen = i + 1;
        vAll[ i ].pQuality = aQual;
        vMix[ i ].pQuality = i % 2 ? aQual : nullptr;
    }
    const SamMode xAll{ &vAll, 5 }, xNone{ &vNone, 0 }, xMix{ &vMix, 5 };
    const std::string sText = "@r\nACGT\n+\nIIII\n", sMate = "@m\nAC\n+\nII\n";
    ma_params xP;
    memset( &xP, 0, sizeof( xP ) );
    {
        title( "construct" );
        Engine xE( (const ma_index*)0x1d, xP );
        for( int iInv = 0; iInv < 2; iInv++ )
        {
            const bool bInv = iInv != 0;
            printf( "==== bInversions=%d\n", iInv );
            title( "run plain (3 reads)" );
            show( *xE.run( vThree, false, false, nullptr, bInv ) );
            title( "run bStages" );
            show( *xE.run( vFour, true, false, nullptr, bInv ) );
            title( "run bStages + bFetchSocQueues" );
            xE.bFetchSocQueues = true;
            show( *xE.run( vFour, true, false, nullptr, bInv ) );
            xE.bFetchSocQueues = false;
            title( "run bPairs" );
            show( *xE.run( vFour, false, true, nullptr, bInv ) );
            title( "run SAM, all reads with qualities" );
            show( *xE.run( vFour, false, false, &xAll, bInv ) );
            title( "run SAM, no read with qualities" );
            show( *xE.run( vFour, false, false, &xNone, bInv ) );
            title( "run SAM, some reads with qualities: records" );
            show( *xE.run( vFour, false, false, &xMix, bInv ) );
            title( "run bPairs + SAM" );
            show( *xE.run( vFour, false, true, &xAll, bInv ) );
            title( "run plain after a SAM run: the recycled result" );
            show( *xE.run( vFour, false, false, nullptr, bInv ) );
            title( "run bPairs after a SAM run: the recycled result" );
            show( *xE.run( vFour, false, true, nullptr, bInv ) );
        }
        title( "runText that fits" );
        show( *xE.runText( sText.data( ), sText.size( ), 5 ) );
        title( "runText with inversions" );
        show( *xE.runText( sText.data( ), sText.size( ), 0, true ) );
        title( "runText, capacity exceeded by a text of 100 reads" );
        g_refuse = 1, g_refuseCount = 100;
        show( *xE.runText( sText.data( ), sText.size( ), 5 ) );
        title( "runText, refused with no count: throws" );
        g_refuse = 1, g_refuseCount = 0;
        try
        {
            xE.runText( sText.data( ), sText.size( ), 5 );
            printf( "no exception\n" );
        }
        catch( const std::runtime_error& rE )
        {
            printf( "runtime_error: %s\n", rE.what( ) );
        }
        title( "run plain after the refusal" );
        show( *xE.run( vThree, false ) );
        title( "runBgzf, head only" );
        show( *xE.runBgzf( sText.data( ), sText.size( ), nullptr, 0, 0, 5 ) );
        title( "runMatesText that fits" );
        show( *xE.runMatesText( sText.data( ), sText.size( ), sMate.data( ), sMate.size( ), true, 5 ) );
        title( "runMatesText with inversions, mates as they are" );
        show( *xE.runMatesText( sText.data( ), sText.size( ), sMate.data( ), sMate.size( ), false, 0, true ) );
        title( "runMatesText, capacity exceeded by texts of 90 pairs" );
        g_refuse = 1, g_refuseCount = 90;
        show( *xE.runMatesText( sText.data( ), sText.size( ), sMate.data( ), sMate.size( ), true, 5 ) );
        title( "runMatesText, refused with no count: throws" );
        g_refuse = 1, g_refuseCount = 0;
        try
        {
            xE.runMatesText( sText.data( ), sText.size( ), sMate.data( ), sMate.size( ), true, 5 );
            printf( "no exception\n" );
        }
        catch( const std::runtime_error& rE )
        {
            printf( "runtime_error: %s\n", rE.what( ) );
        }
        title( "run plain after a paired SAM result: the recycled result" );
        show( *xE.run( vFour, false ) );
        title( "a text of 9000 bytes: the batch grows by bases" );
        const std::string sLong( 9000, 'A' );
        show( *xE.runText( sLong.data( ), sLong.size( ), 0 ) );
        title( "MA_ENGINE_TRACE=1: one run of each form" );
        setenv( "MA_ENGINE_TRACE", "1", 1 );
        show( *xE.run( vFour, false ) );
        show( *xE.runText( sText.data( ), sText.size( ), 5 ) );
        show( *xE.runMatesText( sText.data( ), sText.size( ), sMate.data( ), sMate.size( ), true, 5 ) );
        unsetenv( "MA_ENGINE_TRACE" );
        printf( "uiRuns=%llu\n", U( xE.uiRuns ) );
        title( "destruct" );
    }
    printf( "live batches: %d\n", g_batches );
    return g_batches != 0;
}
