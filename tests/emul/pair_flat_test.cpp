// CPU-only checks of the flat pairing (ma_amd/host/ma_pair_flat.h), the code the device stage runs per pair.
//   pair_flat_test golden <case> <f4 dump> <preset> <out.f4> <sam options> <out.sam>
//       the per-mate lists of an f4 dump of the compiled reference ("f" records) as flat ma_alignment arrays -> pickFlat ->
//       the dump again; its "PAIR" / "p" records must be the reference's.  The same picks through the flat pair formatter
//       (ma_flat_sam.h formatPair): the bytes must be those of the reference's PairedFileWriter.
//   pair_flat_test ties
//       synthetic lists with many candidates of the same key through pickFlat and through PairedReads::execute of
//       ma_modules.h (the container path): same pick, same flags, same mapq bits; and ss::sort_upto32 (the sort the
//       kernel runs on up to 32 candidates) against the real std::sort.  Prints what it compared, exits non-zero on a
//       difference.
#include "../../oracle/dump_format.h"
#include "ma_sam.h"
#include "ma_flat_sam.h"
#include "ma_pair_flat.h"
#include "../../ma_amd/csrc/stdsort.h"

#include <cstdio>
#include <cstring>
#include <random>
#include <sstream>

using namespace libMA;
typedef libMS::ContainerVector<std::shared_ptr<Alignment>> AlnVec;

struct FlatMate
{
    std::vector<ma_alignment> a;
};

static void dumpFlat( FILE* f, const char* tag, const ma_alignment& a, const uint64_t* ops, int iFirst, int iOther )
{
    fprintf( f, "%s %d %d %llu %llu %llu %llu %lld %u %d %d %.17g %zu", tag, iFirst, iOther, (unsigned long long)a.begin_ref,
             (unsigned long long)a.end_ref, (unsigned long long)a.begin_q, (unsigned long long)a.end_q, (long long)a.score, a.soc_index,
             (int)a.secondary, (int)a.supplementary, a.mapq, (size_t)a.n_ops );
    for( uint32_t k = 0; k < a.n_ops; k++ )
        fprintf( f, " %d:%llu", (int)ops[ 2 * ( a.ops_off + k ) ], (unsigned long long)ops[ 2 * ( a.ops_off + k ) + 1 ] );
    fprintf( f, "\n" );
}

static int golden( int argc, char** argv )
{
    if( argc < 8 )
        return 2;
    CaseFile c = readCase( argv[ 2 ] );
    uint64_t uiN = 0;
    for( auto& x : c.contigs )
        uiN += 2 * x.size( );
    const int iOptions = atoi( argv[ 6 ] );
    ma_amd::flat::ContigTable xContigs;
    auto pPack = std::make_shared<Pack>( );
    for( size_t i = 0; i < c.contigs.size( ); i++ )
    {
        pPack->vNames.push_back( c.names[ i ] );
        pPack->vStarts.push_back( uiN / 2 - [ & ] { uint64_t r = 0; for( size_t k = i; k < c.contigs.size( ); k++ ) r += c.contigs[ k ].size( ); return r; }( ) );
        pPack->vLengths.push_back( c.contigs[ i ].size( ) );
    }
    xContigs.set( pPack->vNames, pPack->vStarts, pPack->vLengths );
    ma_amd::flat::SamFormat xFormat;
    xFormat.bSoftClip = ( iOptions & 1 ) != 0;
    xFormat.bOutputMCigar = ( iOptions & 2 ) == 0;
    ma_amd::flat::Arena xSam;
    std::vector<std::string> vReadNames( c.reads.size( ) );
    for( size_t i = 0; i < c.reads.size( ); i++ )
        vReadNames[ i ] = "r" + std::to_string( i );
    auto view = [ & ]( size_t i ) {
        ma_amd::flat::ReadView v;
        v.sName = vReadNames[ i ].data( ), v.uiNameLen = vReadNames[ i ].size( );
        v.pCodes = c.reads[ i ].data( ), v.uiLength = c.reads[ i ].size( );
        return v;
    };
    ma_params P;
    if( ma_params_preset( argv[ 4 ], &P ) )
        return 3;
    const ma_pair::Params xPair = ma_pair::params( P, uiN );
    std::ifstream f( argv[ 3 ] );
    FILE* fo = fopen( argv[ 5 ], "w" );
    std::string line;
    FlatMate fin[ 2 ];
    std::vector<uint64_t> ops;
    long unit = -1;
    unsigned long long l1 = 0, l2 = 0;
    int cur = 0;
    auto flush = [ & ]( ) {
        if( unit < 0 )
            return;
        const uint32_t n1 = (uint32_t)fin[ 0 ].a.size( ), n2 = (uint32_t)fin[ 1 ].a.size( );
        const ma_pair::Pick p = ma_pair::pickFlat( fin[ 0 ].a.data( ), n1, fin[ 1 ].a.data( ), n2, ops.data( ), l1, l2, xPair );
        std::vector<ma_alignment> out( std::max<size_t>( 2, std::max( n1, n2 ) ) );
        std::vector<int32_t> mate( out.size( ) ), other( out.size( ) );
        const uint32_t n = ma_pair::records( p, fin[ 0 ].a.data( ), n1, fin[ 1 ].a.data( ), n2, out.data( ), mate.data( ), other.data( ) );
        fprintf( fo, "P %ld %llu %llu\n", unit, l1, l2 );
        for( int m = 0; m < 2; m++ )
        {
            fprintf( fo, "FIN %d %zu\n", m, fin[ m ].a.size( ) );
            for( auto& a : fin[ m ].a )
                dumpFlat( fo, "f", a, ops.data( ), m == 0 ? 1 : 0, -1 );
        }
        fprintf( fo, "PAIR %u\n", n );
        for( uint32_t k = 0; k < n; k++ )
            dumpFlat( fo, "p", out[ k ], ops.data( ), mate[ k ], other[ k ] );
        ma_amd::flat::formatPair( xSam, xFormat, xContigs, view( 2 * (size_t)unit ), view( 2 * (size_t)unit + 1 ), out.data( ), n, ops.data( ),
                                  mate.data( ), other.data( ) );
        fin[ 0 ].a.clear( ), fin[ 1 ].a.clear( ), ops.clear( );
    };
    while( std::getline( f, line ) )
    {
        std::istringstream ss( line );
        std::string tag;
        ss >> tag;
        if( tag == "P" )
        {
            flush( );
            ss >> unit >> l1 >> l2;
        }
        else if( tag == "FIN" )
            ss >> cur;
        else if( tag == "f" )
        {
            ma_alignment a;
            memset( &a, 0, sizeof( a ) );
            int first, other;
            size_t nops;
            std::string sMq;
            ss >> first >> other >> a.begin_ref >> a.end_ref >> a.begin_q >> a.end_q >> a.score >> a.soc_index >> a.secondary >>
                a.supplementary >> sMq >> nops;
            a.mapq = sMq == "nan" ? NAN : strtod( sMq.c_str( ), nullptr );
            a.n_ops = (uint32_t)nops;
            a.ops_off = ops.size( ) / 2;
            for( size_t k = 0; k < nops; k++ )
            {
                std::string op;
                ss >> op;
                const size_t colon = op.find( ':' );
                ops.push_back( (uint64_t)atoi( op.substr( 0, colon ).c_str( ) ) );
                ops.push_back( strtoull( op.c_str( ) + colon + 1, nullptr, 10 ) );
            }
            fin[ cur ].a.push_back( a );
        }
    }
    flush( );
    fclose( fo );
    auto pStream = std::make_shared<StringOutStream>( );
    sam::writeHeader( *pStream, *pPack, false ); // PairedFileWriter on a stream (fileWriter.h:498-511)
    FILE* fs = fopen( argv[ 7 ], "w" );
    fputs( pStream->sText.c_str( ), fs );
    fwrite( xSam.data( ), 1, xSam.size( ), fs );
    fclose( fs );
    return 0;
}

// ---- ties ----------------------------------------------------------------------------------------------------------
static const uint64_t F = 1000000, N = 2 * F;

struct Synth // one mate's list: flat and as containers
{
    std::vector<ma_alignment> flat;
    std::shared_ptr<AlnVec> vec = std::make_shared<AlnVec>( );
};
static void add( Synth& s, std::vector<uint64_t>& ops, uint64_t begin, int64_t score, const std::vector<std::pair<int, uint64_t>>& d )
{
    ma_alignment a;
    memset( &a, 0, sizeof( a ) );
    a.begin_ref = (int64_t)begin, a.end_ref = (int64_t)begin + 150, a.begin_q = 0, a.end_q = 150, a.score = score;
    a.n_ops = (uint32_t)d.size( ), a.ops_off = ops.size( ) / 2;
    a.secondary = s.flat.empty( ) ? 0 : 1;
    a.mapq = s.flat.empty( ) ? 0.25 : 0.0;
    auto p = std::make_shared<Alignment>( );
    p->uiBeginOnRef = begin, p->uiEndOnRef = begin + 150, p->uiBeginOnQuery = 0, p->uiEndOnQuery = 150, p->iScore = score;
    p->bSecondary = a.secondary != 0, p->bSupplementary = false, p->fMappingQuality = a.mapq;
    for( auto& x : d )
    {
        ops.push_back( (uint64_t)x.first ), ops.push_back( x.second );
        p->data.emplace_back( (MatchType)x.first, x.second );
    }
    s.flat.push_back( a );
    s.vec->push_back( p );
}

static int nCompared = 0, nTiedCases = 0, nSorted = 0;

static bool compareOne( Synth& s1, Synth& s2, const std::vector<uint64_t>& ops, ParameterSetManager& xParams, std::shared_ptr<Pack> pPack,
                        const char* what )
{
    ma_params P = *xParams.getSelected( );
    const ma_pair::Params xPair = ma_pair::params( P, N );
    const uint32_t n1 = (uint32_t)s1.flat.size( ), n2 = (uint32_t)s2.flat.size( );
    const ma_pair::Pick p = ma_pair::pickFlat( s1.flat.data( ), n1, s2.flat.data( ), n2, ops.data( ), 150, 150, xPair );
    std::vector<ma_alignment> out( std::max<size_t>( 2, std::max( n1, n2 ) ) );
    std::vector<int32_t> mate( out.size( ) ), other( out.size( ) );
    const uint32_t n = ma_pair::records( p, s1.flat.data( ), n1, s2.flat.data( ), n2, out.data( ), mate.data( ), other.data( ) );
    // the kernel's sort on the same candidates
    {
        ma_pair::FlatList a{ s1.flat.data( ), n1, ops.data( ) }, b{ s2.flat.data( ), n2, ops.data( ) };
        ma_pair::Scan s = ma_pair::scan( a, b, xPair );
        if( s.nTied > 1 )
            nTiedCases++;
        if( s.nCand && s.nCand <= 32 )
        {
            std::vector<ma_pair::Cand> v( s.nCand ), w;
            ma_pair::fill( a, b, xPair, v.data( ) );
            w = v;
            std::sort( v.begin( ), v.end( ), ma_pair::Before( ) );
            ma::ss::sort_upto32( w.data( ), (i64)w.size( ), ma_pair::Before( ) );
            nSorted++;
            for( size_t k = 0; k < v.size( ); k++ )
                if( v[ k ].key != w[ k ].key || v[ k ].i != w[ k ].i || v[ k ].jp != w[ k ].jp )
                {
                    printf( "%s: sort_upto32 differs from std::sort at %zu of %zu\n", what, k, v.size( ) );
                    return false;
                }
        }
    }
    auto pQ1 = std::make_shared<NucSeq>( ), pQ2 = std::make_shared<NucSeq>( );
    pQ1->xCodes.assign( 150, 0 ), pQ2->xCodes.assign( 150, 0 );
    PairedReads xModule( xParams );
    std::shared_ptr<AlnVec> pRet;
    bool bThrew = false;
    try
    {
        pRet = xModule.execute( pQ1, pQ2, s1.vec, s2.vec, pPack );
    }
    catch( const std::runtime_error& e )
    {
        bThrew = true;
        if( std::string( e.what( ) ) != ma_pair::noCandidateText( ) )
        {
            printf( "%s: error texts differ\n", what );
            return false;
        }
    }
    nCompared++;
    if( bThrew != ( p.kind == ma_pair::NO_CANDIDATE ) )
    {
        printf( "%s: one of the two failed\n", what );
        return false;
    }
    if( bThrew )
        return true;
    if( pRet->size( ) != n )
    {
        printf( "%s: %zu records vs %u\n", what, pRet->size( ), n );
        return false;
    }
    for( uint32_t k = 0; k < n; k++ )
    {
        const Alignment& r = *( *pRet )[ k ];
        int iOther = -1;
        auto pO = r.xStats.pOther.lock( );
        for( size_t j = 0; pO != nullptr && j < pRet->size( ); j++ )
            if( ( *pRet )[ j ] == pO )
                iOther = (int)j;
        uint64_t b1, b2;
        const double d1 = r.fMappingQuality, d2 = out[ k ].mapq;
        memcpy( &b1, &d1, 8 ), memcpy( &b2, &d2, 8 );
        if( r.uiBeginOnRef != (uint64_t)out[ k ].begin_ref || r.iScore != out[ k ].score || r.bSecondary != ( out[ k ].secondary != 0 ) ||
            r.bSupplementary != ( out[ k ].supplementary != 0 ) || b1 != b2 || (int)r.xStats.bFirst != mate[ k ] || iOther != other[ k ] ||
            r.data.size( ) != out[ k ].n_ops )
        {
            printf( "%s: record %u differs (begin %llu / %lld, mapq %.17g / %.17g, other %d / %d)\n", what, k,
                    (unsigned long long)r.uiBeginOnRef, (long long)out[ k ].begin_ref, d1, d2, iOther, other[ k ] );
            return false;
        }
    }
    return true;
}

static int ties( )
{
    ParameterSetManager xParams;
    xParams.setSelected( "illuminapaired" );
    auto pPack = std::make_shared<Pack>( );
    pPack->vNames.push_back( "chr1" );
    pPack->vStarts.push_back( 0 );
    pPack->vLengths.push_back( F );
    const std::vector<std::pair<int, uint64_t>> oneSeed = { { 0, 150 } }, twoSeeds = { { 0, 70 }, { 2, 1 }, { 0, 79 } }, empty0 = { { 1, 0 } };
    bool ok = true;
    // n1 x n2 candidates, every one with the same key; distinct begins tell the records apart
    const int shapes[][ 2 ] = { { 1, 2 }, { 2, 1 }, { 1, 5 }, { 5, 1 }, { 4, 4 }, { 2, 8 }, { 1, 17 }, { 17, 1 }, { 3, 6 }, { 4, 8 }, { 5, 8 },
                                { 8, 5 }, { 6, 7 }, { 3, 11 }, { 1, 33 }, { 20, 2 }, { 7, 9 }, { 10, 10 } };
    for( auto& sh : shapes )
        for( int variant = 0; variant < 4; variant++ )
        {
            // 0: all on one strand (improper), 1: all proper, 2: proper and improper mixed at the same key (bonus 1),
            // 3: like 1 with two seeds per alignment and a lower-scoring tail
            Synth s1, s2;
            std::vector<uint64_t> ops;
            if( variant == 2 )
                xParams.getSelected( )->paired_bonus = 1.0;
            else
                xParams.getSelected( )->paired_bonus = 1.25;
            for( int i = 0; i < sh[ 0 ]; i++ )
                add( s1, ops, 5000 + 3 * i, 290, variant == 3 ? twoSeeds : oneSeed );
            for( int j = 0; j < sh[ 1 ]; j++ )
            {
                uint64_t begin = 5400 + 2 * j; // forward strand
                if( variant == 1 || variant == 3 || ( variant == 2 && j % 2 == 0 ) )
                    begin = N - 1 - ( 5000 + 390 + 2 * j ); // reverse strand, mirrored ~400 behind the first mate
                add( s2, ops, begin, 290, variant == 3 ? twoSeeds : oneSeed );
            }
            if( variant == 3 )
            {
                add( s1, ops, 700000, 200, oneSeed );
                add( s2, ops, 800000, 180, oneSeed );
            }
            char what[ 64 ];
            snprintf( what, sizeof( what ), "%d x %d variant %d", sh[ 0 ], sh[ 1 ], variant );
            ok = compareOne( s1, s2, ops, xParams, pPack, what ) && ok;
        }
    xParams.getSelected( )->paired_bonus = 1.25;
    // random lists: few distinct scores, positions near each other on both strands => ties of every size in between
    std::mt19937_64 rng( 12345 );
    for( int t = 0; t < 3000; t++ )
    {
        Synth s1, s2;
        std::vector<uint64_t> ops;
        const int n1 = (int)( rng( ) % 9 ), n2 = (int)( rng( ) % 9 );
        for( int m = 0; m < 2; m++ )
            for( int i = 0; i < ( m ? n2 : n1 ); i++ )
            {
                uint64_t begin = 5000 + rng( ) % 1200;
                if( rng( ) % 2 )
                    begin = N - 1 - begin;
                const int64_t score = 300 - 2 * (int64_t)( rng( ) % 3 );
                const auto& d = rng( ) % 16 == 0 ? empty0 : ( rng( ) % 2 ? twoSeeds : oneSeed );
                add( m ? s2 : s1, ops, begin, score, d );
            }
        char what[ 64 ];
        snprintf( what, sizeof( what ), "random %d", t );
        ok = compareOne( s1, s2, ops, xParams, pPack, what ) && ok;
    }
    // nothing but alignments of length 0 on one side: both fail with the same text
    {
        Synth s1, s2;
        std::vector<uint64_t> ops;
        add( s1, ops, 5000, 290, empty0 );
        add( s2, ops, 5400, 290, oneSeed );
        ok = compareOne( s1, s2, ops, xParams, pPack, "no candidate" ) && ok;
    }
    printf( "compared %d pairs, %d of them tied, %d sorted with sort_upto32: %s\n", nCompared, nTiedCases, nSorted, ok ? "same" : "DIFFERENT" );
    return ok && nTiedCases > 100 ? 0 : 1;
}

int main( int argc, char** argv )
{
    if( argc >= 2 && !strcmp( argv[ 1 ], "golden" ) )
        return golden( argc, argv );
    if( argc >= 2 && !strcmp( argv[ 1 ], "ties" ) )
        return ties( );
    return 2;
}
