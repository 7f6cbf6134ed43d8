// TEST INFRASTRUCTURE ONLY -- the reference's ExtractSeeds::execute (stripOfConsideration.h:138-157: SegmentVector::forEachSeed,
// Segment::forEachSeed with FMIndex::bwt_sa, setDeltaOfSeed) on GIVEN segments (oracle/_ref/ref_dump_extract, Makefile.ref).
// Our own harness, like ref_dump.cpp: it includes the reference's headers where they lie and copies nothing of them.
//
// usage: ref_dump_extract <case> <segments file> <out> <min_seed_len> <max_ambiguity>
//   <case>           MACASE01 (dump_format.h): the genome and the reads
//   <segments file>  EXSEGS01 (dump_format.h): the segments of every read; any row range inside 1 .. n is taken as it is
//   <out>            appended to: "P <min_seed_len> <max_ambiguity>", then per read "R <read> <length>", "SEED <count>" and one line
//                    "d <q_start> <len> <r_start> <ambiguity> <on_forward> <delta>" per seed, in the module's order
#include "ma/container/fMIndex.h"
#include "ma/container/pack.h"
#include "ma/container/segment.h"
#include "ma/module/stripOfConsideration.h"
#include "dump_format.h"

#include <cstdio>
#include <cstdlib>

using namespace libMA;
using namespace libMS;

static std::shared_ptr<NucSeq> mkSeq( const std::vector<uint8_t>& v )
{
    auto p = std::make_shared<NucSeq>( );
    if( !v.empty( ) )
        p->vAppend( v.data( ), v.size( ) );
    return p;
}

int main( int argc, char** argv )
{
    if( argc != 6 )
    {
        fprintf( stderr, "usage: ref_dump_extract <case> <segments file> <out> <min_seed_len> <max_ambiguity>\n" );
        return 2;
    }
    try
    {
        CaseFile c = readCase( argv[ 1 ] );
        SegsFile s = readSegs( argv[ 2 ] );
        if( s.segOff.size( ) != c.reads.size( ) + 1 )
            throw std::runtime_error( "segments file and case differ in their number of reads" );
        auto pPack = std::make_shared<Pack>( );
        for( size_t i = 0; i < c.contigs.size( ); i++ )
            pPack->vAppendSequence( c.names[ i ], "", *mkSeq( c.contigs[ i ] ) );
        auto pFM = std::make_shared<FMIndex>( pPack );
        ParameterSetManager xParams;
        xParams.setSelected( "default" );
        xParams.getSelected( )->xMinSeedLength->set( atoi( argv[ 4 ] ) );
        xParams.getSelected( )->xMaximalSeedAmbiguity->set( atoi( argv[ 5 ] ) );
        ExtractSeeds xExtract( xParams );
        FILE* f = fopen( argv[ 3 ], "a" );
        if( !f )
            throw std::runtime_error( "cannot open the output" );
        fprintf( f, "P %d %d\n", atoi( argv[ 4 ] ), atoi( argv[ 5 ] ) );
        for( size_t i = 0; i < c.reads.size( ); i++ )
        {
            auto pQ = mkSeq( c.reads[ i ] );
            pQ->sName = "r" + std::to_string( i );
            auto pSegs = std::make_shared<SegmentVector>( );
            for( uint64_t k = s.segOff[ i ]; k < s.segOff[ i + 1 ]; k++ )
            {
                const SegsRecord& x = s.segs[ k ];
                pSegs->push_back( Segment( (nucSeqIndex)x.q_start, (nucSeqIndex)x.q_size,
                                           SAInterval( (t_bwtIndex)x.sa_start, (t_bwtIndex)x.sa_start_rc, (t_bwtIndex)x.sa_size ) ) );
            }
            fprintf( f, "R %zu %zu\n", i, c.reads[ i ].size( ) );
            fflush( f ); // (a case the reference dies on shows as the last read of the file)
            auto pSeeds = xExtract.execute( pSegs, pFM, pQ, pPack );
            fprintf( f, "SEED %zu\n", pSeeds->size( ) );
            for( auto& x : *pSeeds )
                fprintf( f, "d %llu %llu %llu %u %d %llu\n", (unsigned long long)x.start( ), (unsigned long long)x.size( ),
                         (unsigned long long)x.start_ref( ), x.uiAmbiguity, (int)x.bOnForwStrand, (unsigned long long)x.uiDelta );
        }
        fclose( f );
    }
    catch( const std::exception& e )
    {
        fprintf( stderr, "ref_dump_extract: %s\n", e.what( ) );
        return 1;
    }
    return 0;
}
