// What the two test programs of the small-inversion stage share -- inv_dev_test.cpp (the shared logic on the CPU) and
// inv_graph_test.cpp (the host layer and the host module on the GPU): the lists of an f4 dump as flat records.
#pragma once
#include "sam_dev_common.h"

static inline void check( bool b, const std::string& sWhat )
{
    if( !b )
        throw std::runtime_error( sWhat );
}

// the FIN lists of an f4 dump (oracle/ref_dump.cpp) as one unit per read
static inline Input fromF4Dump( const char* sCase, const char* sDump, bool bPaired )
{
    Input in = fromCase( sCase );
    std::vector<std::vector<ma_alignment>> vPerRead( in.vReads.size( ) );
    std::vector<std::vector<std::vector<uint64_t>>> vPerReadOps( in.vReads.size( ) );
    std::ifstream f( sDump );
    check( f.good( ), std::string( "cannot open " ) + sDump );
    std::string line;
    long unit = -1, read = -1;
    while( std::getline( f, line ) )
    {
        std::istringstream is( line );
        std::string tag;
        is >> tag;
        if( tag == "R" || tag == "P" )
            is >> unit;
        else if( tag == "FIN" )
        {
            long m;
            is >> m;
            read = bPaired ? 2 * unit + m : unit;
        }
        else if( tag == "f" )
        {
            long first, other;
            unsigned long long br, er, bq, eq;
            long long score;
            unsigned soc;
            int sec, sup;
            std::string sQ;
            size_t n;
            is >> first >> other >> br >> er >> bq >> eq >> score >> soc >> sec >> sup >> sQ >> n;
            ma_alignment a{ };
            a.begin_ref = (int64_t)br, a.end_ref = (int64_t)er, a.begin_q = (int64_t)bq, a.end_q = (int64_t)eq, a.score = score;
            a.soc_index = soc, a.secondary = sec != 0, a.supplementary = sup != 0, a.mapq = strtod( sQ.c_str( ), nullptr );
            a.n_ops = (uint32_t)n;
            std::vector<uint64_t> ops;
            readOps( is, n, ops );
            vPerRead.at( (size_t)read ).push_back( a );
            vPerReadOps.at( (size_t)read ).push_back( ops );
        }
    }
    in.vOff.assign( 1, 0 );
    for( size_t r = 0; r < in.vReads.size( ); r++ )
    {
        for( size_t k = 0; k < vPerRead[ r ].size( ); k++ )
        {
            ma_alignment a = vPerRead[ r ][ k ];
            a.ops_off = in.vOps.size( ) / 2;
            in.vOps.insert( in.vOps.end( ), vPerReadOps[ r ][ k ].begin( ), vPerReadOps[ r ][ k ].end( ) );
            in.vAlns.push_back( a );
        }
        in.vOff.push_back( in.vAlns.size( ) );
    }
    in.vOps.push_back( 0 ), in.vOps.push_back( 0 );
    return in;
}
