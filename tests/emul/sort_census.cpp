// Test helper for the chain stage's three restatements of libstdc++'s std::sort (ma_amd/csrc/stdsort.h ss::sort, and the
// wave form of wave_sort.h in its LDS and global-memory variants): which lists make introsort fall back to heap sort, and do
// the restatements leave std::sort's permutation on them.
//   sort_census adversary <d> <n>...   one line "n k0 k1 ..." per n: McIlroy's adversary (sort_adversary.h), keys / d
//   sort_census census <file>          file: one list per line, "name n k0 k1 ..."; prints per list
//        name n events=<len>:<ties>,... perms=<0|1> unstable=<0|1>
//     events   every heap-sort event of the plain introsort loop (threshold 16) run with the product's own ss:: primitives:
//              length of the range and whether it holds two equal keys
//     perms    std::sort, ss::sort and the wave skeleton on the host -- the introsort loop at WS_SERIAL with ss::unguarded_partition,
//              the heap sort at depth 0 (lane 0's in the kernel), ss::finish_range on every range it leaves -- give one permutation
//              of (key << WS_KEY_SHIFT | index) under the order of PackedKeyLess
//     unstable std::sort's permutation differs from std::stable_sort's
// WS_SERIAL and WS_KEY_SHIFT come from the product's headers on the compiler's command line (tests/chain_lists.py reads them).
#include "../../ma_amd/csrc/stdsort.h"
#include "sort_adversary.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#if !defined( WS_SERIAL ) || !defined( WS_KEY_SHIFT )
#error "compile with -DWS_SERIAL=<wave_sort.h> -DWS_KEY_SHIFT=<PackedKeyLess, stage_chain.h>"
#endif

using namespace ma;

struct PackedLess
{
    bool operator( )( u64 a, u64 b ) const
    {
        return ( a >> WS_KEY_SHIFT ) < ( b >> WS_KEY_SHIFT );
    }
};

static i64 depth_budget( i64 n ) // 2 * __lg( n )
{
    i64 d = 0;
    for( u64 m = (u64)n; m >>= 1; )
        d += 2;
    return d;
}

struct Event
{
    i64 len;
    bool ties;
};

// __introsort_loop as in ss::sort, with the heap-sort events written down
static void census( std::vector<u64> a, std::vector<Event>& ev )
{
    const i64 n = (i64)a.size( );
    PackedLess less;
    std::vector<i64> stF, stL, stD;
    i64 first = 0, last = n, depth = depth_budget( n );
    while( true )
    {
        while( last - first > 16 )
        {
            if( depth == 0 )
            {
                std::vector<u64> keys;
                for( i64 i = first; i < last; i++ )
                    keys.push_back( a[ i ] >> WS_KEY_SHIFT );
                std::sort( keys.begin( ), keys.end( ) );
                ev.push_back( Event{ last - first, std::adjacent_find( keys.begin( ), keys.end( ) ) != keys.end( ) } );
                ss::heap_sort_range( a.data( ), first, last, less );
                break;
            }
            --depth;
            const i64 mid = first + ( last - first ) / 2;
            ss::move_median_to_first( a.data( ), first, first + 1, mid, last - 1, less );
            const i64 cut = ss::unguarded_partition( a.data( ), first + 1, last, first, less );
            stF.push_back( cut ), stL.push_back( last ), stD.push_back( depth );
            last = cut;
        }
        if( stF.empty( ) )
            break;
        first = stF.back( ), last = stL.back( ), depth = stD.back( );
        stF.pop_back( ), stL.pop_back( ), stD.pop_back( );
    }
}

// ws::wave_std_sort without the wavefront: the same ranges reach the same code with the same depth budget
static void wave_skeleton( std::vector<u64>& a )
{
    const i64 n = (i64)a.size( );
    if( n <= 1 )
        return;
    PackedLess less;
    struct Item
    {
        i64 first, last, depth;
    };
    std::vector<Item> items, stack;
    i64 first = 0, last = n, depth = depth_budget( n );
    while( true )
    {
        while( last - first > WS_SERIAL )
        {
            if( depth == 0 )
            {
                ss::heap_sort_range( a.data( ), first, last, less );
                first = last;
                break;
            }
            --depth;
            const i64 mid = first + ( last - first ) / 2;
            ss::move_median_to_first( a.data( ), first, first + 1, mid, last - 1, less );
            const i64 cut = ss::unguarded_partition( a.data( ), first + 1, last, first, less );
            stack.push_back( Item{ cut, last, depth } );
            last = cut;
        }
        if( last - first > 1 )
            items.push_back( Item{ first, last, depth } );
        if( stack.empty( ) )
            break;
        first = stack.back( ).first, last = stack.back( ).last, depth = stack.back( ).depth;
        stack.pop_back( );
    }
    for( const Item& it : items )
        ss::finish_range( a.data( ), it.first, it.last, it.depth, less );
}

int main( int argc, char** argv )
{
    if( argc >= 4 && !strcmp( argv[ 1 ], "adversary" ) )
    {
        const int d = atoi( argv[ 2 ] );
        for( int k = 3; k < argc; k++ )
        {
            const int n = atoi( argv[ k ] );
            if( d < 1 || n < 1 )
                return 2;
            printf( "%d", n );
            for( long v : sort_adversary_keys( n, d ) )
                printf( " %ld", v );
            printf( "\n" );
        }
        return 0;
    }
    if( argc == 3 && !strcmp( argv[ 1 ], "census" ) )
    {
        std::ifstream in( argv[ 2 ] );
        std::string line;
        while( std::getline( in, line ) )
        {
            std::istringstream ls( line );
            std::string name;
            long n;
            if( !( ls >> name >> n ) )
                continue;
            std::vector<u64> a( n );
            for( long i = 0; i < n; i++ )
            {
                unsigned long long k;
                if( !( ls >> k ) || ( k >> ( 64 - WS_KEY_SHIFT ) ) != 0 || (u64)n >> WS_KEY_SHIFT )
                {
                    fprintf( stderr, "%s: bad list\n", name.c_str( ) );
                    return 2;
                }
                a[ i ] = ( (u64)k << WS_KEY_SHIFT ) | (u64)i;
            }
            std::vector<Event> ev;
            census( a, ev );
            std::vector<u64> s1 = a, s2 = a, s3 = a, s4 = a;
            std::sort( s1.begin( ), s1.end( ), PackedLess( ) );
            ss::sort( s2.data( ), (i64)n, PackedLess( ) );
            wave_skeleton( s3 );
            std::stable_sort( s4.begin( ), s4.end( ), PackedLess( ) );
            printf( "%s %ld events=", name.c_str( ), n );
            for( size_t i = 0; i < ev.size( ); i++ )
                printf( "%s%lld:%d", i ? "," : "", (long long)ev[ i ].len, (int)ev[ i ].ties );
            printf( " perms=%d unstable=%d\n", (int)( s1 == s2 && s1 == s3 ), (int)( s1 != s4 ) );
        }
        return 0;
    }
    fprintf( stderr, "usage: sort_census adversary <d> <n>... | census <file>\n" );
    return 2;
}
