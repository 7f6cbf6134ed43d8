// McIlroy's adversary ("A Killer Adversary for Quicksort", 1999) played against this libstdc++'s std::sort: std::sort runs over
// the indices 0..n-1 with a comparator that decides the key of an element only when it has to ("gas" until then, larger than
// every decided key), and always decides the element that is NOT the likely pivot.  The keys it ends up with, in index order,
// are a concrete input on which every partition of the same algorithm is as lopsided as the comparisons allowed -- introsort
// then runs out of its 2 lg n depth budget and heap-sorts what is left.  Test helper (sort_census.cpp, host_emul.cpp sortcheck).
#pragma once
#include <algorithm>
#include <vector>

// keys[i] / d for i in 0..n-1; with d == 1 the keys are a permutation of 0..n-1
inline std::vector<long> sort_adversary_keys( int n, int d )
{
    std::vector<long> val( n, -1 ); // -1: gas
    long nsolid = 0;
    int candidate = 0;
    std::vector<int> idx( n );
    for( int i = 0; i < n; i++ )
        idx[ i ] = i;
    auto cmp = [ & ]( int x, int y ) {
        if( val[ x ] < 0 && val[ y ] < 0 )
        {
            if( x == candidate )
                val[ x ] = nsolid++;
            else
                val[ y ] = nsolid++;
        }
        if( val[ x ] < 0 )
            candidate = x;
        else if( val[ y ] < 0 )
            candidate = y;
        if( val[ x ] < 0 ) // gas is larger than every solid key
            return false;
        if( val[ y ] < 0 )
            return true;
        return val[ x ] < val[ y ];
    };
    std::sort( idx.begin( ), idx.end( ), cmp );
    // what is still gas was never compared with other gas: any distinct keys above the solid ones agree with every answer given
    for( int i = 0; i < n; i++ )
        if( val[ i ] < 0 )
            val[ i ] = nsolid++;
    for( int i = 0; i < n; i++ )
        val[ i ] /= d;
    return val;
}
