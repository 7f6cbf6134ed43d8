// TEST INFRASTRUCTURE ONLY -- binary case-file readers shared by ref_dump (real reference) and
// oracle_dump (our CPU restatement).  Writers live in tests/ma_testlib.py.
//
// MACASE01: magic[8] | u32 n_contigs | { u32 name_len, name, u64 len, codes[len] (0..3, >=4 = N) }*
//           | u32 n_reads | { u32 len, codes[len] (0..4) }*
// KSWCAS01: magic[8] | u32 n | { i32 qlen, i32 tlen, i32 w, i32 zdrop, i32 flag, q[qlen], t[tlen] }*
// NWSETS01: magic[8] | u64 n_reads | u64 n_sets | u64 n_seeds | u64 hset_off[n_reads + 1] | u64 hseed_off[n_sets + 1]
//           | u32 hset_soc[n_sets] | { i64 q_start, i64 len, i64 r_start, i64 delta, u32 ambiguity, u32 on_forward }[n_seeds]
//           harmonized seed sets for the reads of a MACASE01 file, in the layout of ma_batch_get_hsets / ma_batch_set_hsets: the
//           sets of read r are hset_off[r] .. hset_off[r + 1], the seeds of set s are hseed_off[s] .. hseed_off[s + 1] (records
//           in ma_seed layout, positions on the doubled text), hset_soc[s] is its index_of_strip (writer: tests/nw_sets.py)
// CHSEED01: magic[8] | u64 n_reads | u64 n_seeds | u64 seed_off[n_reads + 1] | { seed record as in NWSETS01 }[n_seeds]
//           seeds for the reads of a MACASE01 file as ExtractSeeds leaves them (reverse-strand seeds mirrored onto forward
//           positions), in the order the chain stage's first sort is to see them (writer: tests/harm_sets.py)
// EXSEGS01: magic[8] | u64 n_reads | u64 n_segs | u64 seg_off[n_reads + 1]
//           | { i64 q_start, i64 q_size, i64 sa_start, i64 sa_start_rc, i64 sa_size }[n_segs]
//           segments for the reads of a MACASE01 file, in the layout of ma_batch_get_segments / ma_batch_set_segments: the segments
//           of read r are seg_off[r] .. seg_off[r + 1] (records in ma_segment layout; writer: tests/extract_lists.py)
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

struct CaseFile
{
    std::vector<std::string> names;
    std::vector<std::vector<uint8_t>> contigs;
    std::vector<std::vector<uint8_t>> reads;
};

struct KswCase
{
    int w, zdrop, flag;
    std::vector<uint8_t> q, t;
};

struct NwSetsSeed
{
    int64_t q_start, len, r_start, delta;
    uint32_t ambiguity, on_forward;
};
struct NwSetsFile
{
    std::vector<uint64_t> hsetOff, hseedOff;
    std::vector<uint32_t> hsetSoc;
    std::vector<NwSetsSeed> seeds;
};

namespace dumpfmt
{
inline void rd( FILE* f, void* p, size_t n )
{
    if( n && fread( p, 1, n, f ) != n )
        throw std::runtime_error( "short read in case file" );
}
template <typename T> inline T rdv( FILE* f )
{
    T x;
    rd( f, &x, sizeof( T ) );
    return x;
}
} // namespace dumpfmt

inline CaseFile readCase( const char* sPath )
{
    FILE* f = fopen( sPath, "rb" );
    if( !f )
        throw std::runtime_error( std::string( "cannot open " ) + sPath );
    char magic[ 8 ];
    dumpfmt::rd( f, magic, 8 );
    if( memcmp( magic, "MACASE01", 8 ) )
        throw std::runtime_error( "bad case magic" );
    CaseFile c;
    uint32_t nC = dumpfmt::rdv<uint32_t>( f );
    for( uint32_t i = 0; i < nC; i++ )
    {
        uint32_t nl = dumpfmt::rdv<uint32_t>( f );
        std::string s( nl, ' ' );
        dumpfmt::rd( f, &s[ 0 ], nl );
        uint64_t len = dumpfmt::rdv<uint64_t>( f );
        std::vector<uint8_t> v( len );
        dumpfmt::rd( f, v.data( ), len );
        c.names.push_back( s );
        c.contigs.push_back( std::move( v ) );
    }
    uint32_t nR = dumpfmt::rdv<uint32_t>( f );
    for( uint32_t i = 0; i < nR; i++ )
    {
        uint32_t len = dumpfmt::rdv<uint32_t>( f );
        std::vector<uint8_t> v( len );
        dumpfmt::rd( f, v.data( ), len );
        c.reads.push_back( std::move( v ) );
    }
    fclose( f );
    return c;
}

inline NwSetsFile readNwSets( const char* sPath )
{
    FILE* f = fopen( sPath, "rb" );
    if( !f )
        throw std::runtime_error( std::string( "cannot open " ) + sPath );
    char magic[ 8 ];
    dumpfmt::rd( f, magic, 8 );
    if( memcmp( magic, "NWSETS01", 8 ) )
        throw std::runtime_error( "bad sets magic" );
    const uint64_t nReads = dumpfmt::rdv<uint64_t>( f ), nSets = dumpfmt::rdv<uint64_t>( f ), nSeeds = dumpfmt::rdv<uint64_t>( f );
    NwSetsFile s;
    s.hsetOff.resize( nReads + 1 );
    s.hseedOff.resize( nSets + 1 );
    s.hsetSoc.resize( nSets );
    s.seeds.resize( nSeeds );
    dumpfmt::rd( f, s.hsetOff.data( ), 8 * ( nReads + 1 ) );
    dumpfmt::rd( f, s.hseedOff.data( ), 8 * ( nSets + 1 ) );
    dumpfmt::rd( f, s.hsetSoc.data( ), 4 * nSets );
    dumpfmt::rd( f, s.seeds.data( ), sizeof( NwSetsSeed ) * nSeeds );
    fclose( f );
    if( s.hsetOff[ 0 ] != 0 || s.hsetOff[ nReads ] != nSets || s.hseedOff[ 0 ] != 0 || s.hseedOff[ nSets ] != nSeeds )
        throw std::runtime_error( "sets file: offsets and counts disagree" );
    for( uint64_t i = 0; i < nReads; i++ )
        if( s.hsetOff[ i + 1 ] < s.hsetOff[ i ] )
            throw std::runtime_error( "sets file: hset_off decreases" );
    for( uint64_t i = 0; i < nSets; i++ )
        if( s.hseedOff[ i + 1 ] < s.hseedOff[ i ] )
            throw std::runtime_error( "sets file: hseed_off decreases" );
    return s;
}

// CHSEED01: seeds for the reads of a MACASE01 file, in the layout of ma_batch_get_seeds / ma_batch_set_seeds (records as NWSETS01's)
struct ChainSeedsFile
{
    std::vector<uint64_t> seedOff;
    std::vector<NwSetsSeed> seeds;
};

inline ChainSeedsFile readChainSeeds( const char* sPath )
{
    FILE* f = fopen( sPath, "rb" );
    if( !f )
        throw std::runtime_error( std::string( "cannot open " ) + sPath );
    char magic[ 8 ];
    dumpfmt::rd( f, magic, 8 );
    if( memcmp( magic, "CHSEED01", 8 ) )
        throw std::runtime_error( "bad seeds magic" );
    const uint64_t nReads = dumpfmt::rdv<uint64_t>( f ), nSeeds = dumpfmt::rdv<uint64_t>( f );
    ChainSeedsFile s;
    s.seedOff.resize( nReads + 1 );
    s.seeds.resize( nSeeds );
    dumpfmt::rd( f, s.seedOff.data( ), 8 * ( nReads + 1 ) );
    dumpfmt::rd( f, s.seeds.data( ), sizeof( NwSetsSeed ) * nSeeds );
    fclose( f );
    if( s.seedOff[ 0 ] != 0 || s.seedOff[ nReads ] != nSeeds )
        throw std::runtime_error( "seeds file: offsets and counts disagree" );
    for( uint64_t i = 0; i < nReads; i++ )
        if( s.seedOff[ i + 1 ] < s.seedOff[ i ] )
            throw std::runtime_error( "seeds file: seed_off decreases" );
    return s;
}

struct SegsRecord
{
    int64_t q_start, q_size, sa_start, sa_start_rc, sa_size;
};
struct SegsFile
{
    std::vector<uint64_t> segOff;
    std::vector<SegsRecord> segs;
};

inline SegsFile readSegs( const char* sPath )
{
    FILE* f = fopen( sPath, "rb" );
    if( !f )
        throw std::runtime_error( std::string( "cannot open " ) + sPath );
    char magic[ 8 ];
    dumpfmt::rd( f, magic, 8 );
    if( memcmp( magic, "EXSEGS01", 8 ) )
        throw std::runtime_error( "bad segments magic" );
    const uint64_t nReads = dumpfmt::rdv<uint64_t>( f ), nSegs = dumpfmt::rdv<uint64_t>( f );
    SegsFile s;
    s.segOff.resize( nReads + 1 );
    s.segs.resize( nSegs );
    dumpfmt::rd( f, s.segOff.data( ), 8 * ( nReads + 1 ) );
    dumpfmt::rd( f, s.segs.data( ), sizeof( SegsRecord ) * nSegs );
    fclose( f );
    if( s.segOff[ 0 ] != 0 || s.segOff[ nReads ] != nSegs )
        throw std::runtime_error( "segments file: offsets and counts disagree" );
    for( uint64_t i = 0; i < nReads; i++ )
        if( s.segOff[ i + 1 ] < s.segOff[ i ] )
            throw std::runtime_error( "segments file: seg_off decreases" );
    return s;
}

inline std::vector<KswCase> readKswCases( const char* sPath )
{
    FILE* f = fopen( sPath, "rb" );
    if( !f )
        throw std::runtime_error( std::string( "cannot open " ) + sPath );
    char magic[ 8 ];
    dumpfmt::rd( f, magic, 8 );
    if( memcmp( magic, "KSWCAS01", 8 ) )
        throw std::runtime_error( "bad ksw case magic" );
    uint32_t n = dumpfmt::rdv<uint32_t>( f );
    std::vector<KswCase> v( n );
    for( auto& k : v )
    {
        int32_t ql = dumpfmt::rdv<int32_t>( f ), tl = dumpfmt::rdv<int32_t>( f );
        k.w = dumpfmt::rdv<int32_t>( f );
        k.zdrop = dumpfmt::rdv<int32_t>( f );
        k.flag = dumpfmt::rdv<int32_t>( f );
        k.q.resize( ql );
        k.t.resize( tl );
        dumpfmt::rd( f, k.q.data( ), ql );
        dumpfmt::rd( f, k.t.data( ), tl );
    }
    fclose( f );
    return v;
}
