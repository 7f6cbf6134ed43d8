// What the three CPU test programs of the flat record formatter (ma_amd/host/ma_sam_dev.h) share -- sam_dev_test.cpp (single
// reads), sam_pair_dev_test.cpp (mate pairs), sam_tags_dev_test.cpp (the NGMLR tags): the inputs, the views the formatter reads,
// the Alignment containers the yardstick reads (FileWriter / PairedFileWriter of ma_amd/host/ma_sam.h, the independent
// implementation), the count-then-write runner of the shared formatter, the text comparison, the parsers of the reference's
// dumps and the readers of the GPU tests' binary dumps.  Each program keeps its generators, its census and its modes.
#pragma once
#include "../../oracle/dump_format.h"
#include "ma_flat_sam.h"
#include "ma_sam.h"
#include "ma_sam_dev.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <random>
#include <sstream>

using namespace libMA;

struct ReadData
{
    std::string sName;
    std::vector<uint8_t> vCodes, vQual;
    bool bQual = false;
    // An empty read has no quality string, as in the host layer (NucSeq::xQuality empty -> no qualities): its QUAL is "*".
    const uint8_t* qual( ) const
    {
        return bQual && !vQual.empty( ) ? vQual.data( ) : nullptr;
    }
    ma_sam::Read view( ) const
    {
        return ma_sam::Read{ sName.data( ), sName.size( ), vCodes.data( ), qual( ), vCodes.size( ) };
    }
    ma_amd::flat::ReadView flatView( ) const
    {
        ma_amd::flat::ReadView v;
        v.sName = sName.data( ), v.uiNameLen = sName.size( );
        v.pCodes = vCodes.data( ), v.pQuality = qual( ), v.uiLength = vCodes.size( );
        return v;
    }
    std::shared_ptr<NucSeq> container( ) const
    {
        auto pQ = std::make_shared<NucSeq>( );
        pQ->sName = sName, pQ->xCodes = vCodes;
        if( bQual )
            pQ->xQuality = vQual;
        return pQ;
    }
};
// The records of a run: one list per unit (a read; for the pair program a pair of two reads).  Genome bases and holes are
// there where the tags need them.
struct Input
{
    std::vector<std::string> vNames;
    std::vector<uint64_t> vStarts, vLengths;
    std::vector<uint8_t> vGenome; // forward strand, one code per base (or empty)
    std::vector<uint64_t> vHoleStart, vHoleLen;
    std::vector<ReadData> vReads;
    std::vector<uint64_t> vOff; // units + 1
    std::vector<ma_alignment> vAlns;
    std::vector<uint64_t> vOps; // (type, length) pairs
    uint64_t forward( ) const
    {
        return vStarts.back( ) + vLengths.back( );
    }
    std::vector<uint8_t> pac( ) const // exactly the bytes of the forward strand
    {
        std::vector<uint8_t> v( ( vGenome.size( ) + 3 ) / 4, 0 );
        for( uint64_t p = 0; p < vGenome.size( ); p++ )
            v[ p >> 2 ] |= (uint8_t)( ( vGenome[ p ] & 3 ) << ( ( ~p & 3 ) << 1 ) );
        return v;
    }
    void addContig( const std::string& sName, uint64_t uiLength )
    {
        vStarts.push_back( vStarts.empty( ) ? 0 : forward( ) );
        vNames.push_back( sName ), vLengths.push_back( uiLength );
    }
    ma_sam::FlatList list( size_t uiUnit ) const
    {
        return ma_sam::FlatList{ vAlns.data( ) + vOff[ uiUnit ], (uint32_t)( vOff[ uiUnit + 1 ] - vOff[ uiUnit ] ), vOps.data( ) };
    }
    ma_amd::flat::ContigTable flatContigs( ) const // (the host writers': once per run, as they build it once per writer)
    {
        ma_amd::flat::ContigTable xC;
        xC.set( vNames, vStarts, vLengths );
        return xC;
    }
    // what the yardstick reads: the pack ...
    std::shared_ptr<Pack> pack( ) const
    {
        auto pPack = std::make_shared<Pack>( );
        pPack->vNames = vNames, pPack->vStarts = vStarts, pPack->vLengths = vLengths;
        pPack->vPacHost = pac( );
        for( size_t i = 0; i < vHoleStart.size( ); i++ )
            pPack->vHoles.emplace_back( vHoleStart[ i ], vHoleLen[ i ] );
        return pPack;
    }
    // ... and FRESH Alignment containers of a unit's list (FileWriter swaps their ops under the tag option)
    std::shared_ptr<libMS::ContainerVector<std::shared_ptr<Alignment>>> containers( size_t uiUnit ) const
    {
        auto pV = std::make_shared<libMS::ContainerVector<std::shared_ptr<Alignment>>>( );
        for( uint64_t k = vOff[ uiUnit ]; k < vOff[ uiUnit + 1 ]; k++ )
        {
            const ma_alignment& a = vAlns[ k ];
            auto pA = std::make_shared<Alignment>( );
            pA->uiBeginOnRef = (uint64_t)a.begin_ref, pA->uiEndOnRef = (uint64_t)a.end_ref;
            pA->uiBeginOnQuery = (uint64_t)a.begin_q, pA->uiEndOnQuery = (uint64_t)a.end_q;
            pA->iScore = a.score, pA->fMappingQuality = a.mapq, pA->bSecondary = a.secondary != 0, pA->bSupplementary = a.supplementary != 0;
            for( uint32_t j = 0; j < a.n_ops; j++ )
                pA->data.emplace_back( (MatchType)vOps[ 2 * ( a.ops_off + j ) ], vOps[ 2 * ( a.ops_off + j ) + 1 ] );
            pV->push_back( pA );
        }
        return pV;
    }
};
// the contig table as ma_sam_dev.h reads it
struct DevContigs
{
    std::vector<char> vNames;
    std::vector<uint64_t> vNameOff;
    ma_sam::Contigs xView;
    explicit DevContigs( const Input& r ) : vNameOff( 1, 0 )
    {
        for( auto& s : r.vNames )
        {
            vNames.insert( vNames.end( ), s.begin( ), s.end( ) );
            vNameOff.push_back( vNames.size( ) );
        }
        xView = ma_sam::Contigs{ vNames.data( ), vNameOff.data( ), r.vStarts.data( ), r.vLengths.data( ), (uint32_t)r.vStarts.size( ) };
    }
};

// options: the MA_SAM_* bits of include/ma_amd.h, for the yardstick and for the host's flat writers
static inline SamOptions optionsOf( uint32_t uiOptions )
{
    SamOptions o;
    o.bSoftClip = ( uiOptions & MA_SAM_SOFT_CLIP ) != 0;
    o.bOutputMCigar = ( uiOptions & MA_SAM_EQX_CIGAR ) == 0;
    o.bNoSecondary = ( uiOptions & MA_SAM_NO_SECONDARY ) != 0;
    o.bNoSupplementary = ( uiOptions & MA_SAM_NO_SUPPLEMENTARY ) != 0;
    o.bCGTag = ( uiOptions & MA_SAM_NO_CG_TAG ) == 0;
    o.bEmulateNgmlrTags = ( uiOptions & MA_SAM_NGMLR_TAGS ) != 0;
    return o;
}
static inline ma_amd::flat::SamFormat formatOf( uint32_t uiOptions )
{
    const SamOptions o = optionsOf( uiOptions );
    ma_amd::flat::SamFormat f;
    f.bSoftClip = o.bSoftClip, f.bOutputMCigar = o.bOutputMCigar, f.bNoSecondary = o.bNoSecondary, f.bNoSupplementary = o.bNoSupplementary;
    f.bCGTag = o.bCGTag;
    return f;
}

// A yardstick run: WRITER (FileWriter / PairedFileWriter) on a string stream; execute( writer, pack, unit ) prints one unit.
// Returns the text behind the header; pOff gets the units' offsets.  Throws what the writer throws.
template <class WRITER, class EXECUTE>
static std::string writerText( const Input& rIn, uint32_t uiOptions, size_t uiUnits, std::vector<uint64_t>* pOff, EXECUTE execute )
{
    auto pPack = rIn.pack( );
    ParameterSetManager xParams;
    xParams.xSam = optionsOf( uiOptions );
    auto pStream = std::make_shared<StringOutStream>( );
    WRITER xWriter( xParams, std::static_pointer_cast<OutStream>( pStream ), pPack );
    const size_t uiHeader = pStream->sText.size( );
    if( pOff )
        pOff->assign( 1, 0 );
    for( size_t u = 0; u < uiUnits; u++ )
    {
        execute( xWriter, pPack, u );
        if( pOff )
            pOff->push_back( pStream->sText.size( ) - uiHeader );
    }
    xWriter.flush( );
    return pStream->sText.substr( uiHeader );
}
// the yardstick of single reads: FileWriter::execute over all reads
static inline std::string fileWriterText( const Input& rIn, uint32_t uiOptions, std::vector<uint64_t>* pOff = nullptr )
{
    return writerText<FileWriter>( rIn, uiOptions, rIn.vReads.size( ), pOff, [ & ]( FileWriter& rWriter, std::shared_ptr<Pack> pPack, size_t r ) {
        rWriter.execute( rIn.vReads[ r ].container( ), rIn.containers( r ), pPack );
    } );
}
// the text of a formatter that throws: its exception's ("" when it does not throw)
template <class F> static std::string errorOf( F format )
{
    try
    {
        format( );
    }
    catch( const std::exception& e )
    {
        return e.what( );
    }
    return "";
}

struct DevResult
{
    std::string sText;
    uint32_t uiErrors = 0, uiKind = 0, uiRecord = 0; // the first error: its kind, the record in its unit ...
    size_t uiUnit = 0; // ... and the unit
    int64_t iValue = 0;
};
// the shared formatter over all units -- format( sink, unit ) -- with the counting sink, then with the writing sink into
// exactly that many bytes
template <class FORMAT> static DevResult countThenWrite( size_t uiUnits, FORMAT format )
{
    DevResult xRes;
    for( size_t u = 0; u < uiUnits; u++ )
    {
        ma_sam::CountSink xCount;
        format( xCount, u );
        if( xCount.nErrors && !xRes.uiErrors )
            xRes.uiKind = xCount.firstKind, xRes.iValue = xCount.firstValue, xRes.uiRecord = xCount.firstRecord, xRes.uiUnit = u;
        xRes.uiErrors += xCount.nErrors;
        std::unique_ptr<char[]> pBuf( new char[ xCount.n ] ); // (exactly: the sanitizer build sees a byte too many)
        ma_sam::WriteSink xWrite{ pBuf.get( ) };
        format( xWrite, u );
        if( xWrite.n != xCount.n )
            throw std::runtime_error( "unit " + std::to_string( u ) + ": the counting sink says " + std::to_string( xCount.n ) + " bytes, " +
                                      std::to_string( xWrite.n ) + " were written" );
        xRes.sText.append( pBuf.get( ), xWrite.n );
    }
    return xRes;
}

static inline void compare( const std::string& sGot, const std::string& sWant, const std::string& sWhat )
{
    if( sGot == sWant )
        return;
    size_t i = 0;
    while( i < sGot.size( ) && i < sWant.size( ) && sGot[ i ] == sWant[ i ] )
        i++;
    const size_t b = sWant.rfind( '\n', i ) == std::string::npos ? 0 : sWant.rfind( '\n', i ) + 1;
    throw std::runtime_error( sWhat + ": texts differ at byte " + std::to_string( i ) + "\n want: " + sWant.substr( b, 400 ) + "\n got:  " +
                              sGot.substr( b < sGot.size( ) ? b : 0, 400 ) );
}

// ---- the reference's dumps -------------------------------------------------------------------------------------------------
// contigs, genome and reads ("r<i>", no qualities) of a case file
static inline Input fromCase( const char* sCase )
{
    CaseFile c = readCase( sCase );
    Input in;
    for( size_t i = 0; i < c.contigs.size( ); i++ )
    {
        in.addContig( c.names[ i ], c.contigs[ i ].size( ) );
        in.vGenome.insert( in.vGenome.end( ), c.contigs[ i ].begin( ), c.contigs[ i ].end( ) );
    }
    for( size_t r = 0; r < c.reads.size( ); r++ )
    {
        ReadData q;
        q.sName = "r" + std::to_string( r );
        q.vCodes = c.reads[ r ];
        in.vReads.push_back( q );
    }
    return in;
}
// the ops of a dump line, "<type>:<length>" each, appended to the pool
static inline void readOps( std::istream& is, size_t n, std::vector<uint64_t>& rOps )
{
    for( size_t k = 0; k < n; k++ )
    {
        std::string t;
        is >> t;
        const size_t colon = t.find( ':' );
        rOps.push_back( (uint64_t)atoi( t.substr( 0, colon ).c_str( ) ) );
        rOps.push_back( strtoull( t.c_str( ) + colon + 1, nullptr, 10 ) );
    }
}
// the MappingQuality records ("m" lines, their ops those of the NW alignment -- "a" line -- they are) of a pipeline dump
static inline Input fromPipeDump( const char* sCase, const char* sPipe )
{
    Input in = fromCase( sCase );
    struct Rec
    {
        unsigned long long br, er, bq, eq;
        long long score;
        std::vector<uint64_t> ops;
    };
    std::vector<Rec> alns;
    std::vector<std::vector<ma_alignment>> vPerRead( in.vReads.size( ) );
    std::vector<std::vector<std::vector<uint64_t>>> vPerReadOps( in.vReads.size( ) );
    std::ifstream f( sPipe );
    std::string line;
    long read = -1;
    while( std::getline( f, line ) )
    {
        std::istringstream is( line );
        std::string tag;
        is >> tag;
        if( tag == "R" )
        {
            is >> read;
            alns.clear( );
        }
        else if( tag == "a" )
        {
            Rec r;
            unsigned soc;
            size_t n;
            is >> r.br >> r.er >> r.bq >> r.eq >> r.score >> soc >> n;
            readOps( is, n, r.ops );
            alns.push_back( r );
        }
        else if( tag == "m" )
        {
            unsigned long long br, er, bq, eq;
            long long score;
            int sec, sup;
            std::string sQ;
            is >> br >> er >> bq >> eq >> score >> sec >> sup >> sQ;
            ma_alignment a{ };
            a.begin_ref = (int64_t)br, a.end_ref = (int64_t)er, a.begin_q = (int64_t)bq, a.end_q = (int64_t)eq, a.score = score;
            a.secondary = sec != 0, a.supplementary = sup != 0, a.mapq = strtod( sQ.c_str( ), nullptr );
            std::vector<uint64_t> ops;
            for( auto& r : alns ) // the MQ record is one of the NW alignments
                if( r.br == br && r.er == er && r.bq == bq && r.eq == eq && r.score == score )
                {
                    ops = r.ops;
                    break;
                }
            a.n_ops = (uint32_t)( ops.size( ) / 2 );
            vPerRead[ (size_t)read ].push_back( a );
            vPerReadOps[ (size_t)read ].push_back( ops );
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
// the record lines of a SAM golden
static inline std::string goldenRecords( const char* sPath )
{
    std::ifstream f( sPath );
    std::string line, sGolden;
    while( std::getline( f, line ) )
        if( line.empty( ) || line[ 0 ] != '@' )
            sGolden += line + "\n";
    return sGolden;
}

// ---- seeded numbers --------------------------------------------------------------------------------------------------------
typedef std::mt19937_64 Rng;
static inline uint64_t below( Rng& g, uint64_t n ) // [0, n)
{
    return n ? g( ) % n : 0;
}
// a number next to a decimal boundary (9/10, 99/100, ... 10^9), or any
static inline uint64_t nearBoundary( Rng& g, uint64_t uiMax )
{
    if( below( g, 4 ) == 0 )
        return below( g, uiMax + 1 );
    uint64_t p = 10;
    for( uint64_t e = below( g, 9 ); e > 0; e-- )
        p *= 10;
    const uint64_t v = p - 2 + below( g, 4 ); // p-2 .. p+1
    return v > uiMax ? uiMax : v;
}

// ---- the GPU tests' binary dumps -------------------------------------------------------------------------------------------
struct DumpFile
{
    FILE* f;
    explicit DumpFile( const char* sPath ) : f( fopen( sPath, "rb" ) )
    {
        if( !f )
            throw std::runtime_error( std::string( "cannot open " ) + sPath );
    }
    ~DumpFile( )
    {
        fclose( f );
    }
    void rd( void* p, size_t n )
    {
        if( n && fread( p, 1, n, f ) != n )
            throw std::runtime_error( "dump too short" );
    }
    uint32_t u32( )
    {
        uint32_t v;
        rd( &v, 4 );
        return v;
    }
    uint64_t u64( )
    {
        uint64_t v;
        rd( &v, 8 );
        return v;
    }
};
// magic, contigs (bGenome: genome bases and holes), reads, the offsets of the units of uiReadsPerUnit reads each, records, ops;
// what a format has behind the ops is the caller's to read
static inline void readDump( DumpFile& f, Input& in, const char* sMagic, bool bGenome, uint32_t uiReadsPerUnit )
{
    char magic[ 8 ];
    f.rd( magic, 8 );
    if( memcmp( magic, sMagic, 8 ) )
        throw std::runtime_error( "bad dump magic" );
    for( uint32_t i = 0, n = f.u32( ); i < n; i++ )
    {
        std::string s( f.u32( ), ' ' );
        f.rd( &s[ 0 ], s.size( ) );
        in.vNames.push_back( s );
        in.vStarts.push_back( f.u64( ) );
        in.vLengths.push_back( f.u64( ) );
    }
    if( bGenome )
    {
        in.vGenome.resize( f.u64( ) );
        f.rd( in.vGenome.data( ), in.vGenome.size( ) );
        for( uint64_t i = 0, n = f.u64( ); i < n; i++ )
        {
            in.vHoleStart.push_back( f.u64( ) );
            in.vHoleLen.push_back( f.u64( ) );
        }
    }
    const uint32_t nR = f.u32( ), bQual = f.u32( );
    if( nR % uiReadsPerUnit )
        throw std::runtime_error( "odd number of reads" );
    for( uint32_t r = 0; r < nR; r++ )
    {
        ReadData q;
        q.sName.assign( f.u32( ), ' ' );
        f.rd( &q.sName[ 0 ], q.sName.size( ) );
        q.vCodes.resize( f.u32( ) );
        f.rd( q.vCodes.data( ), q.vCodes.size( ) );
        q.bQual = bQual != 0;
        if( q.bQual )
        {
            q.vQual.resize( q.vCodes.size( ) );
            f.rd( q.vQual.data( ), q.vQual.size( ) );
        }
        in.vReads.push_back( q );
    }
    const size_t uiUnits = nR / uiReadsPerUnit;
    in.vOff.resize( uiUnits + 1 );
    f.rd( in.vOff.data( ), ( uiUnits + 1 ) * 8 );
    in.vAlns.resize( in.vOff[ uiUnits ] );
    f.rd( in.vAlns.data( ), in.vAlns.size( ) * sizeof( ma_alignment ) );
    in.vOps.resize( 2 * f.u64( ) + 2 );
    f.rd( in.vOps.data( ), ( in.vOps.size( ) - 2 ) * 8 );
}
// mode `dump`: the yardstick's text -- text( &offsets ) -- to <out>, the per-unit offsets (u64) to <out>.off; an exception is
// printed as "ERROR: <text>" (exit code 3)
template <class TEXT> static int writeYardstick( const char* sOut, TEXT text )
{
    std::vector<uint64_t> vOff;
    std::string sText;
    try
    {
        sText = text( &vOff );
    }
    catch( const std::exception& e )
    {
        printf( "ERROR: %s\n", e.what( ) );
        return 3;
    }
    auto write = []( const std::string& sPath, const void* p, size_t n ) {
        FILE* o = fopen( sPath.c_str( ), "wb" );
        if( !o || fwrite( p, 1, n, o ) != n || fclose( o ) != 0 )
            throw std::runtime_error( "cannot write " + sPath );
    };
    write( sOut, sText.data( ), sText.size( ) );
    write( std::string( sOut ) + ".off", vOff.data( ), 8 * vOff.size( ) );
    return 0;
}
