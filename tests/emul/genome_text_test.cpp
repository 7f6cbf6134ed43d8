// CPU-only checks of the rules the device's genome reader runs (ma_amd/host/ma_genome_dev.h: ma_genome_dev::parseHost over the
// functions the kernels and the library call) against the files the reference wrote and against the tree's yardstick,
// FileReader of ma_amd/host/ma_sam.h + packContigs (the base loop of buildIndex, ma_amd/host/ma_modules.h) after srand( seed ).
//   genome_text_test golden <dir>          the committed fixtures: contigs and holes per contig == .ann, holes == .amb, the 2-bit
//                                          bases outside the holes == .pac; and == the yardstick on the same file
//   genome_text_test random <seed> <n>     seeded strict genomes: all accepted, codes after the fill, contig table, vHoles and
//                                          vNumHoles == the yardstick
//   genome_text_test cuts <dir>            every fixture cut behind every line end (two chunks), one line per chunk, and with a
//                                          tail that has no line feed: == the one-piece result
//   genome_text_test refusals              one text per reason, the '@' text, capacity, violations in a second chunk, the state
//                                          after a refusal
//   genome_text_test gen <seed> <n> <dir>  writes the random genomes of `random` as files (the GPU tests read them)
//   genome_text_test dump <seed> <file>... (the yardstick of tests/test_gpu_genome_text.py) parseHost's result per file
// The texts hold exactly their bytes on the heap, so that an AddressSanitizer build sees any byte touched outside of them.
#include "ma_genome_dev.h"
#include "ma_sam.h"
#include <fstream>
#include <random>
#include <unistd.h>

using namespace libMA;
using ma_genome_dev::Genome;

#define CHECK( cond, ... )                                                                                                                           \
    do                                                                                                                                               \
    {                                                                                                                                                \
        if( !( cond ) )                                                                                                                              \
        {                                                                                                                                            \
            printf( "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond );                                                                                 \
            printf( __VA_ARGS__ );                                                                                                                   \
            printf( "\n" );                                                                                                                          \
            exit( 1 );                                                                                                                               \
        }                                                                                                                                            \
    } while( 0 )

static const uint64_t NO_LIMIT = ~(uint64_t)0;

static std::string readFile( const std::string& sPath )
{
    std::ifstream f( sPath, std::ios::binary );
    CHECK( f.good( ), "%s", sPath.c_str( ) );
    return std::string( ( std::istreambuf_iterator<char>( f ) ), std::istreambuf_iterator<char>( ) );
}
// parseHost on exactly the chunk's bytes
static int append( Genome& g, const std::string& sChunk, bool bEnd, uint64_t* pConsumed, std::string* pMessage, uint64_t uiMax = NO_LIMIT )
{
    std::unique_ptr<char[]> pText( new char[ std::max<size_t>( sChunk.size( ), 1 ) ] );
    memcpy( pText.get( ), sChunk.data( ), sChunk.size( ) );
    return ma_genome_dev::parseHost( g, pText.get( ), sChunk.size( ), bEnd, uiMax, pConsumed, pMessage );
}
static Genome whole( const std::string& sText )
{
    Genome g;
    uint64_t uiConsumed;
    std::string sMessage;
    CHECK( append( g, sText, true, &uiConsumed, &sMessage ) == 0, "%s", sMessage.c_str( ) );
    CHECK( uiConsumed == sText.size( ), "consumed %llu of %zu", (unsigned long long)uiConsumed, sText.size( ) );
    return g;
}
static bool same( const Genome& a, const Genome& b )
{
    return a.vNameOff == b.vNameOff && a.sNames == b.sNames && a.vStarts == b.vStarts && a.vLens == b.vLens && a.vNumHoles == b.vNumHoles &&
           a.vHoleStart == b.vHoleStart && a.vHoleLen == b.vHoleLen && a.uiBases == b.uiBases && a.uiHoleBases == b.uiHoleBases &&
           a.uiLines == b.uiLines && a.uiBytes == b.uiBytes && a.bOpen == b.bOpen && a.vCodes == b.vCodes;
}
static std::string nameOf( const Genome& g, size_t i )
{
    return g.sNames.substr( g.vNameOff[ i ], g.vNameOff[ i + 1 ] - g.vNameOff[ i ] );
}

// the yardstick: FileReader on the file, packContigs after srand( seed ); compares with g after fillHost( seed )
static void checkYardstick( const std::string& sPath, Genome g, uint32_t uiSeed )
{
    ParameterSetManager xParameters;
    FileReader xReader( xParameters );
    auto pStream = fileStreamFromPath( sPath );
    std::vector<std::shared_ptr<NucSeq>> vContigs;
    while( auto pContig = xReader.execute( pStream ) )
        vContigs.push_back( pContig );
    auto pPack = std::make_shared<Pack>( );
    std::vector<uint64_t> vLens;
    std::vector<uint8_t> vCat;
    srand( uiSeed );
    packContigs( vContigs, pPack, vLens, vCat );
    ma_genome_dev::fillHost( g, uiSeed );
    CHECK( g.vStarts.size( ) == pPack->vNames.size( ), "%s: %zu contigs, yardstick %zu", sPath.c_str( ), g.vStarts.size( ), pPack->vNames.size( ) );
    for( size_t i = 0; i < g.vStarts.size( ); i++ )
        CHECK( nameOf( g, i ) == pPack->vNames[ i ] && g.vStarts[ i ] == pPack->vStarts[ i ] && g.vLens[ i ] == pPack->vLengths[ i ] &&
                   g.vNumHoles[ i ] == pPack->vNumHoles[ i ],
               "%s: contig %zu", sPath.c_str( ), i );
    CHECK( g.vHoleStart.size( ) == pPack->vHoles.size( ), "%s: %zu holes, yardstick %zu", sPath.c_str( ), g.vHoleStart.size( ), pPack->vHoles.size( ) );
    for( size_t i = 0; i < g.vHoleStart.size( ); i++ )
        CHECK( g.vHoleStart[ i ] == pPack->vHoles[ i ].first && g.vHoleLen[ i ] == pPack->vHoles[ i ].second, "%s: hole %zu", sPath.c_str( ), i );
    CHECK( g.vCodes == vCat, "%s: the codes after the fill differ", sPath.c_str( ) );
}

static const char* const FIXTURES[] = { "mixed", "crlf", "plain" };

static int cmdGolden( const std::string& sDir )
{
    for( const char* pName : FIXTURES )
    {
        const std::string sPrefix = sDir + "/" + pName;
        const Genome g = whole( readFile( sPrefix + ".fa" ) );
        // .ann: "<bases> <contigs> <seed>", then per contig "<gi> <name> <comment...>" and "<start> <length> <holes>"
        std::ifstream xAnn( sPrefix + ".ann" );
        uint64_t uiBases, uiContigs, uiSeed;
        xAnn >> uiBases >> uiContigs >> uiSeed;
        CHECK( uiBases == g.uiBases && uiContigs == g.vStarts.size( ), "%s.ann: %llu bases, %llu contigs", pName, (unsigned long long)uiBases,
               (unsigned long long)uiContigs );
        for( size_t i = 0; i < uiContigs; i++ )
        {
            std::string sGi, sName, sRest;
            uint64_t uiStart, uiLen, uiHoles;
            xAnn >> sGi >> sName;
            std::getline( xAnn, sRest );
            xAnn >> uiStart >> uiLen >> uiHoles;
            CHECK( sName == nameOf( g, i ) && uiStart == g.vStarts[ i ] && uiLen == g.vLens[ i ] && uiHoles == g.vNumHoles[ i ],
                   "%s.ann: contig %zu: %s %llu %llu %llu", pName, i, sName.c_str( ), (unsigned long long)uiStart, (unsigned long long)uiLen,
                   (unsigned long long)uiHoles );
        }
        // .amb: "<bases> <contigs> <holes>", then per hole "<start> <length> N"
        std::ifstream xAmb( sPrefix + ".amb" );
        uint64_t uiHoles;
        xAmb >> uiBases >> uiContigs >> uiHoles;
        CHECK( uiHoles == g.vHoleStart.size( ), "%s.amb: %llu holes, parseHost %zu", pName, (unsigned long long)uiHoles, g.vHoleStart.size( ) );
        std::vector<bool> vInHole( g.uiBases, false );
        for( size_t i = 0; i < uiHoles; i++ )
        {
            uint64_t uiStart, uiLen;
            std::string sN;
            xAmb >> uiStart >> uiLen >> sN;
            CHECK( uiStart == g.vHoleStart[ i ] && uiLen == g.vHoleLen[ i ], "%s.amb: hole %zu: %llu + %llu", pName, i, (unsigned long long)uiStart,
                   (unsigned long long)uiLen );
            for( uint64_t k = 0; k < uiLen; k++ )
                vInHole[ uiStart + k ] = true;
        }
        // .pac: four bases per byte, the first in the top bits; then a zero byte if the length is a multiple of 4, and length % 4
        const std::string sPac = readFile( sPrefix + ".pac" );
        CHECK( sPac.size( ) == ( g.uiBases + 3 ) / 4 + ( g.uiBases % 4 ? 1 : 2 ), "%s.pac: %zu bytes", pName, sPac.size( ) );
        uint64_t uiHoleBases = 0;
        for( uint64_t i = 0; i < g.uiBases; i++ )
        {
            const uint8_t uiRef = ( (uint8_t)sPac[ i >> 2 ] >> ( ( 3 - ( i & 3 ) ) << 1 ) ) & 3u;
            CHECK( vInHole[ i ] == ma_genome_dev::isHole( g.vCodes[ i ] ), "%s: base %llu", pName, (unsigned long long)i );
            uiHoleBases += vInHole[ i ] ? 1 : 0;
            CHECK( vInHole[ i ] || uiRef == g.vCodes[ i ], "%s.pac: base %llu is %u, parseHost %u", pName, (unsigned long long)i, uiRef, g.vCodes[ i ] );
        }
        CHECK( uiHoleBases == g.uiHoleBases, "%s: %llu hole bases", pName, (unsigned long long)g.uiHoleBases );
        checkYardstick( sPrefix + ".fa", g, 1 );
        checkYardstick( sPrefix + ".fa", g, 20261021 );
    }
    printf( "golden ok: %zu fixtures\n", sizeof( FIXTURES ) / sizeof( FIXTURES[ 0 ] ) );
    return 0;
}

// a strict genome: 1-6 contigs of 1-4 000 bases, hole bases in runs at 0-30 %, random line lengths, either line end
static std::string randomGenome( std::mt19937_64& rng )
{
    auto upTo = [ & ]( uint64_t n ) { return (uint64_t)( rng( ) % ( n + 1 ) ); };
    const char* const pEnd = upTo( 1 ) ? "\n" : "\r\n";
    const uint64_t uiContigs = 1 + upTo( 5 );
    const double dHoles = (double)upTo( 30 ) / 100.0;
    static const char aHole[] = "NNNNNNNNnnRYKMSWBDHVUryu", aBase[] = "ACGTACGTACGTacgt";
    std::string s;
    for( uint64_t c = 0; c < uiContigs; c++ )
    {
        s += ">";
        s += upTo( 3 ) == 0 ? "chr" : "contig_";
        s += std::to_string( upTo( 2 ) == 0 ? 1 : c + 1 ); // (same-name contigs among them)
        if( upTo( 2 ) == 0 )
            s += " a comment\twith words";
        s += pEnd;
        const uint64_t uiLen = upTo( 3 ) == 0 ? 1 + upTo( 70 ) : 1 + upTo( 3999 );
        std::string sBases;
        bool bHole = upTo( 99 ) < 100 * dHoles;
        while( sBases.size( ) < uiLen )
        {
            // runs: a hole run of 1-40, a base run long enough for the rate
            uint64_t uiRun = bHole ? 1 + upTo( upTo( 3 ) ? 3 : 39 ) : 1 + upTo( dHoles > 0 ? (uint64_t)( 10 / dHoles ) : 4000 );
            for( ; uiRun && sBases.size( ) < uiLen; uiRun-- )
                sBases += bHole ? aHole[ upTo( sizeof( aHole ) - 2 ) ] : aBase[ upTo( sizeof( aBase ) - 2 ) ];
            bHole = dHoles > 0 && !bHole;
        }
        const uint64_t uiWidth = upTo( 3 ) == 0 ? 1 + upTo( 20 ) : 60 + upTo( 40 );
        for( uint64_t at = 0; at < sBases.size( ); )
        {
            const uint64_t uiLine = upTo( 4 ) == 0 ? 1 + upTo( uiWidth - 1 ) : uiWidth;
            s += sBases.substr( at, uiLine );
            at += uiLine;
            if( at < sBases.size( ) || c + 1 < uiContigs || upTo( 2 ) )
                s += pEnd;
        }
    }
    return s;
}

static int cmdRandom( uint64_t uiSeed, uint64_t n, const char* pDir )
{
    std::mt19937_64 rng( uiSeed );
    uint64_t uiWithHoles = 0, uiHoles = 0;
    for( uint64_t i = 0; i < n; i++ )
    {
        const std::string sText = randomGenome( rng );
        const std::string sPath = pDir ? std::string( pDir ) + "/g" + std::to_string( i ) + ".fa" : "/tmp/genome_text_test." + std::to_string( getpid( ) ) + ".fa";
        {
            std::ofstream f( sPath, std::ios::binary );
            f << sText;
        }
        if( pDir )
            continue;
        const Genome g = whole( sText ); // (a refusal fails: all are accepted)
        checkYardstick( sPath, g, (uint32_t)( uiSeed + i ) );
        uiWithHoles += g.vHoleStart.empty( ) ? 0 : 1;
        uiHoles += g.vHoleStart.size( );
        remove( sPath.c_str( ) );
    }
    if( !pDir )
        CHECK( uiWithHoles * 2 > n, "only %llu genomes with holes", (unsigned long long)uiWithHoles );
    printf( "random ok: %llu genomes, %llu with holes, %llu holes\n", (unsigned long long)n, (unsigned long long)uiWithHoles, (unsigned long long)uiHoles );
    return 0;
}

static std::vector<size_t> lineEnds( const std::string& s ) // offsets behind each '\n'
{
    std::vector<size_t> v;
    for( size_t p = 0; p < s.size( ); p++ )
        if( s[ p ] == '\n' )
            v.push_back( p + 1 );
    return v;
}

static int cmdCuts( const std::string& sDir )
{
    uint64_t uiCuts = 0;
    for( const char* pName : FIXTURES )
    {
        const std::string sText = readFile( sDir + "/" + pName + ".fa" );
        const Genome xWhole = whole( sText );
        const std::vector<size_t> vEnds = lineEnds( sText );
        uint64_t uiConsumed;
        std::string sMessage;
        for( size_t uiCut : vEnds ) // two chunks
        {
            if( uiCut == sText.size( ) )
                continue;
            Genome g;
            CHECK( append( g, sText.substr( 0, uiCut ), false, &uiConsumed, &sMessage ) == 0 && uiConsumed == uiCut, "%s cut %zu: %s", pName, uiCut,
                   sMessage.c_str( ) );
            CHECK( append( g, sText.substr( uiCut ), true, &uiConsumed, &sMessage ) == 0 && uiConsumed == sText.size( ) - uiCut, "%s cut %zu: %s", pName,
                   uiCut, sMessage.c_str( ) );
            CHECK( same( g, xWhole ), "%s cut %zu differs", pName, uiCut );
            uiCuts++;
            // the first chunk with a tail that has no line feed: consumed stops at the last line feed
            for( size_t uiTail : { (size_t)1, (size_t)7 } )
            {
                if( uiCut + uiTail > sText.size( ) || sText.substr( uiCut, uiTail ).find( '\n' ) != std::string::npos )
                    continue;
                Genome t;
                CHECK( append( t, sText.substr( 0, uiCut + uiTail ), false, &uiConsumed, &sMessage ) == 0 && uiConsumed == uiCut, "%s tail %zu: %s",
                       pName, uiCut, sMessage.c_str( ) );
                CHECK( append( t, sText.substr( uiCut ), true, &uiConsumed, &sMessage ) == 0, "%s tail %zu: %s", pName, uiCut, sMessage.c_str( ) );
                CHECK( same( t, xWhole ), "%s tail %zu differs", pName, uiCut );
            }
        }
        Genome g; // one line per chunk
        size_t uiFrom = 0;
        for( size_t uiCut : vEnds )
        {
            CHECK( append( g, sText.substr( uiFrom, uiCut - uiFrom ), false, &uiConsumed, &sMessage ) == 0 && uiConsumed == uiCut - uiFrom,
                   "%s line at %zu: %s", pName, uiFrom, sMessage.c_str( ) );
            uiFrom = uiCut;
        }
        // a chunk without any line feed consumes nothing and changes nothing
        if( uiFrom < sText.size( ) )
        {
            const Genome xBefore = g;
            CHECK( append( g, sText.substr( uiFrom ), false, &uiConsumed, &sMessage ) == 0 && uiConsumed == 0 && same( g, xBefore ), "%s: tail", pName );
        }
        CHECK( append( g, sText.substr( uiFrom ), true, &uiConsumed, &sMessage ) == 0, "%s: %s", pName, sMessage.c_str( ) );
        CHECK( same( g, xWhole ), "%s line by line differs", pName );
    }
    printf( "cuts ok: %llu cuts\n", (unsigned long long)uiCuts );
    return 0;
}

static void refused( Genome& g, const std::string& sChunk, bool bEnd, const std::string& sExpect, uint64_t uiMax = NO_LIMIT )
{
    const Genome xBefore = g;
    uint64_t uiConsumed = 99;
    std::string sMessage;
    CHECK( append( g, sChunk, bEnd, &uiConsumed, &sMessage, uiMax ) == 1, "'%s' was accepted", sExpect.c_str( ) );
    CHECK( sMessage == "ma_genome_append_text: " + sExpect, "'%s' instead of '%s'", sMessage.c_str( ), sExpect.c_str( ) );
    CHECK( uiConsumed == 0 && same( g, xBefore ) && g.bLastHole == xBefore.bLastHole, "the refusal '%s' changed the genome", sExpect.c_str( ) );
}

static int cmdRefusals( )
{
    using namespace ma_text;
    auto line = []( uint64_t uiLine, uint64_t uiByte, uint32_t uiReason ) {
        return "line " + std::to_string( uiLine ) + " (byte " + std::to_string( uiByte ) + "): " + errorText( uiReason );
    };
    const std::string sFirst = ">a x\nACGTN\n", sGood = "NNAC\n>b\nGT\n"; // 11 bytes, 2 lines
    const Genome xOne = whole( sFirst + sGood );
    struct Case
    {
        std::string sChunk;
        bool bEnd;
        std::string sExpect;
    };
    const std::vector<Case> vFirstChunk = {
        { "ACGT\n", true, line( 1, 0, ERR_KIND ) },
        { "@r\nACGT\n+\nIIII\n", true, "a genome is FASTA" },
        { ">a\nAC\rGT\n", true, line( 2, 3, ERR_LONE_CR ) },
        { ">a\nACGT\n\nAC\n", true, line( 3, 8, ERR_SEQ_EMPTY ) },
        { ">a\nACGT\n AC\n", true, line( 3, 8, ERR_SEQ_START ) },
        { ">a\nACGT\n@AC\n", true, line( 3, 8, ERR_SEQ_START ) },
        { ">a\n>b\nAC\n", true, line( 1, 0, ERR_FA_NO_BASES ) },
        { ">a\nAC\n>b\n", true, line( 3, 6, ERR_FA_NO_BASES ) }, // a header that is the file's last line
        { ">a\nAC\n>b", true, line( 3, 6, ERR_FA_NO_BASES ) },
        { ">a\n12\n", true, line( 1, 0, ERR_FA_NO_BASES ) }, // a line without letters gives no bases
    };
    for( const Case& c : vFirstChunk )
    {
        Genome g;
        refused( g, c.sChunk, c.bEnd, c.sExpect );
    }
    // the same violations in a second chunk: line and byte count over both
    const std::vector<Case> vSecondChunk = {
        { "AC\rGT\n", false, line( 3, 11, ERR_LONE_CR ) },
        { "AC\n\n", false, line( 4, 11 + 3, ERR_SEQ_EMPTY ) },
        { " AC\n", false, line( 3, 11, ERR_SEQ_START ) },
        { "@AC\n", false, line( 3, 11, ERR_SEQ_START ) },
        { "AC\n>b\n>c\nAC\n", false, line( 4, 11 + 3, ERR_FA_NO_BASES ) },
        { "AC\n>b\n", true, line( 4, 11 + 3, ERR_FA_NO_BASES ) },
    };
    for( const Case& c : vSecondChunk )
    {
        Genome g;
        uint64_t uiConsumed;
        std::string sMessage;
        CHECK( append( g, sFirst, false, &uiConsumed, &sMessage ) == 0 && uiConsumed == sFirst.size( ), "%s", sMessage.c_str( ) );
        refused( g, c.sChunk, c.bEnd, c.sExpect );
        // the corrected chunk afterwards gives the one-piece result
        CHECK( append( g, sGood, true, &uiConsumed, &sMessage ) == 0 && same( g, xOne ), "after '%s': %s", c.sExpect.c_str( ), sMessage.c_str( ) );
    }
    {
        // a header ends a chunk that is not the file's end: fine; the next chunk must give it bases
        Genome g;
        uint64_t uiConsumed;
        std::string sMessage;
        CHECK( append( g, ">a\nAC\n>b\n", false, &uiConsumed, &sMessage ) == 0 && uiConsumed == 9, "%s", sMessage.c_str( ) );
        refused( g, ">c\nAC\n", false, line( 3, 6, ERR_FA_NO_BASES ) );
        refused( g, "", true, line( 3, 6, ERR_FA_NO_BASES ) );
        CHECK( append( g, "GT\n", true, &uiConsumed, &sMessage ) == 0, "%s", sMessage.c_str( ) );
        CHECK( same( g, whole( ">a\nAC\n>b\nGT\n" ) ), "a header at a chunk's end" );
        // behind the end of a file the next chunk is another file: a header is due
        refused( g, "ACGT\n", false, line( 5, 12, ERR_KIND ) );
        refused( g, "@x\n", false, "a genome is FASTA" );
        CHECK( append( g, ">c\nNN\n", true, &uiConsumed, &sMessage ) == 0 && g.vStarts.size( ) == 3 && g.vHoleStart.size( ) == 1, "a second file" );
    }
    {
        // capacity: exactly max_bases pass, one more is refused with the number the genome would hold
        Genome g;
        uint64_t uiConsumed;
        std::string sMessage;
        CHECK( append( g, ">a\nACGT\n", false, &uiConsumed, &sMessage, 6 ) == 0, "%s", sMessage.c_str( ) );
        refused( g, "ACG\n", false, "genome capacity exceeded (7 bases)", 6 );
        CHECK( append( g, "AC\n", true, &uiConsumed, &sMessage, 6 ) == 0 && g.uiBases == 6, "%s", sMessage.c_str( ) );
        CHECK( ma_genome_dev::buildRefusal( g ) == NULL, "build refused" );
        ma_genome_dev::fillHost( g, 1 );
        refused( g, ">b\nAC\n", true, "the index was already built", 100 );
        CHECK( std::string( ma_genome_dev::buildRefusal( g ) ) == "ma_genome_build_index: the index was already built", "second build" );
        Genome e;
        CHECK( std::string( ma_genome_dev::buildRefusal( e ) ) == "ma_genome_build_index: the genome has no contigs", "empty build" );
        CHECK( append( e, ">a\n", false, &uiConsumed, &sMessage ) == 0, "%s", sMessage.c_str( ) );
        CHECK( std::string( ma_genome_dev::buildRefusal( e ) ) == "ma_genome_build_index: the last contig is still open without bases", "open build" );
    }
    {
        // the size is judged on n_bytes before a byte of the chunk is looked at (the two bytes here are all there are), with and
        // without end_of_file; compressed bytes where a header is due are named
        Genome g;
        uint64_t uiConsumed = 99;
        std::string sMessage;
        CHECK( append( g, ">a\nAC\n", false, &uiConsumed, &sMessage ) == 0, "%s", sMessage.c_str( ) );
        const Genome xBefore = g;
        const char aTwo[ 2 ] = { 'A', 'C' };
        for( bool bEnd : { true, false } )
            for( uint64_t uiBytes : { (uint64_t)1 << 31, ma_text::MAX_TEXT_BYTES + 1 } )
            {
                uiConsumed = 99;
                CHECK( ma_genome_dev::parseHost( g, aTwo, uiBytes, bEnd, NO_LIMIT, &uiConsumed, &sMessage ) == 1 &&
                           sMessage == "ma_genome_append_text: too large" && uiConsumed == 0 && same( g, xBefore ),
                       "too large: '%s'", sMessage.c_str( ) );
            }
        CHECK( append( g, "GT\n", true, &uiConsumed, &sMessage ) == 0 && same( g, whole( ">a\nAC\nGT\n" ) ), "after too large: %s", sMessage.c_str( ) );
        const std::string sGzip = std::string( "\x1f\x8b\x08\x04" ) + "more\n";
        refused( g, sGzip, false, "a genome as BGZF or gzip is not served (plain FASTA text only)" );
        Genome e;
        refused( e, sGzip, true, "a genome as BGZF or gzip is not served (plain FASTA text only)" );
    }
    // the generator is libc's
    for( uint32_t uiSeed : { 0u, 1u, 20261021u, 0xffffffffu } )
    {
        srand( uiSeed );
        ma_genome_dev::Rand xRand( uiSeed );
        for( int i = 0; i < 1000; i++ )
            CHECK( (uint32_t)rand( ) == xRand.next( ), "draw %d of seed %u", i, uiSeed );
    }
    printf( "refusals ok: %zu + %zu texts\n", vFirstChunk.size( ), vSecondChunk.size( ) );
    return 0;
}

static int cmdDump( uint32_t uiSeed, int nFiles, char** ppFiles )
{
    for( int f = 0; f < nFiles; f++ )
    {
        const std::string sText = readFile( ppFiles[ f ] );
        Genome g;
        uint64_t uiConsumed;
        std::string sMessage;
        printf( "file %s\n", ppFiles[ f ] );
        if( append( g, sText, true, &uiConsumed, &sMessage ) )
        {
            printf( "refused %s\n", sMessage.c_str( ) );
            continue;
        }
        printf( "counts %zu %llu %zu %zu %llu\n", g.vStarts.size( ), (unsigned long long)g.uiBases, g.sNames.size( ), g.vHoleStart.size( ),
                (unsigned long long)g.uiHoleBases );
        for( size_t i = 0; i < g.vStarts.size( ); i++ )
            printf( "contig %s %llu %llu %llu\n", nameOf( g, i ).c_str( ), (unsigned long long)g.vStarts[ i ], (unsigned long long)g.vLens[ i ],
                    (unsigned long long)g.vNumHoles[ i ] );
        for( size_t i = 0; i < g.vHoleStart.size( ); i++ )
            printf( "hole %llu %llu\n", (unsigned long long)g.vHoleStart[ i ], (unsigned long long)g.vHoleLen[ i ] );
        std::string sCodes( g.vCodes.size( ), '0' );
        for( size_t i = 0; i < g.vCodes.size( ); i++ )
            sCodes[ i ] = (char)( '0' + g.vCodes[ i ] );
        printf( "codes %s\n", sCodes.c_str( ) );
        ma_genome_dev::fillHost( g, uiSeed );
        for( size_t i = 0; i < g.vCodes.size( ); i++ )
            sCodes[ i ] = (char)( '0' + g.vCodes[ i ] );
        printf( "filled %s\n", sCodes.c_str( ) );
    }
    return 0;
}

int main( int argc, char** argv )
{
    const std::string sCmd = argc > 1 ? argv[ 1 ] : "";
    if( sCmd == "golden" && argc == 3 )
        return cmdGolden( argv[ 2 ] );
    if( sCmd == "random" && argc == 4 )
        return cmdRandom( strtoull( argv[ 2 ], NULL, 10 ), strtoull( argv[ 3 ], NULL, 10 ), NULL );
    if( sCmd == "gen" && argc == 5 )
        return cmdRandom( strtoull( argv[ 2 ], NULL, 10 ), strtoull( argv[ 3 ], NULL, 10 ), argv[ 4 ] );
    if( sCmd == "cuts" && argc == 3 )
        return cmdCuts( argv[ 2 ] );
    if( sCmd == "refusals" )
        return cmdRefusals( );
    if( sCmd == "dump" && argc >= 4 )
        return cmdDump( (uint32_t)strtoull( argv[ 2 ], NULL, 10 ), argc - 3, argv + 3 );
    printf( "usage: genome_text_test golden <dir> | random <seed> <n> | gen <seed> <n> <dir> | cuts <dir> | refusals | dump <seed> <file>...\n" );
    return 2;
}
