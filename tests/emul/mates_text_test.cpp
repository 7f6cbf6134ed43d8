// CPU-only checks of the rules of ma_batch_set_mates_text (ma_amd/host/ma_text_dev.h: ma_text::pairHost, the serial statement the
// kernels are compared with) and of BatchPairedTextReader (ma_amd/host/ma_batch_nodes.h) against the yardstick, PairedFileReader
// of ma_amd/host/ma_sam.h over in-memory streams, and against the reference's own reader output (tests/golden/reader/mates.*).
//   mates_text_test golden <dir>             mates_1.fq / mates_2.fq with rev_comp 0 and 1 equal mates.rc0.ref / mates.rc1.ref
//   mates_text_test random <seed> <n>        seeded strict text pairs: pairHost equals PairedFileReader, with and without rev_comp
//   mates_text_test reasons [print]          the refusals: wording and precedence (print: hex of both texts + message per line)
//   mates_text_test reader <batch bytes>     BatchPairedTextReader's batches: equally many records, concatenating to the inputs
//   mates_text_test dump <rev> <f1> <f2>...  (the yardstick of tests/test_gpu_mates_text.py) per file pair pairHost's result or message
// pairHost gets arrays of exactly the sizes it announced and the texts hold exactly their bytes, so that an AddressSanitizer
// build of this program sees any byte touched outside of them.
#include "ma_batch_nodes.h"
#include "ma_text_dev.h"
#include <fstream>
#include <random>

using namespace libMA;

struct Read
{
    std::string sName;
    std::vector<uint8_t> vCodes, vQual;
    bool operator==( const Read& o ) const
    {
        return sName == o.sName && vCodes == o.vCodes && vQual == o.vQual;
    }
};
struct Paired
{
    bool bAccepted = false;
    std::string sMessage;
    ma_text::PairResult xResult;
    std::vector<Read> vReads; // 2 R
};

static std::unique_ptr<char[]> exactCopy( const std::string& s ) // exactly the text's bytes on the heap (no terminator behind them)
{
    std::unique_ptr<char[]> p( new char[ std::max<size_t>( s.size( ), 1 ) ] );
    memcpy( p.get( ), s.data( ), s.size( ) );
    return p;
}
static Paired host( const std::string& s1, const std::string& s2, bool bRev )
{
    Paired p;
    const auto p1 = exactCopy( s1 ), p2 = exactCopy( s2 );
    if( ma_text::pairHost( p1.get( ), s1.size( ), p2.get( ), s2.size( ), bRev, nullptr, nullptr, nullptr, nullptr, nullptr, &p.xResult ) )
    {
        char aMessage[ 256 ];
        const ma_text::PairResult& r = p.xResult;
        ma_text::messageMates( aMessage, sizeof( aMessage ), r.uiRefusal, r.uiText, r.uiLine, r.uiByte, r.uiReason );
        p.sMessage = aMessage;
        if( r.uiPairs != 0 || r.aConsumed[ 0 ] != 0 || r.aConsumed[ 1 ] != 0 )
            throw std::runtime_error( "pairHost: a refusal with pairs or consumed bytes" );
        return p;
    }
    const ma_text::PairResult r = p.xResult;
    const uint64_t n = 2 * r.uiPairs;
    std::unique_ptr<uint64_t[]> pOff( new uint64_t[ n + 1 ] ), pNameOff( new uint64_t[ n + 1 ] );
    std::unique_ptr<uint8_t[]> pCodes( new uint8_t[ r.uiBases ] ), pQual( new uint8_t[ r.iHasQual ? r.uiBases : 0 ] );
    std::unique_ptr<char[]> pNames( new char[ r.uiNameBytes ] );
    ma_text::PairResult xAgain;
    if( ma_text::pairHost( p1.get( ), s1.size( ), p2.get( ), s2.size( ), bRev, pOff.get( ), pCodes.get( ), pNameOff.get( ), pNames.get( ),
                           r.iHasQual ? pQual.get( ) : nullptr, &xAgain ) ||
        xAgain.uiPairs != r.uiPairs || xAgain.uiBases != r.uiBases || xAgain.uiNameBytes != r.uiNameBytes )
        throw std::runtime_error( "pairHost: the second pass disagrees with the first" );
    if( pOff[ n ] != r.uiBases || pNameOff[ n ] != r.uiNameBytes )
        throw std::runtime_error( "pairHost: the offsets do not end at the sums" );
    uint64_t uiLongest = 0;
    for( uint64_t i = 0; i < n; i++ )
    {
        Read x;
        x.sName.assign( pNames.get( ) + pNameOff[ i ], pNameOff[ i + 1 ] - pNameOff[ i ] );
        x.vCodes.assign( pCodes.get( ) + pOff[ i ], pCodes.get( ) + pOff[ i + 1 ] );
        if( r.iHasQual )
            x.vQual.assign( pQual.get( ) + pOff[ i ], pQual.get( ) + pOff[ i + 1 ] );
        uiLongest = std::max<uint64_t>( uiLongest, x.vCodes.size( ) );
        p.vReads.push_back( std::move( x ) );
    }
    if( uiLongest != r.uiMaxLen )
        throw std::runtime_error( "pairHost: the longest read is not the longest read" );
    p.bAccepted = true;
    return p;
}
// PairedFileReader of ma_sam.h over two in-memory streams
static std::vector<Read> yardstick( const std::string& s1, const std::string& s2, bool bRev )
{
    ParameterSetManager xParameters;
    xParameters.bRevCompPairedReadMates = bRev;
    PairedFileReader xReader( xParameters );
    auto pStreams = std::make_shared<PairedFileStream>( std::make_shared<StringStream>( s1 ), std::make_shared<StringStream>( s2 ) );
    std::vector<Read> v;
    while( auto pPair = xReader.execute( pStreams ) )
        for( auto& pQ : *pPair )
            v.push_back( Read{ pQ->sName, pQ->xCodes, pQ->xQuality } );
    return v;
}
static std::string slurp( const std::string& sPath )
{
    std::ifstream xIn( sPath, std::ios::binary );
    if( !xIn )
        throw std::runtime_error( "cannot read " + sPath );
    std::stringstream xAll;
    xAll << xIn.rdbuf( );
    return xAll.str( );
}

// ---- generated strict texts ---------------------------------------------------------------------------------------------------
typedef std::mt19937_64 Rng;
static size_t pick( Rng& r, size_t n )
{
    return (size_t)( r( ) % n );
}
static std::string record( Rng& r, bool bFastq, const std::string& sName, size_t n, const std::string& sEnd )
{
    static const char aLetters[] = "ACGTACGTACGTACGTNNRYKMSWBDHVUacgtn";
    std::string sBases, sQual;
    for( size_t i = 0; i < n; i++ )
    {
        sBases += aLetters[ pick( r, pick( r, 4 ) ? 16 : sizeof( aLetters ) - 1 ) ];
        sQual += (char)( 33 + pick( r, 94 ) );
    }
    if( n >= 3 && pick( r, 5 ) == 0 )
        sBases[ 1 ] = '*'; // a kept byte that is no nucleotide: code 4, complemented to 5
    const std::string sHeader = sName + ( pick( r, 3 ) == 0 ? " some description" : "" );
    if( bFastq )
        return "@" + sHeader + sEnd + sBases + sEnd + "+" + sEnd + sQual + sEnd;
    std::string s = ">" + sHeader + sEnd;
    for( size_t uiAt = 0; uiAt < n; ) // one to three lines
    {
        const size_t m = pick( r, 2 ) ? n - uiAt : 1 + pick( r, n - uiAt );
        s += sBases.substr( uiAt, m ) + sEnd;
        uiAt += m;
    }
    return s;
}
static size_t length( Rng& r )
{
    static const size_t aEdges[] = { 1, 15, 16, 17, 63, 64, 65, 255, 256, 257 };
    return pick( r, 3 ) == 0 ? aEdges[ pick( r, 10 ) ] : 1 + pick( r, 40 );
}
// uiRecords records of unequal lengths; iMate goes into the names
static std::string mateText( Rng& r, bool bFastq, size_t uiRecords, int iMate, bool bFinalEnd = true )
{
    const std::string sEnd = pick( r, 2 ) ? "\n" : "\r\n";
    std::string s;
    for( size_t k = 0; k < uiRecords; k++ )
        s += record( r, bFastq, "p" + std::to_string( k ) + "/" + std::to_string( iMate ), length( r ), sEnd );
    if( !bFinalEnd && !s.empty( ) )
        s.resize( s.size( ) - sEnd.size( ) );
    return s;
}

// ---- modes ------------------------------------------------------------------------------------------------------------------
static std::vector<Read> refDump( const std::string& sPath )
{
    std::vector<Read> v;
    std::ifstream xIn( sPath );
    std::string sLine;
    while( std::getline( xIn, sLine ) )
    {
        std::istringstream xL( sLine );
        std::string sName, sCodes, sQual;
        size_t n = 0;
        xL >> sName >> n >> sCodes >> sQual;
        Read x;
        x.sName = sName;
        for( char c : sCodes )
            x.vCodes.push_back( (uint8_t)( c - '0' ) );
        x.vQual.assign( sQual.begin( ), sQual.end( ) );
        if( x.vCodes.size( ) != n )
            throw std::runtime_error( "bad line in " + sPath );
        v.push_back( x );
    }
    return v;
}
static int golden( const std::string& sDir )
{
    const std::string s1 = slurp( sDir + "/mates_1.fq" ), s2 = slurp( sDir + "/mates_2.fq" );
    size_t uiReads = 0;
    for( int iRev = 0; iRev < 2; iRev++ )
    {
        const Paired h = host( s1, s2, iRev != 0 );
        const std::vector<Read> vRef = refDump( sDir + ( iRev ? "/mates.rc1.ref" : "/mates.rc0.ref" ) );
        if( !h.bAccepted || vRef.empty( ) || h.vReads != vRef )
            return printf( "FAIL rev_comp %d: %s\n", iRev, h.bAccepted ? "differs from the reference's dump" : h.sMessage.c_str( ) ), 1;
        if( h.vReads != yardstick( s1, s2, iRev != 0 ) )
            return printf( "FAIL rev_comp %d: differs from PairedFileReader\n", iRev ), 1;
        uiReads += h.vReads.size( );
    }
    printf( "golden ok: %zu reads equal\n", uiReads );
    return 0;
}

static int randomPairs( uint64_t uiSeed, size_t n )
{
    Rng r( uiSeed );
    size_t uiReads = 0, uiUnequal = 0;
    for( size_t t = 0; t < n; t++ )
    {
        const bool bFastq = t % 2 == 0;
        const size_t uiRecords = t % 7 == 0 ? 0 : 1 + pick( r, 12 ), uiMore = t % 3 == 0 ? 0 : 1 + pick( r, 3 );
        const size_t uiRecords1 = uiRecords + ( t % 3 == 1 ? uiMore : 0 ), uiRecords2 = uiRecords + ( t % 3 == 2 ? uiMore : 0 );
        const std::string s1 = mateText( r, bFastq, uiRecords1, 1, pick( r, 3 ) != 0 ), s2 = mateText( r, bFastq, uiRecords2, 2, pick( r, 3 ) != 0 );
        for( int iRev = 0; iRev < 2; iRev++ )
        {
            const Paired h = host( s1, s2, iRev != 0 );
            if( !h.bAccepted )
                return printf( "FAIL pair %zu refused: %s\n", t, h.sMessage.c_str( ) ), 1;
            if( h.vReads != yardstick( s1, s2, iRev != 0 ) || h.vReads.size( ) != 2 * std::min( uiRecords1, uiRecords2 ) )
                return printf( "FAIL pair %zu (rev_comp %d) differs from PairedFileReader\n", t, iRev ), 1;
            // what was consumed parses to exactly the pairs; what is left holds the surplus records
            for( int i = 0; i < 2; i++ )
            {
                const std::string& s = i ? s2 : s1;
                const Paired xUsed = host( s.substr( 0, h.xResult.aConsumed[ i ] ), s.substr( 0, h.xResult.aConsumed[ i ] ), false );
                if( !xUsed.bAccepted || xUsed.xResult.uiPairs != h.xResult.uiPairs ||
                    ( h.xResult.aConsumed[ i ] == s.size( ) ) != ( ( i ? uiRecords2 : uiRecords1 ) == h.xResult.uiPairs ) )
                    return printf( "FAIL pair %zu: consumed[ %d ] = %llu\n", t, i, (unsigned long long)h.xResult.aConsumed[ i ] ), 1;
            }
            uiReads += h.vReads.size( );
        }
        uiUnequal += uiRecords1 != uiRecords2;
    }
    printf( "random ok: %zu text pairs, %zu of unequal counts, %zu reads equal\n", n, uiUnequal, uiReads );
    return 0;
}

struct Reason
{
    const char* sWhat;
    std::string sText1, sText2;
    std::string sWant; // behind "ma_batch_set_mates_text: "
};
static std::vector<Reason> reasonTable( )
{
    const std::string sGood = "@r\nACGT\n+\nIIII\n", sShortQual = "@r\nACGT\n+\nIII\n", sNoPlus = "@r\nACGT\nIIII\n@s\n", sFasta = ">r\nACGT\n";
    const std::string sQualLen = std::string( ma_text::errorText( ma_text::ERR_FQ_QUAL_LEN ) ), sPlus = ma_text::errorText( ma_text::ERR_FQ_PLUS );
    return {
        { "violation in text 1", sShortQual, sGood, "text 1: line 4 (byte 10): " + sQualLen },
        { "violation in text 2", sGood, sGood + sShortQual, "text 2: line 8 (byte 25): " + sQualLen },
        { "violations in both: text 1 is named", sGood + sNoPlus, sShortQual, "text 1: line 7 (byte 23): " + sPlus },
        { "violation beyond the pairs", sGood, sGood + sGood + sGood + sNoPlus, "text 2: line 15 (byte 53): " + sPlus },
        { "violation in text 2, text 1 empty", "", sShortQual, "text 2: line 4 (byte 10): " + sQualLen },
        { "text 2 of neither kind", sGood, "ACGT\n", std::string( "text 2: line 1 (byte 0): " ) + ma_text::errorText( ma_text::ERR_KIND ) },
        { "text 1 of neither kind", "x", sShortQual, std::string( "text 1: line 1 (byte 0): " ) + ma_text::errorText( ma_text::ERR_KIND ) },
        { "violation in text 1, text 2 of neither kind", sShortQual, "ACGT\n", "text 1: line 4 (byte 10): " + sQualLen },
        { "FASTA record without bases in text 2", sFasta, sFasta + ">s\n",
          std::string( "text 2: line 3 (byte 8): " ) + ma_text::errorText( ma_text::ERR_FA_NO_BASES ) },
        { "FASTQ against FASTA", sGood, sFasta, "the two texts differ in kind" },
        { "FASTA against FASTQ", sFasta + sFasta, sGood, "the two texts differ in kind" },
        { "a violation wins over the kinds", sFasta, sShortQual, "text 2: line 4 (byte 10): " + sQualLen },
    };
}
static int reasons( bool bPrint )
{
    for( const Reason& x : reasonTable( ) )
    {
        const std::string sWant = "ma_batch_set_mates_text: " + x.sWant;
        if( bPrint ) // the table for the GPU test: both texts in hex ("-": empty), then the message
        {
            for( const std::string* pText : { &x.sText1, &x.sText2 } )
            {
                for( unsigned char c : *pText )
                    printf( "%02x", c );
                printf( pText->empty( ) ? "- " : " " );
            }
            printf( "%s\n", sWant.c_str( ) );
            continue;
        }
        for( int iRev = 0; iRev < 2; iRev++ )
        {
            const Paired h = host( x.sText1, x.sText2, iRev != 0 );
            if( h.bAccepted || h.sMessage != sWant )
                return printf( "FAIL %s: '%s', expected '%s'\n", x.sWhat, h.bAccepted ? "accepted" : h.sMessage.c_str( ), sWant.c_str( ) ), 1;
        }
    }
    char aCapacity[ 256 ];
    ma_text::messageMates( aCapacity, sizeof( aCapacity ), ma_text::MATES_CAPACITY, 0, 0, 0, 0 );
    if( std::string( aCapacity ) != "ma_batch_set_mates_text: batch capacity exceeded" )
        return printf( "FAIL wording: %s\n", aCapacity ), 1;
    if( !bPrint )
        printf( "reasons ok: %zu text pairs\n", reasonTable( ).size( ) );
    return 0;
}

// BatchPairedTextReader over two in-memory streams of uiPairs + uiMore1 and uiPairs + uiMore2 records
static int readerOne( Rng& r, bool bFastq, size_t uiBatchBytes, size_t uiPairs, size_t uiMore1, size_t uiMore2 )
{
    const std::string s1 = mateText( r, bFastq, uiPairs + uiMore1, 1 ), s2 = mateText( r, bFastq, uiPairs + uiMore2, 2, pick( r, 2 ) != 0 );
    const std::string sWhat = std::string( bFastq ? "fastq " : "fasta " ) + std::to_string( uiPairs ) + "+" + std::to_string( uiMore1 ) + "/+" +
                              std::to_string( uiMore2 ) + " pairs, batches of " + std::to_string( uiBatchBytes );
    BatchPairedTextReader xReader{ ParameterSetManager( ) };
    xReader.uiBatchBytes = uiBatchBytes;
    auto pStreams = std::make_shared<PairedFileStream>( std::make_shared<StringStream>( s1 ), std::make_shared<StringStream>( s2 ) );
    std::string sAll1, sAll2;
    std::vector<Read> vAll;
    size_t uiBatches = 0, uiSeen = 0;
    while( auto pBatch = xReader.execute( pStreams ) )
    {
        const Paired h = host( pBatch->sText1, pBatch->sText2, true );
        if( !h.bAccepted )
            return printf( "FAIL %s: batch %zu refused: %s\n", sWhat.c_str( ), uiBatches, h.sMessage.c_str( ) ), 1;
        const size_t c1 = BatchPairedTextReader::countRecords( pBatch->sText1 ), c2 = BatchPairedTextReader::countRecords( pBatch->sText2 );
        uiSeen += h.xResult.uiPairs;
        // every batch holds equally many records in both texts -- but the last one, where the longer file's rest goes out as it is
        if( c1 != c2 && uiSeen != uiPairs )
            return printf( "FAIL %s: batch %zu holds %zu and %zu records\n", sWhat.c_str( ), uiBatches, c1, c2 ), 1;
        if( c1 == c2 && ( h.xResult.aConsumed[ 0 ] != pBatch->sText1.size( ) || h.xResult.aConsumed[ 1 ] != pBatch->sText2.size( ) ) )
            return printf( "FAIL %s: batch %zu is not consumed entirely\n", sWhat.c_str( ), uiBatches ), 1;
        sAll1 += pBatch->sText1.substr( 0, h.xResult.aConsumed[ 0 ] );
        sAll2 += pBatch->sText2.substr( 0, h.xResult.aConsumed[ 1 ] );
        vAll.insert( vAll.end( ), h.vReads.begin( ), h.vReads.end( ) );
        uiBatches++;
    }
    if( xReader.execute( pStreams ) != nullptr )
        return printf( "FAIL %s: a batch behind the end\n", sWhat.c_str( ) ), 1;
    // the concatenation is each input up to the shorter file's record count
    const Paired xWhole = host( s1, s2, true );
    if( !xWhole.bAccepted || xWhole.xResult.uiPairs != uiPairs || sAll1 != s1.substr( 0, xWhole.xResult.aConsumed[ 0 ] ) ||
        sAll2 != s2.substr( 0, xWhole.xResult.aConsumed[ 1 ] ) )
        return printf( "FAIL %s: the batches do not concatenate to the inputs up to pair %zu\n", sWhat.c_str( ), uiPairs ), 1;
    if( vAll != xWhole.vReads || vAll != yardstick( s1, s2, true ) )
        return printf( "FAIL %s: the batches' reads differ from PairedFileReader's\n", sWhat.c_str( ) ), 1;
    return 0;
}
static int reader( size_t uiBatchBytes )
{
    Rng r( 20261020 );
    size_t uiRuns = 0;
    for( bool bFastq : { true, false } )
        for( size_t uiPairs : { 0, 1, 2, 37, 1000 } )
            for( int iMore = 0; iMore < 3; iMore++, uiRuns++ ) // equal counts, file 1 three records longer, file 2 three records longer
                if( readerOne( r, bFastq, uiBatchBytes, uiPairs, iMore == 1 ? 3 : 0, iMore == 2 ? 3 : 0 ) )
                    return 1;
    // a stream without block reads (as a gzip stream is): the reader throws the message BatchTextReader throws
    struct NoBlockStream : public StringStream
    {
        using StringStream::StringStream;
        bool readBlock( std::string&, size_t ) override
        {
            return false;
        }
    };
    try
    {
        BatchPairedTextReader xReader{ ParameterSetManager( ) };
        xReader.execute( std::make_shared<PairedFileStream>( std::make_shared<StringStream>( "@r\nA\n+\nI\n" ), std::make_shared<NoBlockStream>( "@r\nA\n+\nI\n" ) ) );
        return printf( "FAIL: a stream without block reads was read\n" ), 1;
    }
    catch( const std::runtime_error& rE )
    {
        if( std::string( rE.what( ) ).find( "BatchTextReader: the stream" ) != 0 || std::string( rE.what( ) ).find( "BatchFileReader" ) == std::string::npos )
            return printf( "FAIL: '%s' is not BatchTextReader's message\n", rE.what( ) ), 1;
    }
    printf( "reader ok: %zu runs, batches of %zu bytes\n", uiRuns, uiBatchBytes );
    return 0;
}

static int dump( int argc, char** argv )
{
    const bool bRev = atoi( argv[ 2 ] ) != 0;
    for( int k = 3; k + 1 < argc; k += 2 )
    {
        const std::string s1 = slurp( argv[ k ] ), s2 = slurp( argv[ k + 1 ] );
        const Paired h = host( s1, s2, bRev );
        if( !h.bAccepted )
        {
            printf( "ERR %s\n", h.sMessage.c_str( ) );
            continue;
        }
        printf( "OK %zu %d %llu %llu %s\n", h.vReads.size( ), (int)h.xResult.iHasQual, (unsigned long long)h.xResult.aConsumed[ 0 ],
                (unsigned long long)h.xResult.aConsumed[ 1 ], yardstick( s1, s2, bRev ) == h.vReads ? "same" : "different" );
        for( const Read& x : h.vReads )
        {
            printf( "n" );
            for( unsigned char c : x.sName )
                printf( "%02x", c );
            printf( " c" );
            for( uint8_t c : x.vCodes )
                putchar( '0' + c );
            printf( " q" );
            for( unsigned char c : x.vQual )
                printf( "%02x", c );
            printf( "\n" );
        }
    }
    return 0;
}

int main( int argc, char** argv )
{
    try
    {
        const std::string sMode = argc > 1 ? argv[ 1 ] : "";
        if( sMode == "golden" && argc > 2 )
            return golden( argv[ 2 ] );
        if( sMode == "random" && argc > 3 )
            return randomPairs( strtoull( argv[ 2 ], nullptr, 10 ), (size_t)atol( argv[ 3 ] ) );
        if( sMode == "reasons" )
            return reasons( argc > 2 && std::string( argv[ 2 ] ) == "print" );
        if( sMode == "reader" && argc > 2 )
            return reader( (size_t)atol( argv[ 2 ] ) );
        if( sMode == "dump" && argc > 2 )
            return dump( argc, argv );
        fprintf( stderr, "usage: mates_text_test golden <dir> | random <seed> <n> | reasons [print] | reader <bytes> | dump <rev> <file1> <file2>...\n" );
        return 2;
    }
    catch( const std::exception& rE )
    {
        printf( "EXCEPTION %s\n", rE.what( ) );
        return 3;
    }
}
