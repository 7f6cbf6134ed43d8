// CPU-only checks of the rules the device's text parser runs (ma_amd/host/ma_text_dev.h: ma_text::parseHost over the per-line
// functions the kernels call) and of BatchTextReader (ma_amd/host/ma_batch_nodes.h) against the yardstick,
// FileReader::parseRecord of ma_amd/host/ma_sam.h over a StringStream, which tests/test_sam_writer.py pins to the reference's
// reader goldens.
//   text_dev_test golden <dir>            the committed reader fixtures: four accepted and equal to the .ref dumps, four refused
//   text_dev_test strict <seed> <n>       seeded texts in the strict form: all accepted, all equal to the yardstick
//   text_dev_test mutants <seed> <n>      three mutants per strict text: refused, or equal to the yardstick
//   text_dev_test reasons                 one hand-made text per reason code: line, byte and wording of the refusal
//   text_dev_test cut <block bytes> <fq>  BatchTextReader's batches: they concatenate to the file, start at record starts and
//                                         parse to the yardstick's reads; on <fq> and on a generated FASTA
//   text_dev_test dump <file>...          (the yardstick of tests/test_gpu_reads_text.py) per file parseHost's result or message
// parseHost gets arrays of exactly the sizes it announced and the texts hold exactly their bytes, so that an AddressSanitizer
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
struct Parsed
{
    bool bAccepted = false;
    std::string sMessage; // refusal / exception
    ma_text::Result xResult;
    std::vector<Read> vReads;
};

static Parsed yardstick( const std::string& sText )
{
    Parsed p;
    try
    {
        StringStream xStream( sText );
        while( auto pQ = FileReader::parseRecord( xStream ) )
            p.vReads.push_back( Read{ pQ->sName, pQ->xCodes, pQ->xQuality } );
        p.bAccepted = true;
    }
    catch( const std::exception& rE )
    {
        p.sMessage = rE.what( );
    }
    return p;
}

static Parsed host( const std::string& sText )
{
    Parsed p;
    // exactly the text's bytes on the heap (no terminator behind them)
    std::unique_ptr<char[]> pText( new char[ std::max<size_t>( sText.size( ), 1 ) ] );
    memcpy( pText.get( ), sText.data( ), sText.size( ) );
    std::unique_ptr<uint32_t[]> pStart( new uint32_t[ sText.size( ) + 2 ] );
    if( ma_text::parseHost( pText.get( ), sText.size( ), pStart.get( ), nullptr, nullptr, nullptr, nullptr, nullptr, &p.xResult ) )
    {
        char aMessage[ 256 ];
        ma_text::message( aMessage, sizeof( aMessage ), p.xResult.uiLine, p.xResult.uiByte, p.xResult.uiReason );
        p.sMessage = aMessage;
        return p;
    }
    const ma_text::Result r = p.xResult;
    std::unique_ptr<uint64_t[]> pOff( new uint64_t[ r.uiReads + 1 ] ), pNameOff( new uint64_t[ r.uiReads + 1 ] );
    std::unique_ptr<uint8_t[]> pCodes( new uint8_t[ r.uiBases ] ), pQual( new uint8_t[ r.iHasQual ? r.uiBases : 0 ] );
    std::unique_ptr<char[]> pNames( new char[ r.uiNameBytes ] );
    ma_text::Result xAgain;
    if( ma_text::parseHost( pText.get( ), sText.size( ), pStart.get( ), pOff.get( ), pCodes.get( ), pNameOff.get( ), pNames.get( ),
                            r.iHasQual ? pQual.get( ) : nullptr, &xAgain ) ||
        xAgain.uiReads != r.uiReads || xAgain.uiBases != r.uiBases || xAgain.uiNameBytes != r.uiNameBytes )
        throw std::runtime_error( "parseHost: the second pass disagrees with the first" );
    if( pOff[ r.uiReads ] != r.uiBases || pNameOff[ r.uiReads ] != r.uiNameBytes )
        throw std::runtime_error( "parseHost: the offsets do not end at the sums" );
    uint64_t uiLongest = 0;
    for( uint64_t i = 0; i < r.uiReads; i++ )
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
        throw std::runtime_error( "parseHost: the longest read is not the longest read" );
    p.bAccepted = true;
    return p;
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

// ---- the generator of strict texts -------------------------------------------------------------------------------------------
typedef std::mt19937_64 Rng;
static size_t pick( Rng& r, size_t n )
{
    return (size_t)( r( ) % n );
}
static std::string bases( Rng& r, size_t n, bool bJunkInside )
{
    static const char aLetters[] = "ACGTACGTACGTACGTUNRYKMSWBDHVacgtnryk";
    std::string s;
    for( size_t i = 0; i < n; i++ )
        s += aLetters[ pick( r, pick( r, 4 ) ? 16 : sizeof( aLetters ) - 1 ) ];
    if( bJunkInside && n >= 3 )
        s[ 1 + pick( r, n - 2 ) ] = "x*-.1"[ pick( r, 5 ) ]; // a kept byte that is no nucleotide: code 4
    return s;
}
static std::string name( Rng& r )
{
    static const char aChars[] = "abcXYZ019_/.:#@>+-\t";
    std::string s;
    for( size_t n = pick( r, 8 ) ? pick( r, 12 ) : pick( r, 41 ); s.size( ) < n; )
        s += aChars[ pick( r, sizeof( aChars ) - 1 ) ];
    return s;
}
static size_t length( Rng& r )
{
    static const size_t aEdges[] = { 1, 63, 64, 65, 255, 256, 257 };
    return pick( r, 3 ) == 0 ? aEdges[ pick( r, 7 ) ] : 1 + pick( r, 40 );
}
static std::string strictText( Rng& r, bool bFastq, size_t uiLongOne = 0 )
{
    const std::string sEnd = pick( r, 2 ) ? "\n" : "\r\n";
    const size_t uiRecords = 1 + pick( r, 12 ), uiLongAt = pick( r, uiRecords );
    std::string s;
    for( size_t k = 0; k < uiRecords; k++ )
    {
        std::string sHeader = ( bFastq ? "@" : ">" ) + name( r );
        if( pick( r, 3 ) == 0 )
            sHeader += std::string( " desc" ) + ( pick( r, 2 ) ? " more" : "\tmore" );
        else if( pick( r, 4 ) == 0 && sHeader.find( '\t' ) == std::string::npos )
            sHeader += "\tafter a tab"; // (the tab and the word behind it belong to the name, what follows the blank does not)
        s += sHeader + sEnd;
        const size_t n = uiLongOne && k == uiLongAt ? uiLongOne : length( r );
        if( bFastq )
        {
            std::string sBases = bases( r, n, pick( r, 4 ) == 0 );
            if( pick( r, 4 ) == 0 )
                sBases[ 0 ] = "acgtn"[ pick( r, 5 ) ]; // a line that starts with a lower-case letter
            const std::string sJunk = pick( r, 6 ) == 0 ? "**" : "";
            s += sBases + sJunk + sEnd + ( pick( r, 3 ) ? "+" : "+" + sHeader.substr( 1 ) ) + sEnd;
            std::string sQual;
            for( size_t i = 0; i < n; i++ )
                sQual += (char)( 33 + pick( r, 94 ) );
            if( pick( r, 3 ) == 0 )
                sQual[ 0 ] = "@+> "[ pick( r, 4 ) ];
            if( pick( r, 5 ) == 0 )
                sQual[ n - 1 ] = ' ';
            s += sQual + sEnd;
        }
        else
        {
            const size_t uiLines = 1 + pick( r, 4 );
            size_t uiLeft = n;
            for( size_t l = 0; l < uiLines; l++ )
            {
                const size_t m = l + 1 == uiLines ? uiLeft : pick( r, uiLeft + 1 );
                uiLeft -= m;
                std::string sLine = m ? bases( r, m, pick( r, 4 ) == 0 ) : "";
                if( m && pick( r, 4 ) == 0 )
                    sLine[ 0 ] = "acgtn"[ pick( r, 5 ) ];
                if( m == 0 || pick( r, 4 ) == 0 )
                    sLine += "*-"; // trailing junk; a line of junk only contributes nothing
                s += sLine + sEnd;
            }
        }
    }
    if( pick( r, 3 ) == 0 )
        s.resize( s.size( ) - sEnd.size( ) ); // the last line lacks its end
    return s;
}
static std::string mutant( Rng& r, std::string s )
{
    static const char aBytes[] = { '\n', '\r', ' ', '@', '>', '+', 'A', 'x' };
    for( size_t k = 1 + pick( r, 3 ); k > 0 && !s.empty( ); k-- )
    {
        const size_t at = pick( r, s.size( ) );
        const char c = aBytes[ pick( r, sizeof( aBytes ) ) ];
        switch( pick( r, 3 ) )
        {
            case 0:
                s[ at ] = c;
                break;
            case 1:
                s.insert( s.begin( ) + at, c );
                break;
            default:
                s.erase( s.begin( ) + at );
        }
    }
    return s;
}

static std::string show( const std::string& s )
{
    std::string t;
    for( char c : s.substr( 0, 400 ) )
        t += c == '\n' ? "\\n" : c == '\r' ? "\\r" : std::string( 1, c );
    return t;
}

// ---- modes ----------------------------------------------------------------------------------------------------------------------
static std::vector<Read> refDump( const std::string& sPath, size_t uiFirst, size_t uiStep )
{
    std::vector<Read> v;
    std::ifstream xIn( sPath );
    std::string sLine;
    for( size_t i = 0; std::getline( xIn, sLine ); i++ )
    {
        if( i % uiStep != uiFirst )
            continue;
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
    struct Case
    {
        const char *sFile, *sRef;
        size_t uiFirst, uiStep;
    };
    const Case aAccepted[] = { { "small24.fq", nullptr, 0, 1 }, { "mates_1.fq", "mates.rc0.ref", 0, 2 }, { "mates_2.fq", "mates.rc0.ref", 1, 2 },
                               { "reader_plusname.fq", "reader_plusname.fq.ref", 0, 1 } };
    size_t uiReads = 0;
    for( const Case& c : aAccepted )
    {
        const std::string sText = slurp( sDir + "/" + c.sFile );
        const Parsed h = host( sText ), y = yardstick( sText );
        if( !h.bAccepted || !y.bAccepted || h.vReads != y.vReads || h.vReads.empty( ) )
            return printf( "FAIL %s: %s\n", c.sFile, h.bAccepted ? "differs from the yardstick" : h.sMessage.c_str( ) ), 1;
        if( c.sRef != nullptr )
        {
            const std::vector<Read> vRef = refDump( sDir + "/" + c.sRef, c.uiFirst, c.uiStep );
            // (the paired dump ends with the shorter file: it may hold fewer reads than the longer one)
            if( vRef.empty( ) || vRef.size( ) > h.vReads.size( ) || ( c.uiStep == 1 && vRef.size( ) != h.vReads.size( ) ) )
                return printf( "FAIL %s: %zu reads, the dump has %zu\n", c.sFile, h.vReads.size( ), vRef.size( ) ), 1;
            for( size_t i = 0; i < vRef.size( ); i++ )
                if( vRef[ i ].sName != h.vReads[ i ].sName || vRef[ i ].vCodes != h.vReads[ i ].vCodes ||
                    ( !vRef[ i ].vQual.empty( ) && vRef[ i ].vQual != h.vReads[ i ].vQual ) ) // (a dump without quality column: name, length, codes)
                    return printf( "FAIL %s: read %zu differs from %s\n", c.sFile, i, c.sRef ), 1;
        }
        uiReads += h.vReads.size( );
    }
    size_t uiRefused = 0;
    for( const char* sFile : { "reader_multi.fq", "reader_multi.fa", "reader_empty.fa", "reader_notfasta.txt" } )
    {
        const Parsed h = host( slurp( sDir + "/" + sFile ) );
        if( h.bAccepted )
            return printf( "FAIL %s: accepted\n", sFile ), 1;
        printf( "%s: %s\n", sFile, h.sMessage.c_str( ) );
        uiRefused++;
    }
    printf( "golden ok: %zu reads of 4 files equal, %zu files refused\n", uiReads, uiRefused );
    return 0;
}

static int strict( uint64_t uiSeed, size_t n )
{
    Rng r( uiSeed );
    size_t uiRefused = 0, uiReads = 0;
    for( size_t t = 0; t < n; t++ )
    {
        const std::string sText = strictText( r, t % 2 == 0, t == 7 || t == 8 ? 70000 : 0 );
        const Parsed h = host( sText ), y = yardstick( sText );
        if( !h.bAccepted )
        {
            if( uiRefused++ == 0 )
                printf( "REFUSED text %zu: %s\n%s\n", t, h.sMessage.c_str( ), show( sText ).c_str( ) );
            continue;
        }
        if( !y.bAccepted || h.vReads != y.vReads )
            return printf( "FAIL text %zu differs from the yardstick (%s)\n%s\n", t, y.sMessage.c_str( ), show( sText ).c_str( ) ), 1;
        uiReads += h.vReads.size( );
    }
    printf( "strict %s: %zu texts, %zu reads equal, %zu refused\n", uiRefused ? "FAIL" : "ok", n, uiReads, uiRefused );
    return uiRefused ? 1 : 0;
}

static int mutants( uint64_t uiSeed, size_t n )
{
    Rng r( uiSeed );
    size_t uiAccepted = 0, uiRefused = 0, uiDifferent = 0;
    for( size_t t = 0; t < n; t++ )
    {
        const std::string sText = strictText( r, t % 2 == 0 );
        for( int m = 0; m < 3; m++ )
        {
            const std::string sMutant = mutant( r, sText );
            const Parsed h = host( sMutant );
            if( !h.bAccepted )
            {
                uiRefused++;
                continue;
            }
            uiAccepted++;
            const Parsed y = yardstick( sMutant ); // (an exception of the yardstick: the text had to be refused)
            if( !y.bAccepted || h.vReads != y.vReads )
                if( uiDifferent++ == 0 )
                    printf( "DIFFERENT mutant of text %zu (%s)\n%s\n", t, y.sMessage.c_str( ), show( sMutant ).c_str( ) );
        }
    }
    printf( "mutants %s: %zu accepted, %zu refused, %zu different\n", uiDifferent ? "FAIL" : "ok", uiAccepted, uiRefused, uiDifferent );
    return uiDifferent ? 1 : 0;
}

struct Reason
{
    const char* sWhat;
    std::string sText;
    uint64_t uiLine, uiByte; // 1-based line, offset of its first byte
    uint32_t uiReason;
};
static std::vector<Reason> reasonTable( )
{
    using namespace ma_text;
    return {
        { "lone carriage return", "@r\nAC\rGT\n+\nIIIII\n", 2, 3, ERR_LONE_CR },
        { "carriage return as the last byte", "@r\nACGT\n+\nIIII\r", 4, 10, ERR_LONE_CR },
        { "three lines", "@r\nACGT\n+\n", 3, 8, ERR_FQ_COUNT },
        { "+ line missing", "@r\nACGT\nIIII\n@s\n", 3, 8, ERR_FQ_PLUS },
        { "quality one byte short", "@r\nACGT\n+\nIII\n", 4, 10, ERR_FQ_QUAL_LEN },
        { "quality one byte long", "@r\nACGT\n+\nIIIII\n", 4, 10, ERR_FQ_QUAL_LEN },
        { "sequence of junk only", "@r\n*-*\n+\nIII\n", 2, 3, ERR_SEQ_NO_BASES },
        { "sequence starting with @", "@r\n@CGT\n+\nIIII\n", 2, 3, ERR_SEQ_START },
        { "FASTA header followed by header", ">a\nACGT\n>b\n>c\nAC\n", 3, 8, ERR_FA_NO_BASES },
        { "blank-led line", ">a\nAC\n GT\n", 3, 6, ERR_SEQ_START },
        { "first byte A", "ACGT\n", 1, 0, ERR_KIND },
        { "FASTQ header missing", "@r\nAC\n+\nII\nr\nAC\n+\nII\n", 5, 11, ERR_FQ_HEADER },
        { "empty sequence line", "@r\n\n+\n\n", 2, 3, ERR_SEQ_EMPTY },
        { "empty FASTA line", ">a\nAC\n\nGT\n", 3, 6, ERR_SEQ_EMPTY },
        { "FASTA ends with a header", ">a\nAC\n>b\n", 3, 6, ERR_FA_NO_BASES },
        { "two violations: the lower line", "@r\nACGT\n+\nIII\n@s\n+CGT\n+\nIIII\n", 4, 10, ERR_FQ_QUAL_LEN },
    };
}
static int reasons( bool bPrint )
{
    for( const Reason& x : reasonTable( ) )
    {
        const Parsed h = host( x.sText );
        char aWant[ 256 ];
        ma_text::message( aWant, sizeof( aWant ), x.uiLine - 1, x.uiByte, x.uiReason );
        if( bPrint ) // the table for the GPU test: the text in hex, then the message
        {
            for( unsigned char c : x.sText )
                printf( "%02x", c );
            printf( " %s\n", aWant );
            continue;
        }
        if( h.bAccepted || h.sMessage != aWant )
            return printf( "FAIL %s: '%s', expected '%s'\n", x.sWhat, h.bAccepted ? "accepted" : h.sMessage.c_str( ), aWant ), 1;
        if( strncmp( aWant, "ma_batch_set_reads_text: line ", 30 ) != 0 )
            return printf( "FAIL wording: %s\n", aWant ), 1;
    }
    if( !bPrint )
        printf( "reasons ok: %zu texts\n", reasonTable( ).size( ) );
    return 0;
}

static bool recordStart( const std::string& s )
{
    return !s.empty( ) && ( s[ 0 ] == '@' || s[ 0 ] == '>' );
}
static int cutOne( const std::string& sWhat, const std::string& sText, std::shared_ptr<FileStream> pStream, size_t uiBlock )
{
    BatchTextReader xReader{ ParameterSetManager( ) };
    xReader.uiBatchBytes = uiBlock;
    std::string sAll;
    std::vector<Read> vAll;
    size_t uiBatches = 0;
    while( auto pBatch = xReader.execute( pStream ) )
    {
        if( !recordStart( pBatch->sText ) )
            return printf( "FAIL %s: batch %zu does not start at a record\n", sWhat.c_str( ), uiBatches ), 1;
        const Parsed h = host( pBatch->sText );
        if( !h.bAccepted )
            return printf( "FAIL %s: batch %zu refused: %s\n", sWhat.c_str( ), uiBatches, h.sMessage.c_str( ) ), 1;
        vAll.insert( vAll.end( ), h.vReads.begin( ), h.vReads.end( ) );
        sAll += pBatch->sText;
        uiBatches++;
    }
    if( sAll != sText )
        return printf( "FAIL %s: the batches do not concatenate to the file\n", sWhat.c_str( ) ), 1;
    const Parsed y = yardstick( sText );
    if( !y.bAccepted || vAll != y.vReads )
        return printf( "FAIL %s: the batches' reads differ from the yardstick's\n", sWhat.c_str( ) ), 1;
    printf( "%s: %zu batches, %zu reads\n", sWhat.c_str( ), uiBatches, vAll.size( ) );
    return 0;
}
static int cut( size_t uiBlock, const std::string& sFastq )
{
    Rng r( 20261019 );
    std::string sFasta;
    for( int k = 0; k < 6; k++ )
    {
        std::string s = strictText( r, false );
        if( s.back( ) != '\n' )
            s += '\n';
        sFasta += s;
    }
    const std::string sText = slurp( sFastq );
    auto pFile = std::make_shared<StdFileStream>( sFastq );
    pFile->uiBlockBytes = 5; // (the stream's own block: a batch takes what is left of one and goes on with the source)
    if( cutOne( "file", sText, pFile, uiBlock ) || cutOne( "string", sText, std::make_shared<StringStream>( sText ), uiBlock ) ||
        cutOne( "fasta", sFasta, std::make_shared<StringStream>( sFasta ), uiBlock ) )
        return 1;
    // a stream that was read by lines before hands over the rest of its block first
    auto pMixed = std::make_shared<StdFileStream>( sFastq );
    pMixed->uiBlockBytes = 64;
    auto pFirst = FileReader::parseRecord( *pMixed );
    std::string sRest;
    while( !pMixed->eof( ) )
        pMixed->readBlock( sRest, uiBlock );
    const Parsed yAll = yardstick( sText ), yRest = yardstick( sRest );
    if( pFirst == nullptr || !yRest.bAccepted || yRest.vReads.size( ) + 1 != yAll.vReads.size( ) ||
        !std::equal( yRest.vReads.begin( ), yRest.vReads.end( ), yAll.vReads.begin( ) + 1 ) )
        return printf( "FAIL: a block read behind a line read does not continue where it stopped\n" ), 1;
    // a stream without block reads (as a gzip stream is): the reader throws and names the reader that serves it
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
        BatchTextReader xReader{ ParameterSetManager( ) };
        xReader.execute( std::make_shared<NoBlockStream>( sText ) );
        return printf( "FAIL: a stream without block reads was read\n" ), 1;
    }
    catch( const std::runtime_error& rE )
    {
        if( std::string( rE.what( ) ).find( "BatchFileReader" ) == std::string::npos )
            return printf( "FAIL: '%s' does not name BatchFileReader\n", rE.what( ) ), 1;
    }
    printf( "cut ok: block %zu\n", uiBlock );
    return 0;
}

static int dump( int argc, char** argv )
{
    for( int k = 2; k < argc; k++ )
    {
        const std::string sText = slurp( argv[ k ] );
        const Parsed h = host( sText );
        if( !h.bAccepted )
        {
            printf( "ERR %s\n", h.sMessage.c_str( ) );
            continue;
        }
        const Parsed y = yardstick( sText );
        printf( "OK %zu %d %s\n", h.vReads.size( ), (int)h.xResult.iHasQual, y.bAccepted && y.vReads == h.vReads ? "same" : "different" );
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
        if( sMode == "strict" && argc > 3 )
            return strict( strtoull( argv[ 2 ], nullptr, 10 ), (size_t)atol( argv[ 3 ] ) );
        if( sMode == "mutants" && argc > 3 )
            return mutants( strtoull( argv[ 2 ], nullptr, 10 ), (size_t)atol( argv[ 3 ] ) );
        if( sMode == "reasons" )
            return reasons( argc > 2 && std::string( argv[ 2 ] ) == "print" );
        if( sMode == "cut" && argc > 3 )
            return cut( (size_t)atol( argv[ 2 ] ), argv[ 3 ] );
        if( sMode == "dump" )
            return dump( argc, argv );
        fprintf( stderr, "usage: text_dev_test golden <dir> | strict <seed> <n> | mutants <seed> <n> | reasons [print] | cut <bytes> <fq> | dump <file>...\n" );
        return 2;
    }
    catch( const std::exception& rE )
    {
        printf( "EXCEPTION %s\n", rE.what( ) );
        return 3;
    }
}
