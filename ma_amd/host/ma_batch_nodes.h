// ma_batch_nodes.h -- the THROUGHPUT form of the path as graph nodes (adaptor (i)): modules whose containers are
// whole batches, so that reader -> aligner -> writer runs under promiseMe / BasePledge::simultaneousGet like the per-read
// chain of libMA::setUpCompGraph (export.cpp:84-126) does, with a handful of graph threads instead of thousands:
//
//   BatchFileReader : Module<ReadVector, true,  FileStream>                 up to uiBatchReads reads per call, nullptr = EoF
//   BatchAlign      : Module<AlignedBatch, false, FMIndex, ReadVector>      one device batch through ALL stages; the result
//                                                                           stays FLAT (one header + one ops array)
//   BatchFileWriter : Module<Container, false, ReadVector, AlignedBatch, Pack>   SAM text of the batch formatted from the
//                                                                           flat view into byte arenas, ONE write per batch
//
// ReadVector = ContainerVector<shared_ptr<NucSeq>> -- the reference's own way of passing many containers at once
// (needlemanWunsch.h:51-52 takes ContainerVector<shared_ptr<Seeds>>; BinarySeeding::seed takes a vector of queries,
// binarySeeding.h:575-584).  Every graph thread that calls BatchAlign::execute gets its own engine (stream + device batch),
// so the number of graph threads IS the number of device batches in flight.
#pragma once
#include "ma_bgzf_dev.h"
#include "ma_flat_sam.h"
#include "ma_sam.h"
#include <atomic>
#include <thread>

namespace libMA
{
class BatchAlign : public libMS::Module<AlignedBatch, false, FMIndex, ReadVector>
{
    const ma_params xP;
    std::mutex xMutex;
    // engines whose graph thread is between two batches, with the index they are bound to (an engine's ma_batch belongs to ONE
    // ma_index: reusing it for another genome would align against the first one)
    std::vector<std::pair<const ma_index*, std::unique_ptr<detail::Engine>>> vIdle;
    std::mutex xPrimeMutex; // first batches of new engines run one at a time (they allocate GBs and page-lock memory)
    std::atomic<size_t> uiTurn{ 0 }; // which replica of the index takes the next batch

  public:
    // seconds summed over all batches (phases of different batches overlap when several graph threads are at work)
    std::atomic<uint64_t> uiBatches{ 0 }, uiReads{ 0 }, uiAligned{ 0 };
    double fPack = 0, fH2D = 0, fKernels = 0, fD2H = 0;

    BatchAlign( const ParameterSetManager& rParameters ) : xP( *rParameters.getSelected( ) )
    {}

    virtual std::shared_ptr<AlignedBatch> execute( std::shared_ptr<FMIndex> pFM_index, std::shared_ptr<ReadVector> pReads ) override
    {
        auto pRet = std::make_shared<AlignedBatch>( );
        pRet->pReads = pReads;
        pRet->uiFirst = 0;
        // device batches rotate over the replicas of the index (DeviceIndex::vReplicas: one per GPU of the node):
        // the graph of reader -> BatchAlign -> writer stays as it is and feeds all of them
        const ma_index* pIndex = pFM_index->pDev->p;
        if( !pFM_index->pDev->vReplicas.empty( ) )
        {
            const size_t k = uiTurn.fetch_add( 1 ) % ( pFM_index->pDev->vReplicas.size( ) + 1 );
            if( k > 0 )
                pIndex = pFM_index->pDev->vReplicas[ k - 1 ]->p;
        }
        std::unique_ptr<detail::Engine> pEngine;
        {
            std::lock_guard<std::mutex> xGuard( xMutex );
            for( size_t k = 0; k < vIdle.size( ); k++ )
                if( vIdle[ k ].first == pIndex )
                {
                    pEngine = std::move( vIdle[ k ].second );
                    vIdle.erase( vIdle.begin( ) + k );
                    break;
                }
        }
        std::vector<detail::ReadRef> vRefs;
        vRefs.reserve( pReads->size( ) );
        for( const auto& pQ : *pReads )
            vRefs.emplace_back( pQ->xCodes );
        try
        {
            if( pEngine == nullptr || !pEngine->primed( vRefs.size( ) ) )
            {
                // engines before admission: the graph threads all arrive at once at the start of a run; their engines are
                // created and run their first batch one after the other instead of racing for the allocator and the page-locker
                std::lock_guard<std::mutex> xPrime( xPrimeMutex );
                if( pEngine == nullptr )
                    pEngine.reset( new detail::Engine( pIndex, xP ) );
                pRet->pResult = pEngine->run( vRefs, false );
            }
            else
                pRet->pResult = pEngine->run( vRefs, false );
        }
        catch( ... )
        {
            if( pEngine != nullptr )
            {
                std::lock_guard<std::mutex> xGuard( xMutex );
                vIdle.emplace_back( pIndex, std::move( pEngine ) );
            }
            throw;
        }
        std::lock_guard<std::mutex> xGuard( xMutex );
        vIdle.emplace_back( pIndex, std::move( pEngine ) );
        uiBatches++, uiReads += pReads->size( ), uiAligned += pRet->pResult->uiAlignedReads;
        fPack += pRet->pResult->fPack, fH2D += pRet->pResult->fH2D, fKernels += pRet->pResult->fKernels, fD2H += pRet->pResult->fD2H;
        return pRet;
    }
};

// Volatile source of batches out of a FASTA / FASTQ stream: the records are parsed exactly like FileReader does it
// (fileReader.cpp:37-203), up to uiBatchReads of them under ONE acquisition of the stream's lock.
class BatchFileReader : public libMS::Module<ReadVector, true, FileStream>
{
    std::atomic<size_t> uiLastBatchBytes{ 0 }; // text of the previous batch: the next one reserves that much up front

  public:
    size_t uiBatchReads = 1u << 18;
    BatchFileReader( const ParameterSetManager& )
    {}
    virtual std::shared_ptr<ReadVector> execute( std::shared_ptr<FileStream> pStream ) override
    {
        auto pRet = std::make_shared<ReadVector>( );
        std::string sRecords; // the text of the batch, cut out of the stream under its lock ...
        sRecords.reserve( uiLastBatchBytes + uiLastBatchBytes / 8 );
        size_t uiRecords = 0;
        {
            std::lock_guard<std::mutex> xLock( pStream->xMutex );
            const bool bCut = pStream->capture( &sRecords );
            try
            {
                while( pRet->size( ) + uiRecords < uiBatchReads )
                {
                    if( bCut )
                    {
                        if( !FileReader::skipRecord( *pStream ) )
                            break;
                        uiRecords++;
                    }
                    else if( auto pQ = FileReader::parseRecord( *pStream ) ) // a stream that cannot be cut: parse in place
                        pRet->push_back( pQ );
                    else
                        break;
                }
            }
            catch( ... )
            {
                pStream->capture( nullptr );
                throw;
            }
            pStream->capture( nullptr );
        }
        // ... and turned into reads outside of it, while the next graph thread cuts its batch
        if( uiRecords > 0 )
        {
            uiLastBatchBytes = sRecords.size( );
            StringStream xText( std::move( sRecords ) );
            pRet->reserve( uiRecords );
            while( auto pQ = FileReader::parseRecord( xText ) )
                pRet->push_back( pQ );
        }
        if( pRet->empty( ) )
            return nullptr; // end of file (module.h:688-695)
        return pRet;
    }
};

// Volatile source of batches of TEXT out of a FASTA / FASTQ stream, for the device's parser (BatchAligner::executeTextSam):
// about uiBatchBytes are read as a block under the stream's lock, the batch ends before the last record start in the block
// and the tail is carried to the next call.  No line is walked but the last few of a block.  A record start is
//   FASTQ  a line that starts with '@' whose next-but-one line starts with '+'
//   FASTA  a line that starts with '>'
// (the kind is that of the block's first byte).  In strict text (ma_text_dev.h) the cut is exact: a quality line that starts
// with '@' is followed by a header and then by bases, which may not start with '+'.  In any other text the device's check
// refuses the batch: a batch that starts at a record start and passes was consumed line by line as the reference consumes
// it, so the next batch starts at a record start too.  A block without a record start grows; at the end of the stream the rest
// is the batch.  A stream without block reads (gzip) throws: BatchFileReader serves it.
class BatchTextReader : public libMS::Module<TextBatch, true, FileStream>
{
    std::string sCarry; // the tail of the last block (guarded by the stream's lock)

  public:
    size_t uiBatchBytes = 64u << 20;
    BatchTextReader( const ParameterSetManager& )
    {}
    // offset of the last record start of rText behind offset 0, 0 if there is none
    static size_t lastRecordStart( const std::string& rText )
    {
        if( rText.empty( ) || ( rText[ 0 ] != '@' && rText[ 0 ] != '>' ) )
            return 0;
        const bool bFastq = rText[ 0 ] == '@';
        size_t uiNext = std::string::npos, uiNextButOne = std::string::npos; // starts of the two lines behind the one looked at
        for( size_t uiEnd = rText.size( ); uiEnd > 0; )
        {
            const void* const pFeed = memrchr( rText.data( ), '\n', uiEnd );
            if( pFeed == nullptr )
                break;
            const size_t uiStart = (size_t)( (const char*)pFeed - rText.data( ) ) + 1;
            if( uiStart < rText.size( ) )
            {
                if( bFastq ? rText[ uiStart ] == '@' && uiNextButOne != std::string::npos && rText[ uiNextButOne ] == '+' : rText[ uiStart ] == '>' )
                    return uiStart;
                uiNextButOne = uiNext;
                uiNext = uiStart;
            }
            uiEnd = uiStart - 1;
        }
        return 0;
    }
    virtual std::shared_ptr<TextBatch> execute( std::shared_ptr<FileStream> pStream ) override
    {
        auto pRet = std::make_shared<TextBatch>( );
        std::string& rText = pRet->sText;
        const size_t uiWant = std::max<size_t>( uiBatchBytes, 1 );
        {
            std::lock_guard<std::mutex> xLock( pStream->xMutex );
            rText.reserve( sCarry.size( ) + uiWant );
            rText.swap( sCarry );
            sCarry.clear( );
            for( size_t uiAsk = rText.size( ) < uiWant ? uiWant - rText.size( ) : uiWant;; uiAsk = uiWant )
            {
                if( !pStream->readBlock( rText, uiAsk ) )
                    throw std::runtime_error( "BatchTextReader: the stream " + pStream->fileName( ) +
                                              " has no block reads (compressed input?): read it with BatchFileReader" );
                if( pStream->eof( ) )
                    break; // the rest is the batch
                const size_t uiCut = lastRecordStart( rText );
                if( uiCut > 0 )
                {
                    sCarry.assign( rText, uiCut, std::string::npos );
                    rText.resize( uiCut );
                    break;
                }
                if( rText[ 0 ] != '@' && rText[ 0 ] != '>' )
                    break; // neither kind: the device refuses the block as it is
            }
        }
        if( rText.empty( ) )
            return nullptr; // end of file (module.h:688-695)
        return pRet;
    }
};

// BatchTextReader over the COMPRESSED bytes of a BGZF file (what bgzip and htslib write: a chain of independent gzip members, the
// strict form of ma_bgzf_dev.h), the source of BatchAligner::executeBgzfSam.  About uiBatchBytes of the file are read as a block
// behind the carried compressed tail, under the stream's lock, and cut at the last whole member by walking the member headers;
// the rest is carried.  The text is not inflated here but for the LAST member(s): BatchTextReader::lastRecordStart is local and
// exact in strict text, so the last record start of the chunk's text is found in the text of its last member, or of its last
// two, ... -- one member more while none is found, with the carried head when the walk goes all the way back.  The batch is
//   sHead     the text carried from the last batch (what lay behind its cut)
//   sMembers  the members up to and including the one that holds the cut
//   uiDrop    the bytes of that member's text behind the cut: they become the next batch's sHead
// and the members behind that one are carried as they are.  No batch waits for anything the device makes of the one before it.
// At the end of the file the rest is the batch, uiDrop = 0.  A chunk without a record start grows.  A stream that is not BGZF
// -- plain gzip has no size field in its header -- throws with the reason's text, which names GzFileStream.  No zlib.
// (The cut of ONE stream is BgzfStreamCutter: BatchBgzfReader has one, BatchPairedBgzfReader one per file.)
struct BgzfStreamCutter
{
    std::string sCarry, sHeadCarry; // compressed bytes and text behind the last cut (guarded by the stream's lock)
    char cKind = '\0'; // the first byte of the file's text
    uint64_t uiCompressed = 0, uiText = 0; // of the members handed out so far: the stream's running ISIZE-to-compressed ratio

    [[noreturn]] static void refuse( FileStream& rStream, const std::string& sWhat, uint32_t uiReason )
    {
        throw std::runtime_error( "BatchBgzfReader: the stream " + rStream.fileName( ) + ": " + sWhat + ": " + ma_bgzf::errorText( uiReason ) );
    }
    // the text of member rM of rData behind rText
    static void inflateBehind( FileStream& rStream, const std::string& rData, const ma_bgzf::Member& rM, std::string& rText )
    {
        const size_t uiOld = rText.size( );
        rText.resize( uiOld + rM.uiIsize );
        const uint32_t uiReason = ma_bgzf::inflateMember( (const uint8_t*)rData.data( ), rM, (uint8_t*)&rText[ uiOld ] );
        if( uiReason != ma_bgzf::OK )
            refuse( rStream, "the member at byte " + std::to_string( rM.uiIn ) + " of a chunk", uiReason );
    }
    // the members of rBatch are handed out
    void count( const std::string& rData )
    {
        ma_bgzf::Result xWalk;
        ma_bgzf::inflateHost( (const uint8_t*)rData.data( ), rData.size( ), nullptr, &xWalk );
        uiCompressed += rData.size( ), uiText += xWalk.uiBytes;
    }
    // The next batch of the stream, whose lock the caller holds: about uiWant compressed bytes, the carried ones included.
    // False: the end of the file, nothing is left.
    bool cut( const std::shared_ptr<FileStream>& pStream, size_t uiWant, BgzfBatch* pRet )
    {
        std::string& rData = pRet->sMembers;
        rData.reserve( sCarry.size( ) + uiWant );
        rData.swap( sCarry );
        sCarry.clear( );
        pRet->sHead.swap( sHeadCarry );
        sHeadCarry.clear( );
        std::vector<ma_bgzf::Member> vMembers; // the whole members of rData, which end at uiWalked
        size_t uiWalked = 0;
        // (a chunk that has to grow doubles: every attempt inflates its last members again)
        for( size_t uiAsk = rData.size( ) < uiWant ? uiWant - rData.size( ) : uiWant;; uiAsk = std::max( uiWant, rData.size( ) ) )
        {
            if( !pStream->readBlock( rData, uiAsk ) )
                throw std::runtime_error( "BatchBgzfReader: the stream " + pStream->fileName( ) + " has no block reads" );
            while( uiWalked < rData.size( ) )
            {
                ma_bgzf::Member xM;
                const uint32_t uiReason = ma_bgzf::header( (const uint8_t*)rData.data( ), rData.size( ), uiWalked, &xM );
                if( uiReason == ma_bgzf::ERR_TRUNCATED && !pStream->eof( ) )
                    break; // the rest of the member comes with the next block
                if( uiReason != ma_bgzf::OK )
                    refuse( *pStream, "the member at byte " + std::to_string( uiWalked ) + " of a chunk", uiReason );
                vMembers.push_back( xM );
                uiWalked += xM.uiBytes;
            }
            if( cKind == '\0' ) // the first byte of the file's text tells FASTQ from FASTA
                for( size_t i = 0; i < vMembers.size( ) && cKind == '\0'; i++ )
                    if( vMembers[ i ].uiIsize > 0 )
                    {
                        std::string sFirst;
                        inflateBehind( *pStream, rData, vMembers[ i ], sFirst );
                        cKind = sFirst[ 0 ];
                    }
            if( pStream->eof( ) )
                break; // the rest is the batch
            if( cKind != '\0' && cKind != '@' && cKind != '>' )
                break; // neither kind: the device refuses the chunk as it is
            // the last record start of the chunk's text, looked for in the text of its last members
            std::string sTail;
            size_t uiFrom = vMembers.size( ), uiCut = 0; // sTail: the text of members uiFrom .. ; uiCut: offset of the cut in it
            while( uiFrom > 0 && uiCut == 0 )
            {
                std::string sOne;
                inflateBehind( *pStream, rData, vMembers[ --uiFrom ], sOne );
                sTail.insert( 0, sOne );
                if( uiFrom > 0 || pRet->sHead.empty( ) )
                {
                    // (the rule reads the kind off the first byte and looks at line starts behind offset 0 only)
                    const size_t uiAt = BatchTextReader::lastRecordStart( std::string( 1, cKind ) + sTail );
                    uiCut = uiAt > 0 ? uiAt - 1 : 0;
                }
            }
            size_t uiHeadKept = pRet->sHead.size( );
            if( uiCut == 0 && !vMembers.empty( ) && !pRet->sHead.empty( ) )
            {
                const size_t uiAt = BatchTextReader::lastRecordStart( pRet->sHead + sTail );
                if( uiAt >= pRet->sHead.size( ) )
                    uiCut = uiAt - pRet->sHead.size( ); // (0: exactly behind the head)
                else if( uiAt > 0 )
                    uiHeadKept = uiAt; // inside the head: the batch is the head's front, no member
                if( uiAt == 0 )
                    continue; // no record start yet: the chunk grows
            }
            else if( uiCut == 0 )
                continue;
            // members uiFrom .. uiLast - 1 hold the text before the cut
            size_t uiLast = uiFrom, uiBefore = 0; // uiBefore: text of sTail before member uiLast
            if( uiHeadKept == pRet->sHead.size( ) )
                while( uiLast < vMembers.size( ) && uiBefore < uiCut )
                    uiBefore += vMembers[ uiLast++ ].uiIsize;
            else
                uiLast = 0;
            const size_t uiKeep = uiLast > 0 ? (size_t)( vMembers[ uiLast - 1 ].uiIn + vMembers[ uiLast - 1 ].uiBytes ) : 0;
            if( uiHeadKept < pRet->sHead.size( ) )
            {
                sHeadCarry.assign( pRet->sHead, uiHeadKept, std::string::npos );
                pRet->sHead.resize( uiHeadKept );
            }
            else
            {
                pRet->uiDrop = uiBefore - uiCut;
                sHeadCarry.assign( sTail, uiCut, pRet->uiDrop );
            }
            sCarry.assign( rData, uiKeep, std::string::npos );
            rData.resize( uiKeep );
            count( rData );
            return true;
        }
        if( uiWalked != rData.size( ) ) // (never at the end of the file: a truncated member is refused there)
        {
            sCarry.assign( rData, uiWalked, std::string::npos );
            rData.resize( uiWalked );
        }
        bool bText = !pRet->sHead.empty( );
        for( const ma_bgzf::Member& rM : vMembers )
            bText = bText || rM.uiIsize > 0;
        count( rData );
        return bText;
    }
};
class BatchBgzfReader : public libMS::Module<BgzfBatch, true, FileStream>
{
    BgzfStreamCutter xCutter;

  public:
    size_t uiBatchBytes = 16u << 20; // of the compressed file
    BatchBgzfReader( const ParameterSetManager& )
    {}
    // the text of a batch, inflated on the host (tests, and callers without a device)
    static std::string textOf( const BgzfBatch& rBatch )
    {
        ma_bgzf::Result xResult;
        const uint8_t* const pData = (const uint8_t*)rBatch.sMembers.data( );
        char aMessage[ 320 ];
        if( ma_bgzf::inflateHost( pData, rBatch.sMembers.size( ), nullptr, &xResult ) == 0 )
        {
            std::string sText( xResult.uiBytes, '\0' );
            if( ma_bgzf::inflateHost( pData, rBatch.sMembers.size( ), (uint8_t*)&sText[ 0 ], &xResult ) == 0 && rBatch.uiDrop <= sText.size( ) )
            {
                sText.resize( sText.size( ) - rBatch.uiDrop );
                return rBatch.sHead + sText;
            }
        }
        ma_bgzf::message( aMessage, sizeof( aMessage ), xResult.uiMember, xResult.uiByte, xResult.uiReason );
        throw std::runtime_error( aMessage );
    }
    virtual std::shared_ptr<BgzfBatch> execute( std::shared_ptr<FileStream> pStream ) override
    {
        auto pRet = std::make_shared<BgzfBatch>( );
        std::lock_guard<std::mutex> xLock( pStream->xMutex );
        if( !xCutter.cut( pStream, std::max<size_t>( uiBatchBytes, 1 ), pRet.get( ) ) )
            return nullptr; // end of file (module.h:688-695)
        return pRet;
    }
};

// BatchTextReader for mate pairs, the source of BatchAligner::executePairedTextSam: about half of uiBatchBytes are read from each
// of the two streams under the pair stream's lock and cut at BatchTextReader::lastRecordStart; then the two record counts are made
// equal on the host, so that a batch always holds whole pairs (ma_batch_set_mates_text consumes both texts entirely).  Records
// are counted at memchr speed -- FASTQ: lines / 4, FASTA: lines that start with '>' -- and the surplus of the block with more of
// them is moved to that stream's carry by walking back from the block's end.  When the stream with fewer records is at its end
// the rests go out as they are and the pair stream ends: the device drops the surplus records, as PairedFileReader does
// (fileReader.h:590-600).  In text that is not strict the counts mean nothing and the device refuses the batch.  A stream
// without block reads (gzip) throws: PairedFileReader serves it.
class BatchPairedTextReader : public libMS::Module<MatesTextBatch, true, PairedFileStream>
{
    std::string asCarry[ 2 ]; // the tails of the last blocks (guarded by the pair stream's lock)
    bool bDone = false; // one of the streams has ended

  public:
    size_t uiBatchBytes = 64u << 20;
    BatchPairedTextReader( const ParameterSetManager& )
    {}
    // records of a run of whole records
    static size_t countRecords( const std::string& rText )
    {
        if( rText.empty( ) )
            return 0;
        const bool bFastq = rText[ 0 ] == '@';
        size_t uiLines = 0, uiHeaders = rText[ 0 ] == '>' ? 1 : 0;
        const char *p = rText.data( ), *const pEnd = p + rText.size( );
        while( const char* pFeed = (const char*)memchr( p, '\n', (size_t)( pEnd - p ) ) )
        {
            uiLines++;
            p = pFeed + 1;
            if( p < pEnd && *p == '>' )
                uiHeaders++;
        }
        if( p < pEnd )
            uiLines++; // the last line lacks its end
        return bFastq ? uiLines / 4 : uiHeaders;
    }
    // offset at which the last uiRecords records of a run of whole records start (0: it has no more than that)
    static size_t startOfLastRecords( const std::string& rText, size_t uiRecords )
    {
        const bool bFastq = !rText.empty( ) && rText[ 0 ] == '@';
        size_t uiNeed = bFastq ? 4 * uiRecords : uiRecords, uiEnd = rText.size( );
        if( uiEnd > 0 && rText[ uiEnd - 1 ] == '\n' )
            uiEnd--;
        while( uiNeed > 0 )
        {
            const void* const pFeed = uiEnd > 0 ? memrchr( rText.data( ), '\n', uiEnd ) : nullptr;
            const size_t uiStart = pFeed != nullptr ? (size_t)( (const char*)pFeed - rText.data( ) ) + 1 : 0;
            if( bFastq || rText[ uiStart ] == '>' )
                uiNeed--;
            if( uiStart == 0 || uiNeed == 0 )
                return uiStart;
            uiEnd = uiStart - 1;
        }
        return rText.size( );
    }
    virtual std::shared_ptr<MatesTextBatch> execute( std::shared_ptr<PairedFileStream> pStreams ) override
    {
        auto pRet = std::make_shared<MatesTextBatch>( );
        std::string* const apText[ 2 ] = { &pRet->sText1, &pRet->sText2 };
        const std::shared_ptr<FileStream> apStream[ 2 ] = { pStreams->first, pStreams->second };
        const size_t uiWant = std::max<size_t>( uiBatchBytes / 2, 1 );
        std::lock_guard<std::mutex> xLock( pStreams->xMutex );
        if( bDone )
            return nullptr;
        bool abEnd[ 2 ] = { false, false };
        for( int i = 0; i < 2; i++ )
        {
            std::string& rText = *apText[ i ];
            rText.reserve( asCarry[ i ].size( ) + uiWant );
            rText.swap( asCarry[ i ] );
            asCarry[ i ].clear( );
            for( size_t uiAsk = rText.size( ) < uiWant ? uiWant - rText.size( ) : uiWant;; uiAsk = uiWant )
            {
                if( !apStream[ i ]->readBlock( rText, uiAsk ) )
                    throw std::runtime_error( "BatchTextReader: the stream " + apStream[ i ]->fileName( ) +
                                              " has no block reads (compressed input?): read it with BatchFileReader" );
                if( apStream[ i ]->eof( ) )
                {
                    abEnd[ i ] = true; // the rest is the batch
                    break;
                }
                const size_t uiCut = BatchTextReader::lastRecordStart( rText );
                if( uiCut > 0 )
                {
                    asCarry[ i ].assign( rText, uiCut, std::string::npos );
                    rText.resize( uiCut );
                    break;
                }
                if( rText[ 0 ] != '@' && rText[ 0 ] != '>' )
                    break; // neither kind: the device refuses the block as it is
            }
        }
        if( apText[ 0 ]->empty( ) || apText[ 1 ]->empty( ) )
        {
            bDone = true;
            return nullptr; // the shorter file ends the pair stream (module.h:688-695)
        }
        const size_t auiRecords[ 2 ] = { countRecords( *apText[ 0 ] ), countRecords( *apText[ 1 ] ) };
        const int iFewer = auiRecords[ 0 ] <= auiRecords[ 1 ] ? 0 : 1, iMore = 1 - iFewer;
        if( abEnd[ iFewer ] )
            bDone = true; // the rests as they are: the device drops the surplus
        else if( auiRecords[ iMore ] > auiRecords[ iFewer ] )
        {
            std::string& rText = *apText[ iMore ];
            const size_t uiCut = startOfLastRecords( rText, auiRecords[ iMore ] - auiRecords[ iFewer ] );
            if( uiCut > 0 ) // (0: text that is not strict; the device refuses it)
            {
                asCarry[ iMore ].insert( 0, rText, uiCut, std::string::npos );
                rText.resize( uiCut );
            }
        }
        return pRet;
    }
};

// BatchBgzfReader for mate pairs, the source of BatchAligner::executePairedBgzfSam: the COMPRESSED bytes of the two BGZF files of a
// paired-end run.  Each stream is cut as BatchBgzfReader cuts its stream (BgzfStreamCutter: whole members, only the last ones
// inflated to find the last record start, the bytes behind the cut dropped and carried).  The member borders of two files say
// nothing about record counts, and equal counts cannot be had on the host without inflating everything, so the two texts of a
// batch hold whatever they hold: the device pairs min( R1, R2 ) records and the batch hands back what it left over of either
// text (MatesBgzfBatch::handBack, two strings: a test drives it with ma_bgzf::pairBgzfHost).  Batch k + 1's head of stream i is
// rest_i( k ) followed by the bytes dropped at batch k's cut, so execute( ) for batch k + 1 waits, under the pair stream's lock,
// until batch k's rests are back: the set calls of consecutive batches are serial, everything behind them overlaps.  A batch
// destroyed without having handed back releases the wait, and that execute( ) and every later one throw.
// THE CARRY STAYS BOUNDED although one stream may pack more records into a compressed byte than the other: each stream is
// asked for only as many compressed bytes as bring ITS text, head included, to uiBatchBytes / 2, by the stream's running
// ISIZE-to-compressed ratio (the first batch, with no ratio yet, takes what it needs for one record start).  The stream that
// is ahead then reads little or nothing until the other has caught up.  The pair stream ends when a stream has nothing left:
// the one with fewer records is at its end, the other's surplus was dropped by the device, as PairedFileReader drops it
// (fileReader.h:590-600).  A stream that is not BGZF throws BatchBgzfReader's message.
class BatchPairedBgzfReader : public libMS::Module<MatesBgzfBatch, true, PairedFileStream>
{
    BgzfStreamCutter axCutter[ 2 ]; // (guarded by the pair stream's lock)
    const std::shared_ptr<MatesRestLink> pLink = std::make_shared<MatesRestLink>( );
    bool bDone = false; // one of the streams has ended

  public:
    // of text, both streams together.  Measured, not the single-end default: the set calls of consecutive batches are serial and
    // an inflate costs about the same for few members as for many, so a larger batch is cheaper per read (1 M mates of 150 bp,
    // three workers: 0.51 M reads/s at 20 MB, 1.76 M at 82 MB, 2.42 M at 164 MB; profiles/pair_bgzf_device.md)
    size_t uiBatchBytes = 160u << 20;
    BatchPairedBgzfReader( const ParameterSetManager& )
    {}
    virtual std::shared_ptr<MatesBgzfBatch> execute( std::shared_ptr<PairedFileStream> pStreams ) override
    {
        const std::shared_ptr<FileStream> apStream[ 2 ] = { pStreams->first, pStreams->second };
        std::lock_guard<std::mutex> xLock( pStreams->xMutex );
        {
            std::unique_lock<std::mutex> xWait( pLink->xMutex );
            pLink->xCondition.wait( xWait, [ & ] { return !pLink->bPending; } );
            if( pLink->bAbandoned )
                throw std::runtime_error( "BatchPairedBgzfReader: a batch was destroyed without handing back its rests (its worker failed, or the "
                                          "caller dropped it): the records behind it cannot be paired" );
            for( int i = 0; i < 2; i++ )
            {
                axCutter[ i ].sHeadCarry.insert( 0, pLink->asRest[ i ] );
                pLink->asRest[ i ].clear( );
            }
        }
        if( bDone )
            return nullptr;
        auto pRet = std::make_shared<MatesBgzfBatch>( );
        const size_t uiTarget = std::max<size_t>( uiBatchBytes / 2, 1 );
        for( int i = 0; i < 2; i++ )
        {
            BgzfStreamCutter& rCutter = axCutter[ i ];
            const size_t uiHead = rCutter.sHeadCarry.size( ), uiNeed = uiTarget > uiHead ? uiTarget - uiHead : 0;
            const size_t uiWant = rCutter.uiText == 0 ? 1 : (size_t)( (double)uiNeed * (double)rCutter.uiCompressed / (double)rCutter.uiText );
            BgzfBatch xSide;
            const size_t uiHeadCut = uiNeed == 0 ? BatchTextReader::lastRecordStart( rCutter.sHeadCarry ) : 0;
            if( uiHeadCut > 0 )
            {
                // this stream is ahead: its batch is the whole records of what it carries, and nothing is read
                xSide.sHead.assign( rCutter.sHeadCarry, 0, uiHeadCut );
                rCutter.sHeadCarry.erase( 0, uiHeadCut );
            }
            else if( !rCutter.cut( apStream[ i ], std::max<size_t>( uiWant, 1 ), &xSide ) )
                bDone = true; // nothing is left of this stream: the shorter file ends the pair stream
            pRet->asHead[ i ].swap( xSide.sHead );
            pRet->asMembers[ i ].swap( xSide.sMembers );
            pRet->auiDrop[ i ] = xSide.uiDrop;
        }
        if( bDone )
            return nullptr; // (module.h:688-695)
        std::lock_guard<std::mutex> xOut( pLink->xMutex );
        pLink->bPending = true;
        pRet->pLink = pLink;
        return pRet;
    }
};

// Volatile source over reads that already are in memory (benchmarks, callers that hold their reads): consecutive slices.
class BatchSource : public libMS::Module<ReadVector, true>
{
    const std::shared_ptr<ReadVector> pAll;
    std::atomic<size_t> uiNext{ 0 };

  public:
    size_t uiBatchReads = 1u << 18;
    BatchSource( std::shared_ptr<ReadVector> pAll ) : pAll( pAll )
    {}
    virtual std::shared_ptr<ReadVector> execute( ) override
    {
        const size_t lo = uiNext.fetch_add( uiBatchReads );
        if( lo >= pAll->size( ) )
            return nullptr;
        return std::make_shared<ReadVector>( pAll->begin( ) + lo, pAll->begin( ) + std::min( pAll->size( ), lo + uiBatchReads ) );
    }
};

// SAM records of a whole batch (fileWriter.cpp:11-158 per read), formatted from the flat view by uiFormatThreads threads
// into one arena each and written arena by arena -- in input order -- under one acquisition of the writer's lock.
class BatchFileWriter : public libMS::Module<libMS::Container, false, ReadVector, AlignedBatch, Pack>
{
    std::shared_ptr<FileWriter> pPerRead; // owns stream + lock (and serves the options the flat formatter does not)
    ma_amd::flat::SamFormat xFormat;
    ma_amd::flat::ContigTable xContigs;

  public:
    size_t uiFormatThreads = 8;
    std::atomic<uint64_t> uiBytes{ 0 }, uiReads{ 0 };

    BatchFileWriter( const ParameterSetManager& rParameters, std::shared_ptr<OutStream> pOut, std::shared_ptr<Pack> pPack )
        : BatchFileWriter( rParameters, std::make_shared<FileWriter>( rParameters, pOut, pPack ), pPack )
    {}
    // on the stream (and behind the header) of a FileWriter that exists already
    BatchFileWriter( const ParameterSetManager& rParameters, std::shared_ptr<FileWriter> pWriter, std::shared_ptr<Pack> pPack )
        : pPerRead( pWriter )
    {
        const SamOptions& rO = rParameters.xSam;
        xFormat.bNoSecondary = rO.bNoSecondary, xFormat.bNoSupplementary = rO.bNoSupplementary;
        xFormat.bOutputMCigar = rO.bOutputMCigar, xFormat.bCGTag = rO.bCGTag, xFormat.bSoftClip = rO.bSoftClip;
        xContigs.set( pPack->vNames, pPack->vStarts, pPack->vLengths );
    }

    virtual std::shared_ptr<libMS::Container> execute( std::shared_ptr<ReadVector> pReads, std::shared_ptr<AlignedBatch> pAligned,
                                                       std::shared_ptr<Pack> pPack ) override
    {
        const size_t n = pReads->size( );
        if( pAligned->size( ) != n )
            throw std::runtime_error( "BatchFileWriter: the batch of alignments does not belong to these reads" );
        // formatted on the device (BatchAligner::executeFlatSam): the batch's text, or its members, as they are
        if( pAligned->hasSamText( ) || pAligned->hasSamBgzf( ) )
        {
            write( *pAligned );
            return std::make_shared<libMS::Container>( );
        }
        if( pPerRead->xOptions.bEmulateNgmlrTags ) // needs Alignment objects and reference bases: the per-read writer
        {
            for( size_t i = 0; i < n; i++ )
                pPerRead->execute( ( *pReads )[ i ], pAligned->alignmentsOf( i ), pPack );
            uiReads += n;
            return std::make_shared<libMS::Container>( );
        }
        const size_t uiThreads = std::max<size_t>( 1, std::min<size_t>( uiFormatThreads, n / 2048 + 1 ) );
        std::vector<ma_amd::flat::Arena> vArenas( uiThreads );
        std::string sFailure;
        std::mutex xFailure;
        auto format = [ & ]( size_t t ) {
            try
            {
                ma_amd::flat::Arena& rOut = vArenas[ t ];
                const uint64_t* pOff = pAligned->offsets( );
                for( size_t i = n * t / uiThreads; i < n * ( t + 1 ) / uiThreads; i++ )
                {
                    const NucSeq& rQ = *( *pReads )[ i ];
                    ma_amd::flat::ReadView xQ;
                    xQ.sName = rQ.sName.data( ), xQ.uiNameLen = rQ.sName.size( );
                    xQ.pCodes = rQ.xCodes.data( ), xQ.uiLength = rQ.xCodes.size( );
                    xQ.pQuality = rQ.xQuality.empty( ) ? nullptr : rQ.xQuality.data( );
                    ma_amd::flat::formatRead( rOut, xFormat, xContigs, xQ, pAligned->alignments( ) + pOff[ i ], pOff[ i + 1 ] - pOff[ i ],
                                              pAligned->ops( ) );
                }
            }
            catch( const std::exception& rE )
            {
                std::lock_guard<std::mutex> xGuard( xFailure );
                if( sFailure.empty( ) )
                    sFailure = rE.what( );
            }
        };
        std::vector<std::thread> vT;
        for( size_t t = 1; t < uiThreads; t++ )
            vT.emplace_back( format, t );
        format( 0 );
        for( auto& rT : vT )
            rT.join( );
        if( !sFailure.empty( ) )
            throw std::runtime_error( sFailure );
        uiBytes += writeArenas( *pPerRead, vArenas ), uiReads += n;
        return std::make_shared<libMS::Container>( );
    }
    // The arenas of a batch, in order, under one acquisition of the writer's lock.  On a BGZF stream (SamOptions::bBgzf) every
    // arena is deflated first (ma_bgzf::deflateHost), by a thread of its own like the formatting before: the lock is held for
    // the writes of the members alone.  Returns the bytes of text.
    static uint64_t writeArenas( const SamSink& rSink, const std::vector<ma_amd::flat::Arena>& vArenas )
    {
        uint64_t uiTotal = 0;
        const auto pBgzf = rSink.bgzf( );
        std::vector<std::vector<uint8_t>> vMembers( pBgzf != nullptr ? vArenas.size( ) : 0 );
        if( pBgzf != nullptr )
        {
            std::vector<std::thread> vT;
            for( size_t t = 1; t < vArenas.size( ); t++ )
                vT.emplace_back( [ &, t ]( ) { vMembers[ t ] = bgzfMembersOf( vArenas[ t ].data( ), vArenas[ t ].size( ) ); } );
            vMembers[ 0 ] = bgzfMembersOf( vArenas[ 0 ].data( ), vArenas[ 0 ].size( ) );
            for( auto& rT : vT )
                rT.join( );
        }
        std::lock_guard<std::mutex> xGuard( *rSink.pLock );
        for( size_t t = 0; t < vArenas.size( ); t++ )
        {
            if( pBgzf != nullptr )
                pBgzf->writeMembers( vMembers[ t ].data( ), vMembers[ t ].size( ) );
            else
                rSink.pOut->write( vArenas[ t ].data( ), vArenas[ t ].size( ) );
            uiTotal += vArenas[ t ].size( );
        }
        return uiTotal;
    }
    // The text of a batch the device formatted, with one write.  On a BGZF stream (the writer has SamOptions::bBgzf, the aligner
    // has not) the text is cut at multiples of a member's 65 280 bytes into up to uiThreads pieces, every piece is deflated by a
    // thread of its own (ma_bgzf::deflateHost) and the members go out in order: the members of the whole text.
    static void writeDeviceText( const SamSink& rSink, const char* pText, size_t uiBytes, size_t uiThreads )
    {
        const auto pBgzf = rSink.bgzf( );
        if( pBgzf == nullptr )
        {
            std::lock_guard<std::mutex> xGuard( *rSink.pLock );
            rSink.pOut->write( pText, uiBytes );
            return;
        }
        const size_t uiChunks = ( uiBytes + ma_bgzf::DEFLATE_CHUNK - 1 ) / ma_bgzf::DEFLATE_CHUNK;
        const size_t uiPieces = std::max<size_t>( 1, std::min( uiThreads, uiChunks ) );
        std::vector<std::vector<uint8_t>> vMembers( uiPieces );
        auto piece = [ & ]( size_t t ) {
            const size_t uiFrom = std::min( uiBytes, uiChunks * t / uiPieces * ma_bgzf::DEFLATE_CHUNK );
            const size_t uiTo = std::min( uiBytes, uiChunks * ( t + 1 ) / uiPieces * ma_bgzf::DEFLATE_CHUNK );
            vMembers[ t ] = bgzfMembersOf( pText + uiFrom, uiTo - uiFrom );
        };
        std::vector<std::thread> vT;
        for( size_t t = 1; t < uiPieces; t++ )
            vT.emplace_back( piece, t );
        piece( 0 );
        for( auto& rT : vT )
            rT.join( );
        std::lock_guard<std::mutex> xGuard( *rSink.pLock );
        for( const auto& rMembers : vMembers )
            pBgzf->writeMembers( rMembers.data( ), rMembers.size( ) );
    }
    // the members of a batch the device deflated, as they are: only onto a BGZF stream
    static void writeDeviceMembers( const SamSink& rSink, const AlignedBatch& rBatch, const char* sWho )
    {
        const auto pBgzf = rSink.bgzf( );
        if( pBgzf == nullptr )
            throw std::runtime_error( std::string( sWho ) + ": the batch carries BGZF members, the writer's stream is plain (SamOptions::bBgzf)" );
        std::lock_guard<std::mutex> xGuard( *rSink.pLock );
        pBgzf->writeMembers( rBatch.samBgzf( ), rBatch.samBgzfBytes( ) );
    }
    // A batch of BatchAligner::executeFlat / executeFlatSam outside of a graph: device text goes out with ONE write, records
    // are formatted as in execute( ).
    void write( const AlignedBatch& rBatch, std::shared_ptr<Pack> pPack = nullptr )
    {
        if( !rBatch.hasSamText( ) && !rBatch.hasSamBgzf( ) )
        {
            if( pPack == nullptr && pPerRead->xOptions.bEmulateNgmlrTags )
                throw std::runtime_error( "BatchFileWriter::write: the NGMLR tags need the pack" );
            auto pReads = std::make_shared<ReadVector>( rBatch.pReads->begin( ) + rBatch.uiFirst,
                                                        rBatch.pReads->begin( ) + rBatch.uiFirst + rBatch.size( ) );
            auto pView = std::make_shared<AlignedBatch>( );
            pView->pReads = pReads, pView->uiFirst = 0, pView->pResult = rBatch.pResult;
            execute( pReads, pView, pPack );
            return;
        }
        if( pPerRead->xOptions.bEmulateNgmlrTags && !( rBatch.samOptions( ) & MA_SAM_NGMLR_TAGS ) )
            throw std::runtime_error( "BatchFileWriter: device text carries no NGMLR tags" );
        if( !pPerRead->xOptions.bEmulateNgmlrTags && ( rBatch.samOptions( ) & MA_SAM_NGMLR_TAGS ) )
            throw std::runtime_error( "BatchFileWriter: device text carries NGMLR tags the writer's options do not ask for" );
        if( rBatch.hasSamBgzf( ) )
        {
            writeDeviceMembers( *pPerRead, rBatch, "BatchFileWriter" );
            uiBytes += rBatch.samBytes( ), uiReads += rBatch.size( );
            return;
        }
        writeDeviceText( *pPerRead, rBatch.samText( ), rBatch.samBytes( ), uiFormatThreads );
        uiBytes += rBatch.samBytes( ), uiReads += rBatch.size( );
    }
    virtual bool requiresLock( ) const
    {
        return false; // serialises its own output
    }
};

// SAM records of a whole PAIRED batch (BatchAligner::executePairedFlat): PairedFileWriter::execute (fileWriter.cpp:158-383)
// per pair, formatted from the flat pair records (ma_flat_sam.h formatPair) by uiFormatThreads threads into one arena each and
// written in input order under one acquisition of the writer's lock.  A batch that carries the text the device formatted
// (BatchAligner::executePairedFlatSam) goes out as it is, with one write.  The NGMLR tags are refused like PairedFileWriter does.
class BatchPairedFileWriter
{
    std::shared_ptr<PairedFileWriter> pPerPair; // owns stream + lock, writes the header
    ma_amd::flat::SamFormat xFormat;
    ma_amd::flat::ContigTable xContigs;

  public:
    size_t uiFormatThreads = 8;
    std::atomic<uint64_t> uiBytes{ 0 }, uiReads{ 0 };

    BatchPairedFileWriter( const ParameterSetManager& rParameters, std::shared_ptr<OutStream> pOut, std::shared_ptr<Pack> pPack )
        : BatchPairedFileWriter( rParameters, std::make_shared<PairedFileWriter>( rParameters, pOut, pPack ), pPack )
    {}
    // on the stream (and behind the header) of a PairedFileWriter that exists already
    BatchPairedFileWriter( const ParameterSetManager& rParameters, std::shared_ptr<PairedFileWriter> pWriter, std::shared_ptr<Pack> pPack )
        : pPerPair( pWriter )
    {
        const SamOptions& rO = rParameters.xSam;
        xFormat.bNoSecondary = rO.bNoSecondary, xFormat.bNoSupplementary = rO.bNoSupplementary;
        xFormat.bOutputMCigar = rO.bOutputMCigar, xFormat.bCGTag = rO.bCGTag, xFormat.bSoftClip = rO.bSoftClip;
        xContigs.set( pPack->vNames, pPack->vStarts, pPack->vLengths );
    }

    void execute( const AlignedBatch& rBatch )
    {
        if( !rBatch.paired( ) )
            throw std::runtime_error( "BatchPairedFileWriter: not a paired batch" );
        const size_t n = rBatch.pairs( );
        if( rBatch.hasSamBgzf( ) ) // formatted and deflated on the device: the batch's members as they are
        {
            BatchFileWriter::writeDeviceMembers( *pPerPair, rBatch, "BatchPairedFileWriter" );
            uiBytes += rBatch.samBytes( ), uiReads += 2 * n;
            return;
        }
        if( rBatch.hasSamText( ) ) // formatted on the device (BatchAligner::executePairedFlatSam): the batch's text as it is
        {
            BatchFileWriter::writeDeviceText( *pPerPair, rBatch.samText( ), rBatch.samBytes( ), uiFormatThreads );
            uiBytes += rBatch.samBytes( ), uiReads += 2 * n;
            return;
        }
        const size_t uiThreads = std::max<size_t>( 1, std::min<size_t>( uiFormatThreads, n / 1024 + 1 ) );
        std::vector<ma_amd::flat::Arena> vArenas( uiThreads );
        std::string sFailure;
        std::mutex xFailure;
        auto view = []( const NucSeq& rQ ) {
            ma_amd::flat::ReadView xQ;
            xQ.sName = rQ.sName.data( ), xQ.uiNameLen = rQ.sName.size( );
            xQ.pCodes = rQ.xCodes.data( ), xQ.uiLength = rQ.xCodes.size( );
            xQ.pQuality = rQ.xQuality.empty( ) ? nullptr : rQ.xQuality.data( );
            return xQ;
        };
        auto format = [ & ]( size_t t ) {
            try
            {
                const uint64_t* pOff = rBatch.pairOffsets( );
                for( size_t k = n * t / uiThreads; k < n * ( t + 1 ) / uiThreads; k++ )
                    ma_amd::flat::formatPair( vArenas[ t ], xFormat, xContigs, view( *rBatch.read( 2 * k ) ), view( *rBatch.read( 2 * k + 1 ) ),
                                              rBatch.pairAlignments( ) + pOff[ k ], pOff[ k + 1 ] - pOff[ k ], rBatch.pairOps( ),
                                              rBatch.pairMate( ) + pOff[ k ], rBatch.pairOther( ) + pOff[ k ] );
            }
            catch( const std::exception& rE )
            {
                std::lock_guard<std::mutex> xGuard( xFailure );
                if( sFailure.empty( ) )
                    sFailure = rE.what( );
            }
        };
        std::vector<std::thread> vT;
        for( size_t t = 1; t < uiThreads; t++ )
            vT.emplace_back( format, t );
        format( 0 );
        for( auto& rT : vT )
            rT.join( );
        if( !sFailure.empty( ) )
            throw std::runtime_error( sFailure );
        uiBytes += BatchFileWriter::writeArenas( *pPerPair, vArenas ), uiReads += 2 * n;
    }
};
} // namespace libMA
