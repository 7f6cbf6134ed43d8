// The host layer of the genome text path against the host path: buildIndexFromFasta after srand( seed ) and
// buildIndexFromFastaText( seed ) on the same FASTA file, each stored with storeIndex (tests/test_gpu_genome_text.py compares the
// five files of both prefixes).  Needs a device.
//   genome_store_test <genome.fa> <prefix host> <prefix text> <seed> <chunk bytes>
#include "ma_genome.h"
#include "ma_sam.h"

using namespace libMA;

int main( int argc, char** argv )
{
    if( argc != 6 )
        return printf( "usage: genome_store_test <genome.fa> <prefix host> <prefix text> <seed> <chunk bytes>\n" ), 2;
    try
    {
        const uint32_t uiSeed = (uint32_t)strtoul( argv[ 4 ], NULL, 10 );
        std::shared_ptr<Pack> pPack;
        std::shared_ptr<FMIndex> pFM;
        srand( uiSeed );
        buildIndexFromFasta( argv[ 1 ], pPack, pFM );
        storeIndex( argv[ 2 ], pPack, pFM );
        const size_t uiHoles = pPack->vHoles.size( );
        buildIndexFromFastaText( argv[ 1 ], pPack, pFM, uiSeed, strtoull( argv[ 5 ], NULL, 10 ) );
        storeIndex( argv[ 3 ], pPack, pFM );
        printf( "stored ok: %zu contigs, %zu holes (host path %zu)\n", pPack->vNames.size( ), pPack->vHoles.size( ), uiHoles );
    }
    catch( const std::exception& rE )
    {
        return printf( "FAIL: %s\n", rE.what( ) ), 1;
    }
    return 0;
}
