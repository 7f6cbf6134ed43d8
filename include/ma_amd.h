/* ma_amd.h -- C ABI of the MI355X-native seed-and-extend engine (libma_amd.so).
 *
 * This is the drop-in boundary for MA's hot path.  Every entry point is plain C (pointers + sizes,
 * no C++/torch types) so the reference's host code (C++ via a thin wrapper, or Python via ctypes)
 * can bind it.  Each function cites the reference interface it replaces (paths relative to the
 * ITBE-Lab/ma source tree).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; ma_last_error() gives the message
 *     (the C++ module wrappers in ma_amd/host turn that into std::runtime_error, mirroring
 *     libs/ms/inc/ms/module/module.h:339-377).
 *   - nothing here falls back to a CPU path: without a HIP device every compute call fails.
 *   - all positions follow the reference: reference positions r in [0, 2F) on T.revcomp(T),
 *     query positions q in [0,|Q|), bases A0 C1 G2 T3, N = 4 (nucSeq.cpp:17-28).
 */
#ifndef MA_AMD_H
#define MA_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MA_AMD_ABI_VERSION 1

typedef struct ma_index ma_index; /* device-resident FMD-index + pack (FMIndex fMIndex.h:195-230, Pack pack.h:39-176) */
typedef struct ma_batch ma_batch; /* device-resident batch of reads + all stage outputs */

/* Parameters the path reads (parameter.h:521-1060); same fields/meaning as the reference's
 * Presetting/GlobalParameter members named in the comments of ma_params_default(). */
typedef struct
{
    int32_t seeding_technique; /* 0 maxSpan, 1 SMEMs, 2 MEMs    xSeedingTechnique  (binarySeeding.h:560-561) */
    int32_t min_seed_len; /* 16                                  xMinSeedLength */
    int32_t min_ambiguity; /* 0                                  xMinimalSeedAmbiguity */
    int32_t max_ambiguity; /* 100                                xMaximalSeedAmbiguity */
    int32_t min_seed_size_drop; /* 15                            xMinimalSeedSizeDrop */
    int32_t max_num_soc, min_num_soc; /* 30 / 1                  xMaxNumSoC / xMinNumSoC */
    int32_t harm_score_min; /* 18                                xHarmScoreMin */
    int32_t max_score_lookahead; /* 3                            xMaxScoreLookahead */
    int32_t switch_qlen; /* 800                                  xSwitchQlen */
    int32_t min_delta_dist; /* 16                                xMinDeltaDist */
    int32_t max_gap_area; /* 20                                  xMaxGapArea */
    int32_t padding; /* 1000                                     xPadding */
    int32_t bandwidth_ext; /* 512                                xBandwidthDPExtension */
    int32_t min_bandwidth_gap; /* 20                             xMinBandwidthGapFilling */
    int32_t zdrop; /* 200                                        xZDrop */
    int32_t sv_penalty; /* 100                                   pGlobalParams->uiSVPenalty */
    int32_t match, mismatch, gap, extend, gap2, extend2; /* 2 4 4 2 24 1 (pGlobalParams) */
    int32_t disable_heuristics; /* 0                             xDisableHeuristics */
    int32_t soc_width; /* 0                                      xSoCWidth */
    uint32_t srand_seed; /* RANSAC draws: glibc srand(seed) state at the start of each read's Harmonization */
    uint64_t genome_size_disable; /* 10 000 000                  xGenomeSizeDisable */
    double rel_min_seed_size_amount; /* 0.005                    xRelMinSeedSizeAmount */
    double harm_score_min_rel; /* 0.002                          xHarmScoreMinRel */
    double soc_score_decrease_tol; /* 0.1                        xSoCScoreDecreaseTolerance */
    double score_diff_tol; /* 0.0001                             xScoreDiffTolerance */
    double max_delta_dist; /* 0.1                                xMaxDeltaDist */
    int32_t min_alignment_score; /* 75                           xMinAlignmentScore */
    int32_t report_n_best; /* 0                                  xReportN */
    int32_t max_supplementary; /* 1                              xMaxSupplementaryPerPrim */
    double max_overlap_supplementary; /* 0.1                     xMaxOverlapSupplementary */
    /* small inversions: search_inversions is read by the host layer only (it puts the module into the graph,
       ma_inversions_batch into the flat paths); zdrop_inversion by ma_inversions_batch and by the host module SmallInversions */
    int32_t search_inversions; /* 0                              xSearchInversions */
    int32_t zdrop_inversion; /* 100                              xZDropInversion */
    int32_t use_paired_reads; /* 0                               xUsePairedReads (read by the host layer only: it selects the
                                                                 paired graph; ma_pair_batch pairs whenever it is called) */
    int32_t libm_probe; /* 0. Diagnostics only (tests): != 0 nudges every tan / sin / atan / log result of the chaining
                           stage by one ulp (ma_amd/csrc/chain.h LibmProbe); results must not change */
    /* read by ma_pair_batch (with `match`) and by the host module PairedReads */
    double mean_paired_dist; /* 400                              xMeanPairedReadDistance */
    double std_paired_dist; /* 150                               xStdPairedReadDistance */
    double paired_bonus; /* 1.25                                 xPairedBonus */
} ma_params;

/* ParameterSetManager presets (parameter.h:1079-1104): "default" 1081, "illumina" 1083-1087, "illuminapaired" 1089-1094,
 * "pacbio" 1096-1098, "nanopore" 1101-1104. */
void ma_params_default( ma_params* p );
void ma_params_illumina( ma_params* p );
void ma_params_illuminapaired( ma_params* p ); /* illumina + xUsePairedReads (selects the paired graph of the host layer) */
void ma_params_pacbio( ma_params* p ); /* default + xMaxSupplementaryPerPrim 100, xMinNumSoC 5 */
void ma_params_nanopore( ma_params* p ); /* pacbio + SMEM seeding */
/* ParameterSetManager::setSelected (parameter.h:1163-1170) by key, case-insensitive like the reference's map keys are
 * lower case: 0 on success; an unknown key fails with the reference's text ("The presetting '<key>' can not be found."),
 * "sv-illumina" / "sv-pacbio" (1106-1128) fail as not implemented: they switch xRectangularSoc off
 * (stripOfConsideration.h:41-53), which the device path does not have. */
int ma_params_preset( const char* key, ma_params* p );

/* Records (same layout as the oracle's records so parity tests compare raw arrays) */
typedef struct
{
    int64_t q_start, q_size, sa_start, sa_start_rc, sa_size; /* Segment (segment.h:31-113): size = length-1 */
} ma_segment;
typedef struct
{
    int64_t q_start, len, r_start, delta; /* Seed (seed.h:34-46) */
    uint32_t ambiguity, on_forward;
} ma_seed;
typedef struct
{
    int32_t max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, reach_end, n_cigar; /* kswcpp_extz_t (kswcpp.h:31-41) */
} ma_ez;
typedef struct
{
    int64_t begin_ref, end_ref, begin_q, end_q, score; /* Alignment (alignment.h:55-84) */
    uint32_t soc_index, n_ops;
    uint64_t ops_off; /* first (type,len) pair of this alignment in the ops array */
    uint32_t secondary, supplementary;
    double mapq;
} ma_alignment;
typedef struct
{
    uint64_t acc_len; /* SoCOrder (soc.h:26-90): accumulated seed length = the score the queue is ordered by */
    uint32_t ambiguity, n_seeds; /* accumulated seed ambiguity (ties: more = smaller), seeds in the strip */
    uint32_t begin, end; /* its seeds: [begin, end) of the read's seeds re-sorted by reference position (soc.h:196-231) */
} ma_soc;
typedef struct
{
    int32_t qlen, tlen, w, zdrop, flag; /* kswcpp_dispatch arguments (kswcpp.h:165-190) */
    uint32_t reserved;
    uint64_t q_off, t_off; /* offsets into the query / target byte arrays handed to ma_ksw_batch */
} ma_ksw_job;

/* ---- runtime ---- */
const char* ma_last_error( void ); /* thread-local message of the last failing call */
int ma_abi_version( void );
int ma_device_count( int* n );
int ma_set_device( int device );

/* Page-locked host memory for the arrays handed to / filled by the batch calls: uploads and downloads of pageable memory go
 * through the runtime's staging buffers at a fraction of the PCIe rate.  (The reference has no counterpart: its containers
 * live in host memory only; this is what NucSeq / Alignment storage becomes on the way to and from the device.) */
int ma_host_alloc( uint64_t bytes, void** out );
int ma_host_free( void* p );
/* Pins the CALLING host thread (and the threads it starts afterwards) to the CPUs next to GPU `device` -- the local_cpulist of
 * its PCI function in sysfs.  On a two-socket node the scheduler is free to spread the threads that feed a device (launches,
 * size read-backs, stream waits, the copies out of and into page-locked memory) over both sockets, differently from run to run;
 * pinning takes that out of the run-to-run spread of the host-to-host rate (the effect itself is within it).  mode 0: the GPU's CPUs; 1: the OTHER CPUs (the experiment that shows the
 * cost); -1: the mask the thread had when it first called this function.  Every mode stays INSIDE that first mask (a taskset /
 * numactl / SLURM affinity of the caller is never widened).  *n_cpus (optional) = CPUs of the new mask, 0 when the mask was left
 * alone (no topology information, a one-node host, none of the wanted CPUs in the caller's mask).  Fails only for a bad argument.  (No counterpart in the reference: its worker threads are
 * placed by the OS, module.h:303-369.) */
int ma_host_bind_thread( int device, int mode, int* n_cpus );

/* ---- index: replaces FMIndex(std::string) / Pack(std::string) loading (fMIndex.h:952-955, pack.h:513-525) ---- */
/* Upload an index whose arrays were read from the reference's own .bwt/.sa/.pac files. */
int ma_index_create( const uint32_t* bwt_words, uint64_t n_words, const int64_t* sa, uint64_t n_sa,
                     const uint64_t L2[ 5 ], int64_t primary, uint64_t ref_len_fwd_rev, const uint8_t* pac,
                     int32_t n_contigs, const uint64_t* contig_starts, const uint64_t* contig_lens, ma_index** out );
/* Build pack + FMD-index on the GPU from N-free contigs (host codes 0..3); replaces
 * FMIndex::build_FMIndex (fMIndex.cpp:316-391) + Pack::vAppendSequence (pack.h:586-698). Produces
 * byte-identical .bwt/.sa/.pac content. */
int ma_index_build( int32_t n_contigs, const uint64_t* contig_lens, const uint8_t* codes_concat, ma_index** out );
/* Same, for a genome that already lives in device memory as 1 byte/base codes. */
int ma_index_build_device( int32_t n_contigs, const uint64_t* contig_lens, const void* d_codes, ma_index** out );
int ma_index_destroy( ma_index* );
int ma_index_device( const ma_index*, int* device ); /* the GPU the index lives on (every call on it binds to that device) */
int ma_index_sizes( const ma_index*, uint64_t* n_words, uint64_t* n_sa, uint64_t* ref_len, int32_t* n_contigs );
/* Download (for FMIndex::vStoreFMIndex-compatible files and for tests); any pointer may be NULL. */
int ma_index_download( const ma_index*, uint32_t* bwt_words, int64_t* sa, uint64_t L2[ 5 ], int64_t* primary,
                       uint8_t* pac, uint64_t* contig_starts, uint64_t* contig_lens );

/* ---- the genome's FASTA text read on the device (replaces Pack::vAppendFASTA, pack.cpp:510-537 + vAppendSequence, pack.h:586-698,
 * for files; the rules are ma_amd/host/ma_genome_dev.h) ----
 * A genome object takes the text of one or more FASTA files in chunks and keeps the codes (1 byte per base, hole bases -- N and
 * every other letter that is not A C G T -- as 4) on the device, the contig table (name up to the first blank, start, length,
 * number of holes) and the holes (start on the forward strand, length; a run of hole bases inside one contig) on the host.
 * ma_genome_append_text: `text` is a chunk of the file in host memory (page-locked memory uploads fastest), n_bytes < 2 GiB, in the
 *   strict FASTA form of ma_batch_set_reads_text ("\n" or "\r\n" line ends, '>' header lines, non-empty base lines, every record
 *   has bases).  The call consumes whole lines only -- up to and including the chunk's last "\n" -- and says in *consumed how
 *   many bytes that was; the caller carries the rest into its next call.  With end_of_file != 0 an unterminated last line is
 *   consumed too and the file is closed: the next call starts another file with a header.  A chunk after a file's first may
 *   begin with base lines; they continue the open contig.  A chunk without any "\n" and end_of_file == 0 consumes 0 bytes.
 *   It uploads, parses and waits: THREE read-backs per call (the line feeds, which size the per-line work; the sums and the
 *   refusal, which size the lists; the chunk's contig names, starts and holes) -- one call per 256 MiB of text, not per record.
 *   A refusal leaves the object exactly as it was (*consumed = 0) and usable:
 *     "ma_genome_append_text: line <L> (byte <X>): <reason>"   the lowest offending line, L (1-based) and X counted over
 *                                                              everything consumed so far plus this chunk; reasons as
 *                                                              ma_batch_set_reads_text's
 *     "ma_genome_append_text: a genome is FASTA"               an '@' where a header is due
 *     "ma_genome_append_text: genome capacity exceeded (<B> bases)"   B: what the genome would hold after the chunk
 *     "ma_genome_append_text: too large"                       n_bytes of 2 GiB or more (judged on n_bytes, before the chunk is
 *                                                              looked at)
 *     "ma_genome_append_text: the index was already built"
 *     "ma_genome_append_text: a genome as BGZF or gzip is not served (plain FASTA text only)"   the bytes 1f 8b where a header is due
 *   Not served, and refused by these rules: BGZF / gzip bytes and FASTQ genomes.
 * ma_genome_build_index: fills the hole bases -- the k-th in text order becomes rand( ) & 3 of the k-th draw after
 *   srand( srand_seed ) of glibc, drawn from the library's own generator (libc's state is not touched) --, builds the index as
 *   ma_index_build_device does (sampling interval 32) and sets its contig names and holes: ma_sam_batch, ma_pair_sam_batch and
 *   MA_SAM_NGMLR_TAGS work on it with no further call.  Once per genome; fails on a genome without contigs or whose last contig
 *   has no bases yet.  The getters keep serving afterwards, and ma_genome_get_codes then shows the filled bases.
 *   The hole bases are filled before the sort: if the sort then fails (out of memory, say), the genome counts as built and the call
 *   cannot be tried again on it -- read the file into a new genome object.
 * ma_genome_create: device < 0 means the calling thread's current device; a device that does not exist fails here.
 * Getters: any pointer may be NULL.  name_off: n_contigs + 1 offsets into names. */
typedef struct ma_genome ma_genome;
int ma_genome_create( int device, uint64_t max_bases, ma_genome** out );
int ma_genome_append_text( ma_genome*, const char* text /*host*/, uint64_t n_bytes, int32_t end_of_file, uint64_t* consumed );
int ma_genome_counts( const ma_genome*, uint64_t* n_contigs, uint64_t* n_bases, uint64_t* n_name_bytes, uint64_t* n_holes, uint64_t* n_hole_bases );
int ma_genome_get_contigs( const ma_genome*, uint64_t* name_off /*n+1*/, char* names, uint64_t* starts, uint64_t* lens, uint64_t* n_holes );
int ma_genome_get_holes( const ma_genome*, uint64_t* start, uint64_t* len );
int ma_genome_get_codes( const ma_genome*, uint64_t from, uint64_t n, uint8_t* codes ); /* 4 = a hole base not filled yet */
int ma_genome_build_index( ma_genome*, uint32_t srand_seed, ma_index** out );
int ma_genome_destroy( ma_genome* );

/* Pack::vExtract (pack.h:1440-1450, vExtractSubsection 1147-1236) for n ranges [begin[i], end[i]) of the doubled
 * text; codes 0..3 back to back in out (host). Replaces the reference extraction SmallInversions does
 * (smallInversions.h:207). */
int ma_pack_extract( const ma_index*, const uint64_t* begin, const uint64_t* end, uint64_t n, uint8_t* out );

/* ---- primitive ops (tests / SuffixArrayInterface seam, fMIndex.h:155-175) ---- */
/* n independent FMIndex::extend_backward calls (fMIndex.cpp:21-101): ik[3n] -> ok[3n] (host arrays) */
int ma_extend_backward_batch( const ma_index*, const int64_t* ik, const uint8_t* c, uint64_t n, int64_t* ok );
/* n independent FMIndex::bwt_sa calls (fMIndex.h:788-814) */
int ma_bwt_sa_batch( const ma_index*, const int64_t* rows, uint64_t n, int64_t* pos );
/* n independent kswcpp_dispatch calls (kswcpp.h:165-190). ez[n]; the cigar of job j is the ez[j].n_cigar words at
 * cigar[cigar_off[j]] (the cigars are packed densely but NOT in job order); cigar_off[n] = words used in total;
 * returns an error if cigar_cap is too small. */
int ma_ksw_batch( const ma_params*, const ma_ksw_job* jobs, uint64_t n, const uint8_t* q_bytes, uint64_t q_len,
                  const uint8_t* t_bytes, uint64_t t_len, ma_ez* ez, uint64_t* cigar_off, uint32_t* cigar,
                  uint64_t cigar_cap );

/* Same call with the semantics the pipeline uses for its extension / small-gap DP (NeedlemanWunsch::dynPrg,
 * ksw_dual_ext, ksw; needlemanWunsch.cpp:82-622 read only these): ez.max, ez.max_q, ez.max_t, n_cigar and the
 * cigar are those of kswcpp_dispatch, the other ez fields are unspecified.  Runs the packed extension kernel with
 * the exact early stop where a job qualifies (ma_amd/csrc/ksw_ext.h) and the exact kernels otherwise. */
int ma_ksw_ext_batch( const ma_params*, const ma_ksw_job* jobs, uint64_t n, const uint8_t* q_bytes, uint64_t q_len,
                      const uint8_t* t_bytes, uint64_t t_len, ma_ez* ez, uint64_t* cigar_off, uint32_t* cigar,
                      uint64_t cigar_cap );

/* ---- batch pipeline: BinarySeeding -> StripOfConsideration -> Harmonization -> NeedlemanWunsch -> MappingQuality
 *      as wired in libMA::setUpCompGraph (libs/ma/src/util/export.cpp:104-108) ----
 * What a call invalidates.  A batch holds products that are made of one another:
 *
 *   reads - names
 *   reads - SEEDED - EXTRACTED - CHAINED - ALIGNED - inversion view -+- single-end text (needs names) - its BGZF members
 *                                                                    +- pairs - pairs' text (needs names) - its BGZF members
 *
 * A call that makes a product (a stage, a stage input handed in, ma_batch_set_read_text, ma_inversions_batch, ma_pair_batch,
 * a SAM text, its members) first drops that product and everything to its right, and marks it valid when it succeeds; new reads
 * in any form drop everything.  So after a stage call or a stage-input call the products of LATER stages are gone -- their
 * getters fail with "run ... first" until they are made again --, a call that returns 1 leaves the batch at the product before
 * it, and the two that keep something to their left do so on purpose: ma_inversions_batch keeps ALIGNED, ma_pair_batch keeps the
 * single-end text and the inversion view.  A stage input handed in makes the batch jump to that stage; what the earlier stages
 * held is then unspecified.  The rules are written once, in ma_amd/host/ma_batch_state.h. */
int ma_batch_create( const ma_index*, const ma_params*, uint64_t max_reads, uint64_t max_bases, ma_batch** out );
int ma_batch_destroy( ma_batch* );
/* stream: a hipStream_t (as void*) all stage kernels of this batch are launched on; NULL = default stream */
int ma_batch_set_stream( ma_batch*, void* hip_stream );
/* waits of this batch's calls: 0 = the runtime's spinning stream synchronisation (lowest latency, default), 1 = sleep on
 * an interrupt-driven event (hosts running far more threads than cores: the DeviceBatcher of the host layer) */
int ma_batch_set_blocking_sync( ma_batch*, int on );
/* reads as 1 byte/base codes, CSR offsets[n+1]; host or device pointers */
int ma_batch_set_reads( ma_batch*, const uint8_t* codes, const uint64_t* offsets, uint64_t n_reads );
/* the caller's device arrays, which stay the caller's; a call that fails leaves the reads that were set before in place */
int ma_batch_set_reads_device( ma_batch*, const void* d_codes, const void* d_offsets, uint64_t n_reads,
                               uint64_t n_bases );
/* stages (asynchronous on the batch stream; each requires the previous one) */
int ma_seed_batch( ma_batch* ); /* BinarySeeding::execute (binarySeeding.cpp:86-178) */
int ma_extract_seeds_batch( ma_batch* ); /* ExtractSeeds::execute (stripOfConsideration.h:138-157) */
int ma_chain_batch( ma_batch* ); /* StripOfConsiderationSeeds::execute + Harmonization::execute */
int ma_dp_batch( ma_batch* ); /* NeedlemanWunsch::execute + MappingQuality::execute */
int ma_align_batch( ma_batch* ); /* all four */
int ma_batch_sync( ma_batch* ); /* wait for the stream; surfaces asynchronous kernel errors / capacity overflows */

/* streams for callers that keep several batches in flight without including HIP headers (host layer: DeviceBatcher,
 * MultiDeviceAligner); created on the index's device, non-blocking with respect to the default stream */
int ma_stream_create( const ma_index*, void** out_hip_stream );
int ma_stream_destroy( const ma_index*, void* hip_stream );

/* stage INPUTS from the host: a module of this library takes over in the middle of a chain whose earlier stages ran
 * elsewhere (e.g. the reference's BinarySeeding followed by the MI355X StripOfConsideration).  Reads must be set; each
 * call replaces the output of the preceding stage (CSR offsets per read, records as the get functions return them). */
/* Segments from elsewhere (layout of ma_batch_get_segments): the segments of read r are segs[seg_off[r] .. seg_off[r+1]).
 * -> ma_extract_seeds_batch.  Contract, checked on the host before anything is uploaded: seg_off starts at 0 and never
 * decreases; q_start, q_size, sa_start and sa_size are not negative; sa_size >= 1; sa_start >= 1 and sa_start + sa_size <= n + 1,
 * n the length of the doubled text (the BWT has the rows 0 .. n; row 0 is the sentinel's, and no interval of the seeding starts
 * there: FMIndex::init_interval, fMIndex.h:772); q_start + q_size + 1 <= the length of the read (q_size is the seed's length
 * minus 1).  Any row range inside these limits is legal, whether the seeding could have found it or not.  sa_start_rc is not
 * read and not checked.  A violation fails the call with "ma_batch_set_segments: ..." naming the read and the segment; the batch
 * then holds no segments (as before ma_seed_batch) and stays usable. */
int ma_batch_set_segments( ma_batch*, const uint64_t* seg_off /*n+1*/, const ma_segment* segs );
/* Seeds from elsewhere (layout of ma_batch_get_seeds): the seeds of read r are seeds[seed_off[r] .. seed_off[r+1]), in the order the
 * sweep's first sort is to see them, as ExtractSeeds leaves them (segment.h:89-113, stripOfConsideration.h:41-53, 97-112): a match
 * at position p of the doubled text (n = 2 F) has r_start = p, on_forward = 1 if p < F, and is mirrored to r_start = n - 1 - p,
 * on_forward = 0 otherwise.  -> ma_chain_batch.  Contract, checked on the host before anything is uploaded: seed_off starts at 0
 * and never decreases; no field is negative; len >= 1; q_start + len <= the length of the read; on_forward is 0 or 1; r_start < F;
 * the match stays inside the doubled text (forward: r_start + len <= n; mirrored: len <= r_start + 1); delta is the value
 * ExtractSeeds computes for the seed, r_start + (length of the read - q_start) + (length of the read + 1) * index of r_start's
 * contig, which the sweep reads as stored (stripOfConsideration.cpp:33, 81).  A seed MAY cross a contig border or the junction
 * of the strands: the reference's extraction checks neither, the seeding finds such matches, and the stage takes them as the
 * reference does (the DP stage answers a set that bridges contigs with the empty alignment).  Duplicated and nested seeds are
 * legal.  A violation fails the call with "ma_batch_set_seeds: ..." naming the read and the seed; the batch then holds no seeds
 * and no strips (as before ma_extract_seeds_batch) and stays usable. */
int ma_batch_set_seeds( ma_batch*, const uint64_t* seed_off /*n+1*/, const ma_seed* seeds ); /* -> ma_chain_batch */
/* Harmonized seed sets from elsewhere (layout of ma_batch_get_hsets): the sets of read r are hset_off[r] .. hset_off[r+1], the
 * seeds of set s are hseeds[hseed_off[s] .. hseed_off[s+1]), hset_soc[s] is its xStats.index_of_strip.  -> ma_dp_batch.
 * Contract, checked on the host before anything is uploaded: hset_off and hseed_off start at 0 and never decrease; no seed
 * has a negative field; q_start + len <= the length of the set's read; r_start + len <= the length of the doubled text
 * (reverse-strand seeds carry positions >= the forward length).  A violation fails the call with "ma_batch_set_hsets: ..."
 * naming the read and the set; the batch then holds no harmonized sets (as before ma_chain_batch) and stays usable.
 * The order of the seeds inside a set is NOT checked: NeedlemanWunsch::execute_one walks them as given, and so does
 * ma_dp_batch; Harmonization hands them over ordered by q_start.  Empty sets and seeds of length 0 are allowed. */
int ma_batch_set_hsets( ma_batch*, const uint64_t* hset_off /*n+1*/, const uint64_t* hseed_off /*n_hsets+1*/,
                        const uint32_t* hset_soc, const ma_seed* hseeds ); /* -> ma_dp_batch */
/* A SoC queue per read that was swept elsewhere (SoCPriorityQueue soc.h:96-420 as StripOfConsideration::execute returns
 * it, stripOfConsideration.cpp:162-173): sorted_seeds = its pSeeds (re-sorted by reference position), socs = its vMaxima
 * array (layout of ma_batch_get_soc_heap).  -> ma_chain_batch, which then runs Harmonization::execute only.  Contract, checked on
 * the host before anything is uploaded: sorted_seeds keep the contract of ma_batch_set_seeds; soc_off starts at 0 and never
 * decreases; a read has no more strips than seeds; begin <= end <= the read's number of seeds and n_seeds == end - begin for
 * every strip (acc_len and ambiguity are the queue's keys and taken as given).  A violation fails the call with
 * "ma_batch_set_soc_heap: ..." naming the read and the strip or seed; the batch then holds no seeds and no strips and stays usable. */
int ma_batch_set_soc_heap( ma_batch*, const uint64_t* soc_off /*n+1*/, const ma_soc* socs, const uint64_t* seed_off /*n+1*/,
                           const ma_seed* sorted_seeds );
/* MappingQuality::execute (mappingQuality.cpp:11-131) alone: alignments that were computed elsewhere (e.g. by the
 * reference's NeedlemanWunsch), per read in the order NeedlemanWunsch::execute left them (needlemanWunsch.h:131-132), in
 * the layout ma_batch_get_alignments returns.  Runs the MappingQuality kernel; ma_batch_get_mapq_alignments then serves
 * its selection (flags, mapping quality, order), ma_batch_get_alignments the input. */
int ma_batch_set_alignments( ma_batch*, const uint64_t* aln_off /*n+1*/, const ma_alignment* alns, const uint64_t* ops );
/* The SoC queue of every read (StripOfConsiderationSeeds::execute stripOfConsideration.cpp:12-161; requires extracted
 * seeds): socs[soc_off[r] .. soc_off[r+1]) are read r's strips in pop() order (SoCPriorityQueue::pop soc.h:240-284, i.e.
 * index_of_strip = position), their seed ranges refer to sorted_seeds[seed_off[r] ..), the read's seeds re-sorted by
 * reference position as rectangularSoC leaves them.  n_socs first (other pointers NULL), then the arrays. */
int ma_batch_get_socs( ma_batch*, uint64_t* n_socs, uint64_t* soc_off /*n+1*/, ma_soc* socs, uint64_t* seed_off /*n+1*/,
                       ma_seed* sorted_seeds );
/* Same arguments, but socs[] is the queue's internal array `vMaxima` (soc.h:140) as StripOfConsiderationSeeds::execute
 * leaves it -- std::make_heap, then rectangularSoC() without re-heapifying (stripOfConsideration.cpp:152-156) -- instead of
 * the pop order.  A binding on the reference's own SoCPriorityQueue fills pSeeds / vMaxima with it and the reference's
 * own pop() (soc.h:240-284) then yields the reference's order. */
int ma_batch_get_soc_heap( ma_batch*, uint64_t* n_socs, uint64_t* soc_off /*n+1*/, ma_soc* socs, uint64_t* seed_off /*n+1*/,
                           ma_seed* sorted_seeds );

/* results: counts first, then download into caller-allocated arrays (any pointer may be NULL) */
int ma_batch_counts( ma_batch*, uint64_t* n_segments, uint64_t* n_seeds, uint64_t* n_hsets, uint64_t* n_hseeds,
                     uint64_t* n_alignments, uint64_t* n_ops, uint64_t* n_aligned_reads );
int ma_batch_get_segments( ma_batch*, uint64_t* seg_off /*n+1*/, ma_segment* segs );
int ma_batch_get_seeds( ma_batch*, uint64_t* seed_off /*n+1*/, ma_seed* seeds );
int ma_batch_get_hsets( ma_batch*, uint64_t* hset_off /*n+1*/, uint64_t* hseed_off /*n_hsets+1*/, uint32_t* hset_soc,
                        ma_seed* hseeds );
int ma_batch_get_alignments( ma_batch*, uint64_t* aln_off /*n+1*/, ma_alignment* alns, uint64_t* ops /*2*n_ops*/ );
int ma_batch_get_mapq_alignments( ma_batch*, uint64_t* aln_off /*n+1*/, ma_alignment* alns, uint64_t* ops );

/* ---- double-buffered I/O of a batch object (the throughput form of the host-to-host path) ----
 * ma_batch_set_reads / ma_batch_get_mapq_alignments put the upload before and the download after a batch's kernels: with B
 * batch objects in flight every object spends that time with nothing of its own on the device.  These four calls move both
 * onto an I/O stream of the batch object, beside its kernels:
 *   ma_batch_stage_reads         starts the upload of the NEXT reads into the object's second read buffer and returns; the kernels
 *                                of the current reads may be running.  `codes` / `offsets` must stay untouched until
 *   ma_batch_use_staged_reads    has returned: it waits for that upload and makes the staged reads the object's reads (what
 *                                ma_batch_set_reads does in one step).
 *   ma_batch_start_mapq_download after ma_align_batch + ma_batch_sync: packs the MappingQuality records (the arrays of
 *                                ma_batch_get_mapq_alignments, same capacities) on the batch's stream and starts their download
 *                                on the I/O stream; returns at once, the next reads may be aligned on the same object meanwhile.
 *   ma_batch_finish_download     waits for it (no-op when none is pending); the host arrays are complete after it.
 * One staged upload and one download can be pending per object.  (No counterpart in the reference, whose containers never
 * leave host memory; the closest is its reader module pulling the next reads while the graph works, module.h:303-369.) */
int ma_batch_stage_reads( ma_batch*, const uint8_t* codes, const uint64_t* offsets, uint64_t n_reads );
int ma_batch_use_staged_reads( ma_batch* );
int ma_batch_start_mapq_download( ma_batch*, uint64_t* aln_off /*n+1*/, ma_alignment* alns, uint64_t* ops );
int ma_batch_finish_download( ma_batch* );
/* ---- paired reads: PairedReads::execute (pairedReads.cpp:14-131) on the device ----
 * Reads 2k and 2k+1 of the batch are the mates of pair k.  ma_pair_batch runs after ma_dp_batch / ma_align_batch on the batch's
 * stream and picks, per pair, one alignment of each mate out of the two MappingQuality lists: the best combined score, times
 * paired_bonus when the two lie on opposite strands mean_paired_dist +- 3 std_paired_dist apart (ties like the reference's
 * std::sort leaves them); the picked records lose secondary / supplementary and may get the pair's mapping quality.  A pair with
 * one empty list yields the other mate's whole list, unchanged.  It reads mean_paired_dist, std_paired_dist, paired_bonus and
 * match of the batch's parameters and does not look at use_paired_reads.  It waits for the stream (the one read-back that
 * sizes the download) and fails -- with a message, launching nothing -- for an odd number of reads or without a MappingQuality
 * output, and with "PairedReads: no alignment of non-zero length to pair" when both lists of a pair hold alignments of length
 * 0 only.  The MappingQuality records themselves stay as they are (ma_batch_get_mapq_alignments still serves them).
 *   ma_batch_pair_counts           pairs, records and ops (pairs of words) of the download; n_host_pairs = pairs whose pick the
 *                                  library finished on the host (several candidates share the best key among more than the 32
 *                                  the kernel sorts on chip; same result, any pointer may be NULL)
 *   ma_batch_get_pairs             pair k's records are alns[pair_off[k] .. pair_off[k+1]), records and ops in the layout of
 *                                  ma_batch_get_mapq_alignments; mate[i] = 1: record of the first mate; other[i] = index of the
 *                                  partner's record WITHIN the pair, -1 for none (any pointer may be NULL)
 *   ma_batch_start_pair_download   the same without the wait, completed by ma_batch_finish_download (cf.
 *                                  ma_batch_start_mapq_download; one download can be pending per object) */
int ma_pair_batch( ma_batch* );
int ma_batch_pair_counts( ma_batch*, uint64_t* n_pairs, uint64_t* n_records, uint64_t* n_ops, uint64_t* n_host_pairs );
int ma_batch_get_pairs( ma_batch*, uint64_t* pair_off /*n_pairs+1*/, ma_alignment* alns, uint64_t* ops /*2*n_ops*/, int32_t* mate,
                        int32_t* other );
int ma_batch_start_pair_download( ma_batch*, uint64_t* pair_off /*n_pairs+1*/, ma_alignment* alns, uint64_t* ops, int32_t* mate,
                                  int32_t* other );
/* ---- small inversions: SmallInversions::execute (smallInversions.h:22-221) on the device ----
 * The module that sits between MappingQuality and PairedReads / FileWriter in the reference's graph (export.cpp:118-121), for a
 * whole batch: replaces the host module ma_amd::SmallInversions (Alignment containers, ma_pack_extract + ma_ksw_batch round
 * trips) on the flat paths.  ma_inversions_batch runs after ma_dp_batch / ma_align_batch / ma_batch_set_alignments on the batch's
 * stream.  Per record of every MappingQuality list it looks for the stretches between two seeds in which the running score
 * falls zdrop_inversion below its maximum (forAllDropPos, smallInversions.h:53-116), aligns each stretch's query against the
 * reverse-strand window of its reference interval with the kernels of ma_ksw_batch (bandwidth_ext, zdrop, flag 0), splits the M
 * runs into matches and mismatches and keeps the alignment if it scores more than harm_score_min * match (always with
 * disable_heuristics): supplementary, mapping quality 0, the parent's soc_index.  It reads zdrop_inversion, zdrop, bandwidth_ext,
 * harm_score_min, disable_heuristics and the six scores (sv_penalty through Alignment::append) of the batch's parameters and does
 * not look at search_inversions.  It waits for the stream twice: with the read-back of the candidates' number and shapes that
 * sizes the DP launches, and with the records and ops kept; a batch without any candidate waits once and launches one kernel.
 * (Only a batch with more candidates than any before it on the object, or one whose ops pool has no room left, waits once more.)
 * It fails -- with a message that names the read and the record, launching nothing more, the object stays usable -- for a stretch
 * that ends beyond its read or whose window does not lie inside one strand of the doubled text (possible only through
 * ma_batch_set_alignments); nothing outside a read or the text is ever read.
 * Afterwards the lists "after MappingQuality" ARE the final lists, each kept inversion record directly behind its parent,
 * several of one parent in the order of their stretches: ma_batch_get_mapq_alignments, ma_batch_start_mapq_download, n_alignments
 * / n_ops of ma_batch_counts (the capacities of those downloads), ma_pair_batch, ma_sam_batch (with MA_SAM_NGMLR_TAGS too) and
 * ma_pair_sam_batch serve them; ma_batch_get_alignments, ma_batch_get_hsets and the SoC getters serve what they served.  The
 * call always starts from the MappingQuality output (twice gives the same lists).
 *   ma_batch_inversion_counts  drop stretches found, DP jobs among them (both sides non-empty), inversion records kept (any
 *                              pointer may be NULL) */
int ma_inversions_batch( ma_batch* );
int ma_batch_inversion_counts( ma_batch*, uint64_t* n_candidates, uint64_t* n_jobs, uint64_t* n_records );
/* ---- SAM text: FileWriter::execute (fileWriter.cpp:11-158) on the device ----
 * The single-end records of a batch as the bytes the reference's FileWriter prints for them (and ma_amd/host/ma_sam.h, the
 * yardstick, makes of the MappingQuality records), formatted by two kernels and downloaded as ONE text instead of records and
 * ops: per alignment of a read's MappingQuality list one record with Alignment::getSamFlag / getSamPosition / cigarString /
 * getQuerySequence (alignment.h:367-467, 576-623), the CG:B:I tag of cigars from 0x10000 ops on (TagGenerator, fileWriter.h:
 * 327-357), the unmapped record (fileWriter.cpp:126-140) for a read without a printed alignment.  With MA_SAM_NGMLR_TAGS every
 * record also carries the tags of "Emulate NGMLR's tag output" (TagGenerator::computeTag, fileWriter.h:120-326): MD SV AS NM
 * XI XE XR CV SA QS QE, with the CIGAR column M-style and the insertion / deletion pairs of reverse-strand records swapped as
 * the reference's writer leaves them (fileWriter.cpp:27-31); the bases come from the index's packed text, the runs of N from
 * ma_index_set_holes.  The paired writer is the block below; for paired text the tag emulation stays on the host.
 *   ma_index_set_contig_names    the RNAME strings (Pack::nameOfSequenceWithId, pack.h:1040-1046): contig i's name is
 *                                names[name_off[i] .. name_off[i+1]) (no terminators)
 *   ma_index_set_holes           the runs of N of the input that random bases replaced (Pack::vAppendSequence, pack.h:630-666;
 *                                the .amb file): (start, length) on the forward strand, sorted, not overlapping, inside it;
 *                                read by the NM and SV tags.  Setting again replaces the list; an index without the call has
 *                                no holes.  Like the names it is set while no batch of the index runs.
 *   ma_batch_set_read_text       QNAME (NucSeq::sName) and QUAL (NucSeq::pxQualityValues / fastaq quality, nucSeq.h:697-709) of
 *                                the batch's reads, after the reads were set: read r's name is names[name_off[r] ..
 *                                name_off[r+1]), qual is NULL (QUAL "*") or holds one character per base in the reads' CSR.
 *                                Without it ma_sam_batch fails with a message.
 *   ma_sam_batch                 after ma_dp_batch / ma_align_batch / ma_batch_set_alignments on the batch's stream; options =
 *                                MA_SAM_* (the members of FileWriter's settings it serves).  Waits for the stream with the one
 *                                read-back that sizes the download.  A record that ends beyond its read (possible only through
 *                                ma_batch_set_alignments) fails the call with the reference's text, "Query length is off by
 *                                <n>." or "Index out of range (compCharAt)"; nothing beyond a read is ever touched.  With
 *                                MA_SAM_NGMLR_TAGS two more: a record across the two strands or beyond the doubled text fails
 *                                with the reference's "(vExtractSubsection) Try to extract bridging sequence. This is
 *                                impossible.", one whose ops do not cover exactly [begin_ref, end_ref) and [begin_q, end_q)
 *                                with a message that names it; nothing outside [begin_ref, end_ref) of the text is read.
 *   ma_batch_sam_counts          bytes of the text
 *   ma_batch_get_sam             read r's records are text[rec_off[r] .. rec_off[r+1]) (either pointer may be NULL)
 *   ma_batch_start_sam_download  the same without the wait, completed by ma_batch_finish_download (cf.
 *                                ma_batch_start_mapq_download; one download can be pending per object)
 * The MappingQuality records stay as they are (ma_batch_get_mapq_alignments still serves them). */
#define MA_SAM_SOFT_CLIP 1u /* xSoftClip: S clips and the whole read as SEQ instead of H clips */
#define MA_SAM_EQX_CIGAR 2u /* xOutputMCigar off: = and X instead of M */
#define MA_SAM_NO_SECONDARY 4u /* xNoSecondary */
#define MA_SAM_NO_SUPPLEMENTARY 8u /* xNoSupplementary */
#define MA_SAM_NO_CG_TAG 16u /* xCGTag off: cigars of 0x10000 ops and more are printed in the CIGAR column */
#define MA_SAM_NGMLR_TAGS 32u /* xEmulateNgmlrTags (ma_sam_batch only): the tags MD SV AS NM XI XE XR CV SA QS QE */
int ma_index_set_contig_names( ma_index*, const char* names, const uint64_t* name_off /*n_contigs+1*/ );
int ma_index_set_holes( ma_index*, const uint64_t* start, const uint64_t* length, uint64_t n );
int ma_batch_set_read_text( ma_batch*, const char* names, const uint64_t* name_off /*n+1*/, const uint8_t* qual );
int ma_sam_batch( ma_batch*, uint32_t options );
int ma_batch_sam_counts( ma_batch*, uint64_t* n_bytes );
int ma_batch_get_sam( ma_batch*, uint64_t* rec_off /*n+1*/, char* text );
int ma_batch_start_sam_download( ma_batch*, uint64_t* rec_off /*n+1*/, char* text );
/* ---- paired-end SAM text: PairedFileWriter::execute (fileWriter.cpp:158-383) on the device ----
 * The records of a batch's mate pairs (ma_pair_batch) as the bytes the reference's PairedFileWriter prints for them (and
 * ma_amd/host/ma_sam.h, the yardstick, makes of the records of ma_batch_get_pairs), formatted by two kernels from what is in
 * device memory after ma_pair_batch -- nothing is uploaded, nothing packed -- and downloaded as ONE text: per printed record of
 * a pair FLAG with 0x1 | 0x2 | 0x40 / 0x80 (| 0x20: partner on the reverse strand), RNEXT / PNEXT of the partner ("=" on a
 * contig of the same NAME), TLEN 0, MAPQ capped at 255, the cigar's left-over clip taken against the FIRST mate's length (sic);
 * two records for a pair without any printed record (FLAG 0x4 | 0x1 | 0x40 / 0x80 | 0x8, QUAL printed); for one mate without a
 * printed record one record at record 0 of the pair's list (RNEXT "=", QUAL "*").  Contig names and read text as above.
 *   ma_pair_sam_batch                 after ma_pair_batch on the batch's stream; options = MA_SAM_*.  Waits for a pending
 *                                     download, then for the stream with the one read-back that sizes the download.  A record
 *                                     that ends beyond its own mate (possible only through ma_batch_set_alignments) fails the
 *                                     call with the reference's text as ma_sam_batch does; the object stays usable.
 *   ma_batch_pair_sam_counts          pairs (n / 2) and bytes of the text
 *   ma_batch_get_pair_sam             pair k's records are text[pair_off[k] .. pair_off[k+1]) (either pointer may be NULL)
 *   ma_batch_start_pair_sam_download  the same without the wait, completed by ma_batch_finish_download (one download can be
 *                                     pending per object)
 * The text is kept apart from the single-end one: ma_batch_get_sam never returns pair text, and ma_batch_get_pairs /
 * ma_batch_get_mapq_alignments serve their records as before. */
int ma_pair_sam_batch( ma_batch*, uint32_t options );
int ma_batch_pair_sam_counts( ma_batch*, uint64_t* n_pairs, uint64_t* n_bytes );
int ma_batch_get_pair_sam( ma_batch*, uint64_t* pair_off /*n_pairs+1*/, char* text );
int ma_batch_start_pair_sam_download( ma_batch*, uint64_t* pair_off /*n_pairs+1*/, char* text );
/* ---- read text in: FileReader::execute (fileReader.cpp:37-203) + NucSeq's translation (nucSeq.cpp:17-28) on the device ----
 * A FASTQ or FASTA text -- a whole file, or a run of whole records cut out of one -- uploaded as it is and parsed by kernels
 * (ma_amd/csrc/stage_text.h), byte-parallel: replaces the reader module, one NucSeq per read, the gather into code / name /
 * quality arrays and their three uploads.  The device parses the STRICT form, stated once in ma_amd/host/ma_text_dev.h -- four-line
 * FASTQ records, FASTA records of any number of non-empty lines, "\n" or "\r\n", names up to the first blank, bases up to a line's
 * last IUPAC letter -- and refuses every other text with "ma_batch_set_reads_text: line <L> (byte <X>): <reason>", the lowest
 * offending line (1-based) and the offset of its first byte.  It never guesses: the reference's reader on the host stays the path
 * for other files.
 *   ma_batch_set_reads_text  text: host memory, n_bytes < 2 GiB.  Uploads, parses and waits (two read-backs: the line count that
 *                            sizes the per-line work, then reads / bases / name bytes / longest read / refusal).  Afterwards
 *                            the batch is exactly as after ma_batch_set_reads + ma_batch_set_read_text: FASTQ gives qualities,
 *                            FASTA none (QUAL "*"); ma_align_batch, ma_inversions_batch and ma_sam_batch run unchanged.
 *                            n_bytes == 0 gives 0 reads.  More reads than max_reads or more bases than max_bases fail with
 *                            "batch capacity exceeded" (*n_reads then is the number of reads the text holds; it is 0 after
 *                            every other failure).  After ANY failure the batch holds no reads and no text and stays usable.
 *   ma_batch_read_counts     reads, bases, name bytes (0 without text) and whether there are qualities (any pointer may be NULL)
 *   ma_batch_get_reads       the codes (A0 C1 G2 T3, other 4; nucSeq.cpp:17-28) and CSR offsets of the batch's reads, however they
 *                            were set (ma_batch_set_reads, ma_batch_set_reads_device, text); either pointer may be NULL
 *   ma_batch_get_read_text   QNAME and QUAL as ma_batch_set_read_text takes them (any pointer may be NULL; qual must be NULL
 *                            when the reads have none); fails with a message when no text was set */
int ma_batch_set_reads_text( ma_batch*, const char* text /*host*/, uint64_t n_bytes, uint64_t* n_reads );
int ma_batch_read_counts( ma_batch*, uint64_t* n_reads, uint64_t* n_bases, uint64_t* n_name_bytes, int32_t* has_qual );
int ma_batch_get_reads( ma_batch*, uint64_t* offsets /*n+1*/, uint8_t* codes );
int ma_batch_get_read_text( ma_batch*, uint64_t* name_off /*n+1*/, char* names, uint8_t* qual /*may be NULL*/ );
/* ---- paired read text in: PairedFileReader::execute (fileReader.h:568-617) on the device ----
 * Two texts, the R1 and R2 file of a paired-end run or runs of whole records cut out of them, uploaded as they are and parsed
 * by the kernels of ma_batch_set_reads_text, each by exactly its strict rules (ma_amd/host/ma_text_dev.h; ma_text::pairHost is
 * the serial statement of this call): replaces one NucSeq per mate, the host's reverse complement of every second mate, the
 * gather and three uploads.  Record k of text 1 becomes read 2k, record k of text 2 read 2k + 1; with R1 and R2 records there are
 * R = min( R1, R2 ) pairs -- the shorter file ends the stream, as in the reference.  With rev_comp_mates != 0 (the reference's
 * default, xRevCompPairedReadMates) every read 2k + 1 is reversed with its qualities (NucSeq::vReverse, nucSeq.h:373-381) and
 * complemented (vSwitchAllBasePairsToComplement, nucSeq.h:537-543: a code below 4 becomes 3 - c, every other code 5 (sic));
 * names are untouched.
 *   ma_batch_set_mates_text  texts: host memory, each < 2 GiB.  Uploads, parses and waits (two read-backs: the line counts of
 *                            both texts in one copy, then the statistics).  Afterwards the batch is exactly as after
 *                            ma_batch_set_reads on the 2 R interleaved reads + ma_batch_set_read_text (qualities iff FASTQ):
 *                            ma_align_batch, ma_inversions_batch, ma_pair_batch, ma_pair_sam_batch and the getters above run
 *                            unchanged.  *n_pairs = R; consumed[i] = offset in text i of the first byte of record R (n_i when
 *                            the text has exactly R records): a caller carries text_i + consumed[i] into its next call.
 *                            Records beyond R are validated -- a violation anywhere refuses the call -- but count neither
 *                            against the capacity nor into any sum.  n1 == 0 or n2 == 0 gives 0 pairs (the other text is
 *                            still validated).  Refusals, in this order; each leaves the batch without reads and text and
 *                            usable, *n_pairs = 0 and consumed = {0, 0} unless stated:
 *                              "ma_batch_set_mates_text: text <1|2>: line <L> (byte <X>): <reason>"  a rule violation; text 1
 *                                wins over text 2, within a text the lowest line, then the lowest reason
 *                              "ma_batch_set_mates_text: the two texts differ in kind"  one FASTQ, one FASTA
 *                              "ma_batch_set_mates_text: batch capacity exceeded"  2 R > max_reads or more paired bases than
 *                                max_bases; *n_pairs = R then, what a caller sizes the next batch object by */
int ma_batch_set_mates_text( ma_batch*, const char* text1 /*host*/, uint64_t n1, const char* text2 /*host*/, uint64_t n2,
                             int32_t rev_comp_mates, uint64_t* n_pairs, uint64_t consumed[ 2 ] );
/* ---- compressed read text in: BGZF members inflated on the device ----
 * BGZF (what bgzip and htslib write, and what every zlib reader reads as ordinary gzip) is a chain of independent gzip members
 * of at most 64 KiB of text each, every one with its compressed size in its header.  The compressed bytes are uploaded as they
 * are, every member is inflated by a lane of its own (ma_amd/csrc/stage_bgzf.h) into the buffer the parser of
 * ma_batch_set_reads_text reads, and that call's kernels run behind it unchanged.  The STRICT member form and the deflate
 * streams accepted -- exactly zlib's -- are stated once in ma_amd/host/ma_bgzf_dev.h (ma_bgzf::inflateHost is the serial
 * statement): bytes 1f 8b 08 04, one BC subfield of SLEN 2 among the extra field's subfields, BSIZE + 1 inside the data,
 * ISIZE <= 65536, a deflate stream that fills its bytes exactly, inflates to ISIZE bytes and has the trailer's CRC32; a member
 * of ISIZE 0 (the 28-byte end-of-file marker) may stand anywhere.  A file that is ONE gzip member has no such parallelism and
 * is refused by name: it stays with the host's gzip stream.
 *   ma_batch_set_reads_bgzf  head: n_head bytes of text (host, may be NULL with n_head 0); members: n_bytes of whole members
 *                            (host).  The text T is head followed by what the members inflate to, in order, minus its last
 *                            n_drop bytes: head and n_drop let a caller cut a compressed stream into runs of whole records by
 *                            inflating only the last member of a chunk on the host -- the bytes it drops are the next call's
 *                            head -- so that no batch waits for the one before it.  T must be a run of whole records in the
 *                            strict form of ma_batch_set_reads_text; afterwards the batch is exactly as after that call on T.
 *                            Uploads, inflates, parses and waits: TWO read-backs (the line feeds, the inflate's verdict and
 *                            T's first and last byte in one copy; then the statistics, as ma_batch_set_reads_text's second).
 *                            n_bytes == 0 parses the head alone; nothing at all gives 0 reads.  Refusals; each leaves the
 *                            batch without reads and text and usable, and *n_reads = 0 unless stated:
 *                              "ma_batch_set_reads_bgzf: member <k> (byte <X>): <reason>"  member k (0-based), whose first
 *                                byte is at offset X of `members`: the first bad header (found on the host: nothing is
 *                                launched), else the lowest member whose stream or trailer is refused.  The reasons: not
 *                                BGZF ("a gzip member without the BGZF size field: single-member gzip stays with
 *                                GzFileStream ..."), truncated member, ISIZE too large, one per deflate violation, length
 *                                mismatch, CRC mismatch
 *                              "ma_batch_set_reads_bgzf: n_drop is larger than the inflated part of the text"
 *                              "ma_batch_set_reads_bgzf: text: line <L> (byte <X>): <reason>"  a violation in T, L and X as
 *                                in ma_batch_set_reads_text but counted in T, the reasons that call's (a T of 2 GiB or more:
 *                                its "too large")
 *                              "ma_batch_set_reads_bgzf: batch capacity exceeded"  *n_reads = the reads T holds
 *                            With ma_batch_enable_timing, ma_batch_kernel_ms [6] is the time of the two inflate kernels. */
int ma_batch_set_reads_bgzf( ma_batch*, const char* head /*host, may be NULL*/, uint64_t n_head, const void* members /*host*/,
                             uint64_t n_bytes, uint64_t n_drop, uint64_t* n_reads );
/* ---- compressed paired read text in: the two BGZF files of a paired-end run inflated on the device ----
 * ma_batch_set_reads_bgzf's inflate in front of ma_batch_set_mates_text's parse: for each side i, T_i is head followed by what
 * members inflate to, minus its last n_drop bytes, in the strict member form above; the call then is
 * ma_batch_set_mates_text( T_1, T_2, rev_comp_mates ).  The rules and the order of the refusals are stated once in
 * ma_amd/host/ma_mates_bgzf_dev.h (ma_bgzf::pairBgzfHost is the serial statement).  The member borders of two compressed files
 * say nothing about record counts, so a caller cannot cut whole pairs: it cuts each stream into runs of whole records as for
 * ma_batch_set_reads_bgzf, and carries what the device left over of either text into the next call's head.
 *   ma_batch_set_mates_bgzf  side[i]: as the arguments of ma_batch_set_reads_bgzf (host memory; head / members may be NULL with
 *                            their size 0).  Both chains are inflated by ONE launch of the inflate kernels over a joint member
 *                            table; uploads, inflates, parses and waits: TWO read-backs (the line feeds of both texts, the
 *                            inflate's verdict and the first and last byte of both texts in one copy; then the statistics, as
 *                            ma_batch_set_mates_text's second).  Afterwards the batch is exactly as after
 *                            ma_batch_set_mates_text( T_1, T_2 ): the same reads, names and qualities, *n_pairs = R and
 *                            consumed[i] = offset in T_i of the first byte of record R; text_bytes[i] = |T_i|.  An empty T_i
 *                            gives 0 pairs (the other text is still validated); records beyond R are validated, but neither
 *                            counted nor checked against the capacity.  Refusals, in this order; each leaves the batch without
 *                            reads and text and usable, *n_pairs = 0 and consumed = text_bytes = {0, 0} unless stated:
 *                              "ma_batch_set_mates_bgzf: null argument"
 *                              "ma_batch_set_mates_bgzf: text <1|2>: member <k> (byte <X>): <reason>"  k (0-based) and X count
 *                                within that side's members: a bad header found on the host -- text 1's first, else text 2's
 *                                first; nothing is launched -- else the lowest member of text 1 whose stream or trailer the
 *                                device refuses, else the lowest of text 2.  A member that does not inflate wins over every
 *                                refusal below: a text that did not inflate is not parsed
 *                              "ma_batch_set_mates_bgzf: text <1|2>: n_drop is larger than the inflated part of the text"
 *                              "ma_batch_set_mates_bgzf: text <1|2>: line <L> (byte <X>): <reason>"  ma_batch_set_mates_text's
 *                                refusal, L and X counted in T_i.  (A T_i of 2 GiB or more gets its "too large" before
 *                                anything is launched: behind a bad header, in front of everything else.)
 *                              "ma_batch_set_mates_bgzf: the two texts differ in kind"
 *                              "ma_batch_set_mates_bgzf: batch capacity exceeded"  *n_pairs = R
 *                            With ma_batch_enable_timing, ma_batch_kernel_ms [6] is the time of this call's inflate kernels.
 *   ma_batch_get_mates_rest  T_which[ consumed .. |T| ), the records beyond the last pair, which a streaming caller puts in front
 *                            of the next call's head: *n_bytes, and the bytes with out != NULL -- a copy out of the batch's
 *                            text buffer on its stream, no kernel; waits.  Valid from a successful ma_batch_set_mates_bgzf
 *                            until the next call that sets reads in any form (ma_batch_set_reads, _set_reads_device,
 *                            _use_staged_reads, _set_reads_text, _set_reads_bgzf, _set_mates_text, _set_mates_bgzf; not
 *                            ma_batch_set_read_text, which replaces names and qualities only); otherwise it fails with
 *                            "ma_batch_get_mates_rest: run ma_batch_set_mates_bgzf first". */
typedef struct
{
    const char* head; /* host, may be NULL with n_head 0 */
    uint64_t n_head;
    const void* members; /* host, whole BGZF members */
    uint64_t n_bytes;
    uint64_t n_drop;
} ma_bgzf_text;
int ma_batch_set_mates_bgzf( ma_batch*, const ma_bgzf_text side[ 2 ], int32_t rev_comp_mates, uint64_t* n_pairs, uint64_t text_bytes[ 2 ],
                             uint64_t consumed[ 2 ] );
int ma_batch_get_mates_rest( ma_batch*, int32_t which /*0 | 1*/, uint64_t* n_bytes, char* out /*may be NULL: count only*/ );
/* ---- compressed SAM text out: the text of a batch deflated on the device into BGZF members ----
 * The SAM text of the last ma_sam_batch / ma_pair_sam_batch is cut at fixed offsets -- member k holds text[65280 k ..
 * min(65280 (k+1), n)), so ceil(n / 65280) members and none for an empty text -- and every member is deflated by a wavefront
 * of its own (ma_amd/csrc/stage_deflate.h): one dynamic-Huffman block over an LZ77 parse, or one stored block where that is
 * not smaller, in the member form htslib writes (18 header bytes with BSIZE, the stream, CRC32, ISIZE), which is the strict
 * form ma_batch_set_reads_bgzf accepts.  The cuts, the parse, the codes and so every byte are stated once in
 * ma_amd/host/ma_deflate_dev.h; ma_bgzf::deflateHost is the serial statement and gives the same bytes.  Records may straddle
 * members, so the members of consecutive batches, written one after the other and closed with the 28-byte end-of-file marker,
 * are a file samtools, zcat and gzip read.  No member is larger than its text + 31 bytes.
 *   ma_sam_bgzf_batch                 pair == 0: the text of the last ma_sam_batch, else of the last ma_pair_sam_batch; on the
 *                                     batch's stream; waits once, with the one read-back of the compressed size.  Fails with a
 *                                     message when that text has not been made.  The text itself stays (ma_batch_get_sam /
 *                                     ma_batch_get_pair_sam still serve it).
 *   ma_batch_sam_bgzf_counts          members and their bytes
 *   ma_batch_get_sam_bgzf             the members packed back to back; member k is bytes[member_off[k] .. member_off[k+1])
 *                                     (either pointer may be NULL)
 *   ma_batch_start_sam_bgzf_download  the same without the wait, completed by ma_batch_finish_download (one download can be
 *                                     pending per object: a second one is refused under this call's name)
 *   ma_bgzf_deflate                   the primitive: n_bytes of any host bytes through the same kernels on the index's device
 *                                     (the index only names it).  out == NULL only counts (*n_members, *n_out); else cap is the
 *                                     room behind out, and one that is too small fails with the size needed in the message.
 * With ma_batch_enable_timing, ma_batch_kernel_ms [7] is the time of the deflate kernels of the last ma_sam_bgzf_batch (the call
 * then also waits for their end). */
int ma_sam_bgzf_batch( ma_batch*, int32_t pair );
int ma_batch_sam_bgzf_counts( ma_batch*, int32_t pair, uint64_t* n_members, uint64_t* n_bytes );
int ma_batch_get_sam_bgzf( ma_batch*, int32_t pair, uint64_t* member_off /*n_members+1*/, void* bytes );
int ma_batch_start_sam_bgzf_download( ma_batch*, int32_t pair, uint64_t* member_off /*n_members+1*/, void* bytes );
int ma_bgzf_deflate( const ma_index*, const void* text /*host*/, uint64_t n_bytes, uint64_t* n_members, uint64_t* n_out,
                     uint64_t* member_off /*may be NULL*/, void* out /*may be NULL*/, uint64_t cap );
/* work counters for the roofline model (same meaning as the oracle's): [0] extend_backward steps,
 * [1] distinct occ blocks touched, [2] bwt_sa LF steps, [3] SA rows, [4] DP band cells, [5] ksw jobs */
int ma_batch_counters( ma_batch*, uint64_t out[ 8 ] );
/* diagnostics: the kswcpp calls of the last ma_dp_batch, 8 x int32 per call:
 * qlen, tlen, w, zdrop, flag, ez.zdropped, ez.max_q, ez.max_t (shapes may be NULL to only count) */
int ma_batch_get_dp_jobs( ma_batch*, uint64_t* n_jobs, int32_t* shapes, uint64_t cap );
/* per-kernel HIP-event times of the last stage calls in ms: [0] seeding [1] sa-lookup [2] chaining
 * [3] dp-jobs [4] ksw [5] stitch; [6] the inflate of the last ma_batch_set_reads_bgzf / ma_batch_set_mates_bgzf; [7] the deflate of the last ma_sam_bgzf_batch; requires ma_batch_enable_timing(b,1) */
int ma_batch_enable_timing( ma_batch*, int on );
int ma_batch_kernel_ms( ma_batch*, float out[ 8 ] );
/* host wall time in ms of the stage calls of the last ma_align_batch: [0] seed [1] extract [2] chain [3] dp (launches,
 * stream waits and size read-backs included: what a small batch pays beside its kernels) */
int ma_batch_host_ms( ma_batch*, float out[ 8 ] );
/* diagnostics: extension jobs tried on the proven narrow band (ma_amd/csrc/ksw_band.h; MA_KSW_GRP=3) since the library was loaded on
 * the current device: tried, proved, failed check 1 / 2 / 3 / 4, handed back for another reason, diagonals run */
int ma_debug_band_stats( unsigned long long out[ 8 ] );
/* the same for the LONG extension jobs (queries beyond 254 bases: the end extensions of long reads, needlemanWunsch.cpp:708-716,
 * 781-782), one per wavefront on the proven band of 120 cells (ksw_band.h, G = 1; MA_KSW_BANDL=0 switches it off) */
int ma_debug_band_long_stats( unsigned long long out[ 8 ] );
/* diagnostics: kswcpp cells computed / calls answered per DP kernel family since the library was loaded (what bench.py divides a
 * family's instruction count of the rocprofv3 PMC pass by): out[2f], out[2f+1] for f = 0 k_ksw_ext<1>, 1 k_ksw_ext<2>,
 * 2 k_ksw_grp<2>, 3 k_ksw_grp<4>, 4 k_ksw_band (short jobs), 5 k_ksw_pk, 6 k_ksw (state in LDS), 7 k_ksw_band (long jobs); all of
 * them restate kswcpp_core.h:308-879 */
int ma_debug_dp_family_stats( unsigned long long out[ 16 ] );
/* diagnostics: the device libm the chaining stage decides with (harmonization.h:82-89, ransac.cpp:112,131-135 use
 * glibc's): op 0 tan, 1 sin, 2 atan, 3 log over n doubles (host arrays); tests compare the bits with glibc's */
int ma_debug_libm( int op, const double* in, uint64_t n, double* out );
/* diagnostics: the single-precision arithmetic and the "%f" formatter of the XI:f (kind 0: num / den) and CV:f (kind 1:
 * 100 * num / den) tags of MA_SAM_NGMLR_TAGS as the kernels run them, over n pairs (host arrays); pair i's text goes to
 * out[16 i ..), padded with NUL (empty where it would not fit); tests compare with printf of the same arithmetic in float */
int ma_debug_ngmlr_floats( int kind, const uint64_t* num, const uint64_t* den, uint64_t n, char* out /*16 n*/ );

/* ---- synthetic workloads (BASELINE.json configs; deterministic counter-based generators) ---- */
/* genome: d_codes[total] (device, 1 byte/base). reads sampled from it: device CSR. */
int ma_synth_genome_device( uint64_t seed, uint64_t total_len, int32_t with_repeats, void* d_codes );
int ma_synth_reads_device( const ma_index*, uint64_t seed, uint64_t n_reads, uint32_t read_len, double sub_rate,
                           double ins_rate, double del_rate, uint64_t first_read_index, void* d_codes,
                           void* d_offsets, uint64_t codes_cap, uint64_t* n_bases );

#ifdef __cplusplus
}
#endif
#endif /* MA_AMD_H */
