/*
 * peppan_hip.h - C ABI of libpeppan_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the one data-parallel hot path of PEPPAN: the similarity search that
 * modules/uberBlast.py delegates to the `diamond` executable and the single-linkage grouping
 * of its hits.  Plain pointers and sizes only; every buffer handed IN is caller-owned and only
 * read; every buffer handed OUT is filled into caller-allocated memory (sizes are queried first),
 * except pep_result handles, which are released with pep_result_free.  A pep_result stays valid and unchanged
 * whatever is called on its context afterwards (the newest one is served from the context's pinned staging area and is
 * given its own copy before that area is reused).
 *
 * All functions returning int return PEP_OK (0) or a negative PEP_ERR_* code; the message of the
 * last failure on a context is available from pep_last_error().  Nothing is ever silently dropped:
 * capacity problems are errors, not truncation.
 *
 * Threading: one context per GPU; calls on one context must be serialised by the caller; distinct
 * contexts are independent.  A context must be created in the process that uses it (HIP state does
 * not survive fork(); the reference calls uberBlast from forked pool workers, PEPPAN.py:922).
 *
 * Reference interface each entry point replaces (file:line in zheminzhou/PEPPAN):
 *   pep_set_query_nt + K1   transeq(frame='F') + per-gene frame choice     uberBlast.py:525-529, configure.py:160-194
 *   pep_set_ref_nt   + K1   transeq(frames 6|3) + stop-codon chunking      uberBlast.py:535-544
 *   pep_search              `diamond makedb` + 5 x `diamond blastp ... --outfmt 101`   uberBlast.py:531-533, 546-552
 *   pep_hit fields          the SAM fields parseDiamond consumes (POS, CIGAR, |SEQ|, NM, ZR, ZS)   uberBlast.py:25-58
 *   pep_rescore_nt          cigar2score mode 1 inside RunBlast.reScore      uberBlast.py:226-249, 397-415
 *   pep_rescore_codons(_check)   cigar2score modes 2 / 3 (amino-acid / codon-position scoring) inside RunBlast.reScore   uberBlast.py:250-269, 397-415
 *   pep_components(_of_hits) union-find of get_gene_group (partition only)  PEPPAN.py:1598-1607
 *   pep_linclust            `mmseqs createdb / linclust / createtsv`        clust.py:62-66
 *   pep_overlaps            numba tab2overlaps inside returnOverlap          uberBlast.py:73-97, 378-395
 *   pep_sha1, pep_dedup     hashlib.sha1 per gene + the duplicate collapse of writeGenes   PEPPAN.py:62, 1019, 1023-1039
 *   pep_ovl_filter          RunBlast.ovlFilter (host C++)                    uberBlast.py:417-452
 *   pep_linear_merge        RunBlast.linearMerge + _linearMerge (host C++)   uberBlast.py:100-218, 453-460
 *   pep_alleles             aligned-allele strings + base-5 packing of iter_map_bsn   PEPPAN.py:812-835, 846-848
 *   pep_allele_diff         numba compare_seq / compare_seqX of filt_per_group over the rows of the .seq store   PEPPAN.py:296-316, 332-333
 *   pep_group_verdicts      checkDiv over the edge rows, the distances test and the leader grouping of filt_per_group   PEPPAN.py:335-344, 352-366, 371-392
 *   pep_gene_ingroups       determineGroup inside initializing2: the in-group rows of every gene of the .tab store and the gene's score   PEPPAN.py:1041-1056, 1058-1076
 *   pep_store_mat_member / pep_store_seq_member   the 1000-group members of the .mat / .seq stores get_map_bsn writes (host C++:
 *                           the .npy pickle stream emitted from the numeric hit table)   PEPPAN.py:950-966
 *   pep_table_from_hits / pep_cols_fix_end / pep_cols_order / pep_cols_gather   RunBlast.run's numeric chain between a search and the caller (host C++:
 *                           parseDiamond / parseBlast columns, fixEnd, the final sort)   uberBlast.py:25-58, 275-290, 375, 462-480
 *   pep_store_tab_members   all members of the .tab store (gene -> int rows) as finished zip entries, host threads   PEPPAN.py:91-113, 972-975
 *   pep_similar_classify / pep_similar_scan / pep_pair_support / pep_similar_resolve   the pass of get_similar_pairs over the all-vs-all table and its
 *                           get_similar (row-local tests, host state machine, K14 on the GPU, host dictionary)   PEPPAN.py:195-224, 231-276, 294
 *   pep_known_order         compare_prediction over a genome's hit table (host C++)   PEPPAN.py:869-901
 *   pep_synteny_pairs (+ _copy, _check)   the pair loop of ite_synteny_resolver: distance, conflict pairs, the sort of the pairs   PEPPAN.py:1101-1117
 *   pep_synteny_walk                      its merge walk and verdict (host C++, no context)                                     PEPPAN.py:1118-1151
 *   pep_gene_structure (+ _check)   determineGeneStructure for every intact prediction of write_output: the marked-start translation
 *                                   of the window in the tried frames and the search for start and stop   PEPPAN.py:1193-1229
 *   pep_rarefaction_curves (+ _check)   the n_iter x n_genomes loop of writeCurve: genes seen in at least one / in all of the first
 *                                       k + 1 genomes of every random genome order                      PEPPAN_parser.py:74-80
 *   pep_profile_pairs (+ _check)        the pair loop of getDistance: per pair of allelic profiles the genes both carry and the
 *                                       genes where both carry the same allele                          PEPPAN_parser.py:172-179
 *   pep_kimura_pairs, pep_nj_trees (+ _check)   the two rapidnj calls: `rapidnj -i fa -t d` per paralogous group of filt_per_group and
 *                                       `rapidnj -i pd` behind writeCGAV                                 PEPPAN.py:19, 409-417, PEPPAN_parser.py:168
 *   pep_global_diff_walk (+ _size, _copy, _free; host C++) / pep_global_diff (+ _copy, _check)   get_global_difference: the dictionary walk over the
 *                                       selected rows / the cross products per genome pair and their two means   PEPPAN.py:1611-1666
 *   pep_cds_genes (+ _check)            the per-gene work of the GFF front end: iter_readGFF, checkPseu, addGenes   PEPPAN.py:117-182, 992-1010, 1013-1021
 *   pep_out_alleles (+ _check)          the allele pass of write_output: windows, allele bytes, allele numbers   PEPPAN.py:1391-1472
 *   pep_tree_cut (+ _check)             the tree cutting of filt_per_group, which the reference does with ete3   PEPPAN.py:424-482
 *   pep_batch_screen / pep_batch_unsure_walk (host C++) / pep_batch_prune (+ _check each)   the front half of every round of filt_genes   PEPPAN.py:546-656
 */
#ifndef PEPPAN_HIP_H
#define PEPPAN_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 17 gained, additively, the K16 entry points: pep_group_verdicts, pep_group_verdicts_check, pep_verdict_detail_size, pep_verdict_detail_copy,
 * pep_verdict_result_free, pep_group_verdicts_times; and, additively again, K7's codon grid: pep_rescore_codons, pep_rescore_codons_check.
 * 18 gained pep_live_resources; and, additively, the K17 entry points: pep_gene_ingroups, pep_gene_ingroups_check, pep_gene_ingroups_times.
 * 19 took in the sections of K18, K19 and K20, which had headers and version numbers of their own (pep_synteny_version, pep_genestruct_version and
 * pep_parser_version are gone), and replaced the six pep_*_times read-outs of K15 - K20 by pep_call_times.
 * 20 took in the sections of K21 - K26, which had headers of their own, and replaced the trailing `ms` out-array parameter of their eight device entry
 * points by pep_call_times selectors (PEP_CALL_KIMURA_PAIRS .. PEP_CALL_BATCH_PRUNE); struct pep_call_times grew from four to PEP_CALL_MS times. */
#define PEP_ABI_VERSION 20

#define PEP_OK 0
#define PEP_ERR_HIP (-1)       /* a HIP runtime call failed */
#define PEP_ERR_ARG (-2)       /* invalid argument */
#define PEP_ERR_LIMIT (-3)     /* input exceeds a documented limit */
#define PEP_ERR_STATE (-4)     /* call order (e.g. search before sequences were set) */
#define PEP_ERR_INTERNAL (-5)

/* documented limits (candidate key packs q:21 | t:25 | diagonal bin:18) */
#define PEP_MAX_QUERIES ((1u << 21) - 2)
#define PEP_MAX_TARGETS ((1u << 25) - 1)
#define PEP_MAX_SEQ_LEN ((1u << 23) - 256)
#define PEP_MAX_RESIDUES ((1u << 29) - 1)   /* per side, padded */

typedef struct pep_ctx pep_ctx;
typedef struct pep_result pep_result;
typedef struct pep_verdict_result pep_verdict_result;

/* search parameters; pep_default_params fills the protein defaults that mirror the reference's
 * diamond command line (uberBlast.py:550): BLOSUM62, gap 11/1, --evalue 1, --dbsize 5000000, -k 10, 5 splits */
typedef struct {
    int32_t gap_open, gap_ext;    /* a gap of length k costs gap_open + k * gap_ext; 0 <= gap_open <= 255, 1 <= gap_ext <= 255 */
    int32_t n_shapes, base;       /* spaced seeds over a reduced alphabet of `base` letters */
    int32_t weight[4];
    int32_t offs[4][32];
    uint8_t reduce[32];           /* residue code -> reduced letter; 0xFF never seeds */
    int8_t sub[1024];             /* substitution score [q*32 + t]; row and column 31 (padding code) must be <= -64 */
    double min_id_pct;            /* --id           (100 * identities / alignment length) */
    double min_qcov_pct;          /* --query-cover  (100 * aligned query span / query length) */
    int32_t top_k;                /* -k : targets kept per query per split */
    int32_t n_splits;             /* targets are dealt round-robin into this many splits */
    double dbsize, max_evalue;    /* --dbsize, --evalue */
    int32_t use_lds;              /* 1: residues staged in LDS (default); 0: read from global memory */
    int32_t ungapped_min;         /* a seed hit nominates a candidate only if its ungapped x-drop score reaches this (0 = off) */
    int32_t xdrop;                /* x-drop of that ungapped extension (must stay below 64) */
    int32_t ext_right, ext_left;  /* residues scored right of (from) / left of the seed's first position (<= 48 / <= 48) */
    int32_t reserved[3];          /* profiling/test switches, 0 in production: [0] seed-join stage limiter (1 keys, 2 +buckets, 3 +entries)
                                     or a reference path with the same results, for comparison (8 the nucleotide tool's plain 17-mer matcher instead of look-up words
                                     at a stride, 10 the plain stream of a self-search instead of dropping diagonal-0 self hits: tools/ab/self_hits_ab.py), [1] != 0 forces the 32-bit Smith-Waterman passes instead
                                     of the packed 16-bit ones, [2] != 0 forces the count -> scan -> fill build of the query seed index */
    double ka_lambda, ka_k;       /* Karlin-Altschul parameters of the scoring system (protein default 0.267 / 0.041) */
    int32_t hsp_mode;             /* 0: one alignment per (q, t), its best band (diamond --max-hsps 1); 1: every band reaching the
                                     score threshold, duplicates (same end cell) removed - several copies on one subject; 2 (UNPINNED: restated from NCBI's published rules, no blastn binary to hold it to): BLAST's way with the
                                     HSPs of a subject (blastn behind uberBlast.py:294): the bands of (q, t) in the order score descending, band ascending,
                                     one dropped when an ACCEPTED one in front shares its start or its end cell or holds its query and subject ranges
                                     inside its own; top_k counts subjects (the reference sequence a target is a strand / frame of), every alignment of
                                     a kept subject stays.  Needs targets made by pep_translate / pep_use_nt_as_residues. */
    int32_t t_index_base;         /* index of this context's target 0 in the WHOLE reference set when the targets are one shard of it (multi-GPU
                                     target sharding, peppan_amd/dist.py): split membership is (t + t_index_base) mod n_splits, so a shard ranks
                                     its hits exactly as the unsharded search would; 0 otherwise.  Ignored with pep_set_target_groups. */
    int32_t stage1_min;           /* first stage of the ungapped pre-filter (only with ungapped_min > 0): the extension to the right of a seed hit must
                                     have reached this score after its first 16 residues - the seed and a few residues behind it - or the hit is
                                     dropped before the rest of its windows is fetched (chance hits of the reduced alphabet); 0 = off */
    int32_t reserved2;            /* test switches (bits), 0 in production: bit 0 makes the alignment stage synchronise with the host after its selection
                                     step and size the traceback buffers exactly (what it does by itself when its upper bounds would cost too much
                                     memory) instead of running from the candidate count to the result sizes without a host round trip; bit 1 makes the
                                     score pass sweep identical pairs like any other pair instead of settling them by comparison
                                     (pep_stats.candidates_settled), bit 2 makes it settle them also in searches below 16 384 candidates, where
                                     the comparison costs more than it saves */
} pep_search_params;

/* one alignment; coordinates are 1-based, inclusive, in residues of the query / target protein */
typedef struct {
    uint32_t q, t;                /* query index, target (chunk) index */
    uint32_t q_start, q_end;      /* ZS .. */
    uint32_t t_start, t_end;      /* POS .. */
    int32_t score;                /* ZR raw score */
    uint32_t nm;                  /* NM = aln_len - n_ident */
    uint32_t n_ident, aln_len;
    uint32_t cigar_runs;
    int32_t bin;                  /* diagonal bin of the band that produced it */
    uint64_t cigar_off;           /* into the result's CIGAR arena: runs of (len << 2 | op), op 0=M 1=I 2=D */
    uint64_t cells;               /* in-band, in-matrix DP cells of this alignment's band */
} pep_hit;

typedef struct { uint32_t seq, frame, aa_len, nt_len; } pep_query_meta;       /* frame 1..3 */
typedef struct { uint32_t seq, frame, chunk_off, aa_len; } pep_target_meta;   /* frame 1..6; name = seq:frame:chunk_off */

/* a nucleotide-level hit for rescoring (uberBlast.py:412): 1-based inclusive nt coordinates, rs > re = reverse strand */
typedef struct {
    uint32_t q, r;
    uint32_t qs, qe, rs, re;
    uint32_t cigar_runs, pad;
    uint64_t cigar_off;
} pep_nt_hit;

typedef struct {
    uint64_t query_residues, target_residues;
    uint64_t query_seeds, target_seeds, seed_hits, seed_hits_passed;   /* seed_hits_passed: runs of seed hits whose candidate passed the ungapped filter or was known already */
    uint64_t candidates;          /* unique (q, t, band) */
    uint64_t pairs;               /* unique (q, t) */
    uint64_t tracebacks;
    uint64_t hits;
    uint64_t cells;               /* in-band in-matrix DP cells over all candidates, score pass (SW cell updates) */
    uint64_t cells_swept;         /* 64 lanes x anti-diagonal steps executed by the score pass */
    uint64_t dir_bytes;           /* traceback direction workspace written by the SW kernel */
    uint64_t sw_launches;
    uint64_t cells_trace;         /* DP cells recomputed by the traceback pass (selected pairs only) */
    uint64_t cells_swept_trace;   /* 64 lanes x steps executed by the traceback pass */
    uint64_t tracebacks_gapless;  /* of `tracebacks`: pairs whose alignment is one ungapped run, settled without a traceback sweep (rule 5a) */
    uint64_t candidates_settled;  /* of `candidates`: identical pairs the score pass settles without a sweep (same residues, band over diagonal 0, every
                                     residue dominant in the score table: the optimum is the whole diagonal) */
    uint64_t cells_settled;       /* of `cells`: the cells of those candidates (cells - cells_settled = cells the score pass sweeps) */
    double ms_seed, ms_sw, ms_trace, ms_total;   /* HIP-event times on the context's stream; ms_sw = score pass kernel */
    double ms_k1, ms_sw_trace;                   /* ms_sw_trace = traceback-pass kernel (selected pairs only) */
    double ms_seed_match;                        /* seed_match kernel, summed over the seed shapes (one launch per shape) */
    double ms_reserved[3];
} pep_stats;

int pep_version(void);
int pep_device_count(void);
int pep_ctx_create(int device, pep_ctx **out);
void pep_ctx_destroy(pep_ctx *ctx);
/* what the library holds in this process right now, over all contexts: bytes of device buffers, bytes of pinned host buffers, HIP events.  Back at
 * their earlier values once every context made since is destroyed (a result that outlives its context holds host memory only). */
int pep_live_resources(uint64_t *device_bytes, uint64_t *pinned_bytes, uint32_t *events);
const char *pep_last_error(const pep_ctx *ctx);
void pep_default_params(pep_search_params *p);
/* sensitivity of the translated search: 0 = DIAMOND's two default-mode seed shapes (what the reference's command line runs, uberBlast.py:550),
 * 1 = four shapes (recall 0.93 -> 0.985 between 0.45 and 0.7 identity at twice the seed-stage cost).  Rewrites n_shapes / weight / offs. */
int pep_set_sensitivity(pep_search_params *p, int level);
/* smallest raw score passing the e-value cut for a query of qlen residues */
int32_t pep_min_score(uint32_t qlen, double dbsize, double max_evalue);
int32_t pep_min_score_ka(uint32_t qlen, double dbsize, double max_evalue, double ka_lambda, double ka_k);

/* nucleotide inputs (ASCII, any case), concatenated, off[n+1].  Stored on the device; K1 (translation,
 * frame choice / chunking, packing) runs on the GPU at the next pep_translate or pep_search. */
int pep_set_query_nt(pep_ctx *ctx, const uint8_t *nt, const uint64_t *off, uint32_t n, int gtable);
int pep_set_ref_nt(pep_ctx *ctx, const uint8_t *nt, const uint64_t *off, uint32_t n, int frames /* 6 or 3 */, int gtable);
/* protein inputs (residue code = letter - 'A'), used as they are (no K1) */
int pep_set_query_aa(pep_ctx *ctx, const uint8_t *codes, const uint64_t *off, uint32_t n);
int pep_set_ref_aa(pep_ctx *ctx, const uint8_t *codes, const uint64_t *off, uint32_t n);
/* run K1 for the sides given as nucleotides (idempotent until the inputs change; force != 0 re-runs it) */
int pep_translate(pep_ctx *ctx, int force);
/* the protein sets made from nucleotide inputs are stale: the next pep_search translates again (K1), inside the search - both sides queued
 * at once and the seed stage's first kernels behind them, so that the GPU does not wait for the host between K1 and the search as it does
 * with a pep_translate(force) call in front */
int pep_invalidate_translation(pep_ctx *ctx);
/* The nucleotide search (the reference's blastn call, uberBlast.py:294, 482-509) on device-resident inputs: the nucleotide sets given to
 * pep_set_query_nt / pep_set_ref_nt THEMSELVES become the residue sets of the following searches, as base codes A0 C1 G2 T3 (anything
 * else 4), packed on the GPU - queries forward; the reference, per reference set (pep_set_target_groups, else the whole list), all
 * forward strands followed (strands = 2) by all reverse complements.  Target meta: seq = reference sequence, frame 1 forward / 4 reverse.
 * Stays in force until the next pep_translate or pep_set_*: pep_search does not run K1 in between, and a translated search afterwards
 * needs pep_translate first.  PEP_ERR_LIMIT for a sequence beyond PEP_MAX_SEQ_LEN (the caller then windows it, peppan_amd/uberBlast.py). */
int pep_use_nt_as_residues(pep_ctx *ctx, int strands);
int pep_query_count(pep_ctx *ctx, uint32_t *n, uint64_t *residues);
int pep_target_count(pep_ctx *ctx, uint32_t *n, uint64_t *residues);
int pep_get_query_meta(pep_ctx *ctx, pep_query_meta *out, uint32_t cap);
int pep_get_target_meta(pep_ctx *ctx, pep_target_meta *out, uint32_t cap);
/* download the packed proteins (plain concatenation, off[n+1]) - for tests and debugging */
int pep_get_query_aa(pep_ctx *ctx, uint8_t *codes, uint64_t cap, uint64_t *off);
int pep_get_target_aa(pep_ctx *ctx, uint8_t *codes, uint64_t cap, uint64_t *off);

/* Optional: batch several reference sets (e.g. genomes) into one search.  group[i] = set of reference sequence i (sequences
 * of one set must be contiguous).  The top-k / split competition then runs inside each set, with targets numbered from 0
 * inside it, so the hits of a set are exactly those of searching it alone.  n = 0 clears the grouping.  Call after the
 * reference sequences are set; a new pep_set_ref_* clears it. */
int pep_set_target_groups(pep_ctx *ctx, const uint32_t *group, uint32_t n);

/* on_device != 0: the searches of this context leave their hit table on the device (pep_result_device) and skip the copy to the host at
 * the end of pep_search; pep_result_copy / pep_result_data then fetch it on demand, while the result is still the context's newest
 * (PEP_ERR_STATE afterwards).  For callers that go on working on the GPU: the all-gather of a multi-GPU search, K10. */
int pep_set_result_mode(pep_ctx *ctx, int on_device);
/* Phase timers of the searches of this context (the ms_* fields of pep_stats): HIP events recorded on the search's stream, each of which
 * leaves the GPU idle for about 6 us between the two kernels it separates.  level 0 (the default): none, the fields stay 0;
 * 1: the Smith-Waterman score pass only (ms_sw); 2: every phase (sixteen events per search).  ms_k1 (pep_translate) follows the same switch. */
int pep_set_timing(pep_ctx *ctx, int level);
/* The times of the context's newest call of one of K15 - K26: ms[] are kernel times on the context's stream, measured when pep_set_timing is 2 (else 0) unless
 * the kernel's section says otherwise, and the byte counts are what the call moved each way.  What each slot holds is stated in the kernel's section below; a slot
 * or a byte count a kernel does not use reads 0.  The byte counts of K21 - K26 (selectors 6 - 13) are not counted: they read 0.  A call resets its own record when
 * it starts (K20's two calls share one: see there) and touches no other, so a call that its checks refuse leaves zeros.  PEP_ERR_ARG: a null ctx or out, a `which`
 * outside [0, PEP_CALL_COUNT).  (The struct goes by its tag: the function has its name.) */
#define PEP_CALL_ALLELE_DIFF 0        /* pep_allele_diff */
#define PEP_CALL_GROUP_VERDICTS 1     /* pep_group_verdicts (+ pep_verdict_detail_copy) */
#define PEP_CALL_GENE_INGROUPS 2      /* pep_gene_ingroups */
#define PEP_CALL_SYNTENY_PAIRS 3      /* pep_synteny_pairs (+ pep_synteny_pairs_copy) */
#define PEP_CALL_GENE_STRUCTURE 4     /* pep_gene_structure */
#define PEP_CALL_PARSER 5             /* pep_rarefaction_curves and pep_profile_pairs */
#define PEP_CALL_KIMURA_PAIRS 6       /* pep_kimura_pairs */
#define PEP_CALL_NJ_TREES 7           /* pep_nj_trees */
#define PEP_CALL_GLOBAL_DIFF 8        /* pep_global_diff */
#define PEP_CALL_CDS_GENES 9          /* pep_cds_genes */
#define PEP_CALL_OUT_ALLELES 10       /* pep_out_alleles */
#define PEP_CALL_TREE_CUT 11          /* pep_tree_cut */
#define PEP_CALL_BATCH_SCREEN 12      /* pep_batch_screen */
#define PEP_CALL_BATCH_PRUNE 13       /* pep_batch_prune */
#define PEP_CALL_COUNT 14
#define PEP_CALL_MS 8                 /* (pep_out_alleles has six stages) */
struct pep_call_times { double ms[PEP_CALL_MS]; uint64_t bytes_to_device, bytes_to_host; };
int pep_call_times(const pep_ctx *ctx, int which, struct pep_call_times *out);
/* K2..K8: seeds, candidates, banded Smith-Waterman, traceback, filters, top-k.  Hits ordered by (q, t). */
int pep_search(pep_ctx *ctx, const pep_search_params *params, pep_result **out);
int pep_result_size(const pep_result *r, uint64_t *n_hits, uint64_t *n_cigar);
int pep_result_copy(const pep_result *r, pep_hit *hits, uint32_t *cigar);
/* zero-copy access: pointers to the n_hits records / n_cigar runs of pep_result_size, valid until the next call on the result's
 * context that produces a hit table or re-translates (pep_search, pep_translate, pep_linclust), pep_ctx_destroy or pep_result_free,
 * whichever comes first: they point into the context's pinned staging area, which such calls may re-use or re-allocate
 * (use pep_result_copy for anything that must outlive that) */
int pep_result_data(const pep_result *r, const pep_hit **hits, const uint32_t **cigar);
/* device copy of the table (same records, same order), for callers that go on working on the GPU - an all-gather from device memory, K10:
 * pointers into the context's workspace, valid (PEP_OK) only while r is its context's NEWEST result and nothing has reused that workspace
 * (the next pep_search / pep_linclust does); PEP_ERR_STATE and null pointers otherwise */
int pep_result_device(const pep_result *r, const pep_hit **d_hits, const uint32_t **d_cigar);
int pep_result_stats(const pep_result *r, pep_stats *stats);
void pep_result_free(pep_result *r);

/* Host-side (no GPU work, no context): merge of the hit tables of several TARGET shards of one search (multi-GPU, after the
 * all-gather).  hits carry global q and t indices; every (q, t) lives in exactly one shard, each shard already applied top-k per
 * (q, split) locally, and the global top-k of a (q, split) is contained in the union of the local ones.  Ranks inside
 * (q, t mod n_splits) by (score desc, t asc, bin asc) - the order of K8 - keeps rank < top_k and writes the survivors ordered by
 * (q, t, bin) with a compacted CIGAR arena.  out_hits / out_cigar must hold n / n_cigar entries. */
int pep_merge_hits(uint64_t n, const pep_hit *hits, const uint32_t *cigar, uint64_t n_cigar, int32_t top_k, int32_t n_splits,
                   pep_hit *out_hits, uint32_t *out_cigar, uint64_t *n_out, uint64_t *n_cigar_out);

/* K7: integer counts of mode-1 rescoring per hit, out[5*i..] = nMatch, nMismatch, nGap, bGap, mGap.
 * Uses the nucleotide sets given to pep_set_query_nt / pep_set_ref_nt.  rs < re is a forward-strand hit; every other hit, a one-base
 * range (rs == re) included, is read on the reverse strand, complemented, as the reference does (`t[8] < t[9]` is false, uberBlast.py:412).
 * A run with op code 3 is PEP_ERR_ARG ("unknown CIGAR op"), as in pep_alleles. */
int pep_rescore_nt(pep_ctx *ctx, uint64_t n, const pep_nt_hit *hits, const uint32_t *cigar, uint64_t n_cigar, int64_t *out);

/* K7 over the codon grid: the integer counts of rescoring modes 2 and 3 per hit (cigar2score, uberBlast.py:250-269); hits, CIGAR arena, nucleotide sets,
 * base codes and strand rule as for pep_rescore_nt.  The columns of a hit are the columns of its M and I runs in CIGAR order (an I column has a query base
 * and no reference base; D runs only move the reference cursor).  With phase = (qs - 1) % 3 and whole = max(n_col - phase, 0) / 3, column p is kept when
 * p >= phase and p - phase < 3 * whole, as position (p - phase) % 3 of codon (p - phase) / 3: a trailing partial codon is dropped.  out[7*i..]:
 *   mode 3   hit0, hit1, hit2 (kept columns with equal codes at codon position 0 / 1 / 2; an I column never matches), paired (kept columns that have a
 *            reference base), nGap, bGap, mGap (as pep_rescore_nt reports them);
 *   mode 2   aa_match, codons, sub_sum, 0, nGap, bGap, mGap: over the kept codons without an I column, with word = 25 c0 + 5 c1 + c2 of the three codes and
 *            qa = aa_of_word[query word], ra = aa_of_word[reference word]: their number, those with qa == ra, and the (signed) sum of sub[(qa << 5) + ra].
 * The float identity and score are the caller's (peppan_amd.uberBlast.codon_scores_from_counts keeps the reference's order of operations), and so are the
 * two tables: aa_of_word[125] (every entry below 32) and sub[1024], read in mode 2 only (mode 3 takes NULL).
 * PEP_ERR_ARG: a mode other than 2 or 3, a NULL table or an aa_of_word entry of 32 or more in mode 2, and what pep_rescore_nt refuses, in its words behind
 * this function's name.  PEP_ERR_STATE before both nucleotide sets are given.  On an error nothing is written to out and the context stays usable; n == 0
 * is PEP_OK.  pep_rescore_codons_check runs the host checks alone - no context, no device - over the offsets (q_off[n_q + 1], r_off[n_r + 1]) of the two
 * nucleotide sets; the message goes to msg (msg_cap bytes, 0-terminated). */
int pep_rescore_codons(pep_ctx *ctx, uint64_t n, const pep_nt_hit *hits, const uint32_t *cigar, uint64_t n_cigar, int32_t mode,
                       const uint8_t *aa_of_word /*[125], mode 2*/, const int8_t *sub /*[1024], mode 2*/, int64_t *out /*[7 n]*/);
int pep_rescore_codons_check(uint64_t n, const pep_nt_hit *hits, const uint32_t *cigar, uint64_t n_cigar, int32_t mode,
                             const uint8_t *aa_of_word, const int8_t *sub, const uint64_t *q_off, uint64_t n_q,
                             const uint64_t *r_off, uint64_t n_r, char *msg, uint64_t msg_cap);

/* K7 as the tail of every search of this context (-s 1 in PEPPAN's hot call, PEPPAN.py:229-230: every hit of both tools is rescored, uberBlast.py:352-353):
 * with on = 1 pep_search ends with the count of identical nucleotide columns of every hit it emits - K7's n_match, the one of its five counts that needs the
 * sequences - computed from the table on the device (the row a hit becomes follows from the hit and the descriptors of its packed sequences; nothing is
 * uploaded again, same stream, same wait).  pep_result_nt_match hands out the counts, one per hit in hit order (NULL when the search had none or the switch
 * was off); pep_table_from_hits turns them into the rescored identity and score.  Needs packed sets made from the context's nucleotide sets (K1 or
 * pep_use_nt_as_residues): a search over sets given as residues fails with PEP_ERR_STATE while the switch is on. */
int pep_set_nt_match(pep_ctx *ctx, int on);
int pep_result_nt_match(const pep_result *r, const uint32_t **nt_match);

/* K10: connected components; label[x] = smallest node id of x's component */
int pep_components(pep_ctx *ctx, uint32_t n_nodes, uint64_t n_edges, const uint32_t *a, const uint32_t *b, uint32_t *label);
/* the same over the edges of a hit table: (hit.q + q_base, node_of_target[hit.t]) - the single-linkage step of get_gene_group on
 * the table of the all-vs-all search (PEPPAN.py:1598-1607), without building the two edge columns on the caller's side */
int pep_components_of_hits(pep_ctx *ctx, uint32_t n_nodes, uint64_t n_hits, const pep_hit *hits, uint32_t q_base,
                           const uint32_t *node_of_target, uint64_t n_targets, uint32_t *label);

/* the same for a search result: while r is the context's newest result its device copy is read in place (no edge columns are built or
 * uploaded; node_of_target is uploaded only when it changed since the last call), otherwise as pep_components_of_hits */
/* single linkage as the tail of every search of this context (the north-star path: all-vs-all search + grouping, PEPPAN.py:229-230 +
 * 1598-1607): with n_nodes > 0 pep_search ends with K10 over the edges (hit.q + q_base, node_of_target[hit.t]) of the table it has just
 * produced - same stream, no second call, no second wait - and pep_result_labels hands out label[g] = smallest node of g's component.
 * node_of_target needs an entry for every target of the searches that follow (else they fail with PEP_ERR_STATE); n_nodes = 0 switches it off. */
int pep_set_grouping(pep_ctx *ctx, uint32_t n_nodes, uint32_t q_base, const uint32_t *node_of_target, uint64_t n_targets);
int pep_result_labels(const pep_result *r, uint32_t *label, uint32_t n_nodes);
int pep_components_of_result(pep_ctx *ctx, const pep_result *r, uint32_t n_nodes, uint32_t q_base, const uint32_t *node_of_target, uint64_t n_targets,
                             uint32_t *label);

/* K9: linear-time clustering.  codes: residue codes (< base are valid k-mer letters), concatenated, off[n+1].
 * rep[i] = index of sequence i's representative (rep[i] == i for representatives).  stats (may be NULL):
 * [0] selected k-mers, [1] verified (sequence, centre, diagonal) pairs, [2] accepted edges.
 * Pairs that fail on their k-mer diagonal without gaps are aligned by the search's banded Smith-Waterman engine (base 4:
 * +2 / -3, gap 6 + 2k; otherwise residues in the order ACDEFGHIKLMNPQRSTVWY + one code for anything else, BLOSUM62, gap 11 + k).
 * That stage uses the context's packed sequence sets: after pep_linclust a pep_search re-runs K1 for nucleotide inputs and
 * needs pep_set_query_aa / pep_set_ref_aa inputs to be given again (PEP_ERR_STATE otherwise). */
int pep_linclust(pep_ctx *ctx, const uint8_t *codes, const uint64_t *off, uint32_t n, int base, int k, int m,
                 double min_id, double min_cov, uint32_t *rep, uint64_t *stats);

/* K11: overlapping reference intervals (flag -O; tab2overlaps, uberBlast.py:73-97).  Rows sorted by (contig, start, end).
 * out receives (id1, id2, overlap) triples in (i, j) order; *n_pairs is the full count - when it exceeds cap nothing is
 * written and the caller calls again with a buffer of *n_pairs triples. */
int pep_overlaps(pep_ctx *ctx, uint64_t n, const int32_t *contig, const int64_t *start, const int64_t *end, const int64_t *row_id,
                 double ovl_l, double ovl_p, int64_t *out, uint64_t cap, uint64_t *n_pairs);

/* K12: aligned alleles of the genes->genomes mapping (iter_map_bsn, PEPPAN.py:812-835, 846-848).
 * A row is one aligned locus of a gene on a contig; rows of one gene group are contiguous, group g owning rows
 * [grp_off[g], grp_off[g+1]) in the order the reference writes them (later rows overwrite earlier ones where they share
 * query positions).  nt / nt_off[n_contigs+1]: the contigs, ASCII, upper case.  CIGAR runs are len<<2|op (0=M 1=I 2=D), nt.
 * Outputs: in_frame[row] = most M columns falling into one codon frame; orf[row] = longest stretch of the allele string
 * between stop codons (gtable 4: TAA TAG, else TAG TAA TGA); packed = for every group ceil(q_len/3) bytes
 * codes[j]*25 + codes[s+j]*5 + codes[2s+j] over the gene's coordinate system (A1 C2 G3 T4, anything else 0), groups
 * concatenated in order.  packed_cap = bytes available in `packed`. */
typedef struct {
    uint32_t contig;          /* index into nt_off */
    uint32_t q_start;         /* 1-based first query position of the alignment (column 6) */
    uint32_t rs, re;          /* 1-based reference start / end (columns 8, 9); rs >= re = reverse strand */
    uint32_t cigar_runs, group;
    uint64_t cigar_off;
} pep_locus;
int pep_alleles(pep_ctx *ctx, const uint8_t *nt, const uint64_t *nt_off, uint32_t n_contigs, uint64_t n_rows, const pep_locus *rows,
                const uint32_t *cigar, uint64_t n_cigar, uint32_t n_groups, const uint64_t *grp_off, const uint32_t *grp_qlen, int gtable,
                int64_t *in_frame, int64_t *orf, uint8_t *packed, uint64_t packed_cap);

/* K15: pairwise allele differences of gene groups (compare_seq / compare_seqX, PEPPAN.py:296-316, over rows as filt_per_group
 * reads and masks them, :332-333).  Row r is bytes [row_off[r], row_off[r+1]) of `packed` in the .seq store's form - ceil(row_len[r] / 3)
 * bytes c[j] * 25 + c[s + j] * 5 + c[2 s + j], codes 0 = not comparable, 1..4 = ACGT - and counts with its first row_len[r] columns only
 * (digits past them are ignored).  Group g is the list of row indices grp_rows[grp_off[g] .. grp_off[g+1]) into that one table (a row may
 * serve several groups, so the sub-groups of :354-360 need no second upload); all its rows have the same row_len.  With
 * comparable(a, b) = columns where both rows are non-zero and mismatch(a, b) = those of them where the rows differ, a group of n rows
 * writes to out[out_off[g] ...], as int32 pairs (mismatch + 1, comparable + 2) and in this order:
 *   grp_mode[g] bit 0: the n (n - 1) / 2 pairs a < b in row-major order (the packed upper triangle compare_seq fills);
 *   grp_mode[g] bit 1: [2, n, 2] - the first and the last row of the group against every row, itself included (compare_seqX).
 * out_off[g] and out_cap count int32 values.  Empty batches, empty groups and groups of one row are legal.  PEP_ERR_ARG: a row that does
 * not hold ceil(row_len / 3) bytes, a group that mixes row_len, a row index >= n_rows, a byte above 124, outputs that overlap or run
 * past out_cap.  PEP_ERR_LIMIT: the call's output or its bit planes (24 B per 64 columns of a row) exceed PEP_ALLELE_DIFF_MAX_BYTES each;
 * the message says how much was asked for, and the caller splits the batch.  After an error `out` holds nothing usable.
 * (The output limit is reported at the first group that crosses it, with the bytes counted up to that group.)
 * pep_call_times(PEP_CALL_ALLELE_DIFF): of the context's newest pep_allele_diff: ms[0], ms[1] the kernel times - bit planes, pairs - when
 * pep_set_timing is 2 (else zeros; at that level the host waits between the two kernels), and ms[2] the host's wall time from the end of the
 * kernels until the output lies in `out` (always).  No byte counts. */
#define PEP_ALLELE_DIFF_MAX_BYTES (1ull << 31)
int pep_allele_diff(pep_ctx *ctx, const uint8_t *packed, const uint64_t *row_off, const uint32_t *row_len, uint64_t n_rows,
                    uint32_t n_groups, const uint64_t *grp_off, const uint32_t *grp_rows, const uint8_t *grp_mode,
                    int32_t *out, const uint64_t *out_off, uint64_t out_cap);

/* K16: divergence verdicts of gene groups - what filt_per_group decides from the pairs of K15 before it looks at any of them on the host
 * (checkDiv over the first and last row, PEPPAN.py:335-344, 346-351; over the first and last row of every genome's sub-group for in-paralog
 * groups, :352-366; the distances test :371-382; the leader grouping :383-392).  Rows and groups as for pep_allele_diff; grp_genome holds the
 * genome id (column 1 of the group's table) of every entry of grp_rows, grp_inparalog one 0 / 1 per group.  With (mut, aln) = K15's pair
 * (mismatch + 1, comparable + 2) as doubles and, per pair of rows, (gd0, denX, den) = the row of the table below for the two genomes
 * (gd_default when the pair is not in it), or gd0 = denX = den = fmax(self_id, 2 / aln) when both rows are of one genome:
 *   divergent   mut / aln / denX > 1 for a pair (a, b), a != b, a the first or last row of the group / of a sub-group, b any row of it;
 *   beyond      (mut / aln / den) / gd0 > 1 / gd0 for a pair a < b of a divergent group;
 *   leaders     rows in order: row j joins the FIRST leader l with mut(l, j) <= 0.01 * aln(l, j), else it becomes a leader.
 * verdict[g]: 0 = not divergent (the reference returns at :368; also every group of fewer than two rows), 1 = divergent, no pair beyond
 * (returns at :484), 2 = a pair beyond its bound (goes on at :383).  Every operation is a single correctly rounded double operation, so
 * the verdicts equal numpy's bit for bit.  The table is made by the caller (peppan_amd.orthofilter.gd_table): gd_key[i] = g1 << 32 | g2
 * with g1 <= g2, strictly increasing; gd_val[i] = (gd0, gd0 * exp(gd1 * sqrt(allowed_sigma)), gd0 * exp(gd1 * allowed_sigma)).
 * All tables are checked on the host before anything is launched.  PEP_ERR_ARG: what pep_allele_diff names, a key with g1 > g2 or out of
 * order, a value that is not finite or not > 0, self_id not finite or not > 0, grp_inparalog above 1.  PEP_ERR_LIMIT: the packed
 * triangles of all groups of two rows and more (reserved for every group, its verdict is not known in advance) or the bit planes exceed
 * PEP_ALLELE_DIFF_MAX_BYTES; the message names the first group that crosses it, and the caller splits the batch.
 * pep_group_verdicts_check runs those checks alone: no context, no device; the message goes to msg (msg_cap bytes, 0-terminated).
 * The verdicts cost the host n_groups bytes plus one word.  *detail keeps the triangles and leaders of the verdict-2 groups ON THE DEVICE,
 * until the next pep_group_verdicts of the context (pep_verdict_detail_copy then fails with PEP_ERR_STATE); free it with
 * pep_verdict_result_free before the context is destroyed.  pep_verdict_detail_size: pairs of group g's triangle, 0 unless its verdict is 2.
 * pep_verdict_detail_copy: tri (int32 pairs, packed upper triangle as pep_allele_diff's bit 0) and leader (uint32[n]: the row that leads
 * row j, leader[j] == j for a leader); either may be NULL; nothing is written for verdict 0 / 1.
 * pep_call_times(PEP_CALL_GROUP_VERDICTS): of the newest call, ms[0..3] the kernel times - bit planes, edge, pairs, leaders - when pep_set_timing is 2
 * (else zeros), and bytes_to_host what that call and the detail copies of its result have sent to the host. */
int pep_group_verdicts(pep_ctx *ctx, const uint8_t *packed, const uint64_t *row_off, const uint32_t *row_len, uint64_t n_rows, uint32_t n_groups,
                       const uint64_t *grp_off, const uint32_t *grp_rows, const uint32_t *grp_genome, const uint8_t *grp_inparalog, const uint64_t *gd_key,
                       const double *gd_val, uint64_t n_gd, const double *gd_default, double self_id, uint8_t *verdict, pep_verdict_result **detail);
int pep_group_verdicts_check(const uint8_t *packed, const uint64_t *row_off, const uint32_t *row_len, uint64_t n_rows, uint32_t n_groups, const uint64_t *grp_off,
                             const uint32_t *grp_rows, const uint32_t *grp_genome, const uint8_t *grp_inparalog, const uint64_t *gd_key, const double *gd_val,
                             uint64_t n_gd, const double *gd_default, double self_id, char *msg, uint64_t msg_cap);
int pep_verdict_detail_size(const pep_verdict_result *res, uint32_t g, uint64_t *n_pairs);
int pep_verdict_detail_copy(pep_verdict_result *res, uint32_t g, int32_t *tri, uint32_t *leader);
void pep_verdict_result_free(pep_verdict_result *res);

/* K17: in-group rows and gene scores of `initializing` - determineGroup (PEPPAN.py:1041-1056) as initializing2 calls it for every gene of the
 * .tab store, and the gene's score (:1058-1076).  Gene g is rows [gene_off[g], gene_off[g+1]) of the three row tables, in the order of :1069:
 * genome (column 1), iden (column 4 after the rescale of :1070, >= 0), score (column 2).  With thr = (min_iden - 0.02) * 10000 evaluated by the
 * caller as the reference writes it, seed[j] = iden[j] >= thr and, for two rows i < j of one gene,
 *   sc(i, j) = (1. - iden[j] / iden[i]) / den,  den = self_id for two rows of one genome, else column 2 of the table below for the two genomes
 *                                                (gd_default[2] when the pair is not in it),
 *   raw[j]   = seed[j] or there is an i < j with seed[i] and sc(i, j) < 1,
 *   keep[j]  = raw[first row of the gene with genome[j]'s genome]       (:1054-1055),
 *   gene_score[g] = sum of abs(score[j]) over the kept rows that are the first of their genome       (:1074).
 * The reference's ordered walk with its early exit computes the same: only seeds ever act as sources and the flags only grow.  Every operation
 * of sc is a single correctly rounded double operation, so keep equals numpy's bit for bit.  The table is pep_group_verdicts' own
 * (peppan_amd.orthofilter.gd_table with allowed_sigma = nSigma).  All tables are checked on the host before anything is launched.
 * PEP_ERR_ARG: gene_off not ascending from 0 to n_rows, a negative iden, a key with g1 > g2 or out of order, a value that is not finite or
 * not > 0, self_id or thr not finite.  PEP_ERR_LIMIT: n_rows >= 2^32.  Empty batches and empty genes are legal; an empty gene scores 0.  On an
 * error nothing is written and the context stays usable.  The work is quadratic in the rows of a gene in the worst case, as the reference's.
 * pep_gene_ingroups_check runs the checks alone: no context, no device; the message goes to msg (msg_cap bytes, 0-terminated).
 * pep_call_times(PEP_CALL_GENE_INGROUPS): of the newest call, ms[0], ms[1] the kernel times - pairs, finish - when pep_set_timing is 2 (else zeros),
 * and bytes_to_host what the call sent to the host: n_rows + 8 * n_genes. */
int pep_gene_ingroups(pep_ctx *ctx, const uint32_t *genome, const int32_t *iden, const int64_t *score, uint64_t n_rows, uint32_t n_genes, const uint64_t *gene_off,
                      const uint64_t *gd_key, const double *gd_val, uint64_t n_gd, const double *gd_default, double self_id, double thr, uint8_t *keep, int64_t *gene_score);
int pep_gene_ingroups_check(const uint32_t *genome, const int32_t *iden, const int64_t *score, uint64_t n_rows, uint32_t n_genes, const uint64_t *gene_off,
                            const uint64_t *gd_key, const double *gd_val, uint64_t n_gd, const double *gd_default, double self_id, double thr, char *msg, uint64_t msg_cap);

/* ---- K18: neighbourhood paralog splitting (synteny_resolver).
 * most pairs (sum over the groups of n * (n - 1) / 2) of one pep_synteny_pairs call: a single group may hold 16 384 members */
#define PEP_SYNTENY_MAX_PAIRS (1ull << 27)
/* most rank counters of one call: sum over the groups of n * (6 * longest list of the group + 14) */
#define PEP_SYNTENY_MAX_COUNTERS (1ull << 26)
/* longest neighbour list of one member */
#define PEP_SYNTENY_MAX_LIST (1u << 20)

/* K18: the pair loop of ite_synteny_resolver (PEPPAN.py:1097-1151) for a batch of paralogous names.  Group g is members
 * [member_off[g], member_off[g+1]) of genome[] (compared for equality only) and of the neighbour lists in CSR form: member i owns
 * nb[nb_off[i] .. nb_off[i+1]), strictly ascending ortholog codes.  Members are numbered 0 .. n-1 inside their group.  For m < k with
 * c = |N_m & N_k| (:1108-1110):
 *   s = 3 c + max(6 - min(6, |N_m|), 6 - min(6, |N_k|), 0) + 1,   d = 3 n_neighbor - s,   flag = (genome[m] != genome[k]).
 * A pair is a conflict iff flag is false and d > 0 (:1112).  dc[g] is the smallest d of a conflict pair (0 and has_conflict[g] = 0 when there
 * is none).  The call leaves two lists of (m, k) pairs, two uint32 each, in the context:
 *   conf   the conflict pairs, ascending by (m, k);
 *   walk   every pair with d < dc, in the order (d, flag, m, k) - the part of the sorted list (:1117) the walk of :1119-1141 reads before it
 *          stops at the first conflict pair.  Empty for a group without a conflict.
 * Group g owns conf pairs [conf_off[g], conf_off[g+1]) and walk pairs [walk_off[g], walk_off[g+1]) (G + 1 offsets each, counted in pairs).
 * The lists are counted first and the context's buffers sized from the count: nothing is truncated.  pep_synteny_pairs_copy downloads the
 * lists of the newest call: n_conf / n_walk must be conf_off[G] / walk_off[G].
 * PEP_ERR_ARG: n_neighbor outside [1, 2^20], offsets that do not ascend from 0 to their end, a list that is not strictly ascending.
 * PEP_ERR_LIMIT: more pairs than PEP_SYNTENY_MAX_PAIRS (the message names the group at which the sum passes it), more counters than
 * PEP_SYNTENY_MAX_COUNTERS, a list longer than PEP_SYNTENY_MAX_LIST.  All tables are checked on the host before anything is launched.  The
 * kernels keep a fault word for what those checks exclude - a distance beyond the group's bound, a pair beyond the counted lists: it is read
 * after each pass, and the call then fails with PEP_ERR_HIP instead of returning a list.  The four outputs are written only when the call
 * succeeds; on any error nothing is written and the context stays usable.  Integer arithmetic only.
 * pep_synteny_pairs_check runs the checks alone: no context, no device; the message goes to msg (msg_cap bytes, 0-terminated).
 * pep_call_times(PEP_CALL_SYNTENY_PAIRS): of the newest call, ms[0..2] the kernel times - count, scans, emit - when pep_set_timing is 2 (else zeros), and
 * bytes_to_host what the call and its pep_synteny_pairs_copy sent to the host. */
int pep_synteny_pairs(pep_ctx *ctx, uint32_t n_groups, const uint64_t *member_off, const uint32_t *genome, uint64_t n_members, const uint64_t *nb_off, const uint32_t *nb,
                      uint64_t n_nb, int32_t n_neighbor, uint8_t *has_conflict, int32_t *dc, uint64_t *conf_off, uint64_t *walk_off);
int pep_synteny_pairs_copy(pep_ctx *ctx, uint32_t *conf, uint64_t n_conf, uint32_t *walk, uint64_t n_walk);
int pep_synteny_pairs_check(uint32_t n_groups, const uint64_t *member_off, const uint32_t *genome, uint64_t n_members, const uint64_t *nb_off, const uint32_t *nb,
                            uint64_t n_nb, int32_t n_neighbor, char *msg, uint64_t msg_cap);

/* The walk of ite_synteny_resolver over the two lists of pep_synteny_pairs (PEPPAN.py:1118-1151), on the host, without a context.  Every
 * member starts as a component of its own, with list A = [member] when it is an end of a conflict pair and B = [member] otherwise.  For each
 * walk pair (m, k) whose ends lie in different components ti, tj: the merge is skipped iff a conflict pair joins A[ti] and A[tj]; otherwise
 * A[ti] += A[tj], B[ti] += B[tj] (:1124-1141).  verdict[g]: 0 no conflict pair (the reference returns [None, None]), 1 a surviving component
 * has an empty A ([tag, None], :1147-1150), 2 a partition.  For verdict 2, n_comp[g] components in the order of their roots (the dictionary
 * order of :1148): component c of group g has the root comp_root[member_off[g] + c] - the member whose id is its key in the reference's
 * dictionary, not always its smallest - and comp_len[member_off[g] + c] members, and members[member_off[g] ..] holds the lists A + B of the
 * components one after the other (n entries in all).  For the other verdicts n_comp[g] = 0.  The skip test reads per-member conflict
 * adjacency, and components are joined by union-find over linked lists: the walk stays about linear in the pairs.
 * PEP_ERR_ARG: offsets that do not ascend from 0, a pair that is not m < k < n. */
int pep_synteny_walk(uint32_t n_groups, const uint64_t *member_off, const uint64_t *conf_off, const uint32_t *conf, const uint64_t *walk_off, const uint32_t *walk,
                     uint8_t *verdict, uint32_t *n_comp, uint32_t *comp_root, uint32_t *comp_len, uint32_t *members, char *msg, uint64_t msg_cap);

/* ---- K19: the gene structure of predictions (determineGeneStructure).
 * a window holds fewer nucleotides than this */
#define PEP_GENESTRUCT_MAX_WINDOW (1ull << 31)
/* stop_aa of a frame without a stop codon */
#define PEP_GENESTRUCT_NO_STOP 0xFFFFFFFFu
/* kind[]: the outcome of a frame */
#define PEP_GENESTRUCT_CDS 0
#define PEP_GENESTRUCT_NOSTART 1
#define PEP_GENESTRUCT_NOSTOP 2
#define PEP_GENESTRUCT_PREMATURE 3

/* K19: determineGeneStructure (PEPPAN.py:1193-1229) for a batch of predictions.  The nucleotide set is ASCII bytes, sequence i at
 * nt[seq_off[i] .. seq_off[i+1]) (n_seq + 1 offsets).  Prediction p reads the window of win_len[p] nucleotides that starts at the 0-based
 * win_off[p] of sequence seq[p] - forward, or, when bit 0 of flags[p] is set, backward and complemented as the reference's rc() does it
 * (upper-cased, A<->T, C<->G, everything else N: a '-' read backward is an N).  Bits 1-3 of flags[p] are the tried frames 0, 1, 2.
 * Frame f of a window of L nucleotides has n = max(0, (L - f) / 3) codons, codon k = window[f + 3k .. f + 3k + 3) (a partial last codon is
 * dropped, :1197).  A codon with a '-' is neither start nor stop; otherwise a codon with a character outside ACGT (either case) is a stop 'X';
 * otherwise TAA and TAG are stops, TGA too unless table4, and ATG, GTG, TTG are starts 'M' (modules/configure.py:167-172).
 * With a = lp / 3, b = (lp + allowed_vary) / 3, and "first / last in [u, v)" clipped to n as str.find / str.rfind clip:
 *     start = first M in [a, b), else last M in [0, a), else a with the outcome NOSTART
 *     stop  = first X in [start, n)
 *     while 0 <= stop < b and there is a first M in [stop, b): start = that M, stop = first X in [start, n)
 *     no stop: NOSTOP, else (stop - start + 1) * 3 < ref_len - allowed_vary: PREMATURE (both override NOSTART); else NOSTART or CDS.
 * The tried frames are judged in ascending order:
 *     frame[p]      the lowest tried frame whose outcome is CDS, or -1
 *     start_aa[p], stop_aa[p]   start and stop (codon numbers) of that frame; of the FIRST tried frame when frame[p] is -1, with
 *                   PEP_GENESTRUCT_NO_STOP for a frame without a stop
 *     kind[p]       the outcome of the first tried frame (PEP_GENESTRUCT_*)
 * Integer arithmetic only.  The four outputs are written only when the call succeeds; on any error nothing is written and the context
 * stays usable.  All tables are checked on the host before anything is launched:
 * PEP_ERR_ARG: seq_off does not ascend from 0, seq[p] >= n_seq, a window that leaves its sequence, no tried frame or flag bits above bit 3,
 * ref_len[p] == 0.  PEP_ERR_LIMIT: a window of PEP_GENESTRUCT_MAX_WINDOW nucleotides or more; the message names the prediction.
 * pep_gene_structure_check runs exactly these checks: no context, no device, the nucleotides themselves are not read; the message goes to
 * msg (msg_cap bytes, 0-terminated).
 * pep_call_times(PEP_CALL_GENE_STRUCTURE): of the newest call, ms[0] the kernel time when pep_set_timing is 2 (else 0), and the bytes it sent to the
 * device and to the host. */
int pep_gene_structure(pep_ctx *ctx, const uint8_t *nt, const uint64_t *seq_off, uint32_t n_seq, uint32_t n_pred, const uint32_t *seq, const uint64_t *win_off,
                       const uint32_t *win_len, const uint8_t *flags, const uint32_t *lp, const uint32_t *allowed_vary, const uint32_t *ref_len, int table4,
                       int32_t *frame, uint32_t *start_aa, uint32_t *stop_aa, uint8_t *kind);
int pep_gene_structure_check(const uint64_t *seq_off, uint32_t n_seq, uint32_t n_pred, const uint32_t *seq, const uint64_t *win_off, const uint32_t *win_len,
                             const uint8_t *flags, const uint32_t *lp, const uint32_t *allowed_vary, const uint32_t *ref_len, char *msg, uint64_t msg_cap);

/* ---- K20: the two counting loops of PEPPAN_parser.
 * a presence matrix holds fewer genes than this (the counts travel as int32) */
#define PEP_PARSER_MAX_GENES (1ull << 31)
/* n_genomes * n_iter of one pep_rarefaction_curves call stays below this (2 GiB of int32 pairs) */
#define PEP_PARSER_MAX_CURVE_POINTS (1ull << 28)
/* profiles of one pep_profile_pairs call (two n x n int32 matrices of 1 GiB each at the limit) */
#define PEP_PARSER_MAX_PROFILES 16384

/* K20a: the loop of writeCurve (PEPPAN_parser.py:74-80).  bits: the presence matrix as bit rows, uint64[n_genomes][W] with
 * W = (n_genes + 63) / 64, gene e of genome g at bit e % 64 of bits[g * W + e / 64]; the bits of the last word at and above n_genes (the
 * padding) are zero.  orders: uint32[n_iter][n_genomes], every row a permutation of 0 .. n_genomes - 1.
 *     curves[(k * n_iter + t) * 2 + 0]   genes present in at least one of the genomes orders[t][0 .. k]   (np.sum(genes >= 1))
 *     curves[(k * n_iter + t) * 2 + 1]   genes present in all of them                                     (np.sum(genes >= k + 1))
 * - the reference's array curves[n_genomes][n_iter][2], as int32.  Integer arithmetic only; no size of n_genomes, n_genes or n_iter below
 * the limits is special.  curves is written only when the call succeeds; on any error the context stays usable.  Everything is checked on
 * the host before anything is launched:
 * PEP_ERR_ARG: a null table, n_genomes, n_genes or n_iter of 0, an order row that is no permutation (the message names the row and the
 * entry), a padding bit that is set (the message names the genome).  PEP_ERR_LIMIT: n_genes >= PEP_PARSER_MAX_GENES, n_genomes * n_iter >=
 * PEP_PARSER_MAX_CURVE_POINTS.
 * pep_rarefaction_curves_check runs exactly these checks: no context, no device; the message goes to msg (msg_cap bytes, 0-terminated). */
int pep_rarefaction_curves(pep_ctx *ctx, const uint64_t *bits, uint32_t n_genomes, uint64_t n_genes, const uint32_t *orders, uint32_t n_iter, int32_t *curves);
int pep_rarefaction_curves_check(const uint64_t *bits, uint32_t n_genomes, uint64_t n_genes, const uint32_t *orders, uint32_t n_iter, char *msg, uint64_t msg_cap);

/* K20b: the pair loop of getDistance (PEPPAN_parser.py:172-179).  profiles: int32[n][n_genes], a value > 0 is an allele, anything else
 * "no allele".  For i < j
 *     presence[i * n + j]   genes with profiles[i][e] > 0 and profiles[j][e] > 0
 *     shared[i * n + j]     those of them with profiles[i][e] == profiles[j][e]
 * Every other entry of the two int32[n][n] matrices is 0.  Written only when the call succeeds.
 * PEP_ERR_ARG: a null table, n or n_genes of 0.  PEP_ERR_LIMIT: n > PEP_PARSER_MAX_PROFILES, n_genes >= PEP_PARSER_MAX_GENES.
 * pep_profile_pairs_check runs exactly the checks of the sizes: no context, no device. */
int pep_profile_pairs(pep_ctx *ctx, const int32_t *profiles, uint32_t n, uint64_t n_genes, int32_t *shared, int32_t *presence);
int pep_profile_pairs_check(uint32_t n, uint64_t n_genes, char *msg, uint64_t msg_cap);

/* pep_call_times(PEP_CALL_PARSER): ms[0] of the newest pep_rarefaction_curves and ms[1] of the newest pep_profile_pairs of the context: their kernel
 * times when pep_set_timing is 2 (else 0) - each call resets its own slot only -, and the bytes the newer of the two calls sent to the device and to the host */

/* ---- K21: neighbour-joining trees, the two rapidnj calls of the reference (PEPPAN.py:19, 409-417: `rapidnj -i fa -t d` per paralogous group of
 * filt_per_group; PEPPAN_parser.py:168: `rapidnj -i pd` behind writeCGAV).
 * trees of up to this many leaves are joined by one workgroup each (all of them in one launch per size class); larger ones by a chain of launches, two per join */
#define PEP_NJ_BLOCK_LEAVES 256
/* leaves of one tree */
#define PEP_NJ_MAX_LEAVES 8192
/* bytes of distance matrices of one pep_nj_trees call (8 * dist_off[n_trees]); bytes of pair counts of one pep_kimura_pairs call */
#define PEP_NJ_MAX_BYTES (1ull << 30)

/* K21a: the three pair counts of Kimura's distance, which `rapidnj -i fa` computes from the FASTA the reference writes (PEPPAN.py:19, 409-417).  Rows and
 * groups exactly as for pep_allele_diff: base-5 packed rows, row_off[n_rows + 1], row_len[n_rows], grp_off[n_groups + 1], grp_rows = row indices, the rows
 * of a group of one row_len.  For every pair a < b of group g, in the row-major order of pep_allele_diff's packed triangle, three int32 at
 * out[out_off[g] + 3 * pair]: the columns where both codes are 1..4 (comparable), among those the columns A <-> G or C <-> T (transitions: codes 1 <-> 3,
 * 2 <-> 4), and the other mismatching comparable columns (transversions).  Raw counts, without pep_allele_diff's + 1 / + 2; the logarithm is host work
 * (peppan_amd/njtree.py: kimura_distances).  out_off[g] and out_cap count int32 values.  Empty batches, empty groups and groups of one row are legal.
 * PEP_ERR_ARG: what pep_allele_diff names for rows and groups, an output that runs past out_cap or overlaps another group's.  PEP_ERR_LIMIT: more than
 * PEP_NJ_MAX_BYTES of counts, or what pep_allele_diff names for the bit planes; the message says how much was asked for.
 * pep_call_times(PEP_CALL_KIMURA_PAIRS): of the newest call, ms[0], ms[1] the kernel times - bit planes, pairs - when pep_set_timing is 2, zeros otherwise. */
int pep_kimura_pairs(pep_ctx *ctx, const uint8_t *packed, const uint64_t *row_off, const uint32_t *row_len, uint64_t n_rows, uint32_t n_groups,
                     const uint64_t *grp_off, const uint32_t *grp_rows, int32_t *out, const uint64_t *out_off, uint64_t out_cap);

/* K21b: neighbour joining over a batch of distance matrices (what rapidnj does for PEPPAN.py:416 and PEPPAN_parser.py:168).  Matrix t is row-major
 * double[n][n], n = n_leaves[t], at dist + dist_off[t]; only entries with row < column are read.  dist_off and out_off have n_trees + 1 entries, the last
 * one the length of the array (of dist in doubles; of node and length in entries): dist_off[t] + n * n <= dist_off[t + 1] and out_off[t] + 2 n - 3 <=
 * out_off[t + 1] (n = 2: + 2), so no two trees overlap and none runs past its array.  Entries of node / length between two trees are zeroed.
 *
 * The arithmetic, every operation one correctly rounded double operation (nothing is contracted into a fused multiply-add): slots 0 .. n - 1 hold the
 * leaves, node[slot] the node id (leaves 0 .. n - 1, join s creates node n + s).  r[k] = D[k,0] + D[k,1] + .. from 0.0, left to right, the diagonal as 0.
 * With m live slots, m > 3: over live a < b, Q = ((m - 2) * D[a,b] - r[a]) - r[b]; the smallest Q below +infinity wins (a NaN never), ties go to the smaller
 * a, then the smaller b; when no Q is below +infinity, the first two live slots.  la = 0.5 * D[a,b] + (r[a] - r[b]) / (2 * (m - 2)), lb = D[a,b] - la.  For every other
 * live k: du = ((D[a,k] + D[b,k]) - D[a,b]) * 0.5, r[k] = ((r[k] - D[a,k]) - D[b,k]) + du, D[a,k] = D[k,a] = du.  Then r[a] = 0.5 * ((r[a] + r[b]) - m * D[a,b]),
 * slot a becomes node n + s, slot b is retired.  At m = 3, live a < b < c: la = 0.5 * ((D[a,b] + D[a,c]) - D[b,c]), lb = D[a,b] - la, lc = D[a,c] - la.
 * n = 2: both leaves get D[0,1].
 * Output of tree t at out_off[t], 2 n - 3 entries of node[] and length[]: for s = 0 .. n - 4 the two joined node ids (slot a's first) and la, lb; then the
 * last three node ids in slot order with la, lb, lc; n = 2: two entries.  One exception, so that the text of a three-leaf tree is rapidnj's character for
 * character: n = 3 gives leaves 1, 0, 2 with lb, la, lc, the order rapidnj prints them in (('B':..,'A':..,'C':..);).
 * PEP_ERR_ARG: a null table, n < 2, offsets that overlap or run past their arrays, a distance of the read triangle that is not finite (the message names
 * tree, row and column).  PEP_ERR_LIMIT: n > PEP_NJ_MAX_LEAVES, more than PEP_NJ_MAX_BYTES of matrices; the message says how much was asked for.
 * n_trees == 0 is legal.
 * pep_call_times(PEP_CALL_NJ_TREES): of the newest call, ms[0] the time of the one-workgroup-per-tree kernels, ms[1] of the launch chains, when pep_set_timing
 * is 2, zeros otherwise. */
int pep_nj_trees(pep_ctx *ctx, const double *dist, const uint64_t *dist_off, const uint32_t *n_leaves, uint32_t n_trees, uint32_t *node, double *length,
                 const uint64_t *out_off);
/* every check of pep_nj_trees that does not read a distance, without a context or a device: its code, its text in msg[msg_cap] (cut to fit) */
int pep_nj_trees_check(const uint32_t *n_leaves, uint32_t n_trees, const uint64_t *dist_off, const uint64_t *out_off, char *msg, uint64_t msg_cap);

/* ---- K22: the genome-pair identity statistics of the reference's get_global_difference (PEPPAN.py:1611-1666), the (mean, sigma) table that K16
 * (orthofilter.gd_table) and K17 (ingroups.initializing) read.
 *
 * The function is cut in two.  The ORDER-DEPENDENT part (:1632-1659 without its two inner loops) is a dictionary walk over the selected rows that only
 * decides which two member lists meet at each row; it costs the sum of the list lengths and is host C++ (pep_global_diff_walk), like pep_similar_scan.
 * The QUADRATIC part - the cross product of the two lists of every row, grouped by genome pair, and the two means per pair - is the device's
 * (pep_global_diff).  The host tail (:1663-1665: two clamps, np.sqrt, np.exp) stays numpy (peppan_amd/globaldiff.py).
 * distinct genomes of one call: the keys live in a dense triangular table of G (G + 1) / 2 entries */
#define PEP_GDIFF_MAX_GENOMES 16384
/* items (list-pair members, the sum of a_len * b_len over the events) of one call: at most this many */
#define PEP_GDIFF_MAX_ITEMS (1ull << 32)
/* entries of the logarithm table: a value code is 0 .. PEP_GDIFF_TABLE - 1 (1.005 - code / 10000 stays positive) */
#define PEP_GDIFF_TABLE 10050
/* items of one chunk when chunk_items is 0, and the most a caller may ask for (the chunk's keys are sorted by pep_sort_u64) */
#define PEP_GDIFF_CHUNK_ITEMS (1u << 24)
#define PEP_GDIFF_MAX_CHUNK_ITEMS (1u << 26)
/* bytes of device workspace of one call, as computed from its sizes before anything is reserved */
#define PEP_GDIFF_MAX_BYTES (1ull << 34)

/* The host walk (no context, no device).
 * clu / bsn: the selected rows (r, q, value) of the .clu.npy and the .bsn.npy table as int64[n][3], in file order, bsn already without its rows of
 * value <= 0 (:1626).  genes / genome_of: the gene -> genome map, gene ids strictly ascending, the int32 genome of each.  Genome ids are signed (-1 is
 * a legal genome and a legal key member); they are replaced by their ranks 0 .. G - 1 in ascending order over genome_of, which keeps the order of
 * tuple(sorted(...)).
 *
 * The dictionary semantics of :1632-1659, literally.  A dictionary gene -> list, empty at the start.  A list is a span (off, len, cap) of the arena, an
 * append-only array of genome ranks; `the list [g]` below is a new span of one entry at the arena's end.
 *   clu row (r, q, i):  rr = the list of key r if the dictionary has one, else the list [r] (the key r itself, not a root).  qq = the list of key q,
 *       which is REMOVED from the dictionary, else the list [q].  (r == q: rr and qq are the same list when it has one; else two lists [r].)  The event
 *       (rr.off, rr.len, qq.off, qq.len, i, 0).  Then the dictionary's entry of r becomes rr + qq: with need = rr.len + qq.len, if need > rr.cap: when rr ends where
 *       the arena ends the arena grows to make rr.cap = need, else rr moves - cap = 2 * need new entries (zeros) at the arena's end, its len
 *       entries copied; then qq's len entries are copied behind rr's and rr.len = need.  Nothing that an earlier event names is ever overwritten.
 *   bsn row (r, q, i):  rr and qq as above (q's entry removed); the event (.., i, 1); nothing is written back.
 * An event names two prefixes of lists; drop_same = 0 for clu rows (same-genome pairs count), 1 for bsn rows (:1654).
 * PEP_ERR_ARG: a null table; gene ids not strictly ascending; a gene of a row that is not in the map (the message names the gene); a value outside
 * 0 .. PEP_GDIFF_TABLE - 1 (the message names the row: the reference would take the logarithm of a number that is not positive); an arena beyond 2^32 - 1.
 * The message goes to msg (msg_cap bytes, 0-terminated).  *out: a handle to the result, to be freed by pep_global_diff_walk_free on every path that got one. */
typedef struct pep_gdiff_walk pep_gdiff_walk;
int pep_global_diff_walk(const int64_t *clu, uint64_t n_clu, const int64_t *bsn, uint64_t n_bsn, const int64_t *genes, const int32_t *genome_of,
                         uint64_t n_genes, pep_gdiff_walk **out, char *msg, uint64_t msg_cap);
/* events (one per row: n_clu + n_bsn), entries of the arena, distinct genomes G */
int pep_global_diff_walk_size(const pep_gdiff_walk *walk, uint64_t *n_events, uint64_t *arena_len, uint32_t *n_genomes);
/* events: int64[n_events][6] = (a_off, a_len, b_off, b_len, value, drop_same); arena: int32[arena_len] genome ranks; genomes: int32[G], the genome id of every rank */
int pep_global_diff_walk_copy(const pep_gdiff_walk *walk, int64_t *events, int32_t *arena, int32_t *genomes);
void pep_global_diff_walk_free(pep_gdiff_walk *walk);

/* K22.  events and arena as the walk leaves them (a caller may bring its own), n_genomes = G, table = double[PEP_GDIFF_TABLE], for the reference
 * np.log(1.005 - np.arange(10050) / 10000.) made by numpy on the host: element i is bit for bit the reference's logarithm of a value i.
 *
 * Item (a, b) of event e, 0 <= a < a_len, 0 <= b < b_len: key = (min, max) of arena[a_off + a] and arena[b_off + b]; value code = the event's value;
 * sequence number = base(e) + a * b_len + b, base the exclusive sum of a_len * b_len over the events.  An item of two equal ranks in a drop_same event
 * does not exist (its sequence number stays unused).  For every key with at least one item, with x_0 .. x_(n-1) = table[code] of its items in the order
 * of their events (all items of one event have one code, so their order inside the event does not matter):
 *   S(x) = numpy's sum of a float64 array as np.mean computes it: s = 0.0; for every buffer of 8192 elements (the last one shorter), left to right,
 *          s = s + P(buffer).  P(v, n) is numpy's pairwise sum: n < 8: r = 0.0, r = r + v[i] left to right.  n <= 128: eight accumulators r[j] = v[j],
 *          r[j] = r[j] + v[i + j] for i = 8, 16, .. while i + 8 <= n; r = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); then r = r + v[i] for the
 *          rest.  n > 128: P(v, h) + P(v + h, n - h) with h = n / 2 - (n / 2) % 8.
 *   m = S(x) / n,   v = S((x - m) * (x - m)) / n.
 * Every operation is one correctly rounded IEEE double operation; nothing is contracted into a fused multiply-add.
 * The call leaves the keys on the device: *n_keys is their number; pep_global_diff_copy fetches them, ordered by the smallest sequence number of each
 * key - the insertion order of the reference's dictionary, also where two keys first appear inside one event.
 *
 * chunk_items: the lists are filled chunk by chunk - chunks of this many sequence numbers, cut in event order, an event larger than a chunk split by
 * item range; 0 = PEP_GDIFF_CHUNK_ITEMS.  The result does not depend on it.
 * PEP_ERR_ARG: a null table, an event that runs past the arena or has an empty list, a value code outside the table, a drop_same other than 0 / 1, a
 * rank outside 0 .. G - 1 (the message names event or entry), chunk_items above PEP_GDIFF_MAX_CHUNK_ITEMS.  PEP_ERR_LIMIT, with the amount asked for in
 * the message: G > PEP_GDIFF_MAX_GENOMES, more than PEP_GDIFF_MAX_ITEMS items, more than PEP_GDIFF_MAX_BYTES of workspace (keys counted as
 * min(G (G + 1) / 2, items)).  No events, or no genomes, is legal and gives no keys.
 * pep_call_times(PEP_CALL_GLOBAL_DIFF): of the newest call, ms[0] counting and offsets, ms[1] the chunks (emit, sort, copy), ms[2] the sums, when
 * pep_set_timing is 2, zeros otherwise. */
int pep_global_diff(pep_ctx *ctx, const int64_t *events, uint64_t n_events, const int32_t *arena, uint64_t arena_len, uint32_t n_genomes,
                    const double *table, uint64_t chunk_items, uint64_t *n_keys);
/* the keys of the newest pep_global_diff of this context, n_keys of them: the two ranks (g1 <= g2), the number of items, m and v.  PEP_ERR_ARG: n_keys is
 * not what that call reported. */
int pep_global_diff_copy(pep_ctx *ctx, uint64_t n_keys, int32_t *g1, int32_t *g2, uint64_t *n, double *mean, double *var);
/* every check of pep_global_diff, without a context or a device: its code, its text in msg[msg_cap] (cut to fit) */
int pep_global_diff_check(const int64_t *events, uint64_t n_events, const int32_t *arena, uint64_t arena_len, uint32_t n_genomes, uint64_t chunk_items,
                          char *msg, uint64_t msg_cap);

/* ---- K23: the verdict and the digest of every annotated CDS, the per-gene work of the reference's GFF front end - iter_readGFF (PEPPAN.py:117-182),
 * checkPseu (:992-1010) and addGenes (:1013-1021) - which builds the gene dictionary that writeGenes and every later stage start from.
 * The host (peppan_amd/gffgenes.py) reads the files, resolves names and makes the gene texts; the device judges and digests.
 *
 * The inputs.  nt: the contigs of a batch of files, one after another, contig c at nt[contig_off[c] .. contig_off[c + 1]): ASCII, ALREADY UPPER-CASED by
 * the caller (:167).  CDS i is ONE window of ONE contig: win_len[i] bytes from the 0-based win_off[i] of contig contig[i] - the reference keeps the first
 * line of a gene name and ignores every later one (the elif of :158 compares a bare sequence id with a prefixed one and is never true), so :170-172 cut
 * exactly one slice.  strand[i] = 1: the window is read backward and complemented as rc() does (modules/configure.py:152-154): A <-> T, C <-> G, every
 * other byte - N and '-' included - becomes N.  strand[i] = 0: the bytes as they stand.  Call the text so read s, L = win_len[i].
 *
 * The verdict, checkPseu (:992-1010).  The rules in this order, each but the first waived by its bit of `mask`:
 *   1  L < min_cds                                                             (:993)
 *   2  L % 3 != 0, unless PEP_CDS_ALLOW_FRAMESHIFT                             (:997)
 *   The translation is frame 1 with marked starts (:1000; transeq, modules/configure.py:160-194), n = ceil(L / 3) codons, the last one padded with
 *   characters outside the alphabet when L % 3 != 0 (:186-187).  A codon holding a '-' is '-' (:190) - also beside another odd character, also when the
 *   '-' sits in a padded last codon; else a codon with a character outside ACGT is X (:191); else M for ATG GTG TTG (:172, and table[14]), X for TAA TAG
 *   and - unless table4 - TGA (:168-170), anything else otherwise.
 *   3  codon 0 is not M, unless PEP_CDS_ALLOW_NO_START                         (:1001)
 *   4  codon n - 1 is not X, unless PEP_CDS_ALLOW_NO_STOP                      (:1004)
 *   5  an X among codons 0 .. n - 2, unless PEP_CDS_ALLOW_INNER_STOP           (:1007)
 *   0  otherwise.
 * With one codon, codon 0 is codon n - 1.  L = 0 with min_cds = 0 has no codon: the reference raises there (iter_readGFF turns that into its code 6, addGenes
 * lets it escape); the library answers as if no codon were M or X, and its Python callers never send such a window.  Codes 1 and 2 are decided before a
 * byte is read.  Nothing outside the window is read.
 *
 * The digest (:178, :1020).  digest[20 i ..]: SHA-1 of s, the 20 bytes of hashlib.sha1(s).digest(), for every CDS of code 0; twenty zero bytes for the
 * others.  It is computed straight from nt: no copy of s is made anywhere.
 * a window holds fewer bytes than this */
#define PEP_CDS_MAX_WINDOW (1u << 31)
/* CDS of one call: fewer than this (n_cds is 32 bits wide; the Python binding refuses more) */
#define PEP_CDS_MAX_ITEMS (1ull << 32)
/* the bits of `mask`, one per letter of the reference's incompleteCDS parameter: s, i, f, e */
#define PEP_CDS_ALLOW_NO_START 1
#define PEP_CDS_ALLOW_INNER_STOP 2
#define PEP_CDS_ALLOW_FRAMESHIFT 4
#define PEP_CDS_ALLOW_NO_STOP 8

/* every check of pep_cds_genes, without a context or a device (nt is not read): its code, its text in msg[msg_cap] (cut to fit).
 * PEP_ERR_ARG: a null table; contig_off that does not start at 0 or decreases (offsets are 64 bits wide); a contig index outside 0 .. n_contigs - 1; a
 * window that leaves its contig; a strand byte that is not 0 or 1; a mask with bits beyond the four.  PEP_ERR_LIMIT: a window of PEP_CDS_MAX_WINDOW bytes
 * or more.  The message names the CDS.  n_cds = 0 is legal. */
int pep_cds_genes_check(const uint64_t *contig_off, uint32_t n_contigs, uint32_t n_cds, const uint32_t *contig, const uint64_t *win_off,
                        const uint32_t *win_len, const uint8_t *strand, uint32_t mask, char *msg, uint64_t msg_cap);

/* K23: code[n_cds] (0 .. 5) and digest[20 n_cds] as stated above.  Two launches on the context's stream - the verdicts, one wavefront per CDS; the digests of
 * the CDS of code 0, one thread per CDS - with nothing in between; on an error nothing is written.
 * pep_call_times(PEP_CALL_CDS_GENES): of the newest call, ms[0], ms[1] the kernel time of each launch - verdicts, digests - when pep_set_timing is 2, zeros otherwise. */
int pep_cds_genes(pep_ctx *ctx, const uint8_t *nt, const uint64_t *contig_off, uint32_t n_contigs, uint32_t n_cds, const uint32_t *contig,
                  const uint64_t *win_off, const uint32_t *win_len, const uint8_t *strand, uint32_t min_cds, uint32_t mask, int table4,
                  uint8_t *code, uint8_t *digest);

/* ---- K24: the allele pass of the reference's write_output (PEPPAN.py:1391-1472) for a whole prediction table - which window determineGeneStructure is to
 * look at for every prediction, which bytes are its allele, and which number that allele gets in its gene.
 * The host (peppan_amd/outalleles.py) resolves names to indices, evaluates the reference's float expressions in float64 and formats the texts; the
 * device sees integers and bytes only.
 *
 * The inputs.  nt: contigs one after another, contig c at nt[contig_off[c] .. contig_off[c + 1]), ASCII as the reference holds them.  The
 * representative of a gene that has one (clust_ref) is appended as a contig of its own: seed_contig[g] names it, -1 = gene g has no seed.  Row i of the
 * prediction table, in the table's order, is the PEP_OUTA_COLS int32 values rows[PEP_OUTA_COLS i ..]:
 *   PEP_OUTA_GENE    index of column 0 among the distinct names (0 .. n_genes - 1; not read for a skipped row)
 *   PEP_OUTA_CONTIG  index of column 5 (rows of one contig name carry one index: the neighbour search compares it)
 *   PEP_OUTA_FLAGS   PEP_OUTA_MISC: column 15 is misc_feature; PEP_OUTA_NONAME: column 0 is empty; PEP_OUTA_SECONDARY: column 4 is not empty;
 *                    PEP_OUTA_MINUS: column 11 is not '+'
 *   PEP_OUTA_S, _E   columns 9 and 10, 1-based, inclusive: s, e
 *   PEP_OUTA_PART    column 1        PEP_OUTA_QS, _QE  columns 7 and 8        PEP_OUTA_REFLEN  column 12        PEP_OUTA_CLEN  column 13 as it stands at :1390
 *   PEP_OUTA_VARY    allowed_vary = int(col12 * (1 - pseudogene) + 0.01)  (:1408)
 *   PEP_OUTA_SVMIN   0: no structural-variation test; else the smallest allele length that passes it, ceil(pseudogene * len(representative))  (:1461)
 * look9 (optional, int32[n_rows]): column 9 as a row of an EARLIER batch of PEP_OUTA_BATCH rows shows it to a '-' row i with i % PEP_OUTA_BATCH < 5 -
 * the reference writes determineGeneStructure's results back after every batch (:1468-1472), so those rows alone see updated neighbours.  NULL: s.
 *
 * The plan of row i, plan[PEP_OUTA_PLAN_COLS i ..]: class, s2, e2, lp, a, len.
 *   PEP_OUTA_SKIPPED   PEP_OUTA_MISC or PEP_OUTA_NONAME (:1405).  Nothing else of the row is read or checked; it is in no class, its other outputs are zero.
 *   PEP_OUTA_FRAGMENT  column 1 > 1 or e - s + 1 < col12 - allowed_vary (:1415).  s2 = s, e2 = e, lp = 0; the allele is [s - 1, e) of the contig.
 *   PEP_OUTA_INTACT    otherwise (:1422-1458), with 3 int(x / 3) truncating toward zero.  pred2 is, for '+', the LAST row that is not PEP_OUTA_MISC among rows
 *                      i + 1 .. i + 4, for '-' the FARTHEST such row among i - 1 .. i - 5, the walk ending at the table's end or at the first row of another contig.
 *                        '+'  e2 = e + min(3 int((clen - e) / 3), pred2 ? 3 int((e(pred2) + 300 - e) / 3) : 600 + col12 - col8)
 *                             s2 = s - min(3 int((s - 1) / 3), 60 + col7 - 1);  lp = s - s2, rp = e2 - e
 *                        '-'  s2 = s - min(3 int((s - 1) / 3), pred2 ? 3 int((s - s9(pred2) + 300) / 3) : 600 + col12 - col8)
 *                             e2 = e + min(3 int((clen - e) / 3), 60 + col7 - 1);  lp = e2 - e, rp = s - s2
 *                      The window of determineGeneStructure is [s2 - 1, e2).  The allele is window[lp : len - rp] with Python's slice semantics: [s - 1, e) when
 *                      rp >= 0, and the shorter [s - 1, e2) on '+' / [s2 - 1, e) on '-' when rp < 0 (a nested neighbour) - empty when that is no span.
 *   PEP_OUTA_STRUCTVAR intact, and len < PEP_OUTA_SVMIN: the row does not go to determineGeneStructure (:1461-1462).
 * a: the 0-based position of the allele's first byte in its contig, len: its bytes.  On '-' the allele is those bytes upper-cased, complemented and reversed,
 * everything outside ACGTN becoming N (modules/configure.py:152-154); on '+' the bytes as they stand.
 *
 * The numbering.  Two rows that are not skipped are in one class when their genes and their allele bytes are equal; the seed of a gene is in front of all
 * its rows.  first[i]: the smallest row index of the class of row i, -1 when that is the seed, -2 for a skipped row.  rank[i]: 1 + the number of classes of
 * the gene whose first member comes before this one's - the number the reference's dictionary gives (:1420, :1455-1457), the seed being 1.  tflag[i]: 1 when
 * the allele's id carries the 't' prefix, a property of the class's first member: never for the seed, always for a fragment, for an intact row unless
 * PEP_OUTA_SECONDARY is clear, col7 = 1 and col8 = col12 (:1454).  None of it depends on the order in which the device worked.
 *
 * What is refused, PEP_ERR_ARG with the row in the message, for a row that is not skipped: s < 1; e < s - 1; e beyond the actual contig; col7 < 1;
 * lp < 0 (the reference's slice would wrap); e2 < s2 - 1 (no window); e2 beyond the actual contig.  (s2 >= 1 follows from s >= 1.)  Also PEP_ERR_ARG: a
 * null table; contig_off that does not start at 0 or decreases; a gene, contig or seed index out of range; flag bits beyond the four; key_bits > 31.
 * PEP_ERR_LIMIT: a contig of PEP_OUTA_MAX_CONTIG bytes or more (positions are int32); n_rows + n_genes of PEP_OUTA_MAX_ITEMS or more. */
#define PEP_OUTA_COLS 12
#define PEP_OUTA_GENE 0
#define PEP_OUTA_CONTIG 1
#define PEP_OUTA_FLAGS 2
#define PEP_OUTA_S 3
#define PEP_OUTA_E 4
#define PEP_OUTA_PART 5
#define PEP_OUTA_QS 6
#define PEP_OUTA_QE 7
#define PEP_OUTA_REFLEN 8
#define PEP_OUTA_CLEN 9
#define PEP_OUTA_VARY 10
#define PEP_OUTA_SVMIN 11
/* the bits of PEP_OUTA_FLAGS */
#define PEP_OUTA_MISC 1
#define PEP_OUTA_NONAME 2
#define PEP_OUTA_SECONDARY 4
#define PEP_OUTA_MINUS 8
/* the columns of a plan record and the classes */
#define PEP_OUTA_PLAN_COLS 6
#define PEP_OUTA_SKIPPED 0
#define PEP_OUTA_FRAGMENT 1
#define PEP_OUTA_INTACT 2
#define PEP_OUTA_STRUCTVAR 3
/* rows between two write-backs of the reference (:1401) */
#define PEP_OUTA_BATCH 10000
#define PEP_OUTA_MAX_CONTIG (1u << 31)
#define PEP_OUTA_MAX_ITEMS (1u << 30)
/* two rows that the digest put into one class hold different bytes: nothing was merged, nothing was written */
#define PEP_ERR_ALLELE_CLASS (-24)

/* every check of pep_out_alleles, without a context or a device (nt is not read): its code, its text in msg[msg_cap] (cut to fit).  n_rows = 0 is legal. */
int pep_out_alleles_check(const uint64_t *contig_off, uint32_t n_contigs, uint32_t n_genes, const int32_t *seed_contig, uint32_t n_rows,
                          const int32_t *rows, const int32_t *look9, uint32_t key_bits, char *msg, uint64_t msg_cap);

/* K24: plan[PEP_OUTA_PLAN_COLS n_rows], first[n_rows], rank[n_rows], tflag[n_rows] as stated above; on an error nothing is written.
 * plan_only != 0: the plan alone (one launch; nt may be NULL and is not uploaded; first, rank and tflag may be NULL and are not written) - what the first of the
 * reference's two rounds needs before column 9 of the earlier batches is known.
 * Otherwise, on the context's stream: the plan; SHA-1 of every allele read in place, strand-corrected, one thread per allele; a table that gives every
 * (gene, length, digest) its smallest member; a comparison of every member's bytes with that one's - a difference ends the call with PEP_ERR_ALLELE_CLASS and
 * the two rows in the message; the library's radix sort over the first members by (gene, index), from which the ranks follow.
 * key_bits (testing only, 0 in every other use): when 1 .. 31, a class is (gene, the low key_bits bits of the digest's first word) - distinct alleles then
 * share classes, which is the one way to see the comparison refuse them.
 * pep_call_times(PEP_CALL_OUT_ALLELES): of the newest call, ms[0..5] - plan, digest, classes, comparison, sort, ranks - kernel times when pep_set_timing is 2,
 * zeros otherwise (plan_only: ms[0] alone; a call that ends with PEP_ERR_ALLELE_CLASS: zeros). */
int pep_out_alleles(pep_ctx *ctx, const uint8_t *nt, const uint64_t *contig_off, uint32_t n_contigs, uint32_t n_genes, const int32_t *seed_contig,
                    uint32_t n_rows, const int32_t *rows, const int32_t *look9, int plan_only, uint32_t key_bits, int32_t *plan, int32_t *first,
                    uint32_t *rank, uint8_t *tflag);

/* ---- K25: the tree cutting of filt_per_group (PEPPAN.py:424-482), which the reference does with ete3, for a batch of trees.
 *
 * What is restated.  :424-482 are a computation on the UNROOTED tree: a node's score is a sum over (leaves below) x (the component's other leaves) of a
 * symmetric matrix, so it belongs to the branch's bipartition, whichever side is "below"; the two children of the root are one bipartition with one length
 * (:440-442); the smallest leaf name, not the direction of the cut, decides which part stays in place (:466-467); pruning a subtree and suppressing the node
 * of degree two (:462-465) leaves the tree induced on the remaining leaves, whose branches are the distinct non-trivial restrictions of the original
 * bipartitions.  So the device works on bit sets of leaves and never roots a tree.  The rooting shows in exactly one place: an exact tie of the first two
 * sort keys of :458 between two DIFFERENT bipartitions, where the reference reads n.dist, which its doubling of the root branch (:440-442) makes depend on
 * ete3's midpoint rooting.  AT THESE TIES, AND ONLY THERE, THE REFERENCE'S CHOICE IS NOT RESTATED: the rule below decides, and every such tie is counted in
 * n_ties for the caller to see.  ete3 itself cannot be run where this project is built; the contract therefore stands on two legs: PEPPAN.py:326-484
 * themselves, run over a small stand-in for the ete3 calls they make, rooted two ways (tests/golden/make_golden_treecut.py), and a numpy restatement of the
 * definition below, operation for operation (tests/treecut_helpers.py), which the device equals bit for bit.
 *
 * Input of tree t (n = n_leaves[t] leaves, 2 <= n <= PEP_NJ_MAX_LEAVES; words = (n + 63) / 64):
 *   leaves         0 .. n - 1, in the order of the reference's leaf names read as integers (the leader rows g[0], ascending)
 *   branches       B = branch_off[t + 1] - branch_off[t] of them, 1 <= B <= 2 n (2 n - 3 from a text of njtree.newick; 2 for n = 2).  Branch e: the bit
 *                  set of the leaves on one of its sides, `words` 64-bit words at sets + set_off[t] + e * words (leaf l is bit l % 64 of word l / 64),
 *                  and length[branch_off[t] + e], the printed %.5g value, since the reference parses the text
 *   W0, W1         incompatible[:, :, 0] and [:, :, 1] (:400-404) compacted to the leaves, row-major double[n][n] at w0 / w1 + mat_off[t]; symmetric,
 *                  every entry finite and >= 0
 *   strong[leaf]   at strong + leaf_off[t]: non-zero when mat[leader, 4] >= (clust_identity - 0.02) * 10000, which the host evaluates in float64 (:469)
 *   cap[t]         the iterations of one component (:435; the reference's 3000)
 * Every offsets table has n_trees + 1 entries, the last one the length of its arrays: leaf_off[t] + n <= leaf_off[t + 1], mat_off[t] + n * n <=
 * mat_off[t + 1], set_off[t] + B * words <= set_off[t + 1]; branch_off is dense.
 *
 * The definition.  M[a][b] = W1[a][b] where W0[a][b] > W1[a][b], else 0.0.  The queue of components (gene_phys, :431-473) starts as [all leaves]; component
 * q is taken when its turn comes, T its leaves, t0 the smallest of them.  At most cap[t] times:
 *   1. if W0[a][b] <= W1[a][b] for all a, b of T (the diagonal included, :438) the component is finished.
 *   2. every branch e whose far side F = (side_e or its complement, whichever does not hold t0) restricted to T is not empty is a candidate; C = T \ F.
 *      For each of the three matrices X = W0, W1, M the sum over a in F, b in C in this order: for a row a, lane l = 0 .. 63 holds p[l] = 0.0 + X[a][l] +
 *      X[a][l + 64] + .. over the b = l, l + 64, .. that are in C, ascending; then for off = 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l ^ off] for all l at once;
 *      rowsum(a) = p[0].  s = 0.0, then s = s + rowsum(a) over the rows a of F, ascending.  This gives s0, s1, m.
 *      ic0 = s0 / (s1 > 1.0 ? s1 : 1.0); key = ic0 * sqrt(m) (:451-456).  Every operation is one correctly rounded double operation, nothing is contracted;
 *      the order depends on T and the branch alone, not on the batch, the launch geometry or the path.
 *   3. among the candidates with ic0 > 1 whose key is no NaN the largest (key, ic0) wins (:456-458); branches with the same F are ONE candidate.  None: the
 *      component is finished (:471-472).  Several different F with the winner's (key, ic0): the larger sum of the lengths of its inducing branches (0.0 +
 *      length, ascending branch index) wins, then the smaller smallest leaf of F, then the lower branch index; n_ties grows by the number of the OTHER F.
 *   4. the cut: T \ F keeps the component's place in the queue (:466-468); F is appended to the queue when one of its leaves is strong (:469-470) and is
 *      dropped otherwise, its leaves belonging to no output.
 * Output of tree t: part[leaf_off[t] + leaf] the index of the leaf's component in the queue - the order of the reference's returned list -, -1 for a dropped
 * leaf; counts[4 t ..] = n_parts, n_cuts, n_ties, 0; and for cut c = 0 .. n_cuts - 1 (at most n - 1) the record i = leaf_off[t] + c: log_where[2 i] the
 * component's index, log_where[2 i + 1] the lowest inducing branch index; log_val[4 i ..] = s0, s1, m, key.  Entries of part between two trees are -1, log entries
 * behind a tree's records zero.
 *
 * Two paths that give identical bits: trees of up to PEP_NJ_BLOCK_LEAVES leaves are cut by one workgroup each, all of them in one launch, the bit sets in
 * LDS; larger ones by a chain of launches, two per iteration (score, select-and-apply), enqueued PEP_CUT_ROUND iterations at a time with one read of the
 * tree's `done` flag between rounds.  path: PEP_CUT_AUTO, PEP_CUT_BLOCK (PEP_ERR_LIMIT for a larger tree), PEP_CUT_CHAIN (any tree).
 *
 * PEP_ERR_ARG: a null table; n < 2; offsets that overlap or run past their arrays; B < 1 or B > 2 n; a branch that is no bipartition of the tree's leaves
 * (a bit beyond leaf n - 1, an empty side, a side with every leaf); branches that are not pairwise compatible; an unknown path - all of these by
 * pep_tree_cut_check as well -; and by pep_tree_cut alone, which reads them: a W entry or a length that is not finite, a negative W entry, W not symmetric.
 * PEP_ERR_LIMIT: n > PEP_NJ_MAX_LEAVES, PEP_CUT_BLOCK for n > PEP_NJ_BLOCK_LEAVES, more than PEP_NJ_MAX_BYTES of one matrix (8 * mat_off[n_trees]) or of
 * bit sets; the message says how much was asked for.  n_trees == 0 is legal.
 * pep_call_times(PEP_CALL_TREE_CUT): of the newest call, ms[0] the time of the preparation and the one-workgroup kernel, ms[1] of the launch chains, when
 * pep_set_timing is 2, else zeros. */
#define PEP_CUT_AUTO 0
#define PEP_CUT_BLOCK 1
#define PEP_CUT_CHAIN 2
/* iterations of a launch chain that are enqueued between two reads of the `done` flag */
#define PEP_CUT_ROUND 8
/* the reference's iterations per component (PEPPAN.py:435) */
#define PEP_CUT_DEFAULT_CAP 3000

int pep_tree_cut(pep_ctx *ctx, const uint32_t *n_leaves, uint32_t n_trees, const uint64_t *leaf_off, const uint64_t *mat_off, const uint64_t *branch_off,
                 const uint64_t *set_off, const uint64_t *sets, const double *length, const double *w0, const double *w1, const uint8_t *strong,
                 const uint32_t *cap, uint32_t path, int32_t *part, int32_t *counts, int32_t *log_where, double *log_val);
/* every check of pep_tree_cut that reads no matrix and no length, without a context or a device: its code, its text in msg[msg_cap] (cut to fit) */
int pep_tree_cut_check(const uint32_t *n_leaves, uint32_t n_trees, const uint64_t *leaf_off, const uint64_t *mat_off, const uint64_t *branch_off,
                       const uint64_t *set_off, const uint64_t *sets, uint32_t path, char *msg, uint64_t msg_cap);

/* ---- K26: the front half of every round of filt_genes (PEPPAN.py:546-624, and :641-656 for `--orthology sbh`) for one batch of genes: what stands
 * between the gene scores and the `to_run` list of filt_per_group.
 *
 * Tables.  A gene's table is int64[n, 7] rows of the .tab store: 0 exemplar, 1 genome, 2 score x 10^4, 3 identity x 10^4, 4 a copy of column 3, 5 locus id,
 * 6 hit count.  A batch is the tables of its genes one behind the other, handed over column by column: gene g owns the rows gene_off[g] .. gene_off[g + 1] - 1;
 * gene_off has n_genes + 1 entries, starts at 0 and never falls.  The conflict lists (load_conflict, :511-523) are one CSR table over the batch's rows: row r
 * owns cfl[cfl_off[r] .. cfl_off[r + 1] - 1], every value other_locus * 10 + kind (>= 0), in the order of the .conflicts store; cfl_off has gene_off[n_genes]
 * + 1 entries, starts at 0 and never falls.  Locus ids lie in [0, n_loci), n_loci <= PEP_PREP_MAX_LOCI, and no locus comes twice in one gene's table.
 *
 * Stage A, pep_batch_screen (:548-562; device, order-free per gene because `used` is not written in that loop).  used_state[locus] says what `used` holds for
 * the locus: 0 absent, 1 present with a value <= 0, anything else present with a value > 0.  For gene g with m = max(col3) over its rows (m > 0):
 *   out4[r] = trunc((double)(10000 * col3[r]) / (double)m) - the product is an integer one, the quotient ONE float64 division, the cast cuts toward zero (:552);
 *   state 0: out3[r] = col3[r] and the row counts for present[g] = max(0, out4 over these rows); state 1: out3[r] = -col3[r]; else: out3[r] = 0 (:553-558);
 *   excluded[g] = (double)present[g] < threshold, where threshold is (clust_identity - 0.02) * 10000 as the host evaluated it in float64 (:559).
 * The rows that go on are those with out3 != 0 (:562): the caller's gather.
 *
 * Stage B, pep_batch_unsure_walk (:579-593; host C++, no context, because one set `used2` of locus ids is shared by the whole round: a bitmap over
 * [0, n_loci) here).  The genes come in the caller's order - falling score, stable (:580).  Per gene, with pos = the number of its rows with col3 > 0:
 *   unsure = the number of rows with col3 > 0 whose locus is in used2; when (double)unsure >= (double)pos * 0.6 the gene is popped (popped[g] = 1) and nothing
 *   else happens to it (:583-585; pos = 0 pops).  Otherwise, row by row in table order, negative rows included: when the row's locus is not in used2 every
 *   value / 10 of its list enters used2 - at once, so a list can close the door on a later row of the same table; the row's own locus does not enter
 *   (:588-590).  Then every third row with col3 < 0 is negated back, counting from the first one (:591-592).  The rows with col3 > 0 go on (:593).
 * col3 is rewritten in place.
 *
 * Stage C, pep_batch_prune (device, order-free per gene: `used2` is a new set for every gene, :604 / :648).  Rows are named by their index within the gene's
 * table (source rows); `order` is the current sequence of source rows, at first 0 .. n - 1.  Conflict values that name a locus outside the gene's own table
 * have no effect in this stage.  Of an order: G = the number of distinct genomes, best(k) = the first row of the order with the genome of row k (:600),
 * rs(k) = (double)col4[k] / (double)col4[best(k)], one float64 division (:601).  walk(order): used2 empty; row by row, a row whose locus is in used2 is dropped,
 * of any other row every value / 10 of its list enters used2 (:604-610).
 *  mode PEP_PREP_NJ (nj and ml, :596-624):
 *   1. when n >= 2 G: the order sorted by falling column 2; walk; the survivors sorted by falling column 3; G, best, rs anew (:602-613).
 *   2. when n > 3 G and n > 1000 (n now the rows left): cut = the (3 G)-th largest rs; when cut >= clust_identity, cut = the (6 G + 1)-th largest rs when
 *      n > 6 G, else clust_identity; the rows with rs >= cut stay (:614-619).  The k-th largest is taken on the bit patterns of the doubles, a NaN (0 / 0)
 *      above every number; NaN >= x and x >= NaN are false.  (The reference's sorted() gives no defined order to a list that holds a NaN.)
 *   3. inparalog = some genome has more than one of the rows left (:620).  final = (not inparalog and (double)min(col3) >= final_threshold) or at most one row
 *      left (:621), final_threshold being 10000 * clust_identity as the host evaluated it; every other gene is a `to_run` entry (:624).
 *  mode PEP_PREP_SBH (:641-656): rs(k) = min((double)col2[k] / (double)col2[best(k)], (double)col4[k] / (double)col4[best(k)]), a NaN quotient making rs NaN; the
 *   rows with rs >= clust_identity stay, a NaN dropping the row; walk in table order, WITH WHAT :653 COMPUTES: it adds the one-element list [locus * 10] to
 *   the row's list, which is an array of the store wherever it is not empty, and numpy sums the two element by element - so of a kept row with a list
 *   every (value + locus * 10) / 10 = value / 10 + locus enters used2, and of a kept row without one its own locus, which no other row carries; final
 *   always; inparalog as above.
 * TIES.  The reference sorts with numpy's default, unstable sort, whose order of equal keys depends on the machine's SIMD path.  THE REFERENCE'S ORDER OF
 * EQUAL KEYS IS NOT RESTATED: here equal keys keep their current order in both sorts (the position is the low key).  Two rows that tie in column 2 at :603
 * can change which row the walk keeps: n_ties counts, per call, the genes in which that sort met two equal keys.  Ties in column 3 at :611 change the
 * order of the rows alone, never a value: equal |column 3| within one table means equal column 4.
 * Output of gene g: rows[out_off[g] .. out_off[g + 1] - 1] the source rows left, in final order (the host gathers mat[rows]); inparalog[g]; is_final[g].
 *
 * Two paths of pep_batch_prune that give identical bits: a gene of up to PEP_PREP_LDS_ROWS rows has its working arrays (the order, a sort buffer, best) in
 * LDS, a larger one in a slot of the context's workspace; one workgroup per gene either way, both in one call.  path: PEP_PREP_AUTO, PEP_PREP_LDS
 * (PEP_ERR_LIMIT for a larger gene), PEP_PREP_WS (any gene).
 *
 * A DELIBERATE DIFFERENCE lies in front of these functions: for a member of the .conflicts store that does not exist the reference raises inside a pool
 * worker; peppan_amd.paralogfilter reads it as "no conflicts" (empty lists).
 *
 * PEP_ERR_ARG (the message names the gene): a null table; gene_off or cfl_off that does not start at 0, falls (two genes or lists would overlap) or, for
 * cfl_off, runs past the budget below; an empty gene in C; max(col3) <= 0 in A; a locus id outside [0, n_loci); a locus twice in one gene's table; a conflict
 * value below 0 or (B) naming a locus outside [0, n_loci); a genome id outside [0, 2^32); column 3 or 4 (C: column 2 as well, to 2^62) of 2^31 or more in
 * magnitude; an unknown mode or path; n_loci > PEP_PREP_MAX_LOCI.  PEP_ERR_LIMIT, with the amount asked for: a gene of more than PEP_PREP_MAX_ROWS rows;
 * PEP_PREP_LDS for a gene of more than PEP_PREP_LDS_ROWS rows; more than PEP_PREP_MAX_CFL_BYTES of conflict values (8 bytes each) in one call.  n_genes == 0
 * is legal.  Every check is made by the ..._check twin as well, without a context or a device; the context stays usable after a refusal.
 * pep_call_times(PEP_CALL_BATCH_SCREEN) and pep_call_times(PEP_CALL_BATCH_PRUNE): of the newest pep_batch_screen / pep_batch_prune, ms[0] the kernel time of the
 * call when pep_set_timing is 2, else zeros. */
#define PEP_PREP_NJ 0
#define PEP_PREP_SBH 1
#define PEP_PREP_AUTO 0
#define PEP_PREP_LDS 1
#define PEP_PREP_WS 2
/* rows of one gene whose working arrays stay in LDS (a power of two) */
#define PEP_PREP_LDS_ROWS 4096
/* rows of one gene: 2 000 genomes x 32 copies */
#define PEP_PREP_MAX_ROWS 65536
/* conflict values of one call, in bytes */
#define PEP_PREP_MAX_CFL_BYTES (1ull << 31)
#define PEP_PREP_MAX_LOCI (1ull << 40)

int pep_batch_screen(pep_ctx *ctx, uint32_t n_genes, const uint64_t *gene_off, const int64_t *col3, const int64_t *locus, const uint8_t *used_state,
                     uint64_t n_loci, double threshold, int64_t *out3, int64_t *out4, int64_t *present, uint8_t *excluded);
int pep_batch_screen_check(uint32_t n_genes, const uint64_t *gene_off, const int64_t *col3, const int64_t *locus, uint64_t n_loci, char *msg, uint64_t msg_cap);
int pep_batch_unsure_walk(uint32_t n_genes, const uint64_t *gene_off, int64_t *col3, const int64_t *locus, const uint64_t *cfl_off, const int64_t *cfl,
                          uint64_t n_loci, uint8_t *popped, char *msg, uint64_t msg_cap);
int pep_batch_unsure_walk_check(uint32_t n_genes, const uint64_t *gene_off, const int64_t *col3, const int64_t *locus, const uint64_t *cfl_off,
                                const int64_t *cfl, uint64_t n_loci, char *msg, uint64_t msg_cap);
int pep_batch_prune(pep_ctx *ctx, uint32_t mode, uint32_t n_genes, const uint64_t *gene_off, const int64_t *genome, const int64_t *col2, const int64_t *col3,
                    const int64_t *col4, const int64_t *locus, const uint64_t *cfl_off, const int64_t *cfl, uint64_t n_loci, double clust_identity,
                    double final_threshold, uint32_t path, uint64_t *out_off, int32_t *rows, uint8_t *inparalog, uint8_t *is_final, uint64_t *n_ties);
int pep_batch_prune_check(uint32_t mode, uint32_t n_genes, const uint64_t *gene_off, const int64_t *genome, const int64_t *col2, const int64_t *col3,
                          const int64_t *col4, const int64_t *locus, const uint64_t *cfl_off, const int64_t *cfl, uint64_t n_loci, uint32_t path, char *msg,
                          uint64_t msg_cap);

/* K14 and its two host passes: the consumer of the all-vs-all table (get_similar_pairs, PEPPAN.py:194-294).
 *
 * pep_similar_scan (host, no context): ONE ordered pass over the table as RunBlast.run returns it (sorted by query, reference, score).
 *   q / r: gene codes in [0, n_genes) that keep the order of the gene ids.  action[k]: the row-local classification of PEPPAN.py:246-260
 *   (PEP_ROW_*), forward[k] = column 8 < column 9, iden4[k] = int(identity * 10000).  The pass keeps the reference's state - genes absorbed
 *   by a near-identical partner or found repetitive are dead from then on, forward rows of one (q, r) pair are collected until a row of
 *   another pair survives - and reports: alive[g] (0 = absorbed / repetitive), seen_as_query[g], the absorbed edges (kept, dropped, iden4)
 *   in order, and the events that write ortho_pairs, in order: PEP_EVENT_CONFLICT (pair a < b gets -2, PEPPAN.py:249) or
 *   PEP_EVENT_SUPPORT (pair a < b is to be judged by get_similar over rows ev_rows[ev_row_off[e] .. ev_row_off[e+1]), PEPPAN.py:268-276).
 *   Capacities: absorbed 3 n, ev_* n + 1 (ev_row_off n + 2), ev_rows n.
 * pep_pair_support (K14): get_similar (PEPPAN.py:195-224) for many groups of forward alignments at once.  Group g = rows
 *   [grp_off[g], grp_off[g+1]) in table order, all of one (query, reference) pair of lengths grp_qlen / grp_rlen.  value[g] =
 *   PEP_SUPPORT_NONE (no decision), 0 (similar but too short a support) or int(mean identity * 10000), with the mean taken over the
 *   covered query positions exactly as numpy.mean takes it (first-cover order; pairwise summation inside buffers of 8192 positions, the buffers' sums added up left to right).  At most 255 rows per group.
 * pep_similar_resolve (host, no context): the dictionary ortho_pairs from the events and the values K14 returned for them (ev_value[e]
 *   is ignored for conflicts): out = (a, b, value) triples with value != 0 in first-insertion order (capacity 3 n_events). */
#define PEP_ROW_ORDINARY 0
#define PEP_ROW_CONFLICT 1
#define PEP_ROW_ABSORB_QUERY 2
#define PEP_ROW_ABSORB_REF 3
#define PEP_EVENT_CONFLICT 0
#define PEP_EVENT_SUPPORT 1
#define PEP_SUPPORT_NONE (-2147483647 - 1)
typedef struct {
    uint32_t q_start, r_start;    /* columns 6 and 8: 1-based first query / reference nucleotide (forward alignments only) */
    uint32_t cigar_runs, pad;
    uint64_t cigar_off;           /* runs of (len << 2 | op) in nucleotides, op 0=M 1=I 2=D */
    double identity;              /* column 2 */
} pep_support_row;
typedef struct {
    double match_len[3], match_prop[3];   /* params match_len, match_len1, match_len2 / match_prop, match_prop1, match_prop2 (PEPPAN.py:211, 214-216) */
    double identity_x1e4;                 /* params match_identity * 10000 (PEPPAN.py:213) */
    int32_t any_frame, pad;               /* 'f' in params incompleteCDS (PEPPAN.py:205) */
} pep_support_limits;
/* pep_similar_classify (host, no context; ABI 14): the row-local tests of PEPPAN.py:244-263 over the numeric columns, one pass - what pep_similar_scan takes
 *   as action / forward / iden4.  q / r: gene codes; rank_ge[k] / rank_le[k]: priority rank of row k's query gene >= / <= that of its reference gene
 *   (PEPPAN.py:252, 257: the caller compares whatever type its priorities have); near_identity = clust_identity, cover = clust_match_prop.
 *   Float arithmetic as the reference's float() conversions make it (IEEE double, sqrt(cover) correctly rounded). */
int pep_similar_classify(uint64_t n, const int64_t *q, const int64_t *r, const double *iden, const int64_t *qs, const int64_t *qe, const int64_t *ss,
                         const int64_t *se, const int64_t *ql, const int64_t *sl, const uint8_t *rank_ge, const uint8_t *rank_le, double near_identity,
                         double cover, uint8_t *action, uint8_t *forward, int32_t *iden4);
int pep_similar_scan(uint64_t n, const int64_t *q, const int64_t *r, const uint8_t *action, const uint8_t *forward, const int32_t *iden4, uint64_t n_genes,
                     uint8_t *alive, uint8_t *seen_as_query, int64_t *absorbed, uint64_t *n_absorbed,
                     uint8_t *ev_kind, int64_t *ev_a, int64_t *ev_b, uint64_t *ev_row_off, uint64_t *ev_rows, uint64_t *n_events);
int pep_pair_support(pep_ctx *ctx, uint64_t n_rows, const pep_support_row *rows, const uint32_t *cigar, uint64_t n_cigar, uint64_t n_groups,
                     const uint64_t *grp_off, const uint32_t *grp_qlen, const uint32_t *grp_rlen, const pep_support_limits *lim, int32_t *value);
int pep_similar_resolve(uint64_t n_events, const uint8_t *ev_kind, const int64_t *ev_a, const int64_t *ev_b, const int32_t *ev_value,
                        int64_t *out, uint64_t *n_out);
/* the exemplar rewrite at the end of get_similar_pairs (PEPPAN.py:278-288; host, no context): the FASTA file `path` keeps the records whose
 * name (first token of the header line, a decimal integer) is in ids[0..n_ids) (sorted ascending), verbatim; the file is not touched when
 * every record stays.  PEP_ERR_ARG (file untouched) when a name is not a plain decimal integer: the caller then applies its own rules. */
int pep_fasta_keep(const char *path, const int64_t *ids, uint64_t n_ids, uint64_t *n_records, uint64_t *n_kept);
/* the clusterer's input (the FASTA file clust.py:62-66 hands to `mmseqs createdb`; host, no context): the sequences of the FASTA text
 * data[0..n) as codes[] = table[byte] with off[0 .. *n_records] the start of each record's codes.  A record starts at a '>' at the start of a
 * line, its first line is the header; body lines starting with '#' are dropped, ASCII blanks removed.  codes must hold n bytes, off cap + 1
 * entries; PEP_ERR_LIMIT when the text has more than cap records.  *non_ascii = 1 when a body holds a byte >= 0x80 (the caller then applies
 * its own, Unicode-aware rules). */
int pep_fasta_scan(const uint8_t *data, uint64_t n, const uint8_t *table, uint8_t *codes, uint64_t *off, uint64_t cap, uint64_t *n_records,
                   int32_t *non_ascii);
/* the same pass for the sequence reader of the search (readFasta, configure.py:118-128 of the reference, behind uberBlast.py:339-341): also the records' names -
 * name_off[r] / name_len[r] = the first blank-delimited token of record r's header line inside data (length 0: a header without a name).
 * name_off and name_len hold cap entries. */
int pep_fasta_records(const uint8_t *data, uint64_t n, const uint8_t *table, uint8_t *codes, uint64_t *off, uint64_t *name_off, uint32_t *name_len,
                      uint64_t cap, uint64_t *n_records, int32_t *non_ascii);

/* K13: exact-duplicate collapse of gene instances (front end of the clustering path).
 * pep_sha1: digest[20*i..] = SHA-1 of sequence i (bytes[off[i]..off[i+1])), big-endian bytes as hashlib.sha1(seq).digest();
 *   PEPPAN keys duplicates with int(hexdigest, 16) of it (PEPPAN.py:62, 1019).
 * pep_dedup: writeGenes (PEPPAN.py:1023-1039) over n genes ALREADY in priority order: rep[i] = index of the first gene j <= i
 *   with len[j..i] all equal (the same "length run": the reference forgets what it has seen whenever a different length shows
 *   up, PEPPAN.py:1032-1033) and the same digest; rep[i] == i for a gene that is written out. */
int pep_sha1(pep_ctx *ctx, const uint8_t *bytes, const uint64_t *off, uint32_t n, uint8_t *digest);
int pep_dedup(pep_ctx *ctx, uint32_t n, const uint32_t *len, const uint8_t *digest, uint32_t *rep);

/* Host-side C++ (no GPU work, no context): the order-dependent greedy filters of the genome mapping.
 * Both take the numeric columns of the hit table ALREADY SORTED the way the reference sorts it, with reverse-strand
 * reference coordinates negated (uberBlast.py:420, 455): q / r = integer codes of the query / reference names.
 *
 * pep_ovl_filter (flag -f, RunBlast.ovlFilter uberBlast.py:417-452): rows sorted by (r, q, ss, qs).  iden is in/out:
 * a dropped row gets iden = -1.
 *
 * pep_linear_merge (flag -m, RunBlast.linearMerge + _linearMerge uberBlast.py:100-218, 453-460): rows sorted by
 * (q, r, ss, qs).  Per query (maximal run of equal q) it reports
 *   keep_seq[query_off[k] .. query_off[k+1])  row indices that survive, in the insertion order of the reference's `used`
 *                                             dictionary (duplicates possible); query_ascending[k] = 1 when nothing was chained
 *                                             and every row is kept in order.  The reference builds a Python set from this
 *                                             sequence and emits rows in the set's iteration order; the caller does the same.
 *   per row i: grp_score/grp_iden/grp_span[i] and grp_ids[grp_ids_off[i] .. grp_ids_off[i+1]) = column 16 of the reference
 *                                             ([score, identity, span, row ids...]); grp_span = -1 for rows without a group.
 * n_keep / n_ids return the needed sizes; when they exceed keep_cap / ids_cap nothing is written and the caller calls again. */
int pep_ovl_filter(uint64_t n, const int64_t *q, const int64_t *r, const int64_t *qs, const int64_t *qe, const int64_t *ss, const int64_t *se,
                   const double *score, double *iden, double coverage, double delta);
/* pep_known_order (host, no context; ABI 15): compare_prediction (PEPPAN.py:869-901) over the columns of one genome's hit table.  For every hit the largest fraction of an
 * original gene of the same contig that it covers in frame and on the same strand (0.1 when there is none): the genes of contig c (row code ri) are
 * g1 / g2 / g_plus [g_off[c], g_off[c + 1]) - start, end, strand '+' - in the store's order; g_sorted[c] != 0: in start order (every gene between the first whose
 * running maximum of ends reaches the hit and the last that starts at or before its end is judged), else the reference's forward-only pointer sweep.  The table is
 * walked by (contig code, lower reference coordinate) and returned in the order (query code, contig code, score), each stable: order[k] = the row that comes k-th,
 * known[k] = its value. */
int pep_known_order(uint64_t n, const int64_t *ri, const int64_t *r_code, const int64_t *q_code, const int64_t *ss, const int64_t *se, const int64_t *qs,
                    const int64_t *qe, const int64_t *ql, const double *score, uint64_t n_contigs, const uint64_t *g_off, const int64_t *g1, const int64_t *g2,
                    const uint8_t *g_plus, const uint8_t *g_sorted, int64_t *order, double *known);
int pep_linear_merge(uint64_t n, const int64_t *q, const int64_t *r, const double *iden, const int64_t *qs, const int64_t *qe, const int64_t *ss,
                     const int64_t *se, const double *score, const int64_t *ql, const int64_t *sl, const int64_t *rid, double gap_dist, double len_diff,
                     int64_t *keep_seq, uint64_t keep_cap, uint64_t *n_keep, uint64_t *query_off, uint8_t *query_ascending, uint64_t *n_query,
                     double *grp_score, double *grp_iden, int64_t *grp_span, uint64_t *grp_ids_off, int64_t *grp_ids, uint64_t ids_cap, uint64_t *n_ids);

/* Members of the genome-mapping stores (PEPPAN.py:950-966: 1000 groups per member of <prefix>.mat.npz / <prefix>.seq.npz), emitted as
 * the pickle stream numpy writes for an object array, straight from numeric columns - no Python object is made for a stored row.
 * Host C++, no context.
 *   pep_store_mat_member: the stream of ndarray(object)[n_groups] whose element g is ndarray(object)[row_off[g+1] - row_off[g], 16]
 *     of the hit rows [row_off[g], row_off[g+1]) of `cols`: columns 0-15 of the reference's table with q / r
 *     as integers (PEPPAN's encoded names), the CIGAR as text ("150M3D150M", uberBlast.py:480), score as int when score_is_int.
 *   pep_store_seq_member: ndarray(object)[n_groups] of ndarray(uint8) = packed[pack_off[g] .. pack_off[g+1]) (the base-5 packed
 *     alleles, PEPPAN.py:846-848).
 * recon_module: the module that holds numpy's `_reconstruct` ("numpy._core.multiarray" / "numpy.core.multiarray").
 * Both return the length of the stream; when it exceeds `cap` the buffer holds nothing usable and the caller calls again with a
 * larger one (cap = 0 measures).  Negative: PEP_ERR_ARG. */
typedef struct pep_mat_cols {
    const int64_t *q, *r;
    const double *iden;
    const int64_t *aln, *mis, *gap, *qs, *qe, *ss, *se;
    const double *evalue, *score;
    const int64_t *ql, *sl;
    const uint32_t *arena;          /* CIGAR runs len << 2 | op (0 M, 1 I, 2 D), nucleotide units */
    const int64_t *c_off, *c_runs, *rid;
    int32_t score_is_int, reserved;
} pep_mat_cols;
int64_t pep_store_mat_member(const pep_mat_cols *cols, const int64_t *row_off, int64_t n_groups, const char *recon_module, uint8_t *out, int64_t cap);
int64_t pep_store_seq_member(const uint8_t *packed, const int64_t *pack_off, int64_t n_groups, const char *recon_module, uint8_t *out, int64_t cap);

/* The gene table store <prefix>.tab.npz (PEPPAN.py:972-975 through MapBsn.update, PEPPAN.py:91-113) written into an EMPTY archive: the
 * complete zip entries - local file header + payload - of all members back to back in `out`, made by up to `threads` host threads.
 * Member m is the .npy file of int64[off[m+1] - off[m], n_cols] = rows [off[m], off[m+1]) of the row-major table - of the table taken in the
 * order `order` when that is not NULL (row i of the sorted table = row order[i] of `rows`: the gather happens here, by the threads) -, named by the decimal
 * key[m]; stored below 4 KiB, raw deflate (level 1) from there on - what MapBsn writes member by member.  crc / csize / usize / at[m]
 * (offset of the entry in `out`) are what the archive's central directory needs; the caller appends `out` to the archive and lists
 * the entries.  Returns the length of `out`'s content; when it exceeds `cap` nothing usable was written and the caller calls again
 * with that much room.  Negative: PEP_ERR_ARG. */
int64_t pep_store_tab_members(const int64_t *rows, int64_t n_cols, const int64_t *order, const int64_t *off, const int64_t *key, int64_t n_members, uint32_t dos_time, uint32_t dos_date,
                              int32_t threads, uint8_t *out, int64_t cap, uint32_t *crc, int64_t *csize, int64_t *usize, int64_t *at);

/* The same members as a COMPLETE archive: entries, central directory, end record - what <prefix>.tab.npz is when it is written once (no zipfile
 * object is needed for a store that is then closed).  Plain zip: PEP_ERR_LIMIT from 65 535 members or 4 GiB on (the caller then writes member-wise).
 * Returns the archive's length; when it exceeds `cap` nothing usable was written. */
int64_t pep_store_tab_archive(const int64_t *rows, int64_t n_cols, const int64_t *order, const int64_t *off, const int64_t *key, int64_t n_members, uint32_t dos_time, uint32_t dos_date,
                              int32_t threads, uint8_t *out, int64_t cap);

/* ---- RunBlast.run's numeric chain between a search and the caller, host C++ (no GPU work, no context).  The columns of the reference's hit table
 * ("blastab": SURVEY.md section 8) as flat arrays - every column int64 or double, one CIGAR arena of runs len << 2 | op in nucleotide units. */
typedef struct pep_hit_cols {
    int64_t *qi, *ri;               /* indices into the caller's query / reference name tables (columns 0, 1) */
    double *iden;                   /* column 2 */
    int64_t *aln, *mis, *gap, *qs, *qe, *ss, *se;    /* columns 3 - 9 */
    double *evalue, *score;         /* columns 10, 11 */
    int64_t *ql, *sl;               /* columns 12, 13 */
    int64_t *c_off, *c_runs;        /* column 14: the row's runs in the arena */
    int64_t *rid;                   /* column 15 (may be NULL where a function only fills it with -1) */
} pep_hit_cols;

/* Hit records of a search -> the rows the reference's parsers keep, as columns (room for n rows each); returns the number of rows, in hit order.
 * tool 0, the translated search: parseDiamond's algebra (uberBlast.py:25-58) - names q:frame / r:frame:offset from q_meta / t_meta, CIGAR x 3
 *   (arena_out takes all n_cigar runs, rewritten in nucleotides), identity 1 - round(3 NM / length, 3), coordinates on either strand of the
 *   reference, the cuts qm * 3 >= min_cov, qm * 3 / ql >= min_ratio, identity >= min_id.  t_seq .. evalue unused (NULL).
 * tool 1, the nucleotide search: parseBlast's columns (uberBlast.py:275-290): t_seq / t_rev = reference sequence and strand of every target, identity
 *   with blastn's three printed decimals, mismatches = length - identities - gap columns, `evalue[i]` per HIT as the caller computed it, the cuts
 *   identity >= min_id, aligned query span >= min_cov and >= min_ratio * ql; win_off / home_lo / home_hi (NULL or per target): targets that are
 *   windows of a long strand - a hit is shifted to strand coordinates and kept by the window whose home stretch holds its midpoint.  q_meta / t_meta unused.
 * q_len / r_len: nucleotide lengths per sequence.  Negative: PEP_ERR_ARG.
 * nt_match (NULL, or per HIT the count pep_result_nt_match hands out): the rows come out rescored - RunBlast.reScore's mode 1 (uberBlast.py:397-415,
 *   cigar2score :226-249) applied to every kept row: identity = matches / (matches + mismatches + gap bases - gap bases of gaps longer than 3) and
 *   score = 3 matches - mismatches - 5 gaps - gap bases in float64, rounded to three decimals; the cuts still look at the tool's own identity. */
int64_t pep_table_from_hits(int32_t tool, uint64_t n, const pep_hit *hits, const uint32_t *cigar, uint64_t n_cigar, const pep_query_meta *q_meta,
                            const pep_target_meta *t_meta, const int64_t *q_len, const int64_t *r_len, const int64_t *t_seq, const uint8_t *t_rev,
                            const int64_t *win_off, const int64_t *home_lo, const int64_t *home_hi, const double *evalue, double min_id, double min_cov,
                            double min_ratio, pep_hit_cols *out, uint32_t *arena_out, const uint32_t *nt_match);

/* RunBlast.fixEnd (uberBlast.py:462-480) over all rows, in place: an alignment is stretched over an unaligned query head of at most se_lim / tail of
 * at most ee_lim bases as far as the reference sequence allows, its first / last CIGAR run growing by the same amount.  The rows' runs are copied
 * into arena_out (sum of c_runs words; rows may share runs in arena_in) and c_off is rewritten.  Returns the number of rows that changed;
 * PEP_ERR_ARG also for a row without runs that would have to be extended (the reference fails there). */
int64_t pep_cols_fix_end(uint64_t n, pep_hit_cols *cols, const uint32_t *arena_in, uint64_t n_arena_in, uint32_t *arena_out, double se_lim, double ee_lim);

/* The sort that ends RunBlast.run (uberBlast.py:375: DataFrame.sort_values([0, 1, 11])): order[k] = the row that comes k-th by (q_code, r_code,
 * score), stable; the codes are non-negative integers that sort like the names of columns 0 and 1 do (the caller ranks the name tables once). */
int pep_cols_order(uint64_t n, const int64_t *q_code, const int64_t *r_code, const double *score, int64_t *order);

/* order = numpy.lexsort(keys) for n_keys int64 key columns of n rows: stable, the LAST key the primary one - the sorts in front of RunBlast.ovlFilter (uberBlast.py:421:
 * by reference, query, start, query start) and _linearMerge (:455) of every genome's table in the mapping path.  Radix passes over (key - its minimum); PEP_ERR_LIMIT
 * when a key's range needs more than 44 bits (the caller sorts with numpy then). */
int pep_lex_order(uint64_t n, int32_t n_keys, const int64_t *const *keys, int64_t *order);

/* dst[c][k] = src[c][idx[k]] for n_cols columns of 8-byte elements (n_src rows each): the rows `idx` of a whole table in one call */
int pep_cols_gather(int32_t n_cols, const void *const *src, void *const *dst, const int64_t *idx, uint64_t n_idx, uint64_t n_src);

/* Host threads: the passes above (pep_table_from_hits, pep_cols_fix_end, pep_cols_gather) split tables of 16 384 rows and more over up to `n` threads that
 * live for the call (1 .. 16).  Default: the environment's PEPPAN_HOST_THREADS, else a quarter of the hardware threads, four at most; 0 returns to that.
 * Returns the value in force before.  The results do not depend on it. */
int pep_set_host_threads(int n);

/* A raw DEFLATE stream (RFC 1951; what a zip member of method 8 holds) of `src` made of dynamic-Huffman blocks with literals only - entropy
 * coding without a match search, for the members of <prefix>.seq.npz (packed alleles: nothing to match).  Host C++, no context, any inflate
 * reads it.  Returns the stream's length; when it exceeds `cap` nothing usable was written (n + n / 64 + 512 always suffices).  Negative: PEP_ERR_ARG. */
int64_t pep_deflate_literals(const uint8_t *src, int64_t n, uint8_t *out, int64_t cap);

/* A raw DEFLATE stream of `src` with matches found by ONE probe of a 4-byte hash per position (greedy; the matcher of the fastest levels of the
 * modern deflate libraries) in dynamic-Huffman blocks of 64 KiB of input - for the members of <prefix>.mat.npz (PEPPAN.py:959-966; the reference deflates
 * them at zlib's default level inside zipfile): about the size of zlib's level 1 at several times its rate.  Host C++, no context, any inflate reads
 * it.  Returns the stream's length; when it exceeds `cap` nothing usable was written (n + n / 8 + 1024 always suffices).  Negative: PEP_ERR_ARG. */
int64_t pep_deflate_fast(const uint8_t *src, int64_t n, uint8_t *out, int64_t cap);

/* CRC-32 of the zip format (what zlib.crc32 returns) of src[0 .. n) continued from `crc` (0 to start): by carry-less multiplication where the CPU has the
 * instruction (an order of magnitude above zlib's table walk), zlib's otherwise.  Every member MapBsn appends carries one (zipfile computes it inside
 * ZipFile.writestr, PEPPAN.py:81-85 through numpy.savez). */
uint32_t pep_crc32(const uint8_t *src, int64_t n, uint32_t crc);

/* A store member ready for its archive in one call: the raw DEFLATE stream of `src` by coder 0 (pep_deflate_literals) or 1 (pep_deflate_fast) and, in *crc,
 * the CRC-32 of `src`.  Returns the stream's length; beyond `cap` nothing usable was written.  Negative: PEP_ERR_ARG. */
int64_t pep_pack_member(const uint8_t *src, int64_t n, int32_t coder, uint8_t *out, int64_t cap, uint32_t *crc);
/* np.argsort(v.astype(object)) for float64 v without NaN (host, no context): the order numpy's generic index quicksort leaves an object column of
 * Python floats in, ties included - the order of equal scores in the reference's .tab store (PEPPAN.py:957-960 sorts an object array's score column).
 * PEP_ERR_LIMIT when the sort's depth limit is reached (numpy switches to heapsort there: the caller asks numpy itself). */
int pep_argsort_object_order(const double *v, int64_t n, int64_t *order);

#ifdef __cplusplus
}
#endif
#endif
