"""ctypes binding of libpeppan_hip.so (include/peppan_hip.h).  No torch, no CPU fallback:
if the HIP library is missing or no MI355X is visible every entry point raises."""
import ctypes as C
import os
import threading
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libpeppan_hip.so')

ABI_VERSION = 20
MAX_SEQ_LEN = (1 << 23) - 256          # PEP_MAX_SEQ_LEN: longest single sequence of a packed set
ALLELE_DIFF_MAX_BYTES = 1 << 31        # PEP_ALLELE_DIFF_MAX_BYTES: output (and bit planes) of one pep_allele_diff call

# The C signature of every function of include/peppan_hip.h, stated once: name -> (return type, parameter types in the header's order).  load_library() hands them
# to ctypes, which then converts plain Python ints and floats to the parameter's width, returns the full width, and refuses an argument of the wrong kind or a call
# with too few before the library is entered; tests/test_abi.py reads the header's prototypes and holds this table to them.
I, I32, U32, I64, U64, F64 = C.c_int, C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_double
P, S = C.c_void_p, C.c_char_p            # P: every pointer, handle and array parameter (the writable char *msg too); S: a const char * string
SIGNATURES = {
    'pep_version': (I,),
    'pep_device_count': (I,),
    'pep_ctx_create': (I, I, P),
    'pep_ctx_destroy': (None, P),
    'pep_live_resources': (I, P, P, P),
    'pep_last_error': (S, P),
    'pep_default_params': (None, P),
    'pep_set_sensitivity': (I, P, I),
    'pep_min_score': (I32, U32, F64, F64),
    'pep_min_score_ka': (I32, U32, F64, F64, F64, F64),
    'pep_set_query_nt': (I, P, P, P, U32, I),
    'pep_set_ref_nt': (I, P, P, P, U32, I, I),
    'pep_set_query_aa': (I, P, P, P, U32),
    'pep_set_ref_aa': (I, P, P, P, U32),
    'pep_translate': (I, P, I),
    'pep_invalidate_translation': (I, P),
    'pep_use_nt_as_residues': (I, P, I),
    'pep_query_count': (I, P, P, P),
    'pep_target_count': (I, P, P, P),
    'pep_get_query_meta': (I, P, P, U32),
    'pep_get_target_meta': (I, P, P, U32),
    'pep_get_query_aa': (I, P, P, U64, P),
    'pep_get_target_aa': (I, P, P, U64, P),
    'pep_set_target_groups': (I, P, P, U32),
    'pep_set_result_mode': (I, P, I),
    'pep_set_timing': (I, P, I),
    'pep_call_times': (I, P, I, P),
    'pep_search': (I, P, P, P),
    'pep_result_size': (I, P, P, P),
    'pep_result_copy': (I, P, P, P),
    'pep_result_data': (I, P, P, P),
    'pep_result_device': (I, P, P, P),
    'pep_result_stats': (I, P, P),
    'pep_result_free': (None, P),
    'pep_merge_hits': (I, U64, P, P, U64, I32, I32, P, P, P, P),
    'pep_rescore_nt': (I, P, U64, P, P, U64, P),
    'pep_rescore_codons': (I, P, U64, P, P, U64, I32, P, P, P),
    'pep_rescore_codons_check': (I, U64, P, P, U64, I32, P, P, P, U64, P, U64, P, U64),
    'pep_set_nt_match': (I, P, I),
    'pep_result_nt_match': (I, P, P),
    'pep_components': (I, P, U32, U64, P, P, P),
    'pep_components_of_hits': (I, P, U32, U64, P, U32, P, U64, P),
    'pep_set_grouping': (I, P, U32, U32, P, U64),
    'pep_result_labels': (I, P, P, U32),
    'pep_components_of_result': (I, P, P, U32, U32, P, U64, P),
    'pep_linclust': (I, P, P, P, U32, I, I, I, F64, F64, P, P),
    'pep_overlaps': (I, P, U64, P, P, P, P, F64, F64, P, U64, P),
    'pep_alleles': (I, P, P, P, U32, U64, P, P, U64, U32, P, P, I, P, P, P, U64),
    'pep_allele_diff': (I, P, P, P, P, U64, U32, P, P, P, P, P, U64),
    'pep_group_verdicts': (I, P, P, P, P, U64, U32, P, P, P, P, P, P, U64, P, F64, P, P),
    'pep_group_verdicts_check': (I, P, P, P, U64, U32, P, P, P, P, P, P, U64, P, F64, P, U64),
    'pep_verdict_detail_size': (I, P, U32, P),
    'pep_verdict_detail_copy': (I, P, U32, P, P),
    'pep_verdict_result_free': (None, P),
    'pep_gene_ingroups': (I, P, P, P, P, U64, U32, P, P, P, U64, P, F64, F64, P, P),
    'pep_gene_ingroups_check': (I, P, P, P, U64, U32, P, P, P, U64, P, F64, F64, P, U64),
    'pep_synteny_pairs': (I, P, U32, P, P, U64, P, P, U64, I32, P, P, P, P),
    'pep_synteny_pairs_copy': (I, P, P, U64, P, U64),
    'pep_synteny_pairs_check': (I, U32, P, P, U64, P, P, U64, I32, P, U64),
    'pep_synteny_walk': (I, U32, P, P, P, P, P, P, P, P, P, P, P, U64),
    'pep_gene_structure': (I, P, P, P, U32, U32, P, P, P, P, P, P, P, I, P, P, P, P),
    'pep_gene_structure_check': (I, P, U32, U32, P, P, P, P, P, P, P, P, U64),
    'pep_rarefaction_curves': (I, P, P, U32, U64, P, U32, P),
    'pep_rarefaction_curves_check': (I, P, U32, U64, P, U32, P, U64),
    'pep_profile_pairs': (I, P, P, U32, U64, P, P),
    'pep_profile_pairs_check': (I, U32, U64, P, U64),
    'pep_kimura_pairs': (I, P, P, P, P, U64, U32, P, P, P, P, U64),
    'pep_nj_trees': (I, P, P, P, P, U32, P, P, P),
    'pep_nj_trees_check': (I, P, U32, P, P, P, U64),
    'pep_global_diff_walk': (I, P, U64, P, U64, P, P, U64, P, P, U64),
    'pep_global_diff_walk_size': (I, P, P, P, P),
    'pep_global_diff_walk_copy': (I, P, P, P, P),
    'pep_global_diff_walk_free': (None, P),
    'pep_global_diff': (I, P, P, U64, P, U64, U32, P, U64, P),
    'pep_global_diff_copy': (I, P, U64, P, P, P, P, P),
    'pep_global_diff_check': (I, P, U64, P, U64, U32, U64, P, U64),
    'pep_cds_genes_check': (I, P, U32, U32, P, P, P, P, U32, P, U64),
    'pep_cds_genes': (I, P, P, P, U32, U32, P, P, P, P, U32, U32, I, P, P),
    'pep_out_alleles_check': (I, P, U32, U32, P, U32, P, P, U32, P, U64),
    'pep_out_alleles': (I, P, P, P, U32, U32, P, U32, P, P, I, U32, P, P, P, P),
    'pep_tree_cut': (I, P, P, U32, P, P, P, P, P, P, P, P, P, P, U32, P, P, P, P),
    'pep_tree_cut_check': (I, P, U32, P, P, P, P, P, U32, P, U64),
    'pep_batch_screen': (I, P, U32, P, P, P, P, U64, F64, P, P, P, P),
    'pep_batch_screen_check': (I, U32, P, P, P, U64, P, U64),
    'pep_batch_unsure_walk': (I, U32, P, P, P, P, P, U64, P, P, U64),
    'pep_batch_unsure_walk_check': (I, U32, P, P, P, P, P, U64, P, U64),
    'pep_batch_prune': (I, P, U32, U32, P, P, P, P, P, P, P, P, U64, F64, F64, U32, P, P, P, P, P),
    'pep_batch_prune_check': (I, U32, U32, P, P, P, P, P, P, P, P, U64, U32, P, U64),
    'pep_similar_classify': (I, U64, P, P, P, P, P, P, P, P, P, P, P, F64, F64, P, P, P),
    'pep_similar_scan': (I, U64, P, P, P, P, P, U64, P, P, P, P, P, P, P, P, P, P),
    'pep_pair_support': (I, P, U64, P, P, U64, U64, P, P, P, P, P),
    'pep_similar_resolve': (I, U64, P, P, P, P, P, P),
    'pep_fasta_keep': (I, S, P, U64, P, P),
    'pep_fasta_scan': (I, P, U64, P, P, P, U64, P, P),
    'pep_fasta_records': (I, P, U64, P, P, P, P, P, U64, P, P),
    'pep_sha1': (I, P, P, P, U32, P),
    'pep_dedup': (I, P, U32, P, P, P),
    'pep_ovl_filter': (I, U64, P, P, P, P, P, P, P, P, F64, F64),
    'pep_known_order': (I, U64, P, P, P, P, P, P, P, P, P, U64, P, P, P, P, P, P, P),
    'pep_linear_merge': (I, U64, P, P, P, P, P, P, P, P, P, P, P, F64, F64, P, U64, P, P, P, P, P, P, P, P, P, U64, P),
    'pep_store_mat_member': (I64, P, P, I64, S, P, I64),
    'pep_store_seq_member': (I64, P, P, I64, S, P, I64),
    'pep_store_tab_members': (I64, P, I64, P, P, P, I64, U32, U32, I32, P, I64, P, P, P, P),
    'pep_store_tab_archive': (I64, P, I64, P, P, P, I64, U32, U32, I32, P, I64),
    'pep_table_from_hits': (I64, I32, U64, P, P, U64, P, P, P, P, P, P, P, P, P, P, F64, F64, F64, P, P, P),
    'pep_cols_fix_end': (I64, U64, P, P, U64, P, F64, F64),
    'pep_cols_order': (I, U64, P, P, P, P),
    'pep_lex_order': (I, U64, I32, P, P),
    'pep_cols_gather': (I, I32, P, P, P, U64, U64),
    'pep_set_host_threads': (I, I),
    'pep_deflate_literals': (I64, P, I64, P, I64),
    'pep_deflate_fast': (I64, P, I64, P, I64),
    'pep_crc32': (U32, P, I64, U32),
    'pep_pack_member': (I64, P, I64, I32, P, I64, P),
    'pep_argsort_object_order': (I, P, I64, P),
}
EXPORTS = list(SIGNATURES)

# limits and codes of the header's K21 - K26 sections; the host test of each kernel holds them to its #defines
PREP_NJ, PREP_SBH = 0, 1                 # PEP_PREP_NJ, PEP_PREP_SBH: the mode of pep_batch_prune
PREP_AUTO, PREP_LDS, PREP_WS = 0, 1, 2   # PEP_PREP_AUTO ..: its path
PREP_LDS_ROWS = 4096                     # PEP_PREP_LDS_ROWS: rows of a gene whose working arrays stay in LDS
PREP_MAX_ROWS = 65536                    # PEP_PREP_MAX_ROWS: rows of one gene
PREP_MAX_CFL_BYTES = 1 << 31             # PEP_PREP_MAX_CFL_BYTES: conflict values of one call
PREP_MAX_LOCI = 1 << 40                  # PEP_PREP_MAX_LOCI
CUT_AUTO, CUT_BLOCK, CUT_CHAIN = 0, 1, 2   # PEP_CUT_AUTO ..: the path of pep_tree_cut
CUT_ROUND = 8                            # PEP_CUT_ROUND: iterations of a launch chain between two reads of its `done` flag
CUT_DEFAULT_CAP = 3000                   # PEP_CUT_DEFAULT_CAP: the reference's iterations per component
OUTA_COLS, OUTA_PLAN_COLS = 12, 6        # PEP_OUTA_COLS, PEP_OUTA_PLAN_COLS: int32 values of a row record and of a plan record
OUTA_GENE, OUTA_CONTIG, OUTA_FLAGS, OUTA_S, OUTA_E, OUTA_PART, OUTA_QS, OUTA_QE, OUTA_REFLEN, OUTA_CLEN, OUTA_VARY, OUTA_SVMIN = range(12)     # PEP_OUTA_GENE ..
OUTA_MISC, OUTA_NONAME, OUTA_SECONDARY, OUTA_MINUS = 1, 2, 4, 8                  # the bits of PEP_OUTA_FLAGS
OUTA_SKIPPED, OUTA_FRAGMENT, OUTA_INTACT, OUTA_STRUCTVAR = range(4)              # the classes of a plan record
OUTA_BATCH = 10000                       # PEP_OUTA_BATCH: rows between two write-backs of the reference
OUTA_MAX_CONTIG = 1 << 31                # PEP_OUTA_MAX_CONTIG
OUTA_MAX_ITEMS = 1 << 30                 # PEP_OUTA_MAX_ITEMS: rows and genes of one call
ERR_ALLELE_CLASS = -24                   # PEP_ERR_ALLELE_CLASS: two rows of one digest class hold different bytes
CDS_MAX_WINDOW = 1 << 31                 # PEP_CDS_MAX_WINDOW: a window of pep_cds_genes holds fewer bytes than this
CDS_MAX_ITEMS = 1 << 32                  # PEP_CDS_MAX_ITEMS: fewer CDS than this in one call
CDS_ALLOW = {'s': 1, 'i': 2, 'f': 4, 'e': 8}     # PEP_CDS_ALLOW_*: the mask bit of every letter of incompleteCDS
GDIFF_MAX_GENOMES = 16384                # PEP_GDIFF_MAX_GENOMES: distinct genomes of one pep_global_diff call
GDIFF_MAX_ITEMS = 1 << 32                # PEP_GDIFF_MAX_ITEMS: list-pair members of one call
GDIFF_TABLE = 10050                      # PEP_GDIFF_TABLE: entries of the logarithm table, value codes 0 .. 10049
GDIFF_CHUNK_ITEMS = 1 << 24              # PEP_GDIFF_CHUNK_ITEMS: items of one chunk when chunk_items is 0
GDIFF_MAX_BYTES = 1 << 34                # PEP_GDIFF_MAX_BYTES: device workspace of one call
NJ_BLOCK_LEAVES = 256                    # PEP_NJ_BLOCK_LEAVES: trees up to this size are joined by one workgroup, larger ones by a chain of launches
NJ_MAX_LEAVES = 8192                     # PEP_NJ_MAX_LEAVES: leaves of one tree
NJ_MAX_BYTES = 1 << 30                   # PEP_NJ_MAX_BYTES: distance matrices of one pep_nj_trees call, pair counts of one pep_kimura_pairs call

# limits and codes of the header's K18, K19 and K20 sections; the host test of each kernel holds them to its #defines
SYNTENY_MAX_PAIRS = 1 << 27              # PEP_SYNTENY_MAX_PAIRS: pairs of one pep_synteny_pairs call
SYNTENY_MAX_COUNTERS = 1 << 26           # PEP_SYNTENY_MAX_COUNTERS: rank counters of one call, n * (6 * longest list + 14) per group of two members and more
GENESTRUCT_MAX_WINDOW = 1 << 31          # PEP_GENESTRUCT_MAX_WINDOW: a window holds fewer nucleotides than this
GENESTRUCT_NO_STOP = 0xFFFFFFFF          # PEP_GENESTRUCT_NO_STOP: stop_aa of a frame without a stop codon
GENESTRUCT_KINDS = ('CDS', 'nostart', 'nostop', 'premature_stop')      # PEP_GENESTRUCT_CDS .. PEP_GENESTRUCT_PREMATURE
PARSER_MAX_GENES = 1 << 31               # PEP_PARSER_MAX_GENES: a presence matrix or a profile holds fewer genes than this
PARSER_MAX_CURVE_POINTS = 1 << 28        # PEP_PARSER_MAX_CURVE_POINTS: n_genomes * n_iter of one pep_rarefaction_curves call stays below this
PARSER_MAX_PROFILES = 16384              # PEP_PARSER_MAX_PROFILES: profiles of one pep_profile_pairs call


class PepError(RuntimeError):
    pass


class SearchParams(C.Structure):
    _fields_ = [('gap_open', C.c_int32), ('gap_ext', C.c_int32), ('n_shapes', C.c_int32), ('base', C.c_int32),
                ('weight', C.c_int32 * 4), ('offs', (C.c_int32 * 32) * 4), ('reduce', C.c_uint8 * 32),
                ('sub', C.c_int8 * 1024), ('min_id_pct', C.c_double), ('min_qcov_pct', C.c_double),
                ('top_k', C.c_int32), ('n_splits', C.c_int32), ('dbsize', C.c_double), ('max_evalue', C.c_double),
                ('use_lds', C.c_int32), ('ungapped_min', C.c_int32), ('xdrop', C.c_int32), ('ext_right', C.c_int32),
                ('ext_left', C.c_int32), ('reserved', C.c_int32 * 3), ('ka_lambda', C.c_double), ('ka_k', C.c_double), ('hsp_mode', C.c_int32), ('t_index_base', C.c_int32), ('stage1_min', C.c_int32), ('reserved2', C.c_int32)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ('query_residues', 'target_residues', 'query_seeds', 'target_seeds', 'seed_hits',
                                           'seed_hits_passed', 'candidates', 'pairs', 'tracebacks', 'hits', 'cells', 'cells_swept', 'dir_bytes',
                                           'sw_launches', 'cells_trace', 'cells_swept_trace', 'tracebacks_gapless', 'candidates_settled', 'cells_settled')] + \
               [(n, C.c_double) for n in ('ms_seed', 'ms_sw', 'ms_trace', 'ms_total', 'ms_k1', 'ms_sw_trace', 'ms_seed_match', 'ms_reserved0', 'ms_reserved1', 'ms_reserved2')]


HIT_DTYPE = np.dtype([('q', '<u4'), ('t', '<u4'), ('q_start', '<u4'), ('q_end', '<u4'), ('t_start', '<u4'), ('t_end', '<u4'),
                      ('score', '<i4'), ('nm', '<u4'), ('n_ident', '<u4'), ('aln_len', '<u4'), ('cigar_runs', '<u4'),
                      ('bin', '<i4'), ('cigar_off', '<u8'), ('cells', '<u8')])
QUERY_META_DTYPE = np.dtype([('seq', '<u4'), ('frame', '<u4'), ('aa_len', '<u4'), ('nt_len', '<u4')])
TARGET_META_DTYPE = np.dtype([('seq', '<u4'), ('frame', '<u4'), ('chunk_off', '<u4'), ('aa_len', '<u4')])
NT_HIT_DTYPE = np.dtype([('q', '<u4'), ('r', '<u4'), ('qs', '<u4'), ('qe', '<u4'), ('rs', '<u4'), ('re', '<u4'),
                         ('cigar_runs', '<u4'), ('pad', '<u4'), ('cigar_off', '<u8')])

LOCUS_DTYPE = np.dtype([('contig', '<u4'), ('q_start', '<u4'), ('rs', '<u4'), ('re', '<u4'), ('cigar_runs', '<u4'), ('group', '<u4'),
                        ('cigar_off', '<u8')])

SUPPORT_ROW_DTYPE = np.dtype([('q_start', '<u4'), ('r_start', '<u4'), ('cigar_runs', '<u4'), ('pad', '<u4'), ('cigar_off', '<u8'), ('identity', '<f8')])
SUPPORT_NONE = -2 ** 31
ROW_ORDINARY, ROW_CONFLICT, ROW_ABSORB_QUERY, ROW_ABSORB_REF = 0, 1, 2, 3
EVENT_CONFLICT, EVENT_SUPPORT = 0, 1


INGROUP_MAX_IDEN = (1 << 31) - 1         # column 4 of a gene's table travels as int32


CALL_MS = 8                              # PEP_CALL_MS: kernel times of one record


class CallTimes(C.Structure):
    """struct pep_call_times: what pep_call_times reports of the newest call of one of K15 - K26"""
    _fields_ = [('ms', C.c_double * CALL_MS), ('bytes_to_device', C.c_uint64), ('bytes_to_host', C.c_uint64)]


(CALL_ALLELE_DIFF, CALL_GROUP_VERDICTS, CALL_GENE_INGROUPS, CALL_SYNTENY_PAIRS, CALL_GENE_STRUCTURE, CALL_PARSER, CALL_KIMURA_PAIRS, CALL_NJ_TREES, CALL_GLOBAL_DIFF,
 CALL_CDS_GENES, CALL_OUT_ALLELES, CALL_TREE_CUT, CALL_BATCH_SCREEN, CALL_BATCH_PRUNE, CALL_COUNT) = range(15)      # PEP_CALL_*


class SupportLimits(C.Structure):
    _fields_ = [('match_len', C.c_double * 3), ('match_prop', C.c_double * 3), ('identity_x1e4', C.c_double), ('any_frame', C.c_int32), ('pad', C.c_int32)]


def support_limits(params):
    """the thresholds of get_similar (PEPPAN.py:205-216) from PEPPAN's parameter dictionary"""
    lim = SupportLimits()
    for k, (l, p) in enumerate((('match_len', 'match_prop'), ('match_len1', 'match_prop1'), ('match_len2', 'match_prop2'))):
        lim.match_len[k], lim.match_prop[k] = float(params[l]), float(params[p])
    lim.identity_x1e4 = params['match_identity'] * 10000
    lim.any_frame = 1 if 'f' in params['incompleteCDS'] else 0
    return lim


_lib = None


def _tune_malloc():
    """glibc hands every block of 128 KiB and more straight to mmap and back: the host chain's columns - a few MB per table, a dozen tables per call - arrive as fresh
    zero pages every time, and the page faults are a sixth of the hot call's wall time (17.7 -> 14.9 ms with object rows, 30.5 -> 28.4 ms for get_similar_pairs on
    one box).  Blocks up to 32 MiB (the largest threshold glibc accepts) are therefore kept in the heap and reused; at most 1 GiB of free heap top is held back.
    A process-wide setting, made when the library is first loaded; PEPPAN_MALLOC_TUNE=0 leaves the allocator alone."""
    if os.environ.get('PEPPAN_MALLOC_TUNE', '1') == '0':
        return
    try:
        libc = C.CDLL(None)
        libc.mallopt.argtypes, libc.mallopt.restype = [C.c_int, C.c_int], C.c_int
        libc.mallopt(-3, 32 << 20)               # M_MMAP_THRESHOLD
        libc.mallopt(-1, 1 << 30)                # M_TRIM_THRESHOLD
    except (OSError, AttributeError):
        pass                                     # (not glibc: nothing to tune)


def load_library():
    """dlopen the in-tree library; raises PepError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    _tune_malloc()
    if not os.path.exists(LIB_PATH):
        raise PepError('libpeppan_hip.so is not built (run `python -c "import __graft_entry__ as g; g.build()"` '
                       'or `make -C peppan_amd/csrc`); there is no CPU fallback')
    if 'PEPPAN_HOST_THREADS' not in os.environ:
        # threads a pass of the host chain (csrc/hostchain.hip) may use on a large table: a quarter of the CPUs the container grants, four at most
        from .configure import effective_cpus
        os.environ['PEPPAN_HOST_THREADS'] = str(max(1, min(4, effective_cpus() // 4)))
    lib = C.CDLL(LIB_PATH)
    for name, (restype, *argtypes) in SIGNATURES.items():
        if not hasattr(lib, name):
            raise PepError('libpeppan_hip.so does not export ' + name)
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.pep_version() != ABI_VERSION:
        raise PepError('libpeppan_hip.so ABI version mismatch')
    _lib = lib
    return lib


def live_resources():
    """pep_live_resources: (bytes of device buffers, bytes of pinned host buffers, HIP events) the library holds in this process, over all contexts"""
    dev, pin, ev = C.c_uint64(), C.c_uint64(), C.c_uint32()
    if load_library().pep_live_resources(C.byref(dev), C.byref(pin), C.byref(ev)) != 0:
        raise PepError('pep_live_resources failed')
    return dev.value, pin.value, ev.value


DEFAULT_SHAPES = ('111101110111', '111011010010111')          # DIAMOND's two default-sensitivity shapes (weight 10)
SENSITIVE_SHAPES = ('110010011111011', '10111110011011')      # two more weight-10 shapes for the sensitive mode (see default_params)


def set_shapes(p, shapes):
    """seed shapes as '1101...' strings -> the weight / offsets fields of a parameter block (native or oracle)"""
    p.n_shapes = len(shapes)
    for s, sh in enumerate(shapes):
        ones = [k for k, ch in enumerate(sh) if ch == '1']
        p.weight[s] = len(ones)
        for i in range(32):
            p.offs[s][i] = ones[i] if i < len(ones) else 0
    for s in range(len(shapes), 4):
        p.weight[s] = 0


def default_params(min_id_pct=0., min_qcov_pct=0., top_k=10, n_splits=5, dbsize=5e6, max_evalue=1., use_lds=1, ungapped_min=None, sensitive=False):
    """the protein search configured like the reference's diamond call (uberBlast.py:550).  sensitive: four seed shapes instead of DIAMOND's
    two default-mode shapes - against exhaustive Smith-Waterman the recall between 0.45 and 0.7 identity rises from 0.93 to 0.985 on the
    1 000-gene configuration (above 0.7 it is 1.0 either way) at twice the seed-stage cost; the reference itself runs diamond at its default
    sensitivity, so this is an option (RunBlast(sensitive=True) / uberBlast's --sensitive flag / pep_set_sensitivity in the C ABI), not the default"""
    p = SearchParams()
    load_library().pep_default_params(C.byref(p))
    if ungapped_min is not None:
        p.ungapped_min = int(ungapped_min)
    p.min_id_pct, p.min_qcov_pct, p.top_k, p.n_splits = float(min_id_pct), float(min_qcov_pct), int(top_k), int(n_splits)
    p.dbsize, p.max_evalue, p.use_lds = float(dbsize), float(max_evalue), int(use_lds)
    if sensitive:
        if load_library().pep_set_sensitivity(C.byref(p), 1) != 0:
            raise PepError('pep_set_sensitivity failed')
    return p


def min_score(qlen, dbsize=5e6, max_evalue=1.):
    return int(load_library().pep_min_score(int(qlen), float(dbsize), float(max_evalue)))


_NUCL_PARAMS = {}


def nucleotide_params(min_id_pct=0., min_qcov_pct=0., top_k=1000, dbsize=5e6, max_evalue=1e-2, hsp_mode=1):
    """the search engine configured like the reference's blastn call (uberBlast.py:294): residues A0 C1 G2 T3 (other 4),
    exact 17-mers (-word_size 17), reward 2 / penalty -3, gap 6 + 2k, e-value 1e-2 at dbsize 5e6, 1000 targets per query.
    Karlin-Altschul lambda 0.625 / K 0.41 are NCBI's published values for 2/-3 with gap costs 5/2 (closest tabulated)."""
    if hsp_mode not in (1, 2):
        raise ValueError('nucleotide_params: hsp_mode 1 (every band that reaches the threshold) or 2 (BLAST-like culling, top_k counts subjects)')
    key = (float(min_id_pct), float(min_qcov_pct), int(top_k), float(dbsize), float(max_evalue), int(hsp_mode))
    made = _NUCL_PARAMS.get(key)
    if made is not None:                 # (the block is 1.4 KB of fields set one by one below - half a millisecond of every nucleotide search: a copy of the first one)
        return SearchParams.from_buffer_copy(made)
    p = default_params(min_id_pct, min_qcov_pct, top_k, 1, dbsize, max_evalue)
    p.gap_open, p.gap_ext = 6, 2
    p.n_shapes, p.base = 1, 4
    for s in range(4):
        p.weight[s] = 0
    p.weight[0] = 17
    for i in range(32):
        p.offs[0][i] = i if i < 17 else 0
        p.reduce[i] = i if i < 4 else 0xFF
    for a in range(32):
        for b in range(32):
            p.sub[a * 32 + b] = (2 if a == b else -3) if (a < 4 and b < 4) else (-3 if (a < 5 and b < 5) else -64)
    p.ungapped_min, p.xdrop, p.ext_right, p.ext_left = 40, 16, 40, 24
    p.stage1_min = 0                     # (an exact 17-mer scores 32 over its first 16 bases: the first stage has nothing to reject here)
    p.ka_lambda, p.ka_k = 0.625, 0.41
    p.hsp_mode = hsp_mode                # blastn reports every HSP of a subject; a contig can carry several copies of a gene.  2: include/peppan_hip.h
    if len(_NUCL_PARAMS) < 64:
        _NUCL_PARAMS[key] = bytes(p)
    return p


def _pack(seqs):
    """list of str / bytes / uint8 arrays -> (uint8 concatenation, uint64 offsets[n+1]); a ready-made (codes, offsets) tuple passes through"""
    if isinstance(seqs, tuple) and len(seqs) == 2:
        res, off = seqs
        res = np.ascontiguousarray(res, dtype=np.uint8)
        return (res if res.size else np.zeros(1, dtype=np.uint8)), np.ascontiguousarray(off, dtype=np.uint64)
    n = len(seqs)
    off = np.zeros(n + 1, dtype=np.uint64)
    if n >= 4096 and isinstance(seqs, list):                         # big lists of str / bytes: lengths and ONE copy of the bytes in two C loops
        from .hittable import _pyrows
        lens = np.zeros(n, dtype=np.int64)
        total = _pyrows().pep_strs_measure(seqs, lens.ctypes.data)
        if total >= 0:
            res = np.empty(max(total, 1), dtype=np.uint8)
            if _pyrows().pep_strs_pack(seqs, res.ctypes.data, total) == 0:
                off[1:] = np.cumsum(lens)
                return res, off
    if n and all(isinstance(s, str) for s in seqs):                  # one join + one buffer view instead of one array per sequence
        off[1:] = np.cumsum(np.fromiter(map(len, seqs), dtype=np.int64, count=n))
        res = np.frombuffer(''.join(seqs).encode('ascii'), dtype=np.uint8)
    elif n and all(isinstance(s, (bytes, bytearray)) for s in seqs):
        off[1:] = np.cumsum(np.fromiter(map(len, seqs), dtype=np.int64, count=n))
        res = np.frombuffer(b''.join(seqs), dtype=np.uint8)
    else:
        arrs = [np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray)) else
                (np.frombuffer(s.encode('ascii'), dtype=np.uint8) if isinstance(s, str) else np.asarray(s, dtype=np.uint8)) for s in seqs]
        if arrs:
            off[1:] = np.cumsum([a.size for a in arrs])
        res = np.concatenate(arrs) if arrs and off[-1] else np.zeros(1, dtype=np.uint8)
    if res.size == 0:
        res = np.zeros(1, dtype=np.uint8)
    return np.ascontiguousarray(res, dtype=np.uint8), off


def _count(seqs):
    return len(seqs[1]) - 1 if isinstance(seqs, tuple) and len(seqs) == 2 else len(seqs)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _ptr_or_null(a):
    """NULL for an array without entries, where the library asks for that"""
    return _ptr(a) if len(a) else None


def _some(a):
    """`a`, or one zero element of its type when it has no entries, where the library is handed no null pointer"""
    return a if len(a) else np.zeros(1, a.dtype)


def _as_bytes(nt):
    """a nucleotide set given as bytes or as a uint8 array -> flat uint8 array (no copy of bytes)"""
    return np.frombuffer(nt, dtype=np.uint8) if isinstance(nt, (bytes, bytearray, memoryview)) else np.ascontiguousarray(nt, dtype=np.uint8).reshape(-1)


def _calls_within(sizes, budget):
    """packs items of `sizes` bytes, in order, into calls of at most `budget` bytes -> (lo, hi) per call; an item beyond the budget goes alone (the library
    refuses it in its words)"""
    lo = 0
    while lo < len(sizes):
        hi, total = lo + 1, sizes[lo]
        while hi < len(sizes) and total + sizes[hi] <= budget:
            total += sizes[hi]
            hi += 1
        yield lo, hi
        lo = hi


def _check_only(name, *args):
    """one of the device-free pep_*_check functions, its message buffer behind `args`: PepError with the library's code and text, else None"""
    msg = C.create_string_buffer(512)
    rc = getattr(load_library(), name)(*args, msg, len(msg))
    if rc != 0:
        raise PepError('%s failed (%d): %s' % (name, rc, msg.value.decode()))


def _rows_of_groups(packed, row_off, row_len, groups, n):
    """the row table cut down to the rows `groups` (index arrays of n[g] entries, all in range) use -> (packed, row_off, row_len, groups re-indexed)"""
    idx = np.concatenate(groups)
    used, inv = np.unique(idx, return_inverse=True)
    lens = (row_off[1:] - row_off[:-1])[used].astype(np.int64)
    new_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    src = np.repeat(row_off[used].astype(np.int64) - new_off[:-1].astype(np.int64), lens) + np.arange(int(new_off[-1]), dtype=np.int64)
    return packed[src], new_off, row_len[used], np.split(inv.astype(np.uint32), np.cumsum(n)[:-1])


def _group_inputs(who, packed, row_off, row_len, groups):
    """the row table and the groups of an allele_diff / group_verdicts call as flat contiguous arrays of the library's types"""
    packed = np.ascontiguousarray(packed, dtype=np.uint8).reshape(-1)
    row_off = np.ascontiguousarray(row_off, dtype=np.uint64).reshape(-1)
    row_len = np.ascontiguousarray(row_len, dtype=np.uint32).reshape(-1)
    if len(row_off) != len(row_len) + 1:
        raise ValueError('%s: row_off needs one entry more than row_len' % who)
    return packed, row_off, row_len, [np.ascontiguousarray(g, dtype=np.uint32).reshape(-1) for g in groups]


def _group_tables(packed, row_len, groups, per_group=()):
    """what the library reads of a batch: (packed, row_len, grp_off, grp_rows, *per_group), an array without entries replaced by one element
    (the library is handed no null pointer) - the caller keeps them alive over the call"""
    n = np.array([len(g) for g in groups], dtype=np.int64)
    grp_off = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
    grp_rows = np.ascontiguousarray(np.concatenate(groups), dtype=np.uint32) if grp_off[-1] else np.zeros(0, np.uint32)
    return [_some(a) for a in (packed, row_len, grp_off, grp_rows) + tuple(per_group)]


def _plan_batch(who, noun, need, row_len, groups, out_budget):
    """Splits a batch greedily into library calls within `out_budget` bytes of output (need: bytes per group; `noun` names them in the message) and
    the library's budget of bit planes -> [(lo, hi, whole)]: groups[lo:hi] per call, whole = the call takes the row table as it is, else only the
    rows its groups use.  PepError when one group alone exceeds a budget."""
    # bytes of bit planes per row (24 per 64 digits); per group an upper bound of what its rows add to a call (a row shared by two groups counts twice)
    row_planes = 24 * ((3 * ((row_len.astype(np.int64) + 2) // 3) + 63) // 64)
    if any(len(g) and int(g.max()) >= len(row_len) for g in groups):
        # a row index out of range: the whole batch goes to the library as it is, whose check reports it (the same text, split or not)
        return [(0, len(groups), True)]
    planes = np.array([int(row_planes[g].sum()) for g in groups], dtype=np.int64)
    for what, asked, budget in ((noun, need, out_budget), ('bit planes', planes, ALLELE_DIFF_MAX_BYTES)):
        over = np.flatnonzero(asked > budget)
        if len(over):
            raise PepError('%s: group %d (%d rows) needs %d bytes of %s, the budget is %d' % (who, over[0], len(groups[over[0]]), asked[over[0]], what, budget))
    plan, lo = [], 0
    while lo < len(groups):
        hi, total, pl = lo, 0, 0
        while hi < len(groups) and total + need[hi] <= out_budget and pl + planes[hi] <= ALLELE_DIFF_MAX_BYTES:
            total += int(need[hi])
            pl += int(planes[hi])
            hi += 1
        plan.append((lo, hi, lo == 0 and hi == len(groups) and int(row_planes.sum()) <= ALLELE_DIFF_MAX_BYTES))
        lo = hi
    return plan


def _verdict_tables(packed, row_off, row_len, groups, genomes, inparalog, gd):
    """the arrays of one pep_group_verdicts / pep_group_verdicts_check call, in the order of their leading arguments, + the list that keeps them alive"""
    grp_genome = np.ascontiguousarray(np.concatenate(genomes), dtype=np.uint32) if len(genomes) else np.zeros(0, np.uint32)
    keys, vals, default = gd[:3]
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
    vals = np.ascontiguousarray(vals, dtype=np.float64).reshape(-1, 3)
    default = np.ascontiguousarray(default, dtype=np.float64).reshape(3)
    if len(keys) != len(vals):
        raise ValueError('group_verdicts: one row of values per key')
    pk, rl, grp_off, grp_rows, grp_genome, ip, kk, vv = keep = _group_tables(packed, row_len, groups, (grp_genome, inparalog, keys, vals))
    keep += [row_off, default]
    args = [_ptr(pk), _ptr(row_off), _ptr(rl), len(row_len), len(groups), _ptr(grp_off), _ptr(grp_rows), _ptr(grp_genome), _ptr(ip),
            _ptr(kk), _ptr(vv), len(keys), _ptr(default)]
    return args, keep


def _verdict_inputs(packed, row_off, row_len, groups, genomes, inparalog):
    packed, row_off, row_len, groups = _group_inputs('group_verdicts', packed, row_off, row_len, groups)
    genomes = [np.ascontiguousarray(g, dtype=np.uint32).reshape(-1) for g in genomes]
    inparalog = np.ascontiguousarray(inparalog, dtype=np.uint8).reshape(-1)
    if len(genomes) != len(groups) or len(inparalog) != len(groups) or any(len(a) != len(b) for a, b in zip(groups, genomes)):
        raise ValueError('group_verdicts: one genome id per row of every group and one inparalog flag per group')
    return packed, row_off, row_len, groups, genomes, inparalog


def group_verdicts_check(packed, row_off, row_len, groups, genomes, inparalog, gd, self_id):
    """the host checks of pep_group_verdicts alone (no context, no device): PepError with the library's code and text, else None"""
    packed, row_off, row_len, groups, genomes, inparalog = _verdict_inputs(packed, row_off, row_len, groups, genomes, inparalog)
    args, keep = _verdict_tables(packed, row_off, row_len, groups, genomes, inparalog, gd)
    _check_only('pep_group_verdicts_check', *args, self_id)


def _ingroup_tables(genome, iden, score, gene_off, gd):
    """the arrays of one pep_gene_ingroups / pep_gene_ingroups_check call as the library's types -> (leading arguments, n_rows, n_genes, what keeps them alive)"""
    genome = np.ascontiguousarray(genome, dtype=np.uint32).reshape(-1)
    iden = np.ascontiguousarray(iden, dtype=np.int32).reshape(-1)
    score = np.ascontiguousarray(score, dtype=np.int64).reshape(-1)
    gene_off = np.ascontiguousarray(gene_off, dtype=np.uint64).reshape(-1)
    if not (len(genome) == len(iden) == len(score)):
        raise ValueError('gene_ingroups: genome, iden and score hold one entry per row')
    if len(gene_off) < 1:
        raise ValueError('gene_ingroups: gene_off needs one entry more than there are genes')
    keys, vals, default = gd[:3]
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
    vals = np.ascontiguousarray(vals, dtype=np.float64).reshape(-1, 3)
    default = np.ascontiguousarray(default, dtype=np.float64).reshape(3)
    if len(keys) != len(vals):
        raise ValueError('gene_ingroups: one row of values per key')
    n_rows, n_genes = len(genome), len(gene_off) - 1
    keep = [_some(a) for a in (genome, iden, score, gene_off, keys, vals)] + [default]
    g, i, s, o, kk, vv, dd = keep
    args = [_ptr(g), _ptr(i), _ptr(s), n_rows, n_genes, _ptr(o), _ptr(kk), _ptr(vv), len(keys), _ptr(dd)]
    return args, n_rows, n_genes, keep


def gene_ingroups_check(genome, iden, score, gene_off, gd, self_id, thr):
    """the host checks of pep_gene_ingroups alone (no context, no device): PepError with the library's code and text, else None"""
    args, _, _, keep = _ingroup_tables(genome, iden, score, gene_off, gd)
    _check_only('pep_gene_ingroups_check', *args, self_id, thr)


def _synteny_tables(member_off, genome, nb_off, nb, n_neighbor):
    """the arrays of one pep_synteny_pairs / pep_synteny_pairs_check call as the library's types -> (arguments, n_groups, what keeps them alive)"""
    member_off = np.ascontiguousarray(member_off, dtype=np.uint64).reshape(-1)
    genome = np.ascontiguousarray(genome, dtype=np.uint32).reshape(-1)
    nb_off = np.ascontiguousarray(nb_off, dtype=np.uint64).reshape(-1)
    nb = np.ascontiguousarray(nb, dtype=np.uint32).reshape(-1)
    if len(member_off) < 1:
        raise ValueError('synteny_pairs: member_off needs one entry more than there are groups')
    if len(nb_off) != len(genome) + 1:
        raise ValueError('synteny_pairs: nb_off needs one entry more than there are members')
    if int(n_neighbor) != n_neighbor or not -2 ** 31 <= int(n_neighbor) < 2 ** 31:
        raise ValueError('synteny_pairs: n_neighbor must be an integer that fits 32 bits, not %r' % (n_neighbor,))
    keep = [member_off, _some(genome), nb_off, _some(nb)]
    args = [len(member_off) - 1, _ptr(keep[0]), _ptr(keep[1]), len(genome), _ptr(keep[2]), _ptr(keep[3]), len(nb), int(n_neighbor)]
    return args, len(member_off) - 1, keep


def synteny_pairs_check(member_off, genome, nb_off, nb, n_neighbor):
    """the host checks of pep_synteny_pairs alone (no context, no device): PepError with the library's code and text, else None"""
    args, _, keep = _synteny_tables(member_off, genome, nb_off, nb, n_neighbor)
    _check_only('pep_synteny_pairs_check', *args)


def synteny_walk(member_off, conf_off, conf, walk_off, walk):
    """pep_synteny_walk (host C++, no context): the merge walk of ite_synteny_resolver (PEPPAN.py:1118-1151) over the two pair lists of
    Context.synteny_pairs -> (verdict uint8[G]: 0 none, 1 refused, 2 partition; components: per group None or the list of its components as
    (root, int64 array of member numbers in the reference's order), by ascending root - the root is the member whose id keys the component in
    the reference's dictionary)"""
    member_off = np.ascontiguousarray(member_off, dtype=np.uint64).reshape(-1)
    conf_off = np.ascontiguousarray(conf_off, dtype=np.uint64).reshape(-1)
    walk_off = np.ascontiguousarray(walk_off, dtype=np.uint64).reshape(-1)
    conf = np.ascontiguousarray(conf, dtype=np.uint32).reshape(-1, 2)
    walk = np.ascontiguousarray(walk, dtype=np.uint32).reshape(-1, 2)
    n_groups = len(member_off) - 1
    if n_groups < 0 or len(conf_off) != n_groups + 1 or len(walk_off) != n_groups + 1:
        raise ValueError('synteny_walk: one offset more than there are groups in each of the three offset tables')
    if int(conf_off[-1]) != len(conf) or int(walk_off[-1]) != len(walk):
        raise ValueError('synteny_walk: the offsets must end at the length of their list')
    n_members = int(member_off[-1])
    verdict, n_comp = np.zeros(max(n_groups, 1), np.uint8), np.zeros(max(n_groups, 1), np.uint32)
    comp_root, comp_len, members = (np.zeros(max(n_members, 1), np.uint32) for _ in range(3))
    cc, ww = _some(conf), _some(walk)
    _check_only('pep_synteny_walk', n_groups, _ptr(member_off), _ptr(conf_off), _ptr(cc), _ptr(walk_off), _ptr(ww), _ptr(verdict), _ptr(n_comp), _ptr(comp_root),
                _ptr(comp_len), _ptr(members))
    comps = []
    for g in range(n_groups):
        if verdict[g] != 2:
            comps.append(None)
            continue
        lo = int(member_off[g])
        cuts = np.cumsum(comp_len[lo:lo + int(n_comp[g])])[:-1]
        comps.append(list(zip(comp_root[lo:lo + int(n_comp[g])].tolist(), np.split(members[lo:int(member_off[g + 1])].astype(np.int64), cuts))))
    return verdict[:n_groups], comps


def _genestruct_tables(seq_off, seq, win_off, win_len, flags, lp, allowed_vary, ref_len):
    """the tables of one pep_gene_structure / pep_gene_structure_check call as the library's types -> (arguments behind the nucleotides, n_pred, what
    keeps them alive).  Values that do not fit their column raise ValueError here: ctypes and numpy would cut them silently"""
    seq_off = np.ascontiguousarray(seq_off, dtype=np.uint64).reshape(-1)
    if len(seq_off) < 1:
        raise ValueError('gene_structure: seq_off needs one entry more than there are sequences')
    cols = []
    for name, col, dtype in (('seq', seq, np.uint32), ('win_off', win_off, np.uint64), ('win_len', win_len, np.uint32), ('flags', flags, np.uint8), ('lp', lp, np.uint32),
                             ('allowed_vary', allowed_vary, np.uint32), ('ref_len', ref_len, np.uint32)):
        a = np.asarray(col).reshape(-1)
        if a.dtype != dtype:
            if len(a) and a.dtype.kind not in 'iu':
                raise ValueError('gene_structure: %s must hold integers' % name)
            if len(a) and (int(a.min()) < 0 or int(a.max()) > np.iinfo(dtype).max):
                raise ValueError('gene_structure: %s holds values outside [0, %d]' % (name, np.iinfo(dtype).max))
            a = a.astype(dtype)
        cols.append(np.ascontiguousarray(a))
    n_pred = len(cols[0])
    if any(len(c) != n_pred for c in cols):
        raise ValueError('gene_structure: one entry per prediction in each of the seven columns')
    if n_pred >= 1 << 32 or len(seq_off) - 1 >= 1 << 32:
        raise ValueError('gene_structure: more than 2^32 - 1 predictions or sequences in one call')
    keep = [seq_off] + [_some(c) for c in cols]
    return [_ptr(keep[0]), len(seq_off) - 1, n_pred] + [_ptr(c) for c in keep[1:]], n_pred, keep


def gene_structure_check(seq_off, seq, win_off, win_len, flags, lp, allowed_vary, ref_len):
    """the host checks of pep_gene_structure alone (no context, no device, the nucleotides are not read): PepError with the library's code and text, else None"""
    args, _, keep = _genestruct_tables(seq_off, seq, win_off, win_len, flags, lp, allowed_vary, ref_len)
    _check_only('pep_gene_structure_check', *args)


def _cds_tables(contig_off, contig, win_off, win_len, strand):
    """the tables of a pep_cds_genes / pep_cds_genes_check call as the library's types; values that do not fit their column raise ValueError here"""
    contig_off = np.ascontiguousarray(contig_off, dtype=np.uint64).reshape(-1)
    if len(contig_off) == 0:
        raise ValueError('cds_genes: contig_off has n_contigs + 1 entries')
    given = [np.asarray(col).reshape(-1) for col in (contig, win_off, win_len, strand)]
    n_cds = len(given[0])
    if any(len(c) != n_cds for c in given):
        raise ValueError('cds_genes: one entry per CDS in every table')
    if n_cds >= CDS_MAX_ITEMS or len(contig_off) - 1 >= 1 << 32:              # (before any column is looked through)
        raise ValueError('cds_genes: 2^32 CDS or contigs or more in one call')
    cols = []
    for name, col, dtype in zip(('contig', 'win_off', 'win_len', 'strand'), given, (np.uint32, np.uint64, np.uint32, np.uint8)):
        if len(col) and (col.dtype.kind not in 'iub' or (col.dtype.kind == 'i' and (col < 0).any()) or int(col.max()) > np.iinfo(dtype).max):
            raise ValueError('cds_genes: %s must be integers that fit %s' % (name, np.dtype(dtype).name))
        cols.append(np.ascontiguousarray(col, dtype=dtype))
    keep = [contig_off] + [_some(c) for c in cols]
    return [_ptr(keep[0]), len(contig_off) - 1, n_cds] + [_ptr(c) for c in keep[1:]], n_cds, keep


def cds_genes_check(contig_off, contig, win_off, win_len, strand, mask=0):
    """the host checks of pep_cds_genes alone (no context, no device, the contigs are not read): PepError with the library's code and text, else None"""
    args, _, keep = _cds_tables(contig_off, contig, win_off, win_len, strand)
    _check_only('pep_cds_genes_check', *args, int(mask))


def _outalleles_tables(contig_off, seed_contig, rows, look9):
    """the tables of a pep_out_alleles / pep_out_alleles_check call as the library's types; values that do not fit int32 raise ValueError here"""
    contig_off = np.ascontiguousarray(contig_off, dtype=np.uint64).reshape(-1)
    if len(contig_off) == 0:
        raise ValueError('out_alleles: contig_off has n_contigs + 1 entries')
    given = []
    for name, a in (('seed_contig', seed_contig), ('rows', rows), ('look9', look9)):
        if a is None:
            given.append(None)
            continue
        a = np.asarray(a)
        if a.size and (a.dtype.kind not in 'iu' or int(a.min()) < -2 ** 31 or int(a.max()) >= 2 ** 31):
            raise ValueError('out_alleles: %s must be integers that fit int32' % name)
        given.append(np.ascontiguousarray(a, dtype=np.int32))
    seed_contig, rows, look9 = given[0].reshape(-1), given[1], given[2]
    if rows.ndim != 2 or rows.shape[1] != OUTA_COLS:
        raise ValueError('out_alleles: rows is a table [n_rows, %d]' % OUTA_COLS)
    n_rows = rows.shape[0]
    if look9 is not None and look9.shape != (n_rows,):
        raise ValueError('out_alleles: look9 has one entry per row')
    if n_rows + len(seed_contig) >= OUTA_MAX_ITEMS or len(contig_off) - 1 >= 1 << 32:
        raise ValueError('out_alleles: 2^30 rows and genes, or 2^32 contigs, or more in one call')
    keep = [contig_off, _some(seed_contig), _some(rows.reshape(-1)), look9]
    return [_ptr(keep[0]), len(contig_off) - 1, len(seed_contig), _ptr(keep[1]), n_rows, _ptr(keep[2]), None if look9 is None else _ptr(look9)], n_rows, keep


def out_alleles_check(contig_off, seed_contig, rows, look9=None, key_bits=0):
    """the host checks of pep_out_alleles alone (no context, no device, the contigs are not read): PepError with the library's code and text, else None"""
    args, _, keep = _outalleles_tables(contig_off, seed_contig, rows, look9)
    _check_only('pep_out_alleles_check', *args, int(key_bits))


def pack_presence(presence):
    """a presence matrix bool[n_genomes, n_genes] as the bit rows of include/peppan_hip.h (K20): uint64[n_genomes, W], gene e at bit e % 64 of word e // 64, padding zero"""
    presence = np.asarray(presence, dtype=bool)
    if presence.ndim != 2:
        raise ValueError('pack_presence: a matrix [n_genomes, n_genes]')
    n, n_genes = presence.shape
    words = (n_genes + 63) // 64
    padded = np.zeros((n, words * 64), dtype=bool)
    padded[:, :n_genes] = presence
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder='little')).view('<u8').reshape(n, words)


def _curve_tables(bits, n_genes, orders):
    """the tables of one pep_rarefaction_curves / pep_rarefaction_curves_check call as the library's types -> (arguments, n_genomes, n_iter, what keeps them alive).
    Shapes that do not fit each other and values that do not fit their column raise ValueError here: ctypes and numpy would cut them silently"""
    bits = np.asarray(bits)
    orders = np.asarray(orders)
    if bits.ndim != 2 or orders.ndim != 2:
        raise ValueError('rarefaction_curves: bits is [n_genomes, W] and orders [n_iter, n_genomes]')
    if bits.dtype != np.uint64:
        raise ValueError('rarefaction_curves: bits must be uint64 words (pack_presence)')
    n_genes = int(n_genes)
    if n_genes < 0 or n_genes >= 1 << 64 or bits.shape[1] != (n_genes + 63) // 64:
        raise ValueError('rarefaction_curves: %d genes need %d words per genome, not %d' % (n_genes, (n_genes + 63) // 64, bits.shape[1]))
    if orders.shape[1] != bits.shape[0]:
        raise ValueError('rarefaction_curves: an order names every genome once: %d entries for %d genomes' % (orders.shape[1], bits.shape[0]))
    if orders.dtype != np.uint32:
        if orders.size and orders.dtype.kind not in 'iu':
            raise ValueError('rarefaction_curves: orders must hold integers')
        if orders.size and (int(orders.min()) < 0 or int(orders.max()) >= 1 << 32):
            raise ValueError('rarefaction_curves: orders holds values outside [0, 2^32)')
        orders = orders.astype(np.uint32)
    if bits.shape[0] >= 1 << 32 or orders.shape[0] >= 1 << 32:
        raise ValueError('rarefaction_curves: more than 2^32 - 1 genomes or orders in one call')
    keep = [_some(np.ascontiguousarray(bits).reshape(-1)), _some(np.ascontiguousarray(orders).reshape(-1))]
    return [_ptr(keep[0]), bits.shape[0], n_genes, _ptr(keep[1]), orders.shape[0]], bits.shape[0], orders.shape[0], keep


def rarefaction_curves_check(bits, n_genes, orders):
    """the host checks of pep_rarefaction_curves alone (no context, no device): PepError with the library's code and text, else None"""
    args, _, _, keep = _curve_tables(bits, n_genes, orders)
    _check_only('pep_rarefaction_curves_check', *args)


def profile_pairs_check(n, n_genes):
    """the host checks of pep_profile_pairs alone (the sizes; no context, no device): PepError with the library's code and text, else None"""
    if not (0 <= int(n) < 1 << 32 and 0 <= int(n_genes) < 1 << 64):
        raise ValueError('profile_pairs: sizes outside their columns')
    _check_only('pep_profile_pairs_check', int(n), int(n_genes))


def nj_trees_check(n_leaves, dist_off, out_off):
    """the host checks of pep_nj_trees that read no distance (no context, no device): PepError with the library's code and text, else None.  dist_off and out_off
    have one entry more than n_leaves: the lengths of the arrays"""
    n = np.ascontiguousarray(n_leaves, dtype=np.uint32).reshape(-1)
    dist_off, out_off = (np.ascontiguousarray(a, dtype=np.uint64).reshape(-1) for a in (dist_off, out_off))
    if len(dist_off) != len(n) + 1 or len(out_off) != len(n) + 1:
        raise ValueError('nj_trees: dist_off and out_off need one entry more than n_leaves')
    _check_only('pep_nj_trees_check', _ptr(_some(n)), len(n), _ptr(dist_off), _ptr(out_off))


def _tree_cut_tables(n_leaves, sets):
    """the offsets tables of a pep_tree_cut / pep_tree_cut_check call laid out densely, and the bit sets as one array: sets[t] is uint64[B, words]"""
    n = np.ascontiguousarray(n_leaves, dtype=np.uint32).reshape(-1)
    if len(sets) != len(n):
        raise ValueError('tree_cuts: one array of bit sets per tree')
    sets = [np.ascontiguousarray(s, dtype=np.uint64) for s in sets]
    for t, s in enumerate(sets):
        if s.ndim != 2 or s.shape[1] != (int(n[t]) + 63) // 64:
            raise ValueError('tree_cuts: the bit sets of tree %d are %s, not [branches, %d words]' % (t, s.shape, (int(n[t]) + 63) // 64))
    n64 = n.astype(np.int64)
    leaf_off = np.concatenate([[0], np.cumsum(n64)]).astype(np.uint64)
    mat_off = np.concatenate([[0], np.cumsum(n64 * n64)]).astype(np.uint64)
    branch_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.uint64)
    set_off = np.concatenate([[0], np.cumsum([s.size for s in sets])]).astype(np.uint64)
    flat = np.concatenate([s.reshape(-1) for s in sets]) if sets else np.zeros(0, np.uint64)
    return n, leaf_off, mat_off, branch_off, set_off, _some(flat)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64).reshape(-1)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)


def _prep_offsets(what, gene_off, cols, cfl_off=None, cfl=None):
    """the tables of a K26 call as the library takes them; ValueError where an array is shorter than its offsets table says (the library cannot see lengths)"""
    gene_off = _u64(gene_off)
    if len(gene_off) < 1:
        raise ValueError('%s: gene_off needs one entry more than there are genes' % what)
    n_rows = int(gene_off[-1])
    cols = [_i64(c) for c in cols]
    if any(len(c) != n_rows for c in cols):
        raise ValueError('%s: every column needs gene_off[-1] = %d entries' % (what, n_rows))
    if cfl_off is None:
        return gene_off, cols
    cfl_off, cfl = _u64(cfl_off), _i64(cfl)
    if len(cfl_off) != n_rows + 1 or int(cfl_off[-1]) != len(cfl):
        raise ValueError('%s: cfl_off needs one entry per row and one more, and must end at the length of cfl' % what)
    return gene_off, cols, cfl_off, cfl


def batch_screen_check(gene_off, col3, locus, n_loci):
    """every check of Context.batch_screen, without a context or a device: PepError with the library's code and text, else None"""
    gene_off, (col3, locus) = _prep_offsets('batch_screen', gene_off, (col3, locus))
    _check_only('pep_batch_screen_check', len(gene_off) - 1, _ptr(gene_off), _ptr(_some(col3)), _ptr(_some(locus)), int(n_loci))


def batch_unsure_walk(gene_off, col3, locus, cfl_off, cfl, n_loci, check_only=False):
    """pep_batch_unsure_walk (host C++, no context): stage B of include/peppan_hip.h (PEPPAN.py:579-593) over the genes in the order given ->
    (col3 as the walk leaves it, popped uint8[n_genes]); check_only: pep_batch_unsure_walk_check, None"""
    gene_off, (col3, locus), cfl_off, cfl = _prep_offsets('batch_unsure_walk', gene_off, (col3, locus), cfl_off, cfl)
    n = len(gene_off) - 1
    if check_only:
        return _check_only('pep_batch_unsure_walk_check', n, _ptr(gene_off), _ptr(_some(col3)), _ptr(_some(locus)), _ptr(cfl_off), _ptr(_some(cfl)), int(n_loci))
    col3, popped = col3.copy() if len(col3) else np.zeros(1, np.int64), np.zeros(max(n, 1), np.uint8)
    _check_only('pep_batch_unsure_walk', n, _ptr(gene_off), _ptr(col3), _ptr(_some(locus)), _ptr(cfl_off), _ptr(_some(cfl)), int(n_loci), _ptr(popped))
    return col3[:int(gene_off[-1])], popped[:n]


def batch_prune_check(mode, gene_off, genome, col2, col3, col4, locus, cfl_off, cfl, n_loci, path=0):
    """every check of Context.batch_prune, without a context or a device"""
    gene_off, cols, cfl_off, cfl = _prep_offsets('batch_prune', gene_off, (genome, col2, col3, col4, locus), cfl_off, cfl)
    _check_only('pep_batch_prune_check', int(mode), len(gene_off) - 1, _ptr(gene_off), *[_ptr(_some(c)) for c in cols], _ptr(cfl_off), _ptr(_some(cfl)), int(n_loci), int(path))


def tree_cut_check(n_leaves, leaf_off, mat_off, branch_off, set_off, sets, path=0):
    """the host checks of pep_tree_cut that read no matrix (no context, no device) on the caller's own tables: PepError with the library's code and text, else
    None.  Every offsets table has one entry more than n_leaves; sets: the uint64 words of all bit sets; None for a table hands the library a null pointer"""
    n = np.ascontiguousarray(n_leaves, dtype=np.uint32).reshape(-1)
    tabs = [None if a is None else np.ascontiguousarray(a, dtype=np.uint64).reshape(-1) for a in (leaf_off, mat_off, branch_off, set_off, sets)]
    for a in tabs[:4]:
        if a is not None and len(a) != len(n) + 1:
            raise ValueError('tree_cuts: every offsets table needs one entry more than n_leaves')
    _check_only('pep_tree_cut_check', _ptr(_some(n)), len(n), *[None if a is None else _ptr(_some(a)) for a in tabs], int(path))


def _gdiff_tables(events, arena):
    """events and arena of a pep_global_diff / pep_global_diff_check call as the library's types; values that do not fit their column raise ValueError here"""
    events = np.asarray(events)
    if events.size == 0:
        events = np.zeros((0, 6), dtype=np.int64)
    if events.ndim != 2 or events.shape[1] != 6 or events.dtype.kind not in 'iu':
        raise ValueError('global_diff: events is integer [n, 6]: a_off, a_len, b_off, b_len, value, drop_same')
    arena = np.asarray(arena)
    if arena.size and (arena.ndim != 1 or arena.dtype.kind not in 'iu'):
        raise ValueError('global_diff: arena is a vector of genome ranks')
    if arena.size and (int(arena.min()) < -(1 << 31) or int(arena.max()) >= 1 << 31):
        raise ValueError('global_diff: arena holds values outside int32')
    return np.ascontiguousarray(events, dtype=np.int64), np.ascontiguousarray(arena.reshape(-1), dtype=np.int32)


def global_diff_check(events, arena, n_genomes, chunk_items=0):
    """the host checks of pep_global_diff alone (no context, no device): PepError with the library's code and text, else None"""
    events, arena = _gdiff_tables(events, arena)
    _check_only('pep_global_diff_check', _ptr_or_null(events), len(events), _ptr_or_null(arena), len(arena), int(n_genomes), int(chunk_items))


def global_diff_walk(clu, bsn, genes, genome_of):
    """pep_global_diff_walk: the dictionary walk of get_global_difference (PEPPAN.py:1632-1659) over the selected rows -> (events int64[n, 6], arena int32[],
    genomes int32[G]: the genome id of every rank).  clu / bsn: integer [n, 3] rows (r, q, value) in file order; genes ascending, genome_of their genomes.
    No context, no device; PepError with the library's code and text (a gene that is not in the map, a value outside 0 .. 10049)."""
    lib = load_library()
    clu, bsn = (np.ascontiguousarray(np.asarray(t).reshape(-1, 3), dtype=np.int64) for t in (clu, bsn))
    genes = np.ascontiguousarray(genes, dtype=np.int64).reshape(-1)
    genome_of = np.asarray(genome_of).reshape(-1)
    if len(genome_of) != len(genes):
        raise ValueError('global_diff_walk: one genome per gene')
    if len(genome_of) and (int(genome_of.min()) < -(1 << 31) or int(genome_of.max()) >= 1 << 31):
        raise ValueError('global_diff_walk: genome ids outside int32')
    genome_of = np.ascontiguousarray(genome_of, dtype=np.int32)
    walk, msg = C.c_void_p(), C.create_string_buffer(512)
    rc = lib.pep_global_diff_walk(_ptr_or_null(clu), len(clu), _ptr_or_null(bsn), len(bsn), _ptr_or_null(genes), _ptr_or_null(genome_of), len(genes),
                                  C.byref(walk), msg, len(msg))
    if rc != 0:
        raise PepError('pep_global_diff_walk failed (%d): %s' % (rc, msg.value.decode()))
    try:
        n_events, arena_len, n_genomes = C.c_uint64(), C.c_uint64(), C.c_uint32()
        if lib.pep_global_diff_walk_size(walk, C.byref(n_events), C.byref(arena_len), C.byref(n_genomes)) != 0:
            raise PepError('pep_global_diff_walk_size failed')
        events, arena = np.zeros((n_events.value, 6), dtype=np.int64), np.zeros(arena_len.value, dtype=np.int32)
        genomes = np.zeros(n_genomes.value, dtype=np.int32)
        if lib.pep_global_diff_walk_copy(walk, _ptr_or_null(events), _ptr_or_null(arena), _ptr_or_null(genomes)) != 0:
            raise PepError('pep_global_diff_walk_copy failed')
    finally:
        lib.pep_global_diff_walk_free(walk)
    return events, arena, genomes


def codon_tables(table_id=11):
    """(aa_of_word uint8[125], sub int8[1024]) for rescoring mode 2, made from the module tables of peppan_amd.uberBlast / configure - the one source, the library
    holds no copy: gtable (for table 4 entry 56 becomes 22, the reference's own patch, uberBlast.py:223-224) and blosum62 padded to 32 x 32"""
    from .uberBlast import gtable
    from .configure import blosum62
    aa = np.array(gtable).reshape(-1)
    if table_id == 4:
        aa = aa.copy()
        aa[56] = 22
    sub = np.zeros(1024, dtype=np.float64)
    flat = np.asarray(blosum62, dtype=np.float64).reshape(-1)
    assert aa.shape == (125,) and len(flat) <= 1024
    sub[:len(flat)] = flat
    for name, t, lo, hi in (('gtable', aa, 0, 255), ('blosum62', sub, -128, 127)):
        assert np.all(t == np.round(t)) and t.min() >= lo and t.max() <= hi, name + ': entries must be integers in range'
    return np.ascontiguousarray(aa, dtype=np.uint8), np.ascontiguousarray(sub, dtype=np.int8)


def _codon_args(nt_hits, cigar, mode, tables):
    """the leading arguments of pep_rescore_codons / pep_rescore_codons_check behind the context + what keeps them alive; tables: (aa_of_word, sub) or None"""
    nt_hits = np.ascontiguousarray(nt_hits, dtype=NT_HIT_DTYPE)
    cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
    hh, cg = _some(nt_hits), _some(cigar)
    aa, sub = (None, None) if tables is None else (None if t is None else np.ascontiguousarray(t, dtype=d) for t, d in zip(tables, (np.uint8, np.int8)))
    args = [len(nt_hits), _ptr(hh), _ptr(cg), len(cigar), int(mode), None if aa is None else _ptr(aa), None if sub is None else _ptr(sub)]
    return args, [hh, cg, aa, sub]


def rescore_codons_check(nt_hits, cigar, mode, q_off, r_off, table_id=11, tables='module'):
    """the host checks of pep_rescore_codons alone (no context, no device): PepError with the library's code and text, else None.  q_off / r_off:
    offsets [n + 1] of the two nucleotide sets; tables: (aa_of_word, sub) instead of the module's own for table_id (None, or a None entry: a NULL pointer)"""
    args, keep = _codon_args(nt_hits, cigar, mode, codon_tables(table_id) if isinstance(tables, str) else tables)
    q_off, r_off = np.ascontiguousarray(q_off, dtype=np.uint64), np.ascontiguousarray(r_off, dtype=np.uint64)
    _check_only('pep_rescore_codons_check', *args, _ptr(q_off), len(q_off) - 1, _ptr(r_off), len(r_off) - 1)


def ovl_filter(q, r, qs, qe, ss, se, score, iden, coverage, delta):
    """pep_ovl_filter on sorted numeric columns; `iden` (float64) is updated in place: dropped rows get -1"""
    lib = load_library()
    n = len(q)
    arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (q, r, qs, qe, ss, se)]
    score = np.ascontiguousarray(score, dtype=np.float64)
    assert iden.dtype == np.float64 and iden.flags['C_CONTIGUOUS']
    rc_ = lib.pep_ovl_filter(n, *[_ptr(a) for a in arrs], _ptr(score), _ptr(iden), coverage, delta)
    if rc_ != 0:
        raise PepError('pep_ovl_filter failed (%d)' % rc_)


def known_order(T, genes_of):
    """pep_known_order: compare_prediction over a HitTable's columns -> (order int64[n], known float64[n]) - the rows in the order (query, contig, score) and their
    column 10.  genes_of(c): the original genes of the contig with row code c as (start int64[], end int64[], plus bool[]) in the store's order, or None"""
    lib = load_library()
    n = len(T)
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    ri, r_code, q_code = i64(T.ri), i64(T.r_codes()), i64(T.q_codes())
    n_contigs = len(T.r_tab)
    g_off = np.zeros(n_contigs + 1, dtype=np.uint64)
    parts, is_sorted = {}, np.ones(max(n_contigs, 1), dtype=np.uint8)
    for c in (np.unique(ri).tolist() if n else []):
        g = genes_of(c)
        if g is not None and len(g[0]):
            parts[c] = g
            g_off[c + 1] = len(g[0])
            is_sorted[c] = 0 if (np.diff(g[0]) < 0).any() else 1
    np.cumsum(g_off, out=g_off)
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([parts[c][k] for c in sorted(parts)]) if parts else np.zeros(1), dtype=dt)
    g1, g2, plus = cat(0, np.int64), cat(1, np.int64), cat(2, np.uint8)
    cols = [i64(a) for a in (T.ss, T.se, T.qs, T.qe, T.ql)]
    score = np.ascontiguousarray(T.score, dtype=np.float64)
    order, known = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.float64)
    rc_ = lib.pep_known_order(n, _ptr(ri), _ptr(r_code), _ptr(q_code), *([_ptr(c) for c in cols] + [_ptr(score), n_contigs, _ptr(g_off), _ptr(g1), _ptr(g2),
                              _ptr(plus), _ptr(is_sorted), _ptr(order), _ptr(known)]))
    if rc_ != 0:
        raise PepError('pep_known_order failed (%d)' % rc_)
    return order, known


def linear_merge(q, r, iden, qs, qe, ss, se, score, ql, sl, rid, gap_dist, len_diff):
    """pep_linear_merge on sorted numeric columns -> (keep_seq, query_off, query_ascending, grp_score, grp_iden, grp_span, grp_ids_off, grp_ids)"""
    lib = load_library()
    n = len(q)
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    q, r, qs, qe, ss, se, ql, sl, rid = (i64(a) for a in (q, r, qs, qe, ss, se, ql, sl, rid))
    iden, score = f64(iden), f64(score)
    keep_cap, ids_cap = 2 * n + 16, 2 * n + 16
    for _ in range(2):
        keep = np.zeros(keep_cap, dtype=np.int64)
        q_off = np.zeros(n + 2, dtype=np.uint64)
        asc = np.zeros(n + 1, dtype=np.uint8)
        g_score, g_iden, g_span = np.zeros(n + 1), np.zeros(n + 1), np.zeros(n + 1, dtype=np.int64)
        ids_off = np.zeros(n + 2, dtype=np.uint64)
        ids = np.zeros(ids_cap, dtype=np.int64)
        n_keep, n_query, n_ids = C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc_ = lib.pep_linear_merge(n, _ptr(q), _ptr(r), _ptr(iden), _ptr(qs), _ptr(qe), _ptr(ss), _ptr(se), _ptr(score), _ptr(ql), _ptr(sl),
                                   _ptr(rid), gap_dist, len_diff, _ptr(keep), keep_cap, C.byref(n_keep), _ptr(q_off),
                                   _ptr(asc), C.byref(n_query), _ptr(g_score), _ptr(g_iden), _ptr(g_span), _ptr(ids_off), _ptr(ids), ids_cap,
                                   C.byref(n_ids))
        if rc_ != 0:
            raise PepError('pep_linear_merge failed (%d)' % rc_)
        if n_keep.value <= keep_cap and n_ids.value <= ids_cap:
            nq = n_query.value
            return (keep[:n_keep.value], q_off[:nq + 1].astype(np.int64), asc[:nq], g_score[:n], g_iden[:n], g_span[:n], ids_off[:n + 1].astype(np.int64),
                    ids[:n_ids.value])
        keep_cap, ids_cap = n_keep.value + 16, n_ids.value + 16
    raise PepError('pep_linear_merge: inconsistent sizes')


class MatCols(C.Structure):
    """pep_mat_cols (include/peppan_hip.h): the sixteen stored columns of the hit table as pointers"""
    _fields_ = [(n, C.c_void_p) for n in ('q', 'r', 'iden', 'aln', 'mis', 'gap', 'qs', 'qe', 'ss', 'se', 'evalue', 'score', 'ql', 'sl', 'arena', 'c_off', 'c_runs', 'rid')] + \
               [('score_is_int', C.c_int32), ('reserved', C.c_int32)]


_RECON_MODULE = None


def _recon_module():
    """the module numpy's own pickles name for `_reconstruct` (numpy._core.multiarray since numpy 2, numpy.core.multiarray before)"""
    global _RECON_MODULE
    if _RECON_MODULE is None:
        _RECON_MODULE = np.empty(0).__reduce__()[0].__module__.encode()
    return _RECON_MODULE


def _npy_object_header(n):
    """the .npy header of a 1-D object array of n elements (what np.lib.format.write_array puts in front of the pickle)"""
    import io
    buf = io.BytesIO()
    np.lib.format.write_array_header_1_0(buf, {'descr': '|O', 'fortran_order': False, 'shape': (int(n),)})
    return buf.getvalue()


def store_mat_member(cols, row_off, score_is_int):
    """pep_store_mat_member: the complete .npy member (header + pickle stream) of one chunk of the .mat store (PEPPAN.py:959-966).
    cols: the 18 arrays of MatCols in field order (q and r as int64 names per row); row_off int64[n_groups + 1]."""
    lib = load_library()
    keep = [np.ascontiguousarray(a, dtype=dt) for a, dt in zip(cols, (np.int64, np.int64, np.float64) + (np.int64,) * 7 + (np.float64, np.float64, np.int64, np.int64,
                                                                                                                       np.uint32, np.int64, np.int64, np.int64))]
    mc = MatCols(*[a.ctypes.data for a in keep], int(bool(score_is_int)), 0)
    row_off = np.ascontiguousarray(row_off, dtype=np.int64)
    n_groups = len(row_off) - 1
    n_rows = int(row_off[-1] - row_off[0]) if n_groups else 0
    head = _npy_object_header(n_groups)
    cap = 256 + 64 * n_groups + 200 * n_rows + 12 * int(keep[16][row_off[0]:row_off[-1]].sum() if n_rows else 0)
    for _ in range(2):
        buf = np.empty(len(head) + cap, dtype=np.uint8)
        need = lib.pep_store_mat_member(C.byref(mc), _ptr(row_off), n_groups, _recon_module(), buf.ctypes.data + len(head), cap)
        if need < 0:
            raise PepError('pep_store_mat_member failed (%d)' % need)
        if need <= cap:
            buf[:len(head)] = np.frombuffer(head, dtype=np.uint8)
            return buf[:len(head) + need].tobytes()
        cap = int(need)
    raise PepError('pep_store_mat_member: inconsistent sizes')


def store_seq_member(packed, pack_off):
    """pep_store_seq_member: the complete .npy member of one chunk of the .seq store (PEPPAN.py:950-957): object array of uint8 arrays"""
    lib = load_library()
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    pack_off = np.ascontiguousarray(pack_off, dtype=np.int64)
    n_groups = len(pack_off) - 1
    head = _npy_object_header(n_groups)
    cap = 256 + 64 * n_groups + (int(pack_off[-1] - pack_off[0]) if n_groups else 0)
    buf = np.empty(len(head) + cap, dtype=np.uint8)
    need = lib.pep_store_seq_member(_ptr(packed), _ptr(pack_off), n_groups, _recon_module(), buf.ctypes.data + len(head), cap)
    if need < 0 or need > cap:
        raise PepError('pep_store_seq_member failed (%d)' % need)
    buf[:len(head)] = np.frombuffer(head, dtype=np.uint8)
    return buf[:len(head) + need].tobytes()


def deflate_literals(data):
    """pep_deflate_literals: bytes -> raw DEFLATE stream (zlib.decompress(x, -15) gives them back), Huffman coding only"""
    lib = load_library()
    src = np.frombuffer(data, dtype=np.uint8)
    cap = len(src) + len(src) // 64 + 512
    out = np.empty(cap, dtype=np.uint8)
    n = lib.pep_deflate_literals(_ptr_or_null(src), len(src), _ptr(out), cap)
    if n < 0 or n > cap:
        raise PepError('pep_deflate_literals failed (%d)' % n)
    return out[:n].tobytes()


def crc32(data, crc=0):
    """pep_crc32: zlib.crc32 of a bytes-like object, by carry-less multiplication where the CPU has it"""
    lib = load_library()
    src = np.frombuffer(data, dtype=np.uint8)
    return int(lib.pep_crc32(_ptr_or_null(src), len(src), crc))


def pack_member(data, coder):
    """pep_pack_member: bytes -> (raw DEFLATE stream, crc32 of the bytes); coder 0 = literals only (deflate_literals), 1 = single-probe matcher (deflate_fast)"""
    lib = load_library()
    src = np.frombuffer(data, dtype=np.uint8)
    cap = len(src) + len(src) // 8 + 1024
    out = np.empty(cap, dtype=np.uint8)
    crc = C.c_uint32()
    n = lib.pep_pack_member(_ptr_or_null(src), len(src), coder, _ptr(out), cap, C.byref(crc))
    if n < 0 or n > cap:
        raise PepError('pep_pack_member failed (%d)' % n)
    return out[:n].tobytes(), int(crc.value)


def deflate_fast(data):
    """pep_deflate_fast: bytes -> raw DEFLATE stream (zlib.decompress(x, -15) gives them back): single-probe matcher + dynamic Huffman blocks"""
    lib = load_library()
    src = np.frombuffer(data, dtype=np.uint8)
    cap = len(src) + len(src) // 8 + 1024
    out = np.empty(cap, dtype=np.uint8)
    n = lib.pep_deflate_fast(_ptr_or_null(src), len(src), _ptr(out), cap)
    if n < 0 or n > cap:
        raise PepError('pep_deflate_fast failed (%d)' % n)
    return out[:n].tobytes()


class HitCols(C.Structure):
    """pep_hit_cols: pointers to the columns of a hit table"""
    FIELDS = ('qi', 'ri', 'iden', 'aln', 'mis', 'gap', 'qs', 'qe', 'ss', 'se', 'evalue', 'score', 'ql', 'sl', 'c_off', 'c_runs', 'rid')
    FLOATS = ('iden', 'evalue', 'score')
    _fields_ = [(f, C.c_void_p) for f in FIELDS]

    @classmethod
    def over(cls, arrays):
        """the struct over a dict of contiguous int64 / float64 arrays (field -> array; a missing 'rid' is NULL)"""
        c = cls()
        for f in cls.FIELDS:
            a = arrays.get(f)
            if a is not None:
                assert a.flags['C_CONTIGUOUS'] and a.dtype == (np.float64 if f in cls.FLOATS else np.int64), f
                setattr(c, f, a.ctypes.data)
        return c

    @classmethod
    def blank(cls, n):
        """n uninitialised rows: field -> array"""
        block = np.empty([len(cls.FIELDS), max(n, 1)], dtype=np.int64)
        return {f: (block[k].view(np.float64) if f in cls.FLOATS else block[k]) for k, f in enumerate(cls.FIELDS)}


def table_from_hits(tool, hits, cigar, q_len, r_len, min_id, min_cov, min_ratio, q_meta=None, t_meta=None, t_seq=None, t_rev=None, windows=None, evalue=None, nt_match=None):
    """pep_table_from_hits: hit records -> ({field: column[m]}, CIGAR arena in nucleotides).  tool 0 = translated search (q_meta / t_meta), tool 1 =
    nucleotide search (t_seq / t_rev [, windows = (offset, home_lo, home_hi) per target], evalue per hit).  nt_match (uint32 per hit, Context.last_nt_match):
    identity and score come out rescored (reScore mode 1)"""
    lib = load_library()
    n = len(hits)
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
    arena = np.empty(max(len(cigar), 1), dtype=np.uint32)
    cols = HitCols.blank(n)
    i64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int64)
    q_len, r_len, t_seq = i64(q_len), i64(r_len), i64(t_seq)
    t_rev = None if t_rev is None else np.ascontiguousarray(t_rev, dtype=np.uint8)
    w = [i64(a) for a in windows] if windows is not None else [None, None, None]
    evalue = None if evalue is None else np.ascontiguousarray(evalue, dtype=np.float64)
    qm = None if q_meta is None else np.ascontiguousarray(q_meta, dtype=QUERY_META_DTYPE)
    tm = None if t_meta is None else np.ascontiguousarray(t_meta, dtype=TARGET_META_DTYPE)
    if nt_match is not None:
        nt_match = np.ascontiguousarray(nt_match, dtype=np.uint32)
        if len(nt_match) != n:
            raise ValueError('table_from_hits: one nt_match count per hit')
    p = lambda a: None if a is None else _ptr(a)
    hc = HitCols.over(cols)
    m = lib.pep_table_from_hits(tool, n, p(hits), p(cigar), len(cigar), p(qm), p(tm), p(q_len), p(r_len), p(t_seq), p(t_rev),
                                p(w[0]), p(w[1]), p(w[2]), p(evalue), min_id, min_cov, min_ratio, C.byref(hc), _ptr(arena), p(nt_match) if n else None)
    if m < 0:
        raise PepError('pep_table_from_hits failed (%d)' % m)
    return {f: a[:m] for f, a in cols.items()}, arena[:len(cigar)]


def cols_fix_end(cols, arena, se_lim, ee_lim):
    """pep_cols_fix_end over {field: column} in place -> the rows' private arena (c_off rewritten)"""
    lib = load_library()
    n = len(cols['qs'])
    out = np.empty(max(int(cols['c_runs'].sum()) if n else 0, 1), dtype=np.uint32)
    hc = HitCols.over(cols)
    arena = np.ascontiguousarray(arena, dtype=np.uint32)
    rc_ = lib.pep_cols_fix_end(n, C.byref(hc), _ptr_or_null(arena), len(arena), _ptr(out), se_lim, ee_lim)
    if rc_ < 0:
        raise IndexError('fix_end: a row without CIGAR runs cannot be extended (the reference fails on cigar[0] here, uberBlast.py:468), or runs outside the arena')
    return out[:int(cols['c_runs'].sum()) if n else 0]


def lex_order(keys):
    """pep_lex_order: numpy.lexsort(keys) for int64 key columns (the last key is the primary one), by radix passes; numpy's own for keys it does not take"""
    lib = load_library()
    keys = [np.ascontiguousarray(k) for k in keys]
    n = len(keys[0]) if keys else 0
    if not keys or n < 64 or any(k.dtype != np.int64 or len(k) != n for k in keys):
        return np.lexsort(keys)
    order = np.empty(n, dtype=np.int64)
    ptrs = (C.c_void_p * len(keys))(*[k.ctypes.data for k in keys])
    rc_ = lib.pep_lex_order(n, len(keys), ptrs, _ptr(order))
    if rc_ != 0:
        return np.lexsort(keys)
    return order


def set_host_threads(n):
    """pep_set_host_threads: the most threads a pass of the host chain may use (0: the default again); returns the value before"""
    return int(load_library().pep_set_host_threads(int(n)))


def cols_order(q_code, r_code, score):
    """pep_cols_order: the row order of a stable sort by (q_code, r_code, score); codes non-negative"""
    lib = load_library()
    n = len(q_code)
    q_code, r_code = np.ascontiguousarray(q_code, dtype=np.int64), np.ascontiguousarray(r_code, dtype=np.int64)
    score = np.ascontiguousarray(score, dtype=np.float64)
    order = np.empty(n, dtype=np.int64)
    if n and lib.pep_cols_order(n, _ptr(q_code), _ptr(r_code), _ptr(score), _ptr(order)) != 0:
        raise PepError('pep_cols_order failed (negative name codes?)')
    return order


def cols_gather(columns, idx):
    """pep_cols_gather: [column[idx] for column in columns] for contiguous 8-byte columns of one length, in one call"""
    lib = load_library()
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    k, n = len(columns), len(idx)
    out = np.empty([max(k, 1), max(n, 1)], dtype=np.int64)
    src = (C.c_void_p * max(k, 1))(*[a.ctypes.data for a in columns])
    dst = (C.c_void_p * max(k, 1))(*[out[c].ctypes.data for c in range(k)])
    for a in columns:
        assert a.flags['C_CONTIGUOUS'] and a.dtype.itemsize == 8
    n_src = len(columns[0]) if k else 0
    if lib.pep_cols_gather(k, src, dst, _ptr_or_null(idx), n, n_src) != 0:
        raise IndexError('take: row index outside the table')
    return [out[c][:n].view(a.dtype) for c, a in enumerate(columns)]


def store_tab_members(rows, off, keys, date_time, threads=None, order=None):
    """pep_store_tab_members: the finished zip entries of all members of the .tab store (PEPPAN.py:91-113, 972-975) ->
    (bytes of all entries, crc uint32[m], compressed size int64[m], size int64[m], offset of the entry int64[m])"""
    lib = load_library()
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    off, keys = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(keys, dtype=np.int64)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.int64)
    m = len(keys)
    if rows.ndim != 2 or len(off) != m + 1:
        raise ValueError('store_tab_members: rows int64[n, c], off int64[m + 1], keys int64[m]')
    crc, csize, usize, at = np.empty(m, np.uint32), np.empty(m, np.int64), np.empty(m, np.int64), np.empty(m, np.int64)
    y, mo, d, h, mi, sec = date_time
    dos_date, dos_time = (y - 1980) << 9 | mo << 5 | d, h << 11 | mi << 5 | (sec // 2)
    if threads is None:
        from .configure import effective_cpus
        threads = max(1, min(16, effective_cpus()))
    cap = rows.nbytes + rows.nbytes // 512 + 512 * m + 4096         # an upper bound (deflateBound + .npy header + entry header per member): one call; untouched pages cost nothing
    for _ in range(2):
        buf = np.empty(cap, dtype=np.uint8)
        need = lib.pep_store_tab_members(_ptr(rows), rows.shape[1], None if order is None else _ptr(order), _ptr(off), _ptr(keys), m, dos_time, dos_date, threads,
                                         _ptr(buf), cap, _ptr(crc), _ptr(csize), _ptr(usize), _ptr(at))
        if need < 0:
            raise PepError('pep_store_tab_members failed (%d)' % need)
        if need <= cap:
            return buf[:need], crc, csize, usize, at
        cap = int(need)
    raise PepError('pep_store_tab_members: the entries did not fit the size it had asked for')


_ARGSORT_OK = None


def _argsort_matches_numpy():
    """once per process: does pep_argsort_object_order still leave EQUAL elements where the installed numpy's generic index sort leaves them?  (it restates a private
    routine of numpy - npy_aquicksort - step by step; a release that changes that routine would change the row order of the .tab store silently.)  A few tie-heavy arrays
    of the sizes a genome's rows have; on a difference numpy itself is asked from then on - as _fast_append_ok guards the zip fast path."""
    global _ARGSORT_OK
    if _ARGSORT_OK is None:
        rng = np.random.default_rng(20261003)
        ok = True
        lib = load_library()
        for n, k in ((17, 3), (200, 5), (1500, 30)):
            v = np.ascontiguousarray(rng.integers(0, k, size=n).astype(np.float64))
            out = np.empty(n, dtype=np.int64)
            ok = ok and lib.pep_argsort_object_order(_ptr(v), n, _ptr(out)) == 0 and np.array_equal(out, np.argsort(v.astype(object)))
        _ARGSORT_OK = bool(ok)
    return _ARGSORT_OK


def argsort_object_order(values):
    """np.argsort(values.astype(object)) for float64 values without NaN - the same steps as numpy's generic index sort, on the doubles (pep_argsort_object_order)"""
    v = np.ascontiguousarray(values, dtype=np.float64)
    if (len(v) and np.isnan(v).any()) or not _argsort_matches_numpy():
        return np.argsort(v.astype(object))
    out = np.empty(len(v), dtype=np.int64)
    rc_ = load_library().pep_argsort_object_order(_ptr(v), len(v), _ptr(out))
    if rc_ == -3:                                    # the sort's depth limit: numpy goes on with heapsort there
        return np.argsort(v.astype(object))
    if rc_ != 0:
        raise PepError('pep_argsort_object_order failed (%d)' % rc_)
    return out


def store_tab_archive(rows, off, keys, date_time, threads=None, order=None):
    """pep_store_tab_archive: the .tab store as one complete zip archive (uint8 array), or None when it would need zip64 (>= 65 535 members, >= 4 GiB)"""
    lib = load_library()
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    off, keys = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(keys, dtype=np.int64)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.int64)
    m = len(keys)
    y, mo, d, h, mi, sec = date_time
    dos_date, dos_time = (y - 1980) << 9 | mo << 5 | d, h << 11 | mi << 5 | (sec // 2)
    if threads is None:
        from .configure import effective_cpus
        threads = max(1, min(16, effective_cpus()))
    cap = rows.nbytes + rows.nbytes // 512 + 640 * m + 4096         # an upper bound, as above, plus the directory: one call
    for _ in range(2):
        buf = np.empty(cap, dtype=np.uint8)
        need = lib.pep_store_tab_archive(_ptr(rows), rows.shape[1], None if order is None else _ptr(order), _ptr(off), _ptr(keys), m, dos_time,
                                         dos_date, threads, _ptr(buf), cap)
        if need == -3:
            return None
        if need < 0:
            raise PepError('pep_store_tab_archive failed (%d)' % need)
        if need <= cap:
            return buf[:need]
        cap = int(need)
    raise PepError('pep_store_tab_archive: the archive did not fit the size it had asked for')


def similar_classify(T, q, r, rank_ge, rank_le, near_identity, cover):
    """pep_similar_classify: the row-local tests of PEPPAN.py:244-263 over a HitTable's columns -> (action uint8[n], forward uint8[n], iden4 int32[n])"""
    lib = load_library()
    n = len(T)
    i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
    q, r = i64(q), i64(r)
    cols = [i64(T.qs), i64(T.qe), i64(T.ss), i64(T.se), i64(T.ql), i64(T.sl)]
    iden = np.ascontiguousarray(T.iden, dtype=np.float64)
    ge, le = np.ascontiguousarray(rank_ge, dtype=np.uint8), np.ascontiguousarray(rank_le, dtype=np.uint8)
    action, forward, iden4 = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.int32)
    rc_ = lib.pep_similar_classify(n, _ptr(q), _ptr(r), _ptr(iden), *([_ptr(c) for c in cols] + [_ptr(ge), _ptr(le), near_identity, cover,
                                   _ptr(action), _ptr(forward), _ptr(iden4)]))
    if rc_ != 0:
        raise PepError('pep_similar_classify failed (%d)' % rc_)
    return action, forward, iden4


def similar_scan(q, r, action, forward, iden4, n_genes):
    """pep_similar_scan: the ordered pass of get_similar_pairs (PEPPAN.py:231-276) over numeric columns -> dict(alive, seen_as_query,
    absorbed int64[m, 3], ev_kind, ev_a, ev_b, ev_row_off, ev_rows)"""
    lib = load_library()
    n = len(q)
    q, r = np.ascontiguousarray(q, dtype=np.int64), np.ascontiguousarray(r, dtype=np.int64)
    action, forward = np.ascontiguousarray(action, dtype=np.uint8), np.ascontiguousarray(forward, dtype=np.uint8)
    iden4 = np.ascontiguousarray(iden4, dtype=np.int32)
    alive, seen = np.zeros(max(n_genes, 1), dtype=np.uint8), np.zeros(max(n_genes, 1), dtype=np.uint8)
    absorbed = np.zeros((n + 1, 3), dtype=np.int64)
    ev_kind, ev_a, ev_b = np.zeros(n + 1, dtype=np.uint8), np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    ev_row_off, ev_rows = np.zeros(n + 2, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    na, ne = C.c_uint64(), C.c_uint64()
    rc_ = lib.pep_similar_scan(n, _ptr(q), _ptr(r), _ptr(action), _ptr(forward), _ptr(iden4), n_genes, _ptr(alive), _ptr(seen),
                               _ptr(absorbed), C.byref(na), _ptr(ev_kind), _ptr(ev_a), _ptr(ev_b), _ptr(ev_row_off), _ptr(ev_rows), C.byref(ne))
    if rc_ != 0:
        raise PepError('pep_similar_scan failed (%d)' % rc_)
    ne, na = ne.value, na.value
    off = ev_row_off[:ne + 1].astype(np.int64)
    return dict(alive=alive[:n_genes], seen_as_query=seen[:n_genes], absorbed=absorbed[:na], ev_kind=ev_kind[:ne], ev_a=ev_a[:ne], ev_b=ev_b[:ne],
                ev_row_off=off, ev_rows=ev_rows[:int(off[-1])].astype(np.int64))


def fasta_keep(path, ids):
    """pep_fasta_keep: rewrite the FASTA file so that only records named by one of the integers `ids` stay -> (records, kept), or None when
    a record's name is not a plain decimal integer (file untouched: the caller goes its own way)"""
    lib = load_library()
    ids = np.unique(np.asarray(ids, dtype=np.int64))
    nr, nk = C.c_uint64(), C.c_uint64()
    rc_ = lib.pep_fasta_keep(os.fsencode(path), _ptr(_some(ids)), len(ids), C.byref(nr), C.byref(nk))
    if rc_ == -2:                                   # PEP_ERR_ARG: a name that is not a plain integer, or no such file
        return None
    if rc_ != 0:
        raise PepError('pep_fasta_keep failed (%d)' % rc_)
    return nr.value, nk.value


def fasta_scan(data, table, n_records):
    """pep_fasta_scan: the sequences of FASTA text `data` (bytes) as (codes uint8[total], off uint64[n + 1]) with codes = table[byte], or None when
    the text does not hold exactly n_records records or a sequence holds non-ASCII bytes (the caller then goes its own way)"""
    lib = load_library()
    table = np.ascontiguousarray(table, dtype=np.uint8)
    assert len(table) == 256
    codes = np.empty(max(len(data), 1), dtype=np.uint8)
    off = np.zeros(n_records + 2, dtype=np.uint64)
    nr, high = C.c_uint64(), C.c_int32()
    rc_ = lib.pep_fasta_scan(data, len(data), _ptr(table), _ptr(codes), _ptr(off), n_records, C.byref(nr), C.byref(high))
    if rc_ == -3 or (rc_ == 0 and (nr.value != n_records or high.value)):          # PEP_ERR_LIMIT: more records than the caller counted
        return None
    if rc_ != 0:
        raise PepError('pep_fasta_scan failed (%d)' % rc_)
    return codes[:int(off[n_records])], off[:n_records + 1]


_UPPER = np.frombuffer(bytes(range(256)).upper(), dtype=np.uint8)


_SCRATCH = threading.local()


def fasta_records(data, as_dict=False):
    """pep_fasta_records: the records of FASTA text `data` (ASCII bytes without carriage returns) as (names, text, off): names = list of str (first word
    of every header line), text = all sequences upper-cased and without blanks in one str, off = int64[n + 1] where each record's sequence starts in it.
    None when a header has no name or a sequence holds non-ASCII bytes: the caller then goes its own way.  as_dict: the records as {name: sequence}
    (of two records with one name the later one) instead."""
    lib = load_library()
    # the cleaned sequences land in a scratch buffer this thread keeps (a fresh 10 MB array costs a page fault per 4 KiB - a third of the scan)
    codes = getattr(_SCRATCH, 'codes', None)
    if codes is None or len(codes) < len(data) or not as_dict:
        codes = np.empty(max(len(data), 1), dtype=np.uint8)
        if as_dict and len(data) <= (64 << 20):
            _SCRATCH.codes = codes
    nr, high = C.c_uint64(), C.c_int32()
    cap = max(1024, len(data) // 128)                # (a guess; a file of shorter records is counted and scanned again)
    while True:
        off, name_off, name_len = np.empty(cap + 1, dtype=np.uint64), np.empty(cap, dtype=np.uint64), np.empty(cap, dtype=np.uint32)
        rc_ = lib.pep_fasta_records(data, len(data), _ptr(_UPPER), _ptr(codes), _ptr(off), _ptr(name_off), _ptr(name_len), cap,
                                    C.byref(nr), C.byref(high))
        if rc_ != -3 or cap >= len(data):            # PEP_ERR_LIMIT: more records than guessed
            break
        cap = data.count(b'>') + 1
    if rc_ != 0:
        raise PepError('pep_fasta_records failed (%d)' % rc_)
    n = nr.value
    if high.value or (n and int(name_len[:n].min()) == 0):
        return None
    if as_dict:                                      # {name: sequence} made by one C loop over the buffers (csrc/pyrows.c)
        from .hittable import _pyrows
        return _pyrows().pep_records_dict(data, name_off.ctypes.data, name_len.ctypes.data, codes.ctypes.data, off.ctypes.data, n)
    a = name_off[:n].astype(np.int64)
    b = a + name_len[:n]
    names = [data[x:y].decode('ascii') for x, y in zip(a.tolist(), b.tolist())]
    off = off[:n + 1].astype(np.int64)
    return names, str(codes[:int(off[n])].data, 'ascii'), off


def similar_resolve(ev_kind, ev_a, ev_b, ev_value):
    """pep_similar_resolve: ortho_pairs as the reference's dictionary builds it -> int64[m, 3] (a, b, value), value != 0, insertion order"""
    lib = load_library()
    n = len(ev_kind)
    ev_kind = np.ascontiguousarray(ev_kind, dtype=np.uint8)
    ev_a, ev_b = np.ascontiguousarray(ev_a, dtype=np.int64), np.ascontiguousarray(ev_b, dtype=np.int64)
    ev_value = np.ascontiguousarray(ev_value, dtype=np.int32)
    out = np.zeros((n + 1, 3), dtype=np.int64)
    no = C.c_uint64()
    rc_ = lib.pep_similar_resolve(n, _ptr(ev_kind), _ptr(ev_a), _ptr(ev_b), _ptr(ev_value), _ptr(out), C.byref(no))
    if rc_ != 0:
        raise PepError('pep_similar_resolve failed (%d)' % rc_)
    return out[:no.value]


def merge_hits(hits, cigar, top_k, n_splits, out=None):
    """pep_merge_hits: the union of the hit tables of several TARGET shards (global q / t indices) -> the table of the unsharded
    search: top-k per (q, t mod n_splits) re-applied, rows ordered by (q, t, bin), CIGAR arena compacted.
    `out`: optional dict that keeps the output arrays between calls (the result is then only valid until the next call)."""
    lib = load_library()
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
    if out is None:
        out_h = np.empty(max(len(hits), 1), dtype=HIT_DTYPE)
        out_c = np.empty(max(len(cigar), 1), dtype=np.uint32)
    else:
        if len(out.get('h', ())) < max(len(hits), 1):
            out['h'] = np.empty(int(len(hits) * 1.5) + 64, dtype=HIT_DTYPE)
        if len(out.get('c', ())) < max(len(cigar), 1):
            out['c'] = np.empty(int(len(cigar) * 1.5) + 64, dtype=np.uint32)
        out_h, out_c = out['h'], out['c']
    nh, nc = C.c_uint64(), C.c_uint64()
    rc_ = lib.pep_merge_hits(len(hits), _ptr_or_null(hits), _ptr_or_null(cigar), len(cigar),
                             int(top_k), int(n_splits), _ptr(out_h), _ptr(out_c), C.byref(nh), C.byref(nc))
    if rc_ != 0:
        raise PepError('pep_merge_hits failed (%d)' % rc_)
    return out_h[:nh.value], out_c[:nc.value]


class Context(object):
    """one GPU context (one per process per device; create it AFTER any fork)"""

    def __init__(self, device=0):
        self._lib = load_library()
        if self._lib.pep_device_count() <= 0:
            raise PepError('no HIP device visible: peppan_amd needs an MI355X (there is no CPU fallback)')
        h = C.c_void_p()
        rc = self._lib.pep_ctx_create(int(device), C.byref(h))
        self._h = h
        self._view = None
        self._nt_match_on, self.last_nt_match = False, None
        self._grouping, self.labels = 0, None           # set_grouping: K10 as the tail of every search
        self._totals = {}                    # call_times(which, total=True): slot -> [ms, bytes to the device, bytes to the host], kept by _sum_times
        self.upload_generation = 0           # bumped by every call that replaces a device-resident sequence set (see RunBlast._ensure_nt)
        self.q_nt_token = self.r_nt_token = None     # what the nucleotide sets on the device were made from (set by RunBlast._ensure_nt, cleared by any set_*)
        if rc != 0:
            msg = self._lib.pep_last_error(h).decode() if h else 'pep_ctx_create failed'
            if h:
                self._lib.pep_ctx_destroy(h)
                self._h = None
            raise PepError('pep_ctx_create(%d): %d %s' % (device, rc, msg))
        self.device = device

    def close(self):
        if getattr(self, '_h', None):
            if getattr(self, '_view', None) is not None:
                self._lib.pep_result_free(self._view)
                self._view = None
            self._lib.pep_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            raise PepError('%s failed (%d): %s' % (what, rc, self._lib.pep_last_error(self._h).decode()))

    def _call(self, name, *args):
        """the library's function `name` on this context; PepError with its name, its code and pep_last_error when it fails"""
        rc = getattr(self._lib, name)(self._h, *args)
        if rc != 0:
            self._check(rc, name)

    def _call_on(self, handle, name, *args):
        """the same for a function that takes a result or verdict handle of this context in the context's place"""
        rc = getattr(self._lib, name)(handle, *args)
        if rc != 0:
            self._check(rc, name)

    # ---- inputs
    def set_query_nt(self, seqs, gtable=11):
        self.upload_generation += 1
        self.q_nt_token = None
        nt, off = _pack(seqs)
        self._call('pep_set_query_nt', _ptr(nt), _ptr(off), _count(seqs), gtable)

    def set_ref_nt(self, seqs, frames=6, gtable=11):
        self.upload_generation += 1
        self.r_nt_token = None
        nt, off = _pack(seqs)
        self._call('pep_set_ref_nt', _ptr(nt), _ptr(off), _count(seqs), frames, gtable)

    def set_query_aa(self, seqs):
        self.upload_generation += 1
        self.q_nt_token = None
        aa, off = _pack(seqs)
        self._call('pep_set_query_aa', _ptr(aa), _ptr(off), _count(seqs))

    def set_ref_aa(self, seqs):
        self.upload_generation += 1
        self.r_nt_token = None
        aa, off = _pack(seqs)
        self._call('pep_set_ref_aa', _ptr(aa), _ptr(off), _count(seqs))

    def set_target_groups(self, groups):
        """groups: one non-decreasing id per reference sequence (None / empty clears): batch of reference sets in one search"""
        g = np.ascontiguousarray(groups if groups is not None else [], dtype=np.uint32)
        self._call('pep_set_target_groups', _ptr_or_null(g), len(g))

    def use_nt_as_residues(self, strands=2):
        """the device-resident nucleotide sets themselves become the residue sets (base codes; reference: forward strands, then reverse
        complements, per target group) - the inputs of the nucleotide search.  Until the next translate() / set_*."""
        self._drop_view()
        self._call('pep_use_nt_as_residues', strands)

    def set_timing(self, level):
        """phase timers of the searches (the ms_* statistics): 0 none (default), 1 the score pass only, 2 every phase - each HIP event costs
        the GPU about 6 us of idle time between two kernels"""
        self._call('pep_set_timing', level)

    def set_grouping(self, n_nodes, node_of_target=None, q_base=0):
        """every search of this context ends with single linkage (K10) over its own hit table: edges (hit.q + q_base, node_of_target[hit.t]);
        the labels of the newest search are in self.labels afterwards.  n_nodes = 0 switches it off."""
        nn = np.ascontiguousarray(node_of_target if node_of_target is not None else [], dtype=np.uint32)
        self._call('pep_set_grouping', n_nodes, q_base, _ptr_or_null(nn), len(nn))
        self._grouping = int(n_nodes)
        self.labels = None

    def _take_labels(self, r):
        if getattr(self, '_grouping', 0):
            lab = np.empty(self._grouping, dtype=np.uint32)
            self._call_on(r, 'pep_result_labels', _ptr(lab), self._grouping)
            self.labels = lab

    def invalidate_translation(self):
        """the next search() runs K1 again, inside the search (cheaper than translate(force=True) in front of it: no host wait between K1 and the search)"""
        self._call('pep_invalidate_translation')

    def translate(self, force=False):
        self._call('pep_translate', 1 if force else 0)

    # ---- K1 products
    def _counts(self, count_fn):
        n, r = C.c_uint32(), C.c_uint64()
        self._call(count_fn, C.byref(n), C.byref(r))
        return n.value, r.value

    def _get_meta(self, count_fn, get_fn, dtype):
        out = np.zeros(self._counts(count_fn)[0], dtype=dtype)
        self._call(get_fn, _ptr(out), len(out))
        return out

    def query_meta(self):
        return self._get_meta('pep_query_count', 'pep_get_query_meta', QUERY_META_DTYPE)

    def target_meta(self):
        return self._get_meta('pep_target_count', 'pep_get_target_meta', TARGET_META_DTYPE)

    def _get_aa(self, count_fn, get_fn):
        n, r = self._counts(count_fn)
        codes = np.zeros(max(1, r), dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uint64)
        self._call(get_fn, _ptr(codes), r, _ptr(off))
        return codes[:r], off

    def query_aa(self):
        return self._get_aa('pep_query_count', 'pep_get_query_aa')

    def target_aa(self):
        return self._get_aa('pep_target_count', 'pep_get_target_aa')

    def _drop_view(self):
        if self._view is not None:                      # the handle behind the previous zero-copy views: released first, so that
            self._lib.pep_result_free(self._view)       # the library does not preserve a table nobody may look at any more
            self._view = None

    # ---- search
    def search(self, params=None, copy=True):
        """returns (hits [HIT_DTYPE], cigar uint32 [len<<2|op], stats dict).
        copy=False: the arrays are views of the library's pinned staging memory - no 2 MB copy and no fresh pages - valid only
        until the next search on this context (for callers that consume the table at once, like hits_to_blastab)."""
        self._drop_view()
        r = C.c_void_p()
        self._call('pep_search', C.byref(params) if params is not None else None, C.byref(r))
        try:
            nh, nc = C.c_uint64(), C.c_uint64()
            self._call_on(r, 'pep_result_size', C.byref(nh), C.byref(nc))
            st = Stats()
            self._call_on(r, 'pep_result_stats', C.byref(st))
            self._take_labels(r)
            self.last_nt_match = None
            if self._nt_match_on and nh.value:
                pm = C.c_void_p()
                self._call_on(r, 'pep_result_nt_match', C.byref(pm))
                if pm.value:
                    self.last_nt_match = np.frombuffer((C.c_char * (nh.value * 4)).from_address(pm.value), dtype=np.uint32).copy()
            if copy or nh.value == 0:
                hits = np.empty(nh.value, dtype=HIT_DTYPE)
                cig = np.empty(nc.value, dtype=np.uint32)
                self._call_on(r, 'pep_result_copy', _ptr(hits), _ptr(cig))
            else:
                ph, pc = C.c_void_p(), C.c_void_p()
                self._call_on(r, 'pep_result_data', C.byref(ph), C.byref(pc))
                hits = np.frombuffer((C.c_char * (nh.value * HIT_DTYPE.itemsize)).from_address(ph.value), dtype=HIT_DTYPE)
                cig = (np.frombuffer((C.c_char * (nc.value * 4)).from_address(pc.value), dtype=np.uint32) if nc.value else np.empty(0, np.uint32))
                self._view, r = r, None                 # keep the handle alive while the views may be in use
        finally:
            if r is not None:
                self._lib.pep_result_free(r)
        return hits, cig, {n: getattr(st, n) for n, _ in Stats._fields_}

    def search_on_device(self, params=None):
        """the search with its hit table LEFT ON THE DEVICE: -> (n_hits, n_cigar, stats dict, (address of the hit records, address of the
        CIGAR arena)).  The addresses point into the context's workspace and stay valid until the next search / linclust on this context;
        result_to_host() fetches the table afterwards if somebody wants it after all."""
        if self._view is not None:
            self._lib.pep_result_free(self._view)
            self._view = None
        self._call('pep_set_result_mode', 1)
        r = C.c_void_p()
        try:
            self._call('pep_search', C.byref(params) if params is not None else None, C.byref(r))
        finally:
            self._lib.pep_set_result_mode(self._h, 0)
        nh, nc = C.c_uint64(), C.c_uint64()
        st = Stats()
        ph, pc = C.c_void_p(), C.c_void_p()
        self._view = r
        self._call_on(r, 'pep_result_size', C.byref(nh), C.byref(nc))
        self._call_on(r, 'pep_result_stats', C.byref(st))
        if nh.value:
            self._call_on(r, 'pep_result_device', C.byref(ph), C.byref(pc))
        return nh.value, nc.value, {n: getattr(st, n) for n, _ in Stats._fields_}, (ph.value or 0, pc.value or 0)

    def result_to_host(self):
        """(hits, cigar) of the result search_on_device() is holding"""
        nh, nc = C.c_uint64(), C.c_uint64()
        self._call_on(self._view, 'pep_result_size', C.byref(nh), C.byref(nc))
        hits, cig = np.empty(nh.value, dtype=HIT_DTYPE), np.empty(nc.value, dtype=np.uint32)
        self._call_on(self._view, 'pep_result_copy', _ptr(hits), _ptr(cig))
        return hits, cig

    # ---- K7
    def set_nt_match(self, on):
        """pep_set_nt_match: the searches of this context also count the identical nucleotide columns of every hit (K7's n_match) -> last_nt_match after search()"""
        self._call('pep_set_nt_match', 1 if on else 0)
        self._nt_match_on = bool(on)

    def rescore_nt(self, nt_hits, cigar):
        nt_hits = np.ascontiguousarray(nt_hits, dtype=NT_HIT_DTYPE)
        cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
        out = np.zeros((len(nt_hits), 5), dtype=np.int64)
        if len(nt_hits):
            cg = _some(cigar)
            self._call('pep_rescore_nt', len(nt_hits), _ptr(nt_hits), _ptr(cg), len(cigar), _ptr(out))
        return out

    def rescore_codons(self, nt_hits, cigar, mode, table_id=11):
        """K7 over the codon grid (pep_rescore_codons): the integer counts of rescoring modes 2 / 3 per hit -> int64[n, 7], mode 3
        (hit0, hit1, hit2, paired, n_gap, b_gap, m_gap), mode 2 (aa_match, codons, sub_sum, 0, n_gap, b_gap, m_gap); uberBlast.codon_scores_from_counts
        turns them into identity and score.  The amino-acid and substitution tables of mode 2 are this package's (codon_tables)"""
        args, keep = _codon_args(nt_hits, cigar, mode, codon_tables(table_id) if mode == 2 else None)
        out = np.zeros((len(nt_hits), 7), dtype=np.int64)
        self._call('pep_rescore_codons', *args, _ptr(out if len(out) else np.zeros(7, np.int64)))
        return out

    # ---- K14
    def pair_support(self, rows, cigar, grp_off, grp_qlen, grp_rlen, limits):
        """get_similar (PEPPAN.py:195-224) for groups of forward alignments: rows SUPPORT_ROW_DTYPE, group g = rows [grp_off[g], grp_off[g+1])
        -> int32 per group: SUPPORT_NONE | 0 | int(mean identity * 10000)"""
        rows = np.ascontiguousarray(rows, dtype=SUPPORT_ROW_DTYPE)
        cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
        grp_off = np.ascontiguousarray(grp_off, dtype=np.uint64)
        grp_qlen, grp_rlen = np.ascontiguousarray(grp_qlen, dtype=np.uint32), np.ascontiguousarray(grp_rlen, dtype=np.uint32)
        ng = len(grp_qlen)
        value = np.full(max(ng, 1), SUPPORT_NONE, dtype=np.int32)
        if ng:
            cg = _some(cigar)
            rr = _some(rows)
            self._call('pep_pair_support', len(rows), _ptr(rr), _ptr(cg), len(cigar), ng, _ptr(grp_off), _ptr(grp_qlen), _ptr(grp_rlen), C.byref(limits), _ptr(value))
        return value[:ng]

    # ---- K9
    def linclust(self, seqs, min_id, min_cov, base=4, k=17, m=20):
        """seqs: list of uint8 code arrays, or their (concatenation, uint64 offsets[n + 1]) -> (uint32 representative index per sequence, stats dict)"""
        codes, off = _pack(seqs)
        n = _count(seqs)
        self.upload_generation += 1                     # the gapped stage takes over the packed sequence sets
        rep = np.zeros(n, dtype=np.uint32)
        stats = np.zeros(3, dtype=np.uint64)
        if n:
            self._call('pep_linclust', _ptr(codes), _ptr(off), n, base, k, m, min_id, min_cov, _ptr(rep), _ptr(stats))
        return rep, dict(selected=int(stats[0]), verified=int(stats[1]), accepted=int(stats[2]))

    # ---- K11
    def overlaps(self, contig, start, end, row_id, ovl_l, ovl_p):
        """rows sorted by (contig, start, end) -> int64[m, 3] (id1, id2, overlap) in sweep order"""
        contig = np.ascontiguousarray(contig, dtype=np.int32)
        start, end, row_id = (np.ascontiguousarray(x, dtype=np.int64) for x in (start, end, row_id))
        n = len(contig)
        if n == 0:
            return np.zeros((0, 3), dtype=np.int64)
        m = C.c_uint64()
        cap = max(1024, 4 * n)
        for _ in range(2):
            out = np.zeros((cap, 3), dtype=np.int64)
            self._call('pep_overlaps', n, _ptr(contig), _ptr(start), _ptr(end), _ptr(row_id), ovl_l, ovl_p, _ptr(out), cap, C.byref(m))
            if m.value <= cap:
                return out[:m.value]
            cap = m.value
        raise PepError('pep_overlaps: inconsistent pair count')

    # ---- K12
    def alleles(self, contigs, rows, cigar, grp_off, grp_qlen, gtable=11):
        """contigs: list of ASCII contig strings/bytes; rows: LOCUS_DTYPE records, the rows of group g at [grp_off[g], grp_off[g+1]);
        cigar: uint32 runs len<<2|op -> (in_frame int64[n], orf int64[n], packed uint8[sum ceil(q_len/3)])"""
        rows = np.ascontiguousarray(rows, dtype=LOCUS_DTYPE)
        cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
        grp_off = np.ascontiguousarray(grp_off, dtype=np.uint64)
        grp_qlen = np.ascontiguousarray(grp_qlen, dtype=np.uint32)
        nt, off = _pack(contigs)
        n, ng = len(rows), len(grp_qlen)
        in_frame, orf = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64)
        total = int(((grp_qlen.astype(np.int64) + 2) // 3).sum())
        packed = np.zeros(max(total, 1), dtype=np.uint8)
        cg = _some(cigar)
        self._call('pep_alleles', _ptr(nt), _ptr(off), len(contigs), n, _ptr(rows), _ptr(cg), len(cigar), ng, _ptr(grp_off), _ptr_or_null(grp_qlen), gtable,
                   _ptr(in_frame), _ptr(orf), _ptr(packed), total)
        return in_frame[:n], orf[:n], packed[:total]

    # ---- K15
    def allele_diff(self, packed, row_off, row_len, groups, modes, out_budget=1 << 30):
        """compare_seq / compare_seqX (PEPPAN.py:296-316) for many groups of base-5 packed rows at once.  packed: uint8 concatenation of the
        rows (row r = packed[row_off[r]:row_off[r+1]], ceil(row_len[r] / 3) bytes as the .seq store holds them); groups: one array of row
        indices per group; modes: per group (or one int for all) bit 0 = all pairs a < b, bit 1 = first and last row against all rows.
        -> list of (tri int32[n(n-1)/2, 2] or None, edge int32[2, n, 2] or None), values (mismatch + 1, comparable + 2).
        A batch whose output exceeds `out_budget` bytes (at most the library's PEP_ALLELE_DIFF_MAX_BYTES), or whose bit planes exceed the
        library's budget, goes to the library in several calls, each with the rows its groups use; PepError when one group alone exceeds a
        budget.  The arrays of one library call are views into ONE output buffer: holding any of them keeps that whole buffer alive
        (copy what is to be kept for long)."""
        out_budget = min(int(out_budget), ALLELE_DIFF_MAX_BYTES)
        packed, row_off, row_len, groups = _group_inputs('allele_diff', packed, row_off, row_len, groups)
        modes = np.full(len(groups), modes, dtype=np.uint8) if np.isscalar(modes) else np.ascontiguousarray(modes, dtype=np.uint8).reshape(-1)
        if len(modes) != len(groups):
            raise ValueError('allele_diff: one mode per group')
        n = np.array([len(g) for g in groups], dtype=np.int64)
        tri = np.where((modes & 1) > 0, n * (n - 1) // 2, 0)
        edge = np.where((modes & 2) > 0, 2 * n, 0)
        need = 2 * (tri + edge)                                       # int32 values per group
        results = []
        for lo, hi, whole in _plan_batch('allele_diff', 'output', 4 * need, row_len, groups, out_budget):
            results += self._allele_diff_call(packed, row_off, row_len, groups[lo:hi], modes[lo:hi], n[lo:hi], tri[lo:hi], need[lo:hi], whole)
        return results

    def _allele_diff_call(self, packed, row_off, row_len, groups, modes, n, tri, need, whole):
        if not whole and len(groups):
            # part of a split batch: upload the rows these groups use, not the whole table
            packed, row_off, row_len, groups = _rows_of_groups(packed, row_off, row_len, groups, n)       # (indices are in range: allele_diff sends a batch with a bad one whole)
        pk, rl, grp_off, grp_rows, md = _group_tables(packed, row_len, groups, (modes,))
        out_off = np.concatenate([[0], np.cumsum(need)]).astype(np.uint64)
        total = int(out_off[-1])
        out = np.empty(max(total, 1), dtype=np.int32)
        self._call('pep_allele_diff', _ptr(pk), _ptr(row_off), _ptr(rl), len(row_len), len(groups), _ptr(grp_off), _ptr(grp_rows), _ptr(md),
                   _ptr(out), _ptr(out_off), total)
        res = []
        for g in range(len(groups)):
            a, ng = int(out_off[g]), int(n[g])
            t = out[a:a + 2 * int(tri[g])].reshape(-1, 2) if modes[g] & 1 else None
            e = out[a + 2 * int(tri[g]):int(out_off[g + 1])].reshape(2, ng, 2) if modes[g] & 2 else None
            res.append((t, e))
        return res

    def call_times(self, which, total=False):
        """pep_call_times of slot `which` (CALL_*) -> (ms float64[CALL_MS], bytes to the device, bytes to the host): the kernel times, measured when
        set_timing(2) is on and zeros otherwise, and the bytes moved, as the slot's section of include/peppan_hip.h states them.  total=False: of the
        newest library call of the slot.  total=True: summed over the library calls that the newest wrapper call of the slot made - a wrapper that
        splits its batch (group_verdicts, kimura_pairs, nj_trees, tree_cuts) makes several, the wrappers of K21 - K26 that do not split make one;
        zeros for a wrapper call that failed, and for the slots whose wrappers keep no sum (K15, K17 - K20)."""
        if total:
            ms, to_device, to_host = self._totals.get(which, (np.zeros(CALL_MS), 0, 0))
            return ms.copy(), to_device, to_host
        t = CallTimes()
        self._call('pep_call_times', which, C.byref(t))
        return np.array(t.ms[:]), int(t.bytes_to_device), int(t.bytes_to_host)

    def _sum_times(self, which, start=False):
        """keeps the total of slot `which`: start=True as a wrapper call begins (zeros), otherwise after each of its library calls (adds that call's record)"""
        if start:
            self._totals[which] = [np.zeros(CALL_MS), 0, 0]
        else:
            self._totals[which] = [a + b for a, b in zip(self._totals[which], self.call_times(which))]

    def allele_diff_times(self):
        """of the newest allele_diff library call, in ms: (allele_planes, allele_diff) kernel times when set_timing(2) is on, else zeros, and the
        host's wall time from the end of the kernels until the output lay in the caller's buffer"""
        return tuple(self.call_times(CALL_ALLELE_DIFF)[0][:3].tolist())

    # ---- K16
    def group_verdicts(self, packed, row_off, row_len, groups, genomes, inparalog, gd, self_id, detail=True, out_budget=1 << 30):
        """The divergence verdicts of filt_per_group (PEPPAN.py:335-344, 352-366, 371-392) for many groups at once, decided on the GPU.  Rows and
        groups as for allele_diff; genomes: per group the genome id of every row; inparalog: one flag per group; gd: (keys, values, default) as
        orthofilter.gd_table makes them.  -> per group (verdict, tri, leader): verdict 0 not divergent / 1 divergent, no pair beyond its bound /
        2 a pair beyond; for verdict 2 and detail=True tri int32[n(n-1)/2, 2] (K15's packed upper triangle) and leader uint32[n] (the row that
        leads row j in the reference's leader grouping), else None.  Only those leave the device per pair; the verdicts cost one byte a group.
        The packed triangles are reserved on the device for EVERY group, so a batch whose triangles exceed `out_budget` bytes, or whose bit
        planes exceed the library's budget, is split exactly as allele_diff splits; the results do not depend on where."""
        out_budget = min(int(out_budget), ALLELE_DIFF_MAX_BYTES)
        packed, row_off, row_len, groups, genomes, inparalog = _verdict_inputs(packed, row_off, row_len, groups, genomes, inparalog)
        n = np.array([len(g) for g in groups], dtype=np.int64)
        plan = _plan_batch('group_verdicts', 'triangle', 8 * (n * (n - 1) // 2), row_len, groups, out_budget)
        results = []
        self._sum_times(CALL_GROUP_VERDICTS, start=True)
        for lo, hi, whole in plan:
            results += self._group_verdicts_call(packed, row_off, row_len, groups[lo:hi], genomes[lo:hi], inparalog[lo:hi], gd, self_id, detail, n[lo:hi], whole)
        return results

    def _group_verdicts_call(self, packed, row_off, row_len, groups, genomes, inparalog, gd, self_id, detail, n, whole):
        if not whole and len(groups) and int(n.sum()):
            packed, row_off, row_len, groups = _rows_of_groups(packed, row_off, row_len, groups, n)
        args, keep = _verdict_tables(packed, row_off, row_len, groups, genomes, inparalog, gd)
        verdict = np.zeros(max(len(groups), 1), dtype=np.uint8)
        handle = C.c_void_p()
        self._call('pep_group_verdicts', *args, self_id, _ptr(verdict), C.byref(handle))
        try:
            res = []
            for g in range(len(groups)):
                tri = leader = None
                if detail and verdict[g] == 2:
                    pairs = C.c_uint64()
                    self._call_on(handle, 'pep_verdict_detail_size', g, C.byref(pairs))
                    tri, leader = np.empty((pairs.value, 2), dtype=np.int32), np.empty(int(n[g]), dtype=np.uint32)
                    self._call_on(handle, 'pep_verdict_detail_copy', g, _ptr(tri), _ptr(leader))
                res.append((int(verdict[g]), tri, leader))
            self._sum_times(CALL_GROUP_VERDICTS)          # (after the detail copies: their bytes count)
        finally:
            self._lib.pep_verdict_result_free(handle)
        return res

    def group_verdicts_times(self):
        """of the newest pep_group_verdicts library call: (float64[4] kernel times in ms - bit planes, edge, pairs, leaders - when set_timing(2) is on,
        else zeros; bytes that call and the detail copies of its result sent to the host)"""
        ms, _, to_host = self.call_times(CALL_GROUP_VERDICTS)
        return ms[:4], to_host

    def group_verdicts_totals(self):
        """the same two figures summed over the library calls of the newest group_verdicts (one per part of a split batch)"""
        ms, _, to_host = self.call_times(CALL_GROUP_VERDICTS, total=True)
        return ms[:4], to_host

    # ---- K17
    def gene_ingroups(self, genome, iden, score, gene_off, gd, self_id, thr):
        """determineGroup (PEPPAN.py:1041-1056) and the gene score of initializing2 (:1074) for many genes at once.  Gene g is rows
        gene_off[g] .. gene_off[g+1] of genome / iden / score (columns 1, 4 after :1070, 2 of its table in the order of :1069); gd: (keys, vals,
        default) as orthofilter.gd_table makes them with allowed_sigma = nSigma; thr = (min_iden - 0.02) * 10000.
        -> (keep bool[n_rows], gene_score int64[n_genes])"""
        args, n_rows, n_genes, keep_alive = _ingroup_tables(genome, iden, score, gene_off, gd)
        keep = np.zeros(max(n_rows, 1), dtype=np.uint8)
        gene_score = np.zeros(max(n_genes, 1), dtype=np.int64)
        self._call('pep_gene_ingroups', *args, self_id, thr, _ptr(keep), _ptr(gene_score))
        return keep[:n_rows].astype(bool), gene_score[:n_genes]

    def gene_ingroups_times(self):
        """of the newest pep_gene_ingroups: (float64[2] kernel times in ms - pairs, finish - when set_timing(2) is on, else zeros; bytes the call sent to the host)"""
        ms, _, to_host = self.call_times(CALL_GENE_INGROUPS)
        return ms[:2], to_host

    # ---- K18
    def synteny_pairs(self, member_off, genome, nb_off, nb, n_neighbor):
        """the pair loop of ite_synteny_resolver (PEPPAN.py:1101-1117) for a batch of paralogous names.  Group g is members member_off[g] ..
        member_off[g+1] of genome and of the neighbour lists nb[nb_off[i] .. nb_off[i+1]] (strictly ascending).
        -> (has_conflict bool[G], dc int32[G], conf_off int64[G+1], conf uint32[., 2], walk_off int64[G+1], walk uint32[., 2]): the conflict pairs
        (m, k) ascending and the pairs with d < dc in the order (d, flag, m, k), as include/peppan_hip.h states them"""
        args, n_groups, keep_alive = _synteny_tables(member_off, genome, nb_off, nb, n_neighbor)
        has, dc = np.zeros(max(n_groups, 1), np.uint8), np.zeros(max(n_groups, 1), np.int32)
        conf_off, walk_off = np.zeros(n_groups + 1, np.uint64), np.zeros(n_groups + 1, np.uint64)
        self._call('pep_synteny_pairs', *args, _ptr(has), _ptr(dc), _ptr(conf_off), _ptr(walk_off))
        n_conf, n_walk = int(conf_off[-1]), int(walk_off[-1])
        conf, walk = np.zeros((max(n_conf, 1), 2), np.uint32), np.zeros((max(n_walk, 1), 2), np.uint32)
        self._call('pep_synteny_pairs_copy', _ptr(conf), n_conf, _ptr(walk), n_walk)
        return has[:n_groups].astype(bool), dc[:n_groups], conf_off.astype(np.int64), conf[:n_conf], walk_off.astype(np.int64), walk[:n_walk]

    def synteny_times(self):
        """of the newest pep_synteny_pairs: (float64[3] kernel times in ms - count, scans, emit - when set_timing(2) is on, else zeros; bytes it sent to the host)"""
        ms, _, to_host = self.call_times(CALL_SYNTENY_PAIRS)
        return ms[:3], to_host

    # ---- K19
    def gene_structure(self, nt, seq_off, seq, win_off, win_len, flags, lp, allowed_vary, ref_len, table4=False):
        """determineGeneStructure (PEPPAN.py:1193-1229) for a batch of predictions.  nt: the nucleotide set as ASCII bytes (bytes or uint8 array), sequence i
        at nt[seq_off[i] .. seq_off[i+1]].  Prediction p reads win_len[p] nucleotides from the 0-based win_off[p] of sequence seq[p]; flags[p]: bit 0 = read
        backward and complemented, bits 1-3 = the tried frames 0, 1, 2.  table4: TGA is no stop.
        -> (frame int32[n]: the lowest tried frame that is a CDS or -1; start_aa, stop_aa uint32[n]: of that frame, of the first tried one when there is
        none, GENESTRUCT_NO_STOP without a stop; kind uint8[n]: the outcome of the first tried frame, an index of GENESTRUCT_KINDS), as
        include/peppan_hip.h states them"""
        nt = _as_bytes(nt)
        args, n, keep_alive = _genestruct_tables(seq_off, seq, win_off, win_len, flags, lp, allowed_vary, ref_len)
        if len(nt) != int(keep_alive[0][-1]):
            raise ValueError('gene_structure: seq_off must end at the length of nt')
        frame, kind = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8)
        start_aa, stop_aa = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        self._call('pep_gene_structure', _ptr(_some(nt)), *args, 1 if table4 else 0, _ptr(frame), _ptr(start_aa), _ptr(stop_aa), _ptr(kind))
        return frame[:n], start_aa[:n], stop_aa[:n], kind[:n]

    def gene_structure_times(self):
        """of the newest pep_gene_structure: (kernel time in ms when set_timing(2) is on, else 0; bytes it sent to the device; bytes it sent to the host)"""
        ms, to_device, to_host = self.call_times(CALL_GENE_STRUCTURE)
        return float(ms[0]), to_device, to_host

    # ---- K20
    def rarefaction_curves(self, bits, n_genes, orders):
        """the loop of writeCurve (PEPPAN_parser.py:74-80).  bits: the presence matrix as bit rows uint64[n_genomes, W] (pack_presence), n_genes its genes,
        orders: [n_iter, n_genomes], every row a permutation of the genomes.
        -> int64[n_genomes, n_iter, 2]: genes in at least one / in all of the first k + 1 genomes of order t at [k, t], the reference's `curves`, as
        include/peppan_hip.h states them"""
        args, n, n_iter, keep_alive = _curve_tables(bits, n_genes, orders)
        curves = np.zeros((max(n, 1), max(n_iter, 1), 2), np.int32)
        self._call('pep_rarefaction_curves', *args, _ptr(curves))
        return curves[:n, :n_iter].astype(np.int64)

    def profile_pairs(self, profiles):
        """the pair loop of getDistance (PEPPAN_parser.py:172-179).  profiles: int32[n, n_genes], > 0 an allele.
        -> (shared, presence) int32[n, n], symmetric with a zero diagonal: the genes both profiles carry with the same allele / carry at all"""
        profiles = np.asarray(profiles)
        if profiles.ndim != 2:
            raise ValueError('profile_pairs: a matrix [n, n_genes]')
        if profiles.dtype != np.int32:
            if profiles.size and profiles.dtype.kind not in 'iu':
                raise ValueError('profile_pairs: profiles must hold integers')
            if profiles.size and (int(profiles.min()) < -2 ** 31 or int(profiles.max()) >= 2 ** 31):
                raise ValueError('profile_pairs: profiles holds values outside int32')
            profiles = profiles.astype(np.int32)
        profiles = np.ascontiguousarray(profiles)
        n, n_genes = profiles.shape
        if n >= 1 << 32:
            raise ValueError('profile_pairs: more than 2^32 - 1 profiles in one call')
        shared, presence = np.zeros((max(n, 1), max(n, 1)), np.int32), np.zeros((max(n, 1), max(n, 1)), np.int32)
        self._call('pep_profile_pairs', _ptr(_some(profiles.reshape(-1))), n, n_genes, _ptr(shared), _ptr(presence))
        shared, presence = shared[:n, :n], presence[:n, :n]
        return shared + shared.T, presence + presence.T                  # (the library stores the pairs i < j)

    def parser_times(self):
        """of the newest pep_rarefaction_curves and pep_profile_pairs: (their kernel times in ms when set_timing(2) is on, else 0; bytes the newer of the two
        calls sent to the device; bytes it sent to the host)"""
        ms, to_device, to_host = self.call_times(CALL_PARSER)
        return float(ms[0]), float(ms[1]), to_device, to_host

    # ---- K21
    def kimura_pairs(self, packed, row_off, row_len, groups, out_budget=1 << 30):
        """the three pair counts of Kimura's distance, which `rapidnj -i fa` computes (PEPPAN.py:19, 409-417).  Rows and groups as for allele_diff.
        -> per group int32[n (n - 1) / 2, 3]: (comparable columns, transitions, transversions) of every pair a < b in the row-major order of allele_diff's
        packed triangle.  A batch beyond `out_budget` bytes of counts (at most the library's PEP_NJ_MAX_BYTES) or the library's budget of bit planes goes to
        the library in several calls.  The kernel times: call_times(CALL_KIMURA_PAIRS, total=True)."""
        out_budget = min(int(out_budget), NJ_MAX_BYTES)
        packed, row_off, row_len, groups = _group_inputs('kimura_pairs', packed, row_off, row_len, groups)
        n = np.array([len(g) for g in groups], dtype=np.int64)
        need = 3 * (n * (n - 1) // 2)                                 # int32 values per group
        results = []
        self._sum_times(CALL_KIMURA_PAIRS, start=True)
        for lo, hi, whole in _plan_batch('kimura_pairs', 'pair counts', 4 * need, row_len, groups, out_budget):
            pk, ro, rl, gr = packed, row_off, row_len, groups[lo:hi]
            if not whole and len(gr):
                pk, ro, rl, gr = _rows_of_groups(pk, ro, rl, gr, n[lo:hi])
            n_rows = len(rl)
            pk, rl, grp_off, grp_rows = _group_tables(pk, rl, gr)
            out_off = np.concatenate([[0], np.cumsum(need[lo:hi])]).astype(np.uint64)
            out = np.empty(max(int(out_off[-1]), 1), dtype=np.int32)
            self._call('pep_kimura_pairs', _ptr(pk), _ptr(ro), _ptr(rl), n_rows, len(gr), _ptr(grp_off), _ptr(grp_rows),
                       _ptr(out), _ptr(out_off), int(out_off[-1]))
            self._sum_times(CALL_KIMURA_PAIRS)
            results += [out[int(out_off[g]):int(out_off[g + 1])].reshape(-1, 3) for g in range(len(gr))]
        return results

    def nj_trees(self, matrices):
        """neighbour joining (what rapidnj does for PEPPAN.py:416 and PEPPAN_parser.py:168) over a list of square float64 distance matrices, of which the
        entries with row < column are read.  -> per matrix (node uint32[2 n - 3], length float64[2 n - 3]) as include/peppan_hip.h states them: for
        every join the two joined node ids and their branch lengths, then the last three nodes; two entries for n = 2.  Batches beyond the library's
        PEP_NJ_MAX_BYTES of matrices go to it in several calls.  The kernel times: call_times(CALL_NJ_TREES, total=True)."""
        mats = [np.ascontiguousarray(m, dtype=np.float64) for m in matrices]
        for t, m in enumerate(mats):
            if m.ndim != 2 or m.shape[0] != m.shape[1]:
                raise ValueError('nj_trees: matrix %d is %s, not square' % (t, m.shape))
        results = []
        self._sum_times(CALL_NJ_TREES, start=True)
        for lo, hi in _calls_within([m.size * 8 for m in mats], NJ_MAX_BYTES):
            results += self._nj_trees_call(mats[lo:hi])
        return results

    def _nj_trees_call(self, mats):
        n = np.array([m.shape[0] for m in mats], dtype=np.uint32)
        dist_off = np.concatenate([[0], np.cumsum(n.astype(np.int64) ** 2)]).astype(np.uint64)
        out_off = np.concatenate([[0], np.cumsum(np.where(n == 2, 2, 2 * n.astype(np.int64) - 3))]).astype(np.uint64)
        _check_only('pep_nj_trees_check', _ptr(n), len(n), _ptr(dist_off), _ptr(out_off))       # (before the copy below: a tree of one leaf would lay the offsets out wrongly)
        dist = np.concatenate([m.reshape(-1) for m in mats])
        node, length = np.zeros(int(out_off[-1]), np.uint32), np.zeros(int(out_off[-1]), np.float64)
        self._call('pep_nj_trees', _ptr(dist), _ptr(dist_off), _ptr(n), len(n), _ptr(node), _ptr(length), _ptr(out_off))
        self._sum_times(CALL_NJ_TREES)
        return [(node[int(a):int(b)], length[int(a):int(b)]) for a, b in zip(out_off[:-1], out_off[1:])]

    # ---- K25
    def tree_cuts(self, sets, lengths, w0, w1, strong, cap=CUT_DEFAULT_CAP, path=CUT_AUTO):
        """the tree cutting of filt_per_group (PEPPAN.py:424-482) for a batch of trees, as include/peppan_hip.h states it.  Per tree: sets uint64[B, words],
        the leaves on one side of every branch as bits; lengths float64[B]; w0, w1 float64[n, n], incompatible[:, :, 0] and [:, :, 1] compacted to the leaves;
        strong bool[n]; cap: the iterations per component, one number or one per tree; path: CUT_AUTO, CUT_BLOCK, CUT_CHAIN.
        -> per tree (part int32[n]: the leaf's component in the reference's output order, -1 for a dropped leaf; n_parts; n_cuts; n_ties; log_where
        int32[n_cuts, 2]: component and lowest inducing branch of every cut; log_val float64[n_cuts, 4]: s0, s1, m, key).  Batches beyond the library's
        PEP_NJ_MAX_BYTES of one matrix go to it in several calls.  The kernel times: call_times(CALL_TREE_CUT, total=True)."""
        w0 = [np.ascontiguousarray(m, dtype=np.float64) for m in w0]
        w1 = [np.ascontiguousarray(m, dtype=np.float64) for m in w1]
        n_trees = len(w0)
        if not (len(sets) == len(lengths) == len(w1) == len(strong) == n_trees):
            raise ValueError('tree_cuts: one entry per tree in every list')
        for t in range(n_trees):
            if w0[t].ndim != 2 or w0[t].shape[0] != w0[t].shape[1] or w1[t].shape != w0[t].shape:
                raise ValueError('tree_cuts: the matrices of tree %d are %s and %s, not two squares of one size' % (t, w0[t].shape, w1[t].shape))
        caps = np.broadcast_to(np.asarray(cap, dtype=np.int64), (n_trees,))
        if n_trees and (caps.min() < 0 or caps.max() >= 1 << 32):
            raise ValueError('tree_cuts: cap is 0 .. 2^32 - 1')
        results = []
        self._sum_times(CALL_TREE_CUT, start=True)
        for lo, hi in _calls_within([m.size * 8 for m in w0], NJ_MAX_BYTES):
            results += self._tree_cuts_call(sets[lo:hi], lengths[lo:hi], w0[lo:hi], w1[lo:hi], strong[lo:hi], caps[lo:hi], path)
        return results

    def _tree_cuts_call(self, sets, lengths, w0, w1, strong, caps, path):
        n, leaf_off, mat_off, branch_off, set_off, flat = _tree_cut_tables([len(m) for m in w0], sets)
        _check_only('pep_tree_cut_check', _ptr(n), len(n), _ptr(leaf_off), _ptr(mat_off), _ptr(branch_off), _ptr(set_off), _ptr(flat), int(path))
        lengths = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in lengths]
        strong = [np.ascontiguousarray(x).astype(bool).astype(np.uint8).reshape(-1) for x in strong]
        for t in range(len(n)):
            if len(lengths[t]) != int(branch_off[t + 1] - branch_off[t]) or len(strong[t]) != int(n[t]):
                raise ValueError('tree_cuts: tree %d needs one length per branch and one strong flag per leaf' % t)
        length, w0, w1, strong = (np.concatenate([x.reshape(-1) for x in xs]) for xs in (lengths, w0, w1, strong))
        caps = np.ascontiguousarray(caps, dtype=np.uint32)
        n_leaf = int(leaf_off[-1])
        part, counts = np.full(n_leaf, -1, np.int32), np.zeros((len(n), 4), np.int32)
        log_where, log_val = np.zeros((n_leaf, 2), np.int32), np.zeros((n_leaf, 4), np.float64)
        self._call('pep_tree_cut', _ptr(n), len(n), _ptr(leaf_off), _ptr(mat_off), _ptr(branch_off), _ptr(set_off), _ptr(flat), _ptr(length), _ptr(w0), _ptr(w1),
                   _ptr(strong), _ptr(caps), int(path), _ptr(part), _ptr(counts), _ptr(log_where), _ptr(log_val))
        self._sum_times(CALL_TREE_CUT)
        out = []
        for t, (a, b) in enumerate(zip(leaf_off[:-1], leaf_off[1:])):
            a, cuts = int(a), int(counts[t, 1])
            out.append((part[a:int(b)], int(counts[t, 0]), cuts, int(counts[t, 2]), log_where[a:a + cuts], log_val[a:a + cuts]))
        return out

    # ---- K26
    def batch_screen(self, gene_off, col3, locus, used_state, threshold):
        """stage A of K26 in include/peppan_hip.h (PEPPAN.py:548-562) for a batch of genes: column 3 and the locus ids of their tables one behind the other,
        used_state uint8[n_loci] (0 absent, 1 present and <= 0, 2 present and > 0), threshold = (clust_identity - 0.02) * 10000 -> (column 3 rewritten, column 4,
        present_iden int64[n_genes], excluded uint8[n_genes]).  The kernel time: call_times(CALL_BATCH_SCREEN, total=True)."""
        gene_off, (col3, locus) = _prep_offsets('batch_screen', gene_off, (col3, locus))
        used_state = np.ascontiguousarray(used_state, dtype=np.uint8).reshape(-1)
        n, n_rows = len(gene_off) - 1, int(gene_off[-1])
        out3, out4 = np.zeros(max(n_rows, 1), np.int64), np.zeros(max(n_rows, 1), np.int64)
        present, excluded = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.uint8)
        self._sum_times(CALL_BATCH_SCREEN, start=True)
        self._call('pep_batch_screen', n, _ptr(gene_off), _ptr(_some(col3)), _ptr(_some(locus)), _ptr(_some(used_state)), len(used_state), float(threshold),
                   _ptr(out3), _ptr(out4), _ptr(present), _ptr(excluded))
        self._sum_times(CALL_BATCH_SCREEN)
        return out3[:n_rows], out4[:n_rows], present[:n], excluded[:n]

    def batch_prune(self, mode, gene_off, genome, col2, col3, col4, locus, cfl_off, cfl, n_loci, clust_identity, final_threshold, path=PREP_AUTO):
        """stage C of K26 in include/peppan_hip.h (PEPPAN.py:596-624, :641-656) for a batch of genes: columns 1 - 5 of their tables one behind the other, the
        conflict lists as CSR over the rows, final_threshold = 10000 * clust_identity -> (out_off uint64[n_genes + 1], rows int32: per gene the source rows left
        in final order, inparalog uint8[n_genes], final uint8[n_genes], n_ties).  mode: PREP_NJ, PREP_SBH; path: PREP_AUTO, PREP_LDS, PREP_WS.  The kernel time:
        call_times(CALL_BATCH_PRUNE, total=True)."""
        gene_off, cols, cfl_off, cfl = _prep_offsets('batch_prune', gene_off, (genome, col2, col3, col4, locus), cfl_off, cfl)
        n, n_rows = len(gene_off) - 1, int(gene_off[-1])
        out_off, rows = np.zeros(n + 1, np.uint64), np.zeros(max(n_rows, 1), np.int32)
        inparalog, final, n_ties = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8), np.zeros(1, np.uint64)
        self._sum_times(CALL_BATCH_PRUNE, start=True)
        self._call('pep_batch_prune', int(mode), n, _ptr(gene_off), *[_ptr(_some(c)) for c in cols], _ptr(cfl_off), _ptr(_some(cfl)), int(n_loci),
                   float(clust_identity), float(final_threshold), int(path), _ptr(out_off), _ptr(rows), _ptr(inparalog), _ptr(final), _ptr(n_ties))
        self._sum_times(CALL_BATCH_PRUNE)
        return out_off, rows[:int(out_off[-1])], inparalog[:n], final[:n], int(n_ties[0])

    # ---- K23
    def cds_genes(self, nt, contig_off, contig, win_off, win_len, strand, min_cds=0, mask=0, table4=False):
        """checkPseu (PEPPAN.py:992-1010) and the SHA-1 of the kept (:178, :1020) for a batch of CDS, as include/peppan_hip.h states them.  nt: the contigs
        as upper-cased ASCII bytes (bytes or uint8 array), contig c at nt[contig_off[c] .. contig_off[c+1]].  CDS p is win_len[p] bytes from the 0-based
        win_off[p] of contig contig[p], read backward and complemented when strand[p] is 1.  min_cds: 0 .. 2^31; mask: CDS_ALLOW bits; table4: TGA is no stop.
        -> (code uint8[n]: 0 .. 5; digest uint8[n, 20]: hashlib.sha1(text).digest() where the code is 0, zeros elsewhere).  The kernel times:
        call_times(CALL_CDS_GENES, total=True)."""
        nt = _as_bytes(nt)
        args, n, keep_alive = _cds_tables(contig_off, contig, win_off, win_len, strand)
        if len(nt) != int(keep_alive[0][-1]):
            raise ValueError('cds_genes: contig_off must end at the length of nt')
        if not 0 <= int(min_cds) <= CDS_MAX_WINDOW or not 0 <= int(mask) < 1 << 32:
            raise ValueError('cds_genes: min_cds is 0 .. 2^31, mask 32 bits')
        code, digest = np.zeros(max(n, 1), np.uint8), np.zeros((max(n, 1), 20), np.uint8)
        self._sum_times(CALL_CDS_GENES, start=True)
        self._call('pep_cds_genes', _ptr(_some(nt)), *args, int(min_cds), int(mask), 1 if table4 else 0, _ptr(code), _ptr(digest))
        self._sum_times(CALL_CDS_GENES)
        return code[:n], digest[:n]

    # ---- K24
    def out_alleles(self, nt, contig_off, seed_contig, rows, look9=None, plan_only=False, key_bits=0):
        """the allele pass of write_output (PEPPAN.py:1391-1472) for a prediction table, as include/peppan_hip.h states it.  nt: the contigs - and behind
        them the representatives, one contig each - as ASCII bytes (bytes or uint8 array), contig c at nt[contig_off[c] .. contig_off[c+1]]; seed_contig[g]: the
        contig that is gene g's representative, -1 for none; rows int32[n, OUTA_COLS]: the row records; look9 (optional, int32[n]): column 9 as the rows of
        earlier batches show it to the '-' rows at the head of a batch.
        -> (plan int32[n, OUTA_PLAN_COLS]: class, s2, e2, lp, a, len; first int32[n]; rank uint32[n]; tflag uint8[n]).  plan_only: the plan alone, nt is not read
        (None will do) and the other three are None.  key_bits: for tests of the comparison pass alone.  The kernel times:
        call_times(CALL_OUT_ALLELES, total=True)."""
        args, n, keep_alive = _outalleles_tables(contig_off, seed_contig, rows, look9)
        if not 0 <= int(key_bits) < 1 << 32:
            raise ValueError('out_alleles: key_bits is 0 .. 31')
        plan = np.zeros((max(n, 1), OUTA_PLAN_COLS), np.int32)
        self._sum_times(CALL_OUT_ALLELES, start=True)
        if plan_only:
            self._call('pep_out_alleles', None, *args, 1, int(key_bits), _ptr(plan), None, None, None)
            self._sum_times(CALL_OUT_ALLELES)
            return plan[:n], None, None, None
        nt = _as_bytes(nt)
        if len(nt) != int(keep_alive[0][-1]):
            raise ValueError('out_alleles: contig_off must end at the length of nt')
        first, rank, tflag = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint8)
        self._call('pep_out_alleles', _ptr(_some(nt)), *args, 0, int(key_bits), _ptr(plan), _ptr(first), _ptr(rank), _ptr(tflag))
        self._sum_times(CALL_OUT_ALLELES)
        return plan[:n], first[:n], rank[:n], tflag[:n]

    # ---- K22
    def global_diff(self, events, arena, n_genomes, table, chunk_items=0):
        """the genome-pair sums of get_global_difference (PEPPAN.py:1637-1645, 1650-1662) as include/peppan_hip.h states them.  events int64[n, 6] and
        arena as global_diff_walk leaves them, table float64[10050] the logarithm of every value code.  -> (g1, g2, n, mean, var): per genome pair, in the
        order the reference's dictionary first meets them, the two ranks g1 <= g2, the number of values, numpy's mean of their logarithms and of the squared
        deviations.  chunk_items (0 = the library's default) does not change the result.  The kernel times:
        call_times(CALL_GLOBAL_DIFF, total=True)."""
        events, arena = _gdiff_tables(events, arena)
        table = np.ascontiguousarray(table, dtype=np.float64).reshape(-1)
        if len(table) != GDIFF_TABLE:
            raise ValueError('global_diff: the table has %d entries, not %d' % (len(table), GDIFF_TABLE))
        n_keys = C.c_uint64()
        self._sum_times(CALL_GLOBAL_DIFF, start=True)
        self._call('pep_global_diff', _ptr_or_null(events), len(events), _ptr_or_null(arena), len(arena), int(n_genomes), _ptr(table), int(chunk_items),
                   C.byref(n_keys))
        self._sum_times(CALL_GLOBAL_DIFF)
        k = n_keys.value
        g1, g2, n = np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.uint64)
        mean, var = np.zeros(k, dtype=np.float64), np.zeros(k, dtype=np.float64)
        self._call('pep_global_diff_copy', k, _ptr_or_null(g1), _ptr_or_null(g2), _ptr_or_null(n), _ptr_or_null(mean), _ptr_or_null(var))
        return g1, g2, n, mean, var

    # ---- K13
    def sha1(self, seqs):
        """list of str / bytes -> uint8[n, 20] SHA-1 digests (hashlib.sha1(s).digest() of each)"""
        data, off = _pack(seqs)
        out = np.zeros((max(len(seqs), 1), 20), dtype=np.uint8)
        if len(seqs):
            self._call('pep_sha1', _ptr(data), _ptr(off), len(seqs), _ptr(out))
        return out[:len(seqs)]

    def dedup(self, lengths, digests):
        """genes in priority order -> uint32 rep[i] = first gene of the same (length run, digest); rep[i] == i for the ones kept"""
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        digests = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 20)
        assert len(lengths) == len(digests)
        rep = np.zeros(max(len(lengths), 1), dtype=np.uint32)
        if len(lengths):
            self._call('pep_dedup', len(lengths), _ptr(lengths), _ptr(digests), _ptr(rep))
        return rep[:len(lengths)]

    # ---- K10
    def components_of_hits(self, n_nodes, hits, node_of_target, q_base=0):
        """labels of the graph with one edge (hit.q + q_base, node_of_target[hit.t]) per hit"""
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        node_of_target = np.ascontiguousarray(node_of_target, dtype=np.uint32)
        lab = np.zeros(n_nodes, dtype=np.uint32)
        if n_nodes:
            hh = _some(hits)
            nn = _some(node_of_target)
            self._call('pep_components_of_hits', n_nodes, len(hits), _ptr(hh), q_base, _ptr(nn), len(node_of_target), _ptr(lab))
        return lab

    def components_of_search(self, n_nodes, node_of_target, q_base=0):
        """labels of the graph with one edge (hit.q + q_base, node_of_target[hit.t]) per hit of the NEWEST search(copy=False) on this context,
        read from the table's device copy (pep_components_of_result)"""
        if self._view is None:
            raise PepError('components_of_search: no search result is held (call search(copy=False) first)')
        node_of_target = np.ascontiguousarray(node_of_target, dtype=np.uint32)
        lab = np.zeros(n_nodes, dtype=np.uint32)
        if n_nodes:
            nn = _some(node_of_target)
            self._call('pep_components_of_result', self._view, n_nodes, q_base, _ptr(nn), len(node_of_target), _ptr(lab))
        return lab

    def components(self, n_nodes, a, b):
        a = np.ascontiguousarray(a, dtype=np.uint32)
        b = np.ascontiguousarray(b, dtype=np.uint32)
        lab = np.zeros(n_nodes, dtype=np.uint32)
        if n_nodes:
            aa = _some(a)
            bb = _some(b)
            self._call('pep_components', n_nodes, len(a), _ptr(aa), _ptr(bb), _ptr(lab))
        return lab
