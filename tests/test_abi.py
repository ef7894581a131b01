"""CPU-side checks of the drop-in boundary: the library builds, loads and exports every symbol of include/peppan_hip.h."""
import ctypes as C
import os
import re
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native as N
    lib = N.load_library()
    hdr = open(os.path.join(ROOT, 'include', 'peppan_hip.h')).read()
    declared = set(re.findall(r'\b(pep_[a-z0-9_]+)\s*\(', hdr))
    assert declared == set(N.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.pep_version() == N.ABI_VERSION == 20 == int(re.search(r'#define PEP_ABI_VERSION (\d+)', hdr).group(1))


SCALARS = {'int': C.c_int, 'int32_t': C.c_int32, 'uint32_t': C.c_uint32, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64, 'double': C.c_double}


def _header_prototypes():
    """[(return declaration, name, [parameter declaration])] of every prototype of the header, comments stripped"""
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'peppan_hip.h')).read(), flags=re.S)
    found = re.findall(r'^((?:const )?\w+ \*?)(pep_[a-z0-9_]+)\(([^()]*)\);', hdr, flags=re.M)
    return [(ret.strip(), name, [] if params.strip() == 'void' else [' '.join(p.split()) for p in params.split(',')]) for ret, name, params in found]


def _ctypes_of(decl, is_return=False):
    """the ctypes types that may stand for a C declaration of the header: pointers and arrays c_void_p (a char pointer also c_char_p), scalars their own width"""
    if decl == 'void':
        return {None}
    if '*' in decl or '[' in decl:
        if re.match(r'(const )?char \*', decl):
            return {C.c_char_p} if is_return else {C.c_char_p, C.c_void_p}
        return {C.c_void_p}
    return {SCALARS[decl.replace('const ', '').split()[0]]}


def test_signature_table_is_the_header():
    """peppan_amd._native.SIGNATURES states the return and parameter types of every prototype of include/peppan_hip.h, and load_library() has given them to ctypes"""
    from peppan_amd import _native as N
    protos = _header_prototypes()
    assert len(protos) == 115 and sum(len(params) for _, _, params in protos) == 835          # (a prototype the pattern misses shows here)
    assert {name for _, name, _ in protos} == set(N.SIGNATURES) == set(N.EXPORTS) and len(N.EXPORTS) == len(protos)
    lib = N.load_library()
    for ret, name, params in protos:
        restype, *argtypes = N.SIGNATURES[name]
        assert len(argtypes) == len(params), name
        assert restype in _ctypes_of(ret, is_return=True), name
        for k, (decl, t) in enumerate(zip(params, argtypes)):
            assert t in _ctypes_of(decl), (name, k, decl)
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes and fn.restype is restype, name


def test_typing_acts_before_the_library_does():
    """a float for an int64_t parameter and a call with an argument missing are refused by ctypes: the library is never entered"""
    from peppan_amd import _native as N
    lib = N.load_library()
    with pytest.raises((C.ArgumentError, TypeError)):
        lib.pep_crc32(None, 1.5, 0)
    with pytest.raises((C.ArgumentError, TypeError)):
        lib.pep_set_host_threads()


def test_direct_callers_get_the_full_return_width():
    """the return types are set when the library is loaded, not by the wrappers: a call past them is not cut to a C int"""
    import zlib
    import numpy as np
    from peppan_amd import _native as N
    lib = N.load_library()
    assert lib.pep_deflate_literals.restype is C.c_int64 and lib.pep_crc32.restype is C.c_uint32
    data = np.random.default_rng(20261018).integers(0, 256, size=1000, dtype=np.uint8)
    assert lib.pep_crc32(N._ptr(data), len(data), 0) == zlib.crc32(data.tobytes())


HANDLE_FIRST = ['pep_rescore_nt', 'pep_rescore_codons', 'pep_components', 'pep_components_of_hits', 'pep_set_grouping', 'pep_linclust', 'pep_overlaps', 'pep_alleles',
                'pep_sha1', 'pep_dedup', 'pep_allele_diff', 'pep_group_verdicts', 'pep_verdict_detail_size', 'pep_verdict_detail_copy', 'pep_gene_ingroups',
                'pep_call_times', 'pep_synteny_pairs', 'pep_synteny_pairs_copy', 'pep_gene_structure', 'pep_rarefaction_curves', 'pep_profile_pairs',
                'pep_kimura_pairs', 'pep_nj_trees', 'pep_global_diff_walk_size', 'pep_global_diff_walk_copy', 'pep_global_diff', 'pep_global_diff_copy',
                'pep_cds_genes', 'pep_out_alleles', 'pep_tree_cut', 'pep_batch_screen', 'pep_batch_prune']


def test_null_handle_is_an_argument_error():
    """every entry point of K7 and K9 - K26 that takes a pep_ctx *, a pep_verdict_result * or a pep_gdiff_walk * first answers a null one with PEP_ERR_ARG, whatever
    else it is given: the check of the handle comes before anything that would need a device"""
    from peppan_amd import _native as N
    lib = N.load_library()
    for name in HANDLE_FIRST:
        restype, *argtypes = N.SIGNATURES[name]
        assert restype is C.c_int and argtypes[0] is C.c_void_p, name
        assert getattr(lib, name)(*[None if t is C.c_void_p else t(0) for t in argtypes]) == -2, name          # PEP_ERR_ARG


def test_call_times_refuses_a_bad_selector_and_a_null_record():
    """pep_call_times answers which = -1, which = PEP_CALL_COUNT and a null out with PEP_ERR_ARG (here without a context, which alone is refused already; on a live
    context: tests/test_gpu_ctx_resources.py); PEP_CALL_COUNT and the fourteen selectors of the header are _native's"""
    from peppan_amd import _native as N
    lib = N.load_library()
    hdr = open(os.path.join(ROOT, 'include', 'peppan_hip.h')).read()
    names = ('ALLELE_DIFF', 'GROUP_VERDICTS', 'GENE_INGROUPS', 'SYNTENY_PAIRS', 'GENE_STRUCTURE', 'PARSER', 'KIMURA_PAIRS', 'NJ_TREES', 'GLOBAL_DIFF', 'CDS_GENES',
             'OUT_ALLELES', 'TREE_CUT', 'BATCH_SCREEN', 'BATCH_PRUNE', 'COUNT')
    assert [int(re.search(r'#define PEP_CALL_%s (\d+)\b' % n, hdr).group(1)) for n in names] == [getattr(N, 'CALL_' + n) for n in names] == list(range(15))
    out = N.CallTimes()
    for which, record in ((-1, C.byref(out)), (N.CALL_COUNT, C.byref(out)), (0, None), (0, C.byref(out))):
        assert lib.pep_call_times(None, which, record) == -2          # PEP_ERR_ARG


def test_struct_layouts_match_header(tmp_path):
    """sizes and field offsets of every struct that crosses the boundary, taken from the header by a C compiler, equal the ctypes / numpy
    mirrors in peppan_amd/_native.py"""
    import subprocess
    from peppan_amd import _native as N
    probes = [('pep_search_params', 'min_id_pct'), ('pep_search_params', 'dbsize'), ('pep_search_params', 'ka_lambda'), ('pep_search_params', 'hsp_mode'),
              ('pep_search_params', 't_index_base'), ('pep_stats', 'cells_swept_trace'), ('pep_stats', 'candidates_settled'), ('pep_stats', 'cells_settled'), ('pep_stats', 'ms_seed'), ('pep_stats', 'ms_seed_match'),
              ('pep_hit', 'cigar_off'), ('pep_hit', 'cells'), ('pep_nt_hit', 'cigar_off'), ('pep_locus', 'cigar_off'),
              ('pep_mat_cols', 'iden'), ('pep_mat_cols', 'arena'), ('pep_mat_cols', 'rid'), ('pep_mat_cols', 'score_is_int'),
              ('pep_call_times', 'bytes_to_device'), ('pep_call_times', 'bytes_to_host')]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "peppan_hip.h"\nint main(void) {\n'
    for st in ('pep_search_params', 'pep_stats', 'pep_hit', 'pep_nt_hit', 'pep_locus', 'pep_query_meta', 'pep_target_meta', 'pep_mat_cols'):
        src += '  printf("%s %%zu\\n", sizeof(%s));\n' % (st, st)
    src += '  printf("pep_call_times %zu\\n", sizeof(struct pep_call_times));\n'          # (known by its tag: the function has the name)
    for st, f in probes:
        src += '  printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (st, f, 'struct pep_call_times' if st == 'pep_call_times' else st, f)
    src += '  return 0;\n}\n'
    (tmp_path / 'probe.c').write_text(src)
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', str(tmp_path / 'probe'), str(tmp_path / 'probe.c')])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / 'probe')]).decode().splitlines())
    got = {k: int(v) for k, v in got.items()}
    assert got['pep_search_params'] == C.sizeof(N.SearchParams) and got['pep_stats'] == C.sizeof(N.Stats)
    assert got['pep_hit'] == N.HIT_DTYPE.itemsize == 64 and got['pep_nt_hit'] == N.NT_HIT_DTYPE.itemsize == 40
    assert got['pep_locus'] == N.LOCUS_DTYPE.itemsize == 32 and got['pep_mat_cols'] == C.sizeof(N.MatCols)
    assert got['pep_query_meta'] == N.QUERY_META_DTYPE.itemsize == 16 and got['pep_target_meta'] == N.TARGET_META_DTYPE.itemsize == 16
    assert got['pep_call_times'] == C.sizeof(N.CallTimes) == 80
    for st, f in probes:
        mirror = {'pep_search_params': N.SearchParams, 'pep_stats': N.Stats, 'pep_mat_cols': N.MatCols, 'pep_call_times': N.CallTimes}.get(st)
        if mirror is not None:
            assert got[st + '.' + f] == getattr(mirror, f).offset, (st, f)
        else:
            dt = {'pep_hit': N.HIT_DTYPE, 'pep_nt_hit': N.NT_HIT_DTYPE, 'pep_locus': N.LOCUS_DTYPE}[st]
            assert got[st + '.' + f] == dt.fields[f][1], (st, f)


def test_merge_hits_is_the_unsharded_topk():
    """pep_merge_hits (host C++): union of per-shard tables -> top-k per (q, t mod splits) by (score desc, t asc, bin asc), rows by (q, t, bin)"""
    import numpy as np
    from peppan_amd import _native as N
    rng = np.random.default_rng(5)
    rows, cig = [], []
    for q in range(40):
        for t in rng.choice(400, size=int(rng.integers(0, 60)), replace=False).tolist():
            runs = [(int(rng.integers(5, 90)) << 2) | int(k % 3) for k in range(int(rng.integers(1, 5)))]
            rows.append((q, t, 1, 10, 1, 10, int(rng.integers(60, 70)), 0, 10, 10, len(runs), int(rng.integers(0, 3)), len(cig), 7))
            cig += runs
    hits = np.array(rows, dtype=N.HIT_DTYPE)
    cig = np.array(cig, dtype=np.uint32)
    perm = rng.permutation(len(hits))                              # shards arrive in any order
    out_h, out_c = N.merge_hits(hits[perm], cig, 3, 5)
    want = []
    for q in range(40):
        for sp in range(5):
            grp = [h for h in hits if h['q'] == q and h['t'] % 5 == sp]
            grp.sort(key=lambda h: (-int(h['score']), int(h['t']), int(h['bin'])))
            want += grp[:3]
    want.sort(key=lambda h: (int(h['q']), int(h['t']), int(h['bin'])))
    assert len(out_h) == len(want) > 200
    off = 0
    for g, w in zip(out_h, want):
        for f in N.HIT_DTYPE.names:
            if f != 'cigar_off':
                assert g[f] == w[f]
        assert g['cigar_off'] == off
        assert out_c[off:off + int(g['cigar_runs'])].tolist() == cig[int(w['cigar_off']):int(w['cigar_off']) + int(w['cigar_runs'])].tolist()
        off += int(g['cigar_runs'])
    assert off == len(out_c)
    e_h, e_c = N.merge_hits(hits[:0], cig[:0], 3, 5)
    assert len(e_h) == 0 and len(e_c) == 0


def test_no_gpu_is_a_loud_error():
    from peppan_amd import _native as N
    lib = N.load_library()
    if lib.pep_device_count() > 0:
        pytest.skip('a GPU is visible')
    with pytest.raises(N.PepError):
        N.Context(0)


def test_default_params_and_min_score_match_oracle():
    from peppan_amd import _native as N
    from oracle import oracle as O
    p, o = N.default_params(), O.default_params()
    assert list(p.sub) == list(o.sub) and list(p.reduce) == list(o.reduce)
    assert p.base == o.base and p.n_shapes == o.n_shapes and list(p.weight) == list(o.weight)
    assert [list(x) for x in p.offs] == [list(x) for x in o.offs]
    assert (p.gap_open, p.gap_ext, p.top_k, p.n_splits) == (o.gap_open, o.gap_ext, o.top_k, o.n_splits)
    assert (p.ungapped_min, p.xdrop, p.ext_right, p.ext_left) == (o.ungapped_min, o.xdrop, o.ext_right, o.ext_left) == (55, 12, 40, 24)
    assert p.stage1_min == o.stage1_min == 24
    for L in (1, 30, 100, 334, 1000, 3164, 50000):
        assert N.min_score(L) == O.min_score(L)
    assert N.min_score(334) == 68          # ~63/68/72 for 100/334/1000-aa queries
