"""K10-K13 on the GPU against the restatements of tests/small_kernel_cases.py, on the hand-built cases that sit where these kernels branch
(tests/test_small_kernels_host.py holds each case to what its name says).  All cases of a kernel run on one context in the order of the
list, so a large case leaves its workspace to the small one behind it.  Every comparison is np.array_equal: no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_kernel_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

ALLELES = K.alleles_cases()
OVERLAPS = K.overlaps_cases()
COMPONENTS = K.components_cases()
DEDUP = K.dedup_cases()
ids = lambda cases: [c['name'] for c in cases]  # noqa: E731


@pytest.fixture(scope='module')
def ctx():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native as N
    with N.Context(0) as c:
        yield c


@pytest.mark.parametrize('case', ALLELES, ids=ids(ALLELES))
def test_k12_alleles_equal_the_restatement(ctx, case):
    args = (case['contigs'], case['rows'], case['cigar'], case['grp_off'], case['grp_qlen'], case['gtable'])
    got = ctx.alleles(*args)
    for g, w, what in zip(got, K.restate_alleles(*args), ('in_frame', 'orf', 'packed')):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), what


@pytest.mark.parametrize('case', OVERLAPS, ids=ids(OVERLAPS))
def test_k11_overlaps_equal_the_restatement(ctx, case):
    got = ctx.overlaps(case['contig'], case['start'], case['end'], case['rid'], case['ovl_l'], case['ovl_p'])
    want = K.restate_overlaps(case['contig'].tolist(), case['start'].tolist(), case['end'].tolist(), case['rid'].tolist(), case['ovl_l'], case['ovl_p'])
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize('case', COMPONENTS, ids=ids(COMPONENTS))
def test_k10_components_equal_the_restatement(ctx, case):
    got = ctx.components(case['n'], case['a'], case['b'])
    want = K.restate_components(case['n'], case['a'], case['b'])
    assert got.dtype == want.dtype and np.array_equal(got, want)


def test_k10_components_of_hits_with_node_maps_a_b_a(ctx):
    """the table of hits under node map A, under B (A but for its last entry), under A again: each call equals the restatement of its own map"""
    from peppan_amd import _native as N
    h = K.hits_case()
    hits = np.zeros(len(h['q']), dtype=N.HIT_DTYPE)
    hits['q'], hits['t'] = h['q'], h['t']
    labels = []
    for node_of_target in h['maps']:
        got = ctx.components_of_hits(h['n'], hits, node_of_target, q_base=h['q_base'])
        assert np.array_equal(got, K.restate_components(h['n'], h['q'] + h['q_base'], node_of_target[h['t']]))
        labels.append(got)
    assert np.array_equal(labels[0], labels[2]) and not np.array_equal(labels[0], labels[1])


def test_k10_components_of_search_with_node_maps_a_b_a(ctx):
    """the same three maps over the table a search left on the device (pep_components_of_result), where the library keeps the node map it
    uploaded last and uploads another only when it differs"""
    from peppan_amd import _native as N
    rng = np.random.default_rng(12)
    aa = np.frombuffer(b'ARNDCQEGHILKMFPSTWYV', dtype=np.uint8) - 65
    prots = [aa[rng.integers(0, 20, int(rng.integers(60, 121)))].astype(np.uint8) for _ in range(6)]
    prots += [p.copy() for p in prots[:3]]                  # 9 proteins, three of them twice: hits between different proteins
    ctx.set_query_aa(prots)                                 # (the module's context keeps these sets and the search's table; K13's cases behind it do not read them)
    ctx.set_ref_aa(prots)
    view, _, _ = ctx.search(N.default_params(), copy=False)
    hits = np.array(view)
    assert len(hits) >= 9 + 6 and hits['t'].max() == len(prots) - 1
    n, q_base = len(prots) + 4, 4
    map_a = (np.arange(len(prots), dtype=np.uint32) % 5) + q_base
    map_b = map_a.copy()
    map_b[-1] = 0
    labels = []
    for node_of_target in (map_a, map_b, map_a.copy()):
        got = ctx.components_of_search(n, node_of_target, q_base=q_base)
        assert np.array_equal(got, K.restate_components(n, hits['q'] + q_base, node_of_target[hits['t']]))
        labels.append(got)
    assert np.array_equal(labels[0], labels[2]) and not np.array_equal(labels[0], labels[1])


@pytest.mark.parametrize('case', DEDUP, ids=ids(DEDUP))
def test_k13_dedup_equals_the_restatement(ctx, case):
    got = ctx.dedup(case['lengths'], case['digests'])
    want = K.restate_dedup(case['lengths'], case['digests'])
    assert got.dtype == want.dtype and np.array_equal(got, want)
