"""GPU tests of K14 (pep_pair_support, csrc/similar.hip) and of get_similar_pairs' product path against golden G24, the reference's own
get_similar_pairs (PEPPAN.py:194-294) on the edge tables of tests/similar_helpers.py; the CPU half is tests/test_similar_host.py.

Each call handles a few hundred groups of at most a few thousand positions plus a few of 8 191 to 20 000 and one of 40 000 (two to five of numpy's reduction buffers of 8192 elements).
The one-gibibyte scratch budget that splits K14 into several launches cannot be reached at these sizes and stays out of scope here, as does
the clamp of an M run at the query's length (the fixture's alignments stay inside their genes).  Every assertion is == on integers, strings
and lists."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import similar_helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native as N
    with N.Context(0) as c:
        yield c


@pytest.fixture(scope='module')
def g24():
    return H.load_g24()


def test_product_path_equals_the_reference_on_gpu(ctx, g24, tmp_path, monkeypatch):
    """numeric table, classify, scan, K14 on the GPU, resolve and the two rewrites == the recorded pairs, exemplar text and clust.npy"""
    for c in g24['cases']:
        pairs, text, clu = H.run_product(c, tmp_path / c['name'], monkeypatch, ctx)
        assert pairs == c['pairs'], c['name']
        assert text == c['exemplar_out'] and clu == c['clust_npy_out'], c['name']


def test_pair_support_kernel_equals_the_reference(ctx, g24):
    """K14 on the groups of the probed pairs, one call per params set == the outcomes decoded from the reference's result; for the set with
    the group above 32 768 positions also with that group first and with it last: group order and scratch offsets do not matter"""
    from peppan_amd import _native as N
    sets = {}
    for c in g24['cases']:
        if c['probes']:
            sets.setdefault(H.params_key(c['params']), []).append(c)
    n, seen, long_calls = 0, set(), 0
    for cases in sets.values():
        lim = N.support_limits(cases[0]['params'])
        rows, cigar, off, gq, gr, want = H.k14_inputs(cases)
        got = ctx.pair_support(rows, cigar, off, gq, gr, lim)
        assert got.tolist() == want.tolist(), (cases[0]['name'], np.flatnonzero(got != want)[:10])
        n += len(want)
        seen |= {'none' if v == N.SUPPORT_NONE else 'zero' if v == 0 else 'value' for v in got.tolist()}
        if any(p.get('n', 0) > 32768 for c in cases for p in c['probes']):
            m = len(want)
            big = [k for k, (a, b) in enumerate(zip(off[:-1], off[1:])) if b > a and gq[k] > 32768]
            assert len(big) == 1
            rest = [k for k in range(m) if k != big[0]]
            for order in (big + rest, rest[::-1] + big):
                rows, cigar, off2, gq2, gr2, want2 = H.k14_inputs(cases, order)
                got = ctx.pair_support(rows, cigar, off2, gq2, gr2, lim)
                assert got.tolist() == want2.tolist(), np.flatnonzero(got != want2)[:10]
                long_calls += 1
    assert n == sum(len(c['probes']) for c in g24['cases']) and seen == {'none', 'zero', 'value'} and long_calls == 2


def test_random_tables_equal_the_restatement_on_gpu(ctx, tmp_path, monkeypatch):
    """20 seeded tables of 30 to 60 genes put together from the families' row makers, genes shared between pairs: the product path with K14 on
    the GPU == the restatement; over the set all three outcomes of get_similar, absorptions in both directions, conflicts and repeat kills"""
    rng = np.random.default_rng(2424)
    tally = dict(none=0, zero=0, value=0, absorb_query=0, absorb_ref=0, conflict=0, repeat=0)
    for k in range(20):
        c = H.random_case(rng, k).record()
        H.tally_random(c, tally)
        pairs, kept, edges = H.restate_pass(c['table'], H.priorities_of(c), c['params'])
        text, clu = H.expected_files(c, kept, edges)
        got = H.run_product(c, tmp_path / c['name'], monkeypatch, ctx)
        assert got[0] == pairs and got[1] == text and got[2] == clu, c['name']
    assert all(v > 0 for v in tally.values()), tally
