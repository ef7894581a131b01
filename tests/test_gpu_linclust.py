"""K9 (lc_select, lc_insert, lc_verify, lc_assign and the host merge of the gapped stage) against the oracle at the kernel's edges: the cases of
tests/linclust_cases.py, each of which tests/test_linclust_cases_host.py holds to what its name says and the oracle, on each, to a restatement of
its own definition.  Compared: the representative of every sequence and the totals of selected k-mers, verified diagonals and accepted centres."""
import numpy as np
import pytest

import linclust_cases as LC

pytestmark = pytest.mark.gpu

CASES = LC.cases()


@pytest.fixture(scope='module')
def ctx():
    from peppan_amd import _native as N
    c = N.Context(0)
    yield c
    c.close()


def _gpu(ctx, case):
    return ctx.linclust(case['seqs'], case['min_id'], case['min_cov'], base=case['base'], k=case['k'], m=case['m'])


def _check(ctx, case):
    o_rep, o_st = LC.oracle_results()[case['name']]
    g_rep, g_st = _gpu(ctx, case)
    assert g_st == o_st, case['name']
    assert np.array_equal(g_rep, o_rep), case['name']


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_cases_equal_the_oracle(ctx, case):
    _check(ctx, case)


def test_context_reuse_large_calls_before_small_ones(ctx):
    """the whole list again on the same context, last case first: the large calls (the ladders, the 70 000-letter sequence) now come before
    the small ones, whose results would show workspace contents left behind"""
    for case in CASES[::-1]:
        _check(ctx, case)


REFUSED = [dict(m=0), dict(m=33), dict(k=0), dict(k=33), dict(base=1), dict(base=4, k=32), dict(base=8, k=22), dict(base=20, k=15)]


def test_refusals_leave_the_context_usable(ctx):
    from peppan_amd import _native as N
    witness = next(c for c in CASES if c['name'] == 'witness/b4_k17_m20/L-k=129_bad1')
    for kw in REFUSED:
        par = dict(base=4, k=17, m=20)
        par.update(kw)
        with pytest.raises(N.PepError):
            ctx.linclust(witness['seqs'], 0., 0., **par)
        _check(ctx, witness)
