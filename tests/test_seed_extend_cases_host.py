"""The cases of tests/seed_extend_cases.py through the oracle alone: each is what its name says, so that no case of
tests/test_gpu_seed_extend.py can pass vacuously.  A case that fails here is a broken case, not a skip."""
import numpy as np
import pytest

import seed_extend_cases as S
from oracle import oracle as O


def _params(case, **kw):
    p = O.default_params()
    for k, v in dict(case['par'], **kw).items():
        setattr(p, k, v)
    return p


def _candidates(case, **kw):
    return O.search(case['q'], case['t'], _params(case, **kw))[2]['candidates']


TWINS = sorted(set(c['twin'] for c in S.cases() if c['twin']))


def test_cases_stay_small():
    for c in S.cases():
        if c['tool'] == 'protein':
            assert len(c['q']) + len(c['t']) <= 96 and len(c['q']) <= 64 and len(c['t']) <= 64, c['name']
            assert max(len(s) for s in c['q'] + c['t']) <= 200, c['name']
    assert len(TWINS) >= 12


@pytest.mark.parametrize('twin', TWINS)
def test_twins_lie_on_either_side_of_their_edge(twin):
    """the oracle counts what the builder states - a candidate per pair for one twin, none for the other -, so the twins' counts differ"""
    a, b = [c for c in S.cases() if c['twin'] == twin]
    na, nb = _candidates(a), _candidates(b)
    assert (na, nb) == (a['candidates'], b['candidates']), (twin, na, nb)
    assert na != nb
    # the twins differ by one unit: the same number of sequences, lengths within one residue, at most two residues changed per pair
    for x, y in zip(a['q'] + a['t'], b['q'] + b['t']):
        assert abs(len(x) - len(y)) <= 1
        if len(x) == len(y):
            assert int((x != y).sum()) <= 2
        else:
            lo, hi = (x, y) if len(x) < len(y) else (y, x)
            assert np.array_equal(lo, hi[:-1]) or np.array_equal(lo, hi[1:])


@pytest.mark.parametrize('case', [c for c in S.cases() if c['twin'] is None and c['tool'] == 'protein'], ids=lambda c: c['name'])
def test_parameter_sets_reject_and_accept(case):
    """a parameter set's pre-filter lets some of the set's seed hits through and stops others (without one - ungapped_min 0 - every hit nominates)"""
    n, every = _candidates(case), _candidates(case, ungapped_min=0, stage1_min=0)
    if case['par']['ungapped_min'] == 0:
        assert n == every > 0
    else:
        assert 0 < n < every, (case['name'], n, every)


def test_nucleotide_set_rejects_and_accepts():
    from peppan_amd import _native as N
    q, t = S.nucleotide_set()
    assert len(q) == 100
    p = O.params_from(N.nucleotide_params(60., 20.))
    n = O.search(q, t, p)[2]['candidates']
    p.ungapped_min = 0
    assert 0 < n < O.search(q, t, p)[2]['candidates']
