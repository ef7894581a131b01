"""K4b (seed_runs_extend) against the oracle on the edges of the ungapped x-drop pre-filter: the cases of tests/seed_extend_cases.py, each of
which tests/test_seed_extend_cases_host.py holds to what its name says.  Compared: the candidate count, the pairs, the cells and the whole
hit table (not seed_hits_passed, which depends on the order in which the runs meet the candidate set)."""
import numpy as np
import pytest

import seed_extend_cases as S

pytestmark = pytest.mark.gpu

FIELDS = ('q', 't', 'q_start', 'q_end', 't_start', 't_end', 'score', 'nm', 'n_ident', 'aln_len', 'cigar_runs', 'bin', 'cigar_off', 'cells')


@pytest.fixture(scope='module')
def ctx():
    from peppan_amd import _native as N
    c = N.Context(0)
    yield c
    c.close()


def _compare(ctx, q, t, p):
    from oracle import oracle as O
    ctx.set_query_aa(q)
    ctx.set_ref_aa(t)
    gh, gc, st = ctx.search(p)
    ms = np.array([O.min_score(len(s), p.dbsize, p.max_evalue, p.ka_lambda, p.ka_k) for s in q], dtype=np.int32)
    oh, oc, ost = O.search(q, t, O.params_from(p), min_scores=ms)
    assert (st['candidates'], st['pairs'], st['cells']) == (ost['candidates'], ost['pairs'], ost['cells'])
    assert len(gh) == len(oh), (len(gh), len(oh))
    for f in FIELDS:
        assert np.array_equal(gh[f], oh[f]), f
    assert np.array_equal(gc, oc)
    return ost


@pytest.mark.parametrize('case', [c for c in S.cases() if c['tool'] == 'protein'], ids=lambda c: c['name'])
def test_pre_filter_edges(ctx, case):
    from peppan_amd import _native as N
    p = N.default_params(0., 0., 10, 5)
    for k, v in case['par'].items():
        setattr(p, k, v)
    ost = _compare(ctx, case['q'], case['t'], p)
    if case['candidates'] is not None:
        assert ost['candidates'] == case['candidates']


def test_pre_filter_nucleotide_parameters(ctx):
    from peppan_amd import _native as N
    q, t = S.nucleotide_set()
    _compare(ctx, q, t, N.nucleotide_params(60., 20.))
