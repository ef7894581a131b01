"""The alignment passes (csrc/sw.hip: sw_score_kernel, sw_trace_kernel, sw_trace_retry_kernel; csrc/trace.hip behind them) against the oracle at
the limits where they choose another sweep: the cases of tests/align_limit_cases.py, each of which tests/test_align_limit_cases_host.py holds to
what its name says - which side of which limit every candidate is on, from arithmetic restated there and from the oracle's own counters.

Every case runs as given (the packed 16-bit sweeps wherever the rules allow them), with the 32-bit sweeps forced (params.reserved[1] = 1) and
without the LDS staging area (use_lds = 0); the searches with the longest pairs also with every buffer of the traceback stage sized exactly
(params.reserved2 bit 0).  All of them must give the oracle's table field by field and the same bytes as each other.  The oracle's `full_band`
counter is checked on the host side only: which optimal alignment is reported is a deterministic rule, so a GPU that skipped the full-band retry
of a pair that left its sub-band cannot produce the oracle's CIGAR."""
import numpy as np
import pytest

import align_limit_cases as AL
from test_gpu_parity import _cmp_hits

pytestmark = pytest.mark.gpu

CASES = AL.cases()
STATS = ('candidates', 'pairs', 'cells', 'tracebacks', 'tracebacks_gapless')


@pytest.fixture(scope='module')
def ctx():
    from peppan_amd import _native as N
    c = N.Context(0)
    yield c
    c.close()


def _oracle_stats(case):
    _, _, ost, tc = AL.oracle_results()[case['name']]
    return dict(candidates=ost['candidates'], pairs=ost['pairs'], cells=ost['cells'], tracebacks=tc['traced'], tracebacks_gapless=tc['gapless'])


def _search(ctx, case, **kw):
    ctx.set_query_aa(case['q'])
    ctx.set_ref_aa(case['t'])
    return ctx.search(AL.native_params(case, **kw))


def _check(ctx, case, **kw):
    oh, oc, _, _ = AL.oracle_results()[case['name']]
    gh, gc, st = _search(ctx, case, **kw)
    assert {k: st[k] for k in STATS} == _oracle_stats(case), (case['name'], kw)
    _cmp_hits(gh, gc, oh, oc)
    return gh.tobytes(), gc.tobytes()


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_cases_equal_the_oracle(ctx, case):
    ways = [dict(), dict(forced32=True), dict(use_lds=0)]
    if max(len(s) for s in case['q']) >= 2900:
        ways.append(dict(exact=True))
    got = [_check(ctx, case, **kw) for kw in ways]
    assert all(g == got[0] for g in got[1:])


def test_results_do_not_depend_on_what_ran_before(ctx):
    """every case once more on the same context in a shuffled order, as given and then each in one of the three ways: the list of pairs deferred
    to the full-band retry, the counter blocks of the passes and the look-back epochs carry over from search to search"""
    rng = np.random.default_rng(20)
    ways = [dict(), dict(forced32=True), dict(use_lds=0)]
    for k in rng.permutation(len(CASES)):
        _check(ctx, CASES[k])
    for k in rng.permutation(len(CASES)):
        _check(ctx, CASES[k], **ways[int(rng.integers(0, 3))])
