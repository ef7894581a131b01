"""The seed stage's retry loop (seeds.hip, pep_find_candidates) on the cases of tests/seed_retry_cases.py, each of which
tests/test_seed_retry_cases_host.py proves to force the retries it names: a slab that overflows, a hit buffer that grows, a candidate set that grows.

Per case, on a fresh context: the search equals the oracle's in every field of the hit table, the CIGAR arena and the candidate / pair / cell / traceback
counts; seed_hits, target_seeds and query_seeds equal the numpy count of seed_retry_cases.seed_counts (query_seeds not for the nucleotide tool, whose index
holds the stride matcher's 14-mer look-up words: see that module's docstring).

That a growth RAN is shown by the device memory the context holds afterwards (pep_live_resources), against the case's control - the same family cut down
until it takes nothing - on another fresh context: buffers are reserved at 1.25 x the request and never shrink, so one growth of the hit buffer leaves at
least 3 * 8 * 2^22 bytes more, two leave 15 * 8 * 2^22, one growth of the candidate set 3 * 8 * 2^20.  Lower bounds only.  The slab fallback has no such
signature: for it the evidence is the host test's sufficient condition (one key more often than a slab holds) and the equality with the plain build
(params.reserved[2] = 1), which never partitions.

Carried state: nine searches on ONE context, retrying ones between quiet ones, every one byte-identical to its fresh-context result."""
import functools

import numpy as np
import pytest

import seed_retry_cases as S

pytestmark = pytest.mark.gpu

FIELDS = ('q', 't', 'q_start', 'q_end', 't_start', 't_end', 'score', 'nm', 'n_ident', 'aln_len', 'cigar_runs', 'bin', 'cigar_off', 'cells')
HIT_GROWTH = {1: 3 * 8 << 22, 2: 15 * 8 << 22}
SET_GROWTH = 3 * 8 << 20
SEQUENCE = ('quiet', 'hits_x1', 'quiet', 'set_x1', 'quiet', 'slab', 'quiet', 'self_hits', 'quiet')


def _load(ctx, c):
    if c['genes'] is not None:
        ctx.set_query_nt(c['genes'], 11)
        ctx.set_ref_nt(c['genes'], 6, 11)
    else:
        ctx.set_query_aa(c['q'])
        ctx.set_ref_aa(c['t'])


def _search(ctx, c, plain_build=0):
    """-> (hit table bytes, CIGAR bytes, the statistics of seed_retry_cases.STATS)"""
    _load(ctx, c)
    p = S.native_params(c)
    p.reserved[2] = plain_build
    h, cg, st = ctx.search(p)
    return h.tobytes(), cg.tobytes(), tuple(int(st[k]) for k in S.STATS)


@functools.lru_cache(maxsize=None)
def _fresh(name, control=False, plain_build=0):
    """the case on a context of its own -> (_search's result, device bytes the context holds afterwards)"""
    from peppan_amd import _native as N
    c = S.case(name, control)
    before = N.live_resources()[0]
    with N.Context(0) as ctx:
        out = _search(ctx, c, plain_build)
        if c['genes'] is not None:                      # K1 made of the genes what the case says: the oracle's sets are the library's
            for (codes, off), want in ((ctx.query_aa(), c['q']), (ctx.target_aa(), c['t'])):
                assert len(off) - 1 == len(want) and np.array_equal(codes, np.concatenate(want))
                assert np.array_equal(np.diff(off.astype(np.int64)), [len(x) for x in want])
        held = N.live_resources()[0] - before
    return out, held


@pytest.mark.parametrize('name', S.NAMES)
def test_retrying_search_equals_oracle_and_independent_count(name):
    from peppan_amd import _native as N
    c = S.case(name)
    (hb, cb, stats), held = _fresh(name)
    gh, gc, st = np.frombuffer(hb, dtype=N.HIT_DTYPE), np.frombuffer(cb, dtype=np.uint32), dict(zip(S.STATS, stats))
    oh, oc, ost, _ = S.oracle_result(name)
    print(name, st, 'device bytes held', held)
    assert (st['candidates'], st['pairs'], st['cells'], st['tracebacks'], st['hits']) == (ost['candidates'], ost['pairs'], ost['cells'], ost['tracebacks'], len(oh))
    assert len(gh) == len(oh) > 0
    for f in FIELDS:
        assert np.array_equal(gh[f], oh[f]), f
    assert np.array_equal(gc, oc)
    cnt = S.counts(name)
    assert st['seed_hits'] == sum(raw for cq, ct, raw in cnt)
    assert st['target_seeds'] == sum(ct for cq, ct, raw in cnt)
    if c['tool'] != 'nucleotide':
        assert st['query_seeds'] == sum(cq for cq, ct, raw in cnt)
    takes = c['takes']
    if takes['hit_growths'] or takes['set_growths']:
        (_, _, cstats), cheld = _fresh(name, control=True)
        ccnt = S.counts(name, True)
        assert dict(zip(S.STATS, cstats))['seed_hits'] == sum(raw for cq, ct, raw in ccnt)
        print(name, 'control holds', cheld)
        least = HIT_GROWTH.get(takes['hit_growths'], 0) + SET_GROWTH * takes['set_growths']
        assert held - cheld >= least, (held, cheld, least)
    if takes['slab']:
        assert _fresh(name, plain_build=1)[0] == (hb, cb, stats)


@pytest.mark.parametrize('name', [n for n in S.NAMES if n != 'quiet'])
def test_control_takes_the_quiet_path_and_equals_oracle(name):
    """the control of the memory comparison is a search like any other"""
    from peppan_amd import _native as N
    (hb, cb, stats), _ = _fresh(name, control=True)
    oh, oc, ost, _ = S.oracle_result(name, True)
    gh = np.frombuffer(hb, dtype=N.HIT_DTYPE)
    assert len(gh) == len(oh)
    for f in FIELDS:
        assert np.array_equal(gh[f], oh[f]), f
    assert np.array_equal(np.frombuffer(cb, dtype=np.uint32), oc)
    assert dict(zip(S.STATS, stats))['candidates'] == ost['candidates']


def test_state_carried_across_retries_on_one_context():
    """quiet and retrying searches in turn on one context - the set's clean mark, the counter block's, the grown buffers, the self map - then hits_x1 again
    (its buffer is large enough now: no retry) and once more with the table left on the device: every result is the fresh context's, byte for byte"""
    from peppan_amd import _native as N
    with N.Context(0) as ctx:
        for step, name in enumerate(SEQUENCE + ('hits_x1',)):
            assert _search(ctx, S.case(name)) == _fresh(name)[0], (step, name)
        c = S.case('hits_x1')
        _load(ctx, c)
        nh, nc, st, _ = ctx.search_on_device(S.native_params(c))
        h, cg = ctx.result_to_host()
        assert (h.tobytes(), cg.tobytes(), tuple(int(st[k]) for k in S.STATS)) == _fresh('hits_x1')[0]
        assert (nh, nc) == (len(h), len(cg))
