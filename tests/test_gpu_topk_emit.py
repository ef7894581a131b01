"""topk_emit and what it hands on (trace.hip: top-k, the two compactions, hit records, CIGAR runs and the unions of single linkage in one launch;
pack_out behind it flattens the labels and carries the table to the host) against the oracle, on the cases of tests/topk_emit_cases.py - every hit
field, the CIGAR arena, the statistics, and with grouping on the labels of pep_components_of_hits over the ORACLE's table.  Where the cases stand
(selected pairs around the tile sizes, a group across a tile boundary, ...) is proved without a GPU in tests/test_topk_emit_cases.py."""
import numpy as np
import pytest

import topk_emit_cases as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from peppan_amd import _native as N
    c = N.Context(0)
    yield c
    c.close()


def _cmp(got, name):
    gh, gc, st = got
    oh, oc, ost, tc = TC.oracle(name)
    assert len(gh) == len(oh), (name, len(gh), len(oh))
    for f in TC.FIELDS:
        assert np.array_equal(gh[f], oh[f]), (name, f)
    assert np.array_equal(gc, oc), name
    for k in ('candidates', 'pairs', 'tracebacks', 'cells'):
        assert st[k] == ost[k], (name, k, st[k], ost[k])
    assert st['hits'] == len(oh) and st['tracebacks_gapless'] == tc['gapless'], (name, st, tc)


def _search(ctx, name, group='case'):
    """the case on ctx, with the case's grouping (or the one given; None: off) -> (hits, cigar, stats), labels"""
    case = TC.CASES[name]()
    g = case['group'] if group == 'case' else group
    ctx.set_query_aa(case['q'])
    ctx.set_ref_aa(case['t'])
    groups = case['par'].get('groups')
    ctx.set_target_groups(np.repeat(np.arange(len(groups)), groups) if groups else None)      # (a batch of reference sets; None clears)
    if g:
        ctx.set_grouping(g['n_nodes'], g['node_of_target'], q_base=g['q_base'])
    else:
        ctx.set_grouping(0)
    got = ctx.search(TC.native_params(case))
    lab = None if not g else ctx.labels.copy()
    ctx.set_grouping(0)
    ctx.set_target_groups(None)
    return got, lab


def _cmp_labels(ctx, lab, name, g):
    oh = TC.oracle(name)[0]
    want = ctx.components_of_hits(g['n_nodes'], oh, g['node_of_target'], q_base=g['q_base'])
    assert np.array_equal(lab, want), name
    assert np.array_equal(lab, TC.labels_of(g['n_nodes'], g['q_base'], g['node_of_target'], oh)), name


@pytest.mark.parametrize('name', ['sel_0', 'sel_1', 'sel_255', 'sel_256', 'sel_257', 'sel_513', 'straddle_1', 'straddle_5', 'keep_none', 'keep_all',
                                  'long_cigar', 'short', 'hsp_1', 'hsp_2', 'batch'])
def test_case_equals_oracle(ctx, name):
    """twice on the module's context: whatever the staging area held before (too small: the overflow path; large enough: the packed path)"""
    case = TC.CASES[name]()
    for _ in range(2):
        got, lab = _search(ctx, name)
        _cmp(got, name)
        if case['group']:
            _cmp_labels(ctx, lab, name, case['group'])


def test_staging_overflow_then_packed_then_overflow_again():
    """a fresh context's staging area holds the header only: its first search overflows and is copied the classic way, the same search again
    leaves through pack_out, a larger result overflows again - with the labels of single linkage each time"""
    from peppan_amd import _native as N
    with N.Context(0) as c:
        for name in ('sel_255', 'sel_255', 'keep_all', 'keep_all', 'sel_1'):
            case = TC.CASES[name]()
            g = TC.grouping(len(case['q']), len(case['t']), 4, 2)
            got, lab = _search(c, name, g)
            _cmp(got, name)
            _cmp_labels(c, lab, name, g)


def test_grouping_switched_on_and_off_between_searches(ctx):
    """a search with grouping directly behind one without, in one context, and back; another node map behind the first"""
    case = TC.CASES['sel_513']()
    g1 = TC.grouping(len(case['q']), len(case['t']), 9, 4)
    g2 = TC.grouping(len(case['q']), len(case['t']), 0, 1)
    for g in (None, g1, None, g2, g1):
        got, lab = _search(ctx, 'sel_513', g)
        _cmp(got, 'sel_513')
        if g:
            _cmp_labels(ctx, lab, 'sel_513', g)
        else:
            assert lab is None


def test_exactly_sized_path_gives_the_same_bytes(ctx):
    """params.reserved2 bit 0: the two-kernel path (topk, emit) that sizes its table after reading the counts, and K10 queued behind it"""
    for name in ('straddle_5', 'long_cigar', 'hsp_1'):
        case = TC.CASES[name]()
        g = TC.grouping(len(case['q']), len(case['t']), 2, 3)
        ctx.set_query_aa(case['q']); ctx.set_ref_aa(case['t'])
        ctx.set_grouping(g['n_nodes'], g['node_of_target'], q_base=g['q_base'])
        out = []
        for flag in (0, 1):
            p = TC.native_params(case)
            p.reserved2 = flag
            h, c, st = ctx.search(p)
            out.append((h.tobytes(), c.tobytes(), ctx.labels.tobytes()))
            _cmp((h, c, st), name)
        ctx.set_grouping(0)
        assert out[0] == out[1], name
