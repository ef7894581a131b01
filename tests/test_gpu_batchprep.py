"""K26 on the GPU (csrc/batchprep.hip: the front half of a round of filt_genes, PEPPAN.py:546-624 and :641-656) against the plain-Python restatement of
include/peppan_hip.h (tests/batchprep_helpers.py) and against what the reference's own filt_genes recorded (tests/golden/g29_batchprep.json.gz):
rows, flags and counts compared with ==.

The shapes are batchprep_helpers.edge_cases: 1, 2, 63, 64, 65 rows; 4096 rows (the largest gene whose working arrays stay in LDS) and 4097; one batch that
mixes both paths; either path forced; one genome; G = n; empty lists; one list of 5 000 entries; ties in column 2 that decide which row stays; ties in
column 3; a batch of zero genes; a refused call followed by a good one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batchprep_helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu

CI = 0.9
CASES = H.edge_cases()
NAMES = sorted(CASES)


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


@pytest.fixture(scope='module')
def ctx(N):
    with N.Context(0) as c:
        yield c


@pytest.fixture(scope='module')
def golden():
    return H.load_golden()


@pytest.fixture(scope='module')
def restated():
    """(mode, name) -> (rows, inparalog, final, tie), computed once"""
    return {(mode, k): H.prune(CASES[k][0], CASES[k][1], mode, CI, 10000 * CI) for mode in (H.NJ, H.SBH) for k in NAMES}


def prune(ctx, names, mode, path):
    B = H.batch_of([CASES[k] for k in names])
    n_loci = max(max(B['cols'][5]), max(B['cfl'] or [0]) // 10) + 1
    out_off, rows, inparalog, final, n_ties = ctx.batch_prune(mode, B['gene_off'], B['cols'][1], B['cols'][2], B['cols'][3], B['cols'][4], B['cols'][5], B['cfl_off'],
                                                              B['cfl'], n_loci, CI, 10000 * CI, path)
    return {k: (rows[int(out_off[j]):int(out_off[j + 1])].tolist(), bool(inparalog[j]), bool(final[j])) for j, k in enumerate(names)}, n_ties


@pytest.fixture(scope='module')
def batches(ctx, N):
    """every edge case in ONE call per mode and path: (mode, path) -> (name -> result, n_ties).  PREP_AUTO is the batch that mixes both paths"""
    out = {}
    for mode in (H.NJ, H.SBH):
        for path in (N.PREP_AUTO, N.PREP_LDS, N.PREP_WS):
            names = [k for k in NAMES if path != N.PREP_LDS or len(CASES[k][0]) <= N.PREP_LDS_ROWS]
            out[mode, path] = prune(ctx, names, mode, path)
    return out


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('mode', (H.NJ, H.SBH))
def test_both_paths_equal_the_restatement(batches, restated, N, mode, name):
    want = restated[mode, name]
    assert batches[mode, N.PREP_AUTO][0][name] == want[:3]
    assert batches[mode, N.PREP_WS][0][name] == want[:3]                  # identical bits on the forced workspace path ...
    if len(CASES[name][0]) <= N.PREP_LDS_ROWS:
        assert batches[mode, N.PREP_LDS][0][name] == want[:3]             # ... and on the forced LDS path


def test_tie_counts_and_the_tie_rule(batches, restated, N):
    ties = sum(1 for k in NAMES if restated[H.NJ, k][3])
    assert ties >= 2 and restated[H.NJ, 'tie_decides'][3] and restated[H.NJ, 'ties2'][3] and not restated[H.NJ, 'tie3_order'][3]
    assert batches[H.NJ, N.PREP_AUTO][1] == batches[H.NJ, N.PREP_WS][1] == ties
    assert batches[H.SBH, N.PREP_AUTO][1] == 0
    # the first of two tied rows that name each other stays; ties in column 3 keep the order the sort by column 2 left
    assert batches[H.NJ, N.PREP_AUTO][0]['tie_decides'] == ([0, 2, 3], True, False)
    assert batches[H.NJ, N.PREP_AUTO][0]['tie3_order'] == ([3, 2, 1, 0], True, False)


def test_the_cases_reach_what_they_are_meant_to(restated, N):
    seen = {}
    for k in ('lds_max', 'lds_max_plus_1', 'cut_plain'):
        H.prune(CASES[k][0], CASES[k][1], H.NJ, CI, 10000 * CI, seen)
    assert seen.get('walk_skipped') and (seen.get('cut_low', 0) + seen.get('cut_clust', 0) + seen.get('cut_6g', 0)) == 3 and len(set(seen) & {'cut_low', 'cut_clust', 'cut_6g'}) >= 2
    assert len(CASES['lds_max'][0]) == N.PREP_LDS_ROWS and len(CASES['lds_max_plus_1'][0]) == N.PREP_LDS_ROWS + 1
    assert max(len(v) for v in CASES['long_list'][1].values()) == 5000
    assert restated[H.NJ, 'n1'][:3] == ([0], False, True)


def test_zero_genes_and_a_refusal_then_a_good_call(ctx, N, restated):
    out_off, rows, inparalog, final, n_ties = ctx.batch_prune(H.NJ, [0], [], [], [], [], [], [0], [], 0, CI, 9000.0)
    assert out_off.tolist() == [0] and len(rows) == len(inparalog) == len(final) == 0 and n_ties == 0
    assert [len(x) for x in ctx.batch_screen([0], [], [], [], 8800.0)] == [0, 0, 0, 0]
    with pytest.raises(N.PepError, match=r'pep_batch_prune failed \(-3\): pep_batch_prune: gene 0 has 4097 rows, the LDS path takes 4096'):
        prune(ctx, ['lds_max_plus_1'], H.NJ, N.PREP_LDS)
    with pytest.raises(N.PepError, match=r'pep_batch_screen failed \(-2\): pep_batch_screen: gene 0 has no row with column 3 above 0'):
        ctx.batch_screen([0, 2], [0, -4], [0, 1], [0, 0], 8800.0)
    assert prune(ctx, ['n65'], H.NJ, N.PREP_AUTO)[0]['n65'] == restated[H.NJ, 'n65'][:3]


def test_call_times_of_screen_and_prune(ctx, N):
    """pep_call_times(PEP_CALL_BATCH_SCREEN) and (PEP_CALL_BATCH_PRUNE): with every phase timed slot 0, the call's kernel time, is > 0 and the other seven and
    the byte counts 0, each call in its own record; a call that its checks refuse leaves zeros; untimed, every slot is 0.  Each wrapper makes one library
    call: its total is that call's record."""
    screen = lambda: ctx.batch_screen([0, 2], [7000, -4], [0, 1], [0, 0], 8800.0)          # noqa: E731
    ctx.set_timing(2)
    try:
        for which, call in ((N.CALL_BATCH_SCREEN, screen), (N.CALL_BATCH_PRUNE, lambda: prune(ctx, ['n65'], H.NJ, N.PREP_AUTO))):
            other = ctx.call_times(N.CALL_BATCH_SCREEN + N.CALL_BATCH_PRUNE - which)
            call()
            for total in (False, True):
                ms, to_device, to_host = ctx.call_times(which, total=total)
                print('call %d total=%r: ms %r' % (which, total, ms.tolist()))
                assert ms.shape == (8,) and ms[0] > 0 and not ms[1:].any() and (to_device, to_host) == (0, 0)
            assert ctx.call_times(N.CALL_BATCH_SCREEN + N.CALL_BATCH_PRUNE - which)[0].tobytes() == other[0].tobytes()
        with pytest.raises(N.PepError, match='no row with column 3 above 0'):
            ctx.batch_screen([0, 2], [0, -4], [0, 1], [0, 0], 8800.0)
        assert not ctx.call_times(N.CALL_BATCH_SCREEN)[0].any() and not ctx.call_times(N.CALL_BATCH_SCREEN, total=True)[0].any()
        assert ctx.call_times(N.CALL_BATCH_PRUNE)[0][0] > 0
    finally:
        ctx.set_timing(0)
    screen()
    prune(ctx, ['n65'], H.NJ, N.PREP_AUTO)
    for which in (N.CALL_BATCH_SCREEN, N.CALL_BATCH_PRUNE):
        assert not ctx.call_times(which)[0].any() and not ctx.call_times(which, total=True)[0].any()


def test_screen_equals_the_restatement(ctx):
    rng = H.rng_of(126)
    tables, used, locus0 = [], {}, 0
    for n in (1, 2, 63, 64, 65, 257, 700):
        table, _ = H.random_gene(rng, n, max(1, n // 2), locus0)
        for r in table:
            r[4] = r[3]
            if rng.random() < 0.5:
                used[r[5]] = rng.choice((0, -(5000 + 1000), 7000 + 1000))
        tables.append(table)
        locus0 += n
    for r in tables[3]:                                            # a gene `used` holds every row of: nothing present
        used[r[5]] = 0
    B = H.batch_of([(t, {}) for t in tables])
    state = np.zeros(locus0, np.uint8)
    for l, v in used.items():
        state[l] = 2 if v > 0 else 1
    out3, out4, present, excluded = ctx.batch_screen(B['gene_off'], B['cols'][3], B['cols'][5], state, (CI - 0.02) * 10000)
    n_excluded = 0
    for k, t in enumerate(tables):
        want, p, ex = H.screen(t, used, (CI - 0.02) * 10000)
        a, b = B['gene_off'][k], B['gene_off'][k + 1]
        assert (out3[a:b].tolist(), out4[a:b].tolist(), int(present[k]), bool(excluded[k])) == ([r[3] for r in want], [r[4] for r in want], p, ex)
        n_excluded += ex
    assert 1 <= n_excluded < len(tables)


def test_prepare_batch_against_the_fixture(golden, tmp_path_factory):
    from peppan_amd import paralogfilter
    params = H.golden_stores(golden, str(tmp_path_factory.mktemp('batchprep')))
    _, _, conflicting = H.golden_inputs(golden)
    for orthology in ('nj', 'sbh'):
        params['orthology'] = orthology

        def each(rnd, got):
            start = rnd['start']
            res = paralogfilter.prepare_batch(params['map_bsn'] + '.tab.npz', params['map_bsn'] + '.conflicts.npz', [(g, s) for g, s in start['genes']],
                                              dict((k, v) for k, v in start['used']), {int(g): None for g in start['new_groups']}, params,
                                              conflicting=np.array(conflicting).reshape(-1, 2))
            assert not res.abandoned and res.n_ties == got['n_ties'] == 0
            by = lambda s: sorted(g for g, x in res.status.items() if x == s)      # noqa: E731
            assert by('excluded') == sorted(got['excluded']) and by('withdrawn') == got['withdrawn'] and by('popped') == sorted(got['popped'])
            assert {g: s for g, s in res.status.items() if g in got['status']} == got['status']
            for g, m in got['mats'].items():
                assert res.mats[g].tolist() == m and H.recorded(res.mats[g].tolist()) == rnd['after_c']['new_groups'][str(g)]
                assert res.inparalog[g] == got['inparalog'][g]
                assert {l: v.tolist() for l, v in res.conflicts[g].items()} == got['conflicts'][g]

        assert H.check_run(golden, orthology, each=each) == 3


def test_filt_genes_against_the_fixture(golden, tmp_path_factory):
    from peppan_amd import paralogfilter
    params = H.golden_stores(golden, str(tmp_path_factory.mktemp('filt_genes')))
    tab, _, _ = H.golden_inputs(golden)
    for orthology in ('nj', 'sbh'):
        params['orthology'] = orthology
        mat_out, sent = [], []

        def per_groups(to_run):
            sent.append([[int(d[0][0][0]), int(d[0].shape[0]), bool(d[1]), int(d[2])] for d in to_run])
            return [[d[0]] for d in to_run]

        n_ties = paralogfilter.filt_genes(params['map_bsn'] + '.tab.npz', np.array(golden['ortho_groups']), 'unused.npy', params['map_bsn'] + '.conflicts.npz',
                                          {int(k): list(v) for k, v in golden['priorities'].items()}, {int(k): v for k, v in golden['scores'].items()},
                                          {'gene%d' % i: i for i in range(max(tab) + 1)}, params, mat_out, per_groups=per_groups)
        want = golden['runs'][orthology]
        assert n_ties == 0 and mat_out[-1] == [0, 0, 0, []] and len(mat_out) == len(want['mat_out']) + 1
        for got, rec in zip(mat_out, want['mat_out']):
            assert [got[0], got[1], int(got[2]), H.recorded(got[3].tolist())] == rec
        assert sent == [r for r in want['run'] if r]                 # (the reference maps over an empty to_run list too)
