"""No GPU: every case of tests/topk_emit_cases.py is where its name says - proved from the oracle's counters and tables alone -, and the closed form of
a band's cell count (pep_band_cells of common.h, restated in plain Python) equals the loop over the band's 128 diagonals it replaces."""
import numpy as np
import pytest

import topk_emit_cases as TC

TILE = TC.TILE


def _classes(case, t):
    return np.asarray(t, dtype=np.int64) % case['par']['n_splits']


@pytest.mark.parametrize('n_sel', [0, 1, 255, 256, 257, 513])
def test_selected_pairs_stand_around_the_tile_sizes(n_sel):
    name = 'sel_%d' % n_sel
    hits, _, st, _ = TC.oracle(name)
    assert st['tracebacks'] == n_sel
    assert st['candidates'] > 0                                      # (0 selected pairs: the kernels do run, over candidates that all die at the score cut)
    assert len(TC.oracle_selected(name)) == n_sel
    if n_sel:
        assert 0 < len(hits) <= n_sel
    assert TC.CASES['sel_257']()['par']['top_k'] == 1 and len(TC.oracle('sel_257')[0]) < 257      # one of the sizes cuts: kept and dropped pairs side by side


@pytest.mark.parametrize('n_splits', [1, 5])
def test_straddling_group_has_ties_and_more_passing_pairs_than_top_k(n_splits):
    name = 'straddle_%d' % n_splits
    case = TC.CASES[name]()
    sel = TC.oracle_selected(name)
    mine = np.flatnonzero(sel['q'] == case['star'])
    assert mine[0] < TILE <= mine[-1] and np.array_equal(mine, np.arange(mine[0], mine[-1] + 1))      # its slots lie on both sides of the tile boundary
    assert len(sel) > TILE
    passing = TC.oracle_passing(name)
    p = passing[passing['q'] == case['star']]
    cls = _classes(case, p['t'])
    top_k = case['par']['top_k']
    assert all((cls == c).sum() > top_k for c in range(n_splits))      # every class has to cut
    # ties in score between different targets of one class (the three copies of a relative), and the lowest target index wins them
    hits = TC.oracle(name)[0]
    kept = hits[hits['q'] == case['star']]
    assert len(kept) == top_k * n_splits
    tied = 0
    for c in range(n_splits):
        pc, kc = p[cls == c], kept[_classes(case, kept['t']) == c]
        cut = kc['score'].min()
        assert (pc['score'] > cut).sum() < top_k <= (pc['score'] >= cut).sum()
        at_cut = np.sort(pc['t'][pc['score'] == cut])
        tied += len(at_cut) > (kc['score'] == cut).sum()
        assert np.array_equal(np.sort(kc['t'][kc['score'] == cut]), at_cut[:(kc['score'] == cut).sum()])
        assert len(set(pc['score'].tolist())) < len(pc)
    assert tied                                                        # a tie that the cut goes through: the target index decided
    assert (p['t'] >= case['first']).sum() == 30


def test_band_order_decides_between_two_bands_of_one_pair():
    case = TC.CASES['hsp_1']()
    q, t = case['twice']
    both = TC.oracle_passing('hsp_1')
    both = both[(both['q'] == q) & (both['t'] == t)]
    assert len(both) == 2 and both['score'][0] == both['score'][1] and both['bin'][0] != both['bin'][1]
    kept = TC.oracle('hsp_1')[0]
    kept = kept[kept['q'] == q]
    assert len(kept) == 1 and kept['t'][0] == t and kept['bin'][0] == both['bin'].min()


@pytest.mark.parametrize('mode', [1, 2])
def test_mode_cases_stand_one_pair_behind_the_tile(mode):
    hits, _, st, _ = TC.oracle('hsp_%d' % mode)
    assert st['tracebacks'] == TILE + 1 and len(hits) > 0
    assert TC.CASES['hsp_%d' % mode]()['par']['hsp_mode'] == mode


def test_batch_case_cuts_per_reference_set():
    case = TC.CASES['batch']()
    hits, cig, st, _ = TC.oracle('batch')
    assert st['tracebacks'] == TILE + 1 and hits['cigar_runs'].sum() == len(cig)
    assert np.array_equal(hits['cigar_off'], np.concatenate([[0], np.cumsum(hits['cigar_runs'])[:-1]]))
    first = case['par']['groups'][0]
    per_set = [(hits['q'][hits['t'] < first]), (hits['q'][hits['t'] >= first])]
    both = set(per_set[0].tolist()) & set(per_set[1].tolist())
    assert len(both) > 20                                              # queries that keep a hit in either set: one search over all targets would cut one of them
    whole = TC._oracle_search(case['q'], case['t'], {k: v for k, v in case['par'].items() if k != 'groups'})[0]
    assert len(whole) < len(hits)


def test_keep_extremes():
    hits, _, st, _ = TC.oracle('keep_none')
    assert st['tracebacks'] == TILE + 1 and len(hits) == 0
    hits, _, st, _ = TC.oracle('keep_all')
    assert st['tracebacks'] == 2 * TILE + 1 == len(hits)           # every selected pair is a hit: the first two tiles keep all 256


def test_long_cigar_case_has_every_kind_of_run_list():
    case = TC.CASES['long_cigar']()
    hits, cig, st, tc = TC.oracle('long_cigar')
    assert st['tracebacks'] < TILE                                    # one tile
    long = hits[(hits['q'] == case['long_q']) & (hits['t'] == case['long_t'])]
    assert len(long) == 1 and long['cigar_runs'][0] == 2 * case['n_ins'] + 1 > TILE
    assert long['cigar_runs'][0] <= 2 * min(len(case['q'][case['long_q']]), len(case['t'][case['long_t']])) + 1
    assert (hits['cigar_runs'] == 1).sum() > 0 and ((hits['cigar_runs'] > 1) & (hits['cigar_runs'] < 10)).sum() > 0
    assert tc['gapless'] > 0 and tc['traced'] > tc['gapless']         # rule-5a pairs and swept pairs in the one tile
    assert hits['cigar_runs'].sum() == len(cig)


def test_short_case_has_bands_that_leave_the_matrix_on_every_side():
    case = TC.CASES['short']()
    hits = TC.oracle('short')[0]
    kinds = {(False, False): 0, (True, False): 0, (False, True): 0, (True, True): 0}
    for h in hits:
        kinds[TC.clipping(h, case['q'], case['t'])] += 1
        Lq, Lt = len(case['q'][int(h['q'])]), len(case['t'][int(h['t'])])
        assert int(h['cells']) == TC.cells_loop(Lq, Lt, TC.band_dlo(h['bin'])) == TC.cells_closed(Lq, Lt, TC.band_dlo(h['bin']))
    assert kinds[(True, False)] and kinds[(False, True)] and kinds[(True, True)], kinds
    lens = [len(s) for s in case['q'] + case['t']]
    assert min(lens) < 64 and sum(1 for x in lens if x < 64) > 20 and sum(1 for x in lens if 64 <= x < 128) > 20


def test_groupings_cover_the_variants():
    g = {name: TC.CASES[name]()['group'] for name in TC.CASES}
    assert any(x and x['q_base'] != 0 and len(set(x['node_of_target'].tolist())) < len(x['node_of_target']) for x in g.values())      # an offset, several targets per node
    assert any(x and x['q_base'] == 0 for x in g.values()) and any(x is None for x in g.values())
    for name, x in g.items():
        if x:
            case = TC.CASES[name]()
            assert len(x['node_of_target']) == len(case['t']) and int(x['node_of_target'].max()) < x['n_nodes'] and len(case['q']) + x['q_base'] <= x['n_nodes']
    # the plain-Python labels: the smallest node of every component
    lab = TC.labels_of(8, 2, np.array([0, 0, 7], dtype=np.uint32), np.array([(0, 0), (1, 1), (3, 2)], dtype=[('q', '<u4'), ('t', '<u4')]))
    assert lab.tolist() == [0, 1, 0, 0, 4, 5, 6, 5]


def test_closed_form_cells_equal_the_loop_over_the_diagonals():
    """all (Lq, Lt, dlo) with lengths 1 .. 200 and dlo -260 .. 260"""
    lt = np.arange(1, 201, dtype=np.int64)[:, None]
    dlo = np.arange(-260, 261, dtype=np.int64)[None, :]
    for lq in range(1, 201):
        a, b = TC.cells_closed_grid(lq, lt, dlo), TC.cells_loop_grid(lq, lt, dlo)
        assert np.array_equal(a, b), lq
    rng = np.random.default_rng(5)
    for _ in range(300):                                               # the scalar restatements agree with the grids
        Lq, Lt, d = int(rng.integers(1, 201)), int(rng.integers(1, 201)), int(rng.integers(-260, 261))
        assert TC.cells_closed(Lq, Lt, d) == TC.cells_loop(Lq, Lt, d) == int(TC.cells_loop_grid(Lq, Lt, d))
