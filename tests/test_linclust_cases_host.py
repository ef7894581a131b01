"""The cases of tests/linclust_cases.py through the oracle and through the restatement of the oracle's definition (linclust_cases.restate): the
two agree on the representatives and on the three totals wherever the gapped stage rescues nothing, and each case is what its name says, so
that no case of tests/test_gpu_linclust.py can pass vacuously.  A case that fails here is a broken case, not a skip."""
import math

import numpy as np
import pytest

import linclust_cases as LC

CASES = LC.cases()
TOTALS = ('selected', 'verified', 'accepted')
by_family = lambda *fam: [c for c in CASES if c['family'] in fam]
ids = lambda c: c['name']


def _both(case):
    return LC.restated(case['name']), LC.oracle_results()[case['name']]


def test_cases_stay_small():
    assert len(CASES) == len(set(c['name'] for c in CASES))
    for c in CASES:
        assert len(c['seqs']) <= 450, c['name']
        longest = sorted(len(s) for s in c['seqs'])
        assert longest[-1] <= 1300 or (c['family'] == 'long' and longest[-1] == 70000 and longest[-2] <= 1300), c['name']
    grid = set((c['base'], c['k'], c['m'], len(c['seqs'][0]) - c['k']) for c in by_family('witness'))
    assert grid >= set((b, k, m, e) for b, k, m in LC.WITNESS_PARAMS for e, _ in LC.WITNESS_SHAPES) and len(by_family('witness')) == 99 + 3
    assert len(by_family('ties')) == 12 and len(by_family('exact')) == 1 and sum(len(c['pairs']) for c in by_family('ties')) == 216


@pytest.mark.parametrize('case', [c for c in CASES if c['family'] != 'gapped'], ids=ids)
def test_oracle_equals_restatement(case):
    r, (o_rep, o_st) = _both(case)
    assert {t: r[t] for t in TOTALS} == o_st
    assert np.array_equal(r['rep'], o_rep)
    if case['family'] in ('witness', 'long', 'limit', 'repeat', 'shape') or (case['min_id'], case['min_cov']) == (0., 0.):
        assert r['failed'] == 0
    for key in ('selected', 'verified'):
        if key in case:
            assert r[key] == case[key]


def test_gapped_family_is_rescued_with_gaps():
    (case,) = by_family('gapped')
    assert len(case['seqs']) == 12
    r, (o_rep, o_st) = _both(case)
    assert (r['selected'], r['verified']) == (o_st['selected'], o_st['verified'])
    assert r['failed'] > 0 and o_st['accepted'] > r['accepted']
    assert len(set(o_rep.tolist())) < len(set(r['rep'].tolist()))


@pytest.mark.parametrize('case', by_family('witness', 'limit'), ids=ids)
def test_witnesses_spell_out_the_selection(case):
    """a witness per valid window of A; the members of A are the witnesses of the positions A selected: min(m, valid windows) of them"""
    r, (o_rep, _) = _both(case)
    a, k, m, base = case['seqs'][0], case['k'], case['m'], case['base']
    valid = LC.windows(a, base, k)[0].tolist()
    assert case['positions'] == valid and len(case['seqs']) == 1 + len(valid)
    n_flank = min(m - 1, len(a) - k)
    for p, w in zip(valid, case['seqs'][1:]):
        assert len(w) == k + n_flank <= len(a) and (w < base).all()
        at = [i for i in range(n_flank + 1) if np.array_equal(w[i:i + k], a[p:p + k])]
        assert len(at) == 1
        i = at[0]
        assert i == 0 or p == 0 or w[i - 1] != a[p - 1]
        assert i == n_flank or p + k == len(a) or w[i + k] != a[p + k]
    chosen = sorted(p for p, _ in r['sel'][0])
    assert len(chosen) == min(m, len(valid))
    for rep in (r['rep'], o_rep):
        assert [p for p, x in zip(valid, rep[1:]) if x == 0] == chosen
        assert int((rep[1:] == 0).sum()) == min(m, len(valid))


def test_witness_grid_reaches_the_stretches_of_the_selection():
    """ceil(windows / 64) = 1, 2, 3 and 5 positions per lane, lanes without a position, and a bad letter at the three places named"""
    per = set(-(-(len(c['seqs'][0]) - c['k'] + 1) // 64) for c in by_family('witness'))
    assert per == {1, 2, 3, 5}
    named = {c['name'].split('/')[1]: c for c in by_family('witness') if '/bad_' in c['name']}
    assert len(named) == 3
    for c in named.values():
        a = c['seqs'][0]
        (at,) = np.nonzero(a >= 4)[0].tolist()
        assert len(a) - 17 + 1 == 130 and (at % 3 == 2 and 'before_stretch' in c['name'] or at % 3 == 0 and 'stretch_start' in c['name']
                                           or (at - 16) % 3 == 0 and 'first_window_end' in c['name'])


def test_long_sequence_passes_16_bits():
    flanks, bare = by_family('long')
    for case in (flanks, bare):
        r, (o_rep, _) = _both(case)
        assert len(case['seqs'][0]) == 70000 and len(case['positions']) == 40
        chosen = sorted(p for p, _ in r['sel'][0])
        assert chosen == case['chosen'] and chosen[-1] > 65535 > chosen[0] and max(case['positions'][20:]) > 65535
        assert [p for p, x in zip(case['positions'], o_rep[1:]) if x == 0] == chosen
    assert all(len(w) == 17 for w in bare['seqs'][1:]) and bare['min_id'] == 1.


@pytest.mark.parametrize('case', by_family('ladder'), ids=ids)
def test_ladders_are_deep(case):
    r = LC.restated(case['name'])
    assert r['depth'] == case['depth'] >= 20
    assert r['rounds'] >= case.get('rounds_min', 0)
    rep = r['rep']
    assert (rep[rep] == rep).all() and 1 < len(set(rep.tolist())) < len(rep)
    if 'reversed' in case['name']:
        twin = next(c for c in CASES if c['name'] == case['name'].replace('_reversed', ''))
        assert all(np.array_equal(x, y) for x, y in zip(case['seqs'], twin['seqs'][::-1]))
        assert np.array_equal(len(rep) - 1 - rep[::-1], LC.restated(twin['name'])['rep'])      # lengths differ: the order of the indices decides nothing
    if '257' in case['name']:
        assert len(case['seqs']) == 257


def test_ladder_measurements():
    """the depths measured when the ladder was chosen (a property of the seed, stated so that a change of the builder shows)"""
    depth = {c['name']: c['depth'] for c in by_family('ladder')}
    assert (depth['ladder/100_id0_cov0'], depth['ladder/100_id0.9_cov0.5'], depth['ladder/100_id0.9_cov0.9']) == (66, 66, 22)


@pytest.mark.parametrize('case', by_family('ties'), ids=ids)
def test_tie_pairs_sit_on_the_thresholds(case):
    """per pair: the named match counts straddle min_id * ovl, the overlaps straddle min_cov * Lc, the pair is verified once on the slice's
    diagonal, and it is accepted exactly if both comparisons hold in doubles"""
    r, (o_rep, _) = _both(case)
    min_id, min_cov = case['min_id'], case['min_cov']
    assert [(p['Lc'], p['ovl'], p['matches'], p['which']) for p in case['pairs']] == LC.tie_grid(min_id, min_cov)
    seen = set()
    for p in case['pairs']:
        c, s = case['seqs'][p['centre']], case['seqs'][p['member']]
        assert (len(c), len(s)) == (p['Lc'], p['ovl'])
        starts = [x for x in range(len(c) - len(s) + 1) if int((c[x:x + len(s)] == s).sum()) == p['matches']
                  and np.array_equal(c[x:x + 20], s[:20]) and np.array_equal(c[x + len(s) - 20:x + len(s)], s[-20:])]
        assert len(starts) == 1
        x = min_id * p['ovl']
        which = p['which'].split('=')
        assert ('ceil-1' in which) == (p['matches'] == math.ceil(x) - 1) and ('ceil' in which) == (p['matches'] == math.ceil(x)) \
            and ('floor' in which) == (p['matches'] == math.floor(x))
        assert math.ceil(x) - 1 < x <= math.ceil(x) and math.floor(x) <= x
        id_ok, cov_ok = float(p['matches']) >= x, float(p['ovl']) >= min_cov * p['Lc']
        assert id_ok == ('ceil-1' not in which)
        assert cov_ok == (p['ovl'] >= math.ceil(min_cov * p['Lc']))
        seen.add((p['Lc'], p['ovl'] - math.ceil(min_cov * p['Lc']), id_ok))
        for rep in (r['rep'], o_rep):
            assert rep[p['centre']] == p['centre'] and rep[p['member']] == (p['centre'] if id_ok and cov_ok else p['member'])
    assert seen == set((lc, e, ok) for lc in LC.TIE_LC for e in (-1, 0, 1) for ok in (False, True))
    assert r['verified'] == len(case['pairs']) and r['accepted'] == sum(1 for lc, e, ok in seen if e >= 0 and ok)


def test_ties_hold_exact_equalities():
    """Where threshold * length is an integer in exact arithmetic, the one rounding of the double product lands on that integer (0.9 * 100 ==
    90.0), so a count equal to it passes `>=`: the grid holds such pairs for both comparisons, and nowhere in it do doubles and rationals
    put a count on different sides"""
    from fractions import Fraction
    exact_id = exact_cov = 0
    for case in by_family('ties'):
        fid, fcov = Fraction(repr(case['min_id'])), Fraction(repr(case['min_cov']))
        for p in case['pairs']:
            assert math.ceil(case['min_id'] * p['ovl']) == math.ceil(fid * p['ovl']) and math.ceil(case['min_cov'] * p['Lc']) == math.ceil(fcov * p['Lc'])
            exact_id += p['matches'] == fid * p['ovl']
            exact_cov += p['ovl'] == fcov * p['Lc']
    assert 0.9 * 100 == 90.0 and exact_id >= 12 and exact_cov >= 12
    case = next(c for c in CASES if c['name'] == 'ties/id0.9_cov0.9')
    (p,) = [p for p in case['pairs'] if (p['Lc'], p['ovl'], p['matches']) == (100, 90, 81)]
    assert LC.restated(case['name'])['rep'][p['member']] == p['centre']


def test_exact_ties_are_decided_without_gaps():
    """equality holds as named, the pair is a member, and one unit in the last place of the threshold parts it from its centre for good: the
    gapped stage does not bring it back, so the `>=` of the ungapped comparisons decides these pairs"""
    from oracle import oracle as O
    (case,) = by_family('exact')
    r, (o_rep, _) = _both(case)
    min_id, min_cov = case['min_id'], case['min_cov']
    assert set(e for p in case['pairs'] for e in p['exact']) == {'id', 'cov'} and any(p['exact'] == ('id',) for p in case['pairs']) \
        and any(p['exact'] == ('cov',) for p in case['pairs'])
    for p in case['pairs']:
        c, s = case['seqs'][p['centre']], case['seqs'][p['member']]
        assert (len(c), len(s)) == (p['Lc'], p['ovl']) and any(int((c[x:x + len(s)] == s).sum()) == p['matches'] for x in range(len(c) - len(s) + 1))
        assert ('id' in p['exact']) == (float(p['matches']) == min_id * p['ovl']) and ('cov' in p['exact']) == (float(p['ovl']) == min_cov * p['Lc'])
        assert float(p['matches']) >= min_id * p['ovl'] and float(p['ovl']) >= min_cov * p['Lc']
        assert r['rep'][p['member']] == o_rep[p['member']] == p['centre']
        if 'id' in p['exact']:
            assert O.linclust([c, s], float(np.nextafter(min_id, 2.)), min_cov)[0].tolist() == [0, 1]
        if 'cov' in p['exact']:
            assert O.linclust([c, s], min_id, float(np.nextafter(min_cov, 2.)))[0].tolist() == [0, 1]


def test_repeats_and_shapes():
    named = {c['name']: c for c in by_family('repeat', 'shape')}
    r = LC.restated('repeat/40_identical')
    assert (r['rep'] == 0).all() and r['verified'] == 39
    # equal lengths: the lowest index is every key's centre, in both orders
    for name in ('repeat/equal_length_variants', 'repeat/equal_length_variants_reversed'):
        assert len(set(len(s) for s in named[name]['seqs'])) == 1 and (LC.restated(name)['rep'] == 0).all()
    # two centres of one length accept the member, each by itself; together the lower index takes it, and both orders occur
    two = named['repeat/two_centres_of_equal_length']
    rep = LC.restated(two['name'])['rep']
    for t in two['triples']:
        a, b, s = (two['seqs'][t[x]] for x in 'abs')
        assert len(a) == len(b) > len(s)
        for c in (a, b):
            assert LC.restate([c, s], two['min_id'], two['min_cov'], 4, 17, 20)['rep'].tolist() == [0, 0]
        assert rep[t['a']] == t['a'] and rep[t['b']] == t['b'] and rep[t['s']] == min(t['a'], t['b'])
    assert set(t['a'] < t['b'] for t in two['triples']) == {False, True}
    # sequences of one, four and twenty-three distinct k-mers: many diagonals to one centre
    few = ('repeat/A100_A60', 'repeat/ACGT30_ACGT20_less_first', 'repeat/unit23x9_slice')
    one_key = [LC.restated(n) for n in few]
    assert [len(set(LC.windows(named[n]['seqs'][0], 4, 17)[1].tolist())) for n in few] == [1, 4, 23]
    assert one_key[0]['verified'] == 20 and sum(r['verified'] for r in one_key) == 41
    assert all(r['rep'].tolist() == [0, 0] and r['accepted'] == 1 for r in one_key)
    assert sorted(len(named['shape/n%d' % n]['seqs']) for n in (1, 3, 4, 5)) == [1, 3, 4, 5]
    assert all(len(s) < 17 for s in named['shape/all_shorter_than_k']['seqs']) and LC.restated('shape/all_shorter_than_k')['selected'] == 0
    assert sum(len(s) for s in named['shape/all_empty']['seqs']) == 0
    lens = [len(s) for s in named['shape/empty_between_full']['seqs']]
    assert lens[0] == lens[-1] == 0 and lens.count(0) == 5 and len(set(LC.restated('shape/empty_between_full')['rep'].tolist())) < len(lens)
    only = named['shape/only_code_base']
    assert (only['seqs'][1] == 4).all() and len(only['seqs'][1]) > 17 and LC.restated(only['name'])['rep'].tolist() == [0, 1, 0, 3]
