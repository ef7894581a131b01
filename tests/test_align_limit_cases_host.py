"""The cases of tests/align_limit_cases.py through the oracle: each is what its name says, and together they stand below, on and above every
limit at which the alignment passes of csrc/sw.hip choose another sweep - so that no case of tests/test_gpu_align_limits.py can pass
vacuously.  A case that fails here is a broken case, not a skip.

What is held: the oracle nominates exactly the candidates the case planted (their number and their cell total), reports one traced,
gapped alignment per planted pair in the planted band, ending on the planted diagonal; its `full_band` counter equals the number of
pairs that align_limit_cases.side() says leave their sub-band; every reported score is the optimum of the whole matrix
(oracle/full_sw.py).  The census tests then read side() over all cases.

align_limit_cases.py cannot see sw.hip: WHOEVER MOVES A LIMIT THERE (fits16, PK_BIAS, the 8 KiB / 3 072 byte caps of pep_sw_run, the window
sizes of the packed sweeps, the gate `nb < 2040`, SUB_LANES) MOVES THE CONSTANT AT THE TOP OF THAT FILE, and the census below then says which
cases have to move with it.  Every limit is covered from two below to two above it, so a limit moved by one unannounced still has cases on
both sides."""
import collections

import numpy as np
import pytest

import align_limit_cases as AL

CASES = AL.cases()
ids = lambda c: c['name']
by_family = lambda *fam: [c for c in CASES if c['family'] in fam]
SIDES = {c['name']: AL.side(c) for c in CASES}
PACKED_SCORE, PACKED_TRACE = ('pk16', 'pk16_chunked'), ('pk16x4', 'pk16x4_chunked')


def rows(which, pred=lambda c: True):
    """(case, row) of side() over all cases"""
    return [(c, r) for c in CASES if pred(c) for r in SIDES[c['name']][which]]


def test_cases_stay_small():
    assert len(CASES) == len(set(c['name'] for c in CASES))
    assert set(c['family'] for c in CASES) == {'eligibility', 'half_word_edge', 'staging', 'step_counter', 'tails', 'sub_band_exit'}
    for c in CASES:
        assert len(c['q']) <= 9 and len(c['t']) <= 9, c['name']
        longest = max(len(s) for s in c['q'] + c['t'])
        assert longest <= 3200 or (c['family'] == 'step_counter' and longest <= 20009), c['name']


@pytest.mark.parametrize('case', CASES, ids=ids)
def test_case_is_what_it_plants(case):
    hits, cig, st, tc = AL.oracle_results()[case['name']]
    planted = AL.candidates(case)
    assert st['candidates'] == len(planted)
    assert st['cells'] == sum(AL.cand_cells(len(case['q'][q]), len(case['t'][t]), b) for q, t, b in planted)
    # one hit per planted pair, from the planted band, ending on the planted diagonal (side() takes the lane of the sub-band from it)
    assert len(hits) == len(case['pairs']) > 0 and st['pairs'] == len(case['pairs'])
    assert sorted((int(h['q']), int(h['t']), int(h['bin'])) for h in hits) == sorted((p['q'], p['t'], p['bin']) for p in case['pairs'])
    end = {(int(h['q']), int(h['t'])): int(h['t_end']) - int(h['q_end']) for h in hits}
    assert all(end[p['q'], p['t']] == p['d_end'] for p in case['pairs'])
    # every pair is traced and none is one ungapped run (rule 5a would settle it without a traceback sweep)
    assert tc['traced'] == st['tracebacks'] == len(case['pairs']) and tc['gapless'] == 0
    for h in hits:
        ops = cig[int(h['cigar_off']):int(h['cigar_off']) + int(h['cigar_runs'])] & 3
        assert (ops != 0).any()
    s = SIDES[case['name']]
    assert tc['full_band'] == sum(r['leaver'] for r in s['trace'])
    # which sweep a candidate takes follows from the arithmetic alone, but for the two cases that say otherwise
    undecided = [r for r in s['score'] + s['trace'] if r['sweep'] is None]
    assert bool(undecided) == bool(case.get('order_dependent', False))


@pytest.mark.parametrize('case', CASES, ids=ids)
def test_reported_scores_are_the_optimum_of_the_whole_matrix(case):
    hits = AL.oracle_results()[case['name']][0]
    full = AL.full_matrix_scores()
    by_pair = {(p['q'], p['t']): p for p in case['pairs']}
    for h in hits:
        assert int(h['score']) == full[AL.pair_key(case, by_pair[int(h['q']), int(h['t'])])]


def test_parameter_blocks_of_both_sides_agree():
    """the block Context.search gets and the block the oracle gets differ in nothing the oracle reads (needs the library, not a GPU)"""
    from oracle import oracle as O
    for c in CASES:
        assert bytes(O.params_from(AL.native_params(c))) == bytes(AL.oracle_params(c)), c['name']


def test_sub_band_never_outgrows_its_band():
    """pep_sw_run keeps one block of room (`the sub-band may need one block more than the band`): over every geometry tried it never does, so
    the limit of the traceback pass is nb_limit on the blocks of the band alone, and the cases around it cover that room too"""
    rng = np.random.default_rng(7)
    geoms = [(Lq, Lt, d) for Lq in (1, 2, 15, 16, 17, 63, 64, 65, 129, 500) for Lt in (1, 2, 16, 31, 64, 127, 128, 300, 501) for d in range(-Lq - 70, Lt + 70, 7)]
    geoms += [(int(a), int(b), int(d)) for a, b, d in zip(rng.integers(1, 3000, 3000), rng.integers(1, 3000, 3000), rng.integers(-3000, 3000, 3000))]
    seen = 0
    for Lq, Lt, d in geoms:
        b = AL.bin_of(d)
        nb = AL.cand_blocks(Lq, Lt, b)
        for end_lane in (0, 15, 16, 17, 31, 32, 33, 47, 48, 63):
            sub = AL.sub_geom(Lq, Lt, b, end_lane)[2]
            assert sub <= nb
            seen += sub == nb > 0
    assert seen > 10000


# ---------------------------------------------------------------------------------------------------------------- the census
def test_census_eligibility():
    """fits16: per table the largest eligible length, one and two around it, and items that hold both kinds"""
    for tab, limit, msub, beyond in (('blosum62', 2961, 11, 3100), ('w127', 256, 127, 300)):
        assert AL.fits16(limit, limit + 5, msub) and not AL.fits16(limit + 1, limit + 5, msub)          # (checked again here: the limit IS the rule's)
        for L in (limit - 1, limit, limit + 1, limit + 2, beyond):
            c = next(c for c in CASES if c['name'] == 'eligibility/%s_w_rich_%d' % (tab, L))
            s = SIDES[c['name']]
            assert AL.max_sub(AL.oracle_params(c)) == msub and len(s['trace']) == 4 and len(s['score']) >= 4
            # the query is the shorter member of each of its four pairs, so the whole search lies on one side of the rule: packed in both passes up to
            # the limit, 32 bits in both passes beyond it
            assert all(min(len(c['q'][r['q']]), len(c['t'][r['t']])) == L and r['eligible'] == (L <= limit) for r in s['score'] + s['trace'])
            assert all((r['sweep'] in PACKED_SCORE) == (L <= limit) for r in s['score'])
            assert all((r['sweep'] in PACKED_TRACE) == (L <= limit) and (r['sweep'] in PACKED_TRACE or r['sweep'].startswith('s32')) for r in s['trace'])
    for c, r in rows('score') + rows('trace'):
        assert r['sweep'] is None or r['eligible'] or r['sweep'].startswith('s32'), c['name']
    # mixed items: an eligible candidate that takes the 32-bit sweep because of its neighbour, in both passes, in searches of 2, 3, 4 and 5
    for n in (2, 3, 4, 5):
        s = SIDES['eligibility/mixed_%d_one_ineligible' % n]
        assert len(s['score']) == n and sum(not r['eligible'] for r in s['score']) == 1
        assert sum(r['sweep'].endswith('+mixed') for r in s['score']) == 1
        assert sum(r['sweep'].endswith('+mixed') for r in s['trace']) == (3 if n >= 4 else 0)
    for name in ('blosum62', 'w127'):
        s = SIDES['eligibility/%s_w_rich_item_with_one_ineligible' % name]
        assert [r['eligible'] for r in s['trace']] == [False, True, True, True] and all(r['sweep'].startswith('s32') for r in s['trace'])


def test_census_scores_at_the_edge_of_the_half_word():
    """per table: a score beyond the half word, where only the 32-bit sweeps may run, and one within 32 000 .. 32 575 from the packed sweeps of both
    passes; gap costs from one end of what pep_search accepts to the other"""
    tables = collections.defaultdict(lambda: dict(beyond=0, edge=0))
    for c in CASES:
        key = (c['params']['table'], bool(c['params'].get('raise')))
        s = SIDES[c['name']]
        if c.get('order_dependent'):
            continue
        sweep = {(r['q'], r['t'], r['bin']): (r['sweep'], None) for r in s['score']}
        for r in s['trace']:
            sweep[r['q'], r['t'], r['bin']] = (sweep[r['q'], r['t'], r['bin']][0], r['sweep'])
        for h in AL.oracle_results()[c['name']][0]:
            sc, tr = sweep[int(h['q']), int(h['t']), int(h['bin'])]
            if h['score'] > AL.HALF_WORD:
                assert sc.startswith('s32') and tr.startswith('s32')
                tables[key]['beyond'] += 1
            if 32000 <= h['score'] <= AL.HALF_WORD - AL.FITS16_SLACK - AL.PK_BIAS and sc in PACKED_SCORE and tr.split('+')[0] in PACKED_TRACE:
                tables[key]['edge'] += 1
    assert set(tables) >= {('blosum62', False), ('blosum62', True), ('edge', False)}
    for key in (('blosum62', False), ('blosum62', True), ('edge', False)):
        assert tables[key]['beyond'] >= 1 and tables[key]['edge'] >= 1, (key, tables[key])
    assert {c['params']['gap'] for c in by_family('half_word_edge')} == set(AL.HALF_WORD_GAPS) == {(11, 1), (0, 1), (255, 1), (1, 255), (255, 255)}
    for c in by_family('half_word_edge'):
        if 'beyond' not in c['name']:
            assert {len(q) for q in c['q']} == {256} and all(r['sweep'] == 'pk16x4' for r in SIDES[c['name']]['trace'])
            assert {p['diags'][-1] for p in c['pairs']} == {1, 19 if c['params']['gap'][1] == 1 else 4}


def _around(limit, seen, below, above, reach=2):
    """block counts limit - reach .. limit + reach are all there; up to the limit every sweep is `below`, beyond it `above`"""
    for nb in range(limit - reach, limit + reach + 1):
        assert seen[nb], (limit, nb)
        assert seen[nb] == ({below} if nb <= limit else {above}), (limit, nb, seen[nb])


def test_census_staging_limits():
    sc, tr = AL.staging(4000, 0, False), AL.staging(4000, 0, True)
    assert (sc['lds_res_bytes'], sc['nb_limit'], sc['chunk'], tr['lds_res_bytes'], tr['nb_limit'], tr['chunk']) == (8192, 117, 38, 8192, 57, 58)
    # longest query + longest target at which split_long comes on: 1 872 residues in the score pass, 912 in the traceback pass
    assert [AL.staging(n, 0, False)['split_long'] for n in (1871, 1872)] == [False, True]
    assert [AL.staging(n, 0, True)['split_long'] for n in (911, 912)] == [False, True]
    stag = lambda c: c['family'] == 'staging' and c['name'].startswith('staging/four_pairs_of')
    # traceback pass, nb_limit, split_long on: whole items of four on either side
    seen = collections.defaultdict(set)
    for c, r in rows('trace', stag):
        if SIDES[c['name']]['staging_trace']['split_long']:
            assert r['nblk_sub'] == r['nblk']
            seen[r['nblk']].add(r['sweep'])
    _around(tr['nb_limit'], seen, 'pk16x4', 'pk16x4_chunked')
    # ... and with split_long off (no pair and no bystander long enough) nothing is above a limit, up to the last block count that can be built so
    off = [(c, r) for c, r in rows('trace', stag) if not SIDES[c['name']]['staging_trace']['split_long']]
    assert {r['nblk'] for c, r in off} == {55, 56, 57} and all(r['sweep'] == 'pk16x4' and not r['long'] for c, r in off)
    # score pass, nb_limit: split_long on by the bystander or by the pairs themselves, and off
    seen, seen_off = collections.defaultdict(set), collections.defaultdict(set)
    for c, r in rows('score', stag):
        (seen if SIDES[c['name']]['staging_score']['split_long'] else seen_off)[r['nblk']].add(r['sweep'])
    _around(sc['nb_limit'], seen, 'pk16', 'pk16_chunked')
    assert set(seen_off) == {55, 56, 57, 58, 59, 60, 115, 116, 117} and all(v == {'pk16'} for v in seen_off.values())
    # the `fits` test of the score pass: 118 blocks are the last that fit 8 KiB.  Behind nb_limit it decides nothing (a candidate above 117 blocks is
    # in the long launch, and without split_long the staging area is sized for the longest pair): the block counts around it are there, all packed
    fits_limit = (AL.LDS_CAP // 8 - AL.SCORE_WIN_PAD) // 8
    assert fits_limit == 118 and all(seen[nb] == {'pk16_chunked'} for nb in range(fits_limit, fits_limit + 3)) and seen[fits_limit - 1] == seen[fits_limit - 2] == {'pk16'}
    # items and pairs that straddle a limit
    assert [r['sweep'] for r in SIDES['staging/score_limit_straddled']['score']] == ['pk16_chunked', 'pk16_chunked', 'pk16', 'pk16']
    assert [r['sweep'] for r in SIDES['staging/trace_limit_four_and_four']['trace']] == ['pk16x4_chunked'] * 4 + ['pk16x4'] * 4
    assert [r['sweep'] for r in SIDES['staging/trace_limit_straddled']['trace']] == ['s32_lds'] * 4          # two above, two below: both items are tails
    assert [r['sweep'] for r in SIDES['staging/five_long_three_short']['trace']] == ['pk16x4_chunked'] * 4 + ['s32_lds'] * 4


def test_census_chunk_multiples():
    """k chunks and k chunks + 1 block, as whole items (the chunk loop runs over the longest member of an item)"""
    sc, tr = AL.staging(4000, 0, False), AL.staging(4000, 0, True)
    for k in (1, 2, 3):
        for extra in (0, 1):
            t = SIDES['staging/trace_chunks_%d_plus_%d' % (k, extra)]['trace']
            assert [(r['nblk_sub'], r['sweep']) for r in t] == [(k * tr['chunk'] + extra, 'pk16x4_chunked')] * 4
    for k in (1, 2, 3, 4, 5, 6):
        for extra in (0, 1):
            s = SIDES['staging/score_chunks_%d_plus_%d' % (k, extra)]['score']
            # one, two and three chunks are below nb_limit: the long launch never sees them, the plain sweep stages them whole
            assert [(r['nblk'], r['sweep']) for r in s] == [(k * sc['chunk'] + extra, 'pk16_chunked' if k >= 4 else 'pk16')] * 4
    assert 3 * sc['chunk'] + 1 <= sc['nb_limit'] < 4 * sc['chunk']


def test_census_step_counter():
    """all eligible, all in the long launch: only the gate decides.  An item's block count is its longest member's"""
    top = {}
    for c in by_family('step_counter'):
        t = SIDES[c['name']]['trace']
        assert len(t) == 4 and all(r['eligible'] and r['long'] and r['nblk_sub'] == r['nblk'] and not r['leaver'] for r in t)
        assert all(r['eligible'] and r['sweep'] == 'pk16_chunked' for r in SIDES[c['name']]['score'])
        sweeps = {r['sweep'] for r in t}
        assert len(sweeps) == 1
        top[max(r['nblk_sub'] for r in t)] = sweeps.pop()
    assert top == {2038: 'pk16x4_chunked', 2039: 'pk16x4_chunked', 2040: 's32_global', 2041: 's32_global', 2501: 's32_global'}
    assert AL.STEP_GATE == 2040 and 16 * (AL.STEP_GATE - 1) < 0x8000


def test_census_tails():
    got = {}
    for c in by_family('tails'):
        s = SIDES[c['name']]
        inel = sum(not r['eligible'] for r in s['trace'])
        assert len(s['score']) == len(s['trace']) and inel == sum(not r['eligible'] for r in s['score']) == (1 if 'ineligible' in c['name'] else 0)
        n = len(s['trace'])
        got[n, inel] = ([r['sweep'] for r in s['score']], [r['sweep'] for r in s['trace']])
        # score pass: an odd count leaves the last candidate alone in its wavefront, still packed (with itself); the ineligible one is the longest
        # and takes its neighbour along.  Traceback pass: the last n mod 4 take the 32-bit sweep, and so does the item of the ineligible one
        if not inel:
            assert got[n, 0] == (['pk16'] * n, ['pk16x4'] * (n - n % 4) + ['s32_lds'] * (n % 4))
        else:
            assert got[n, 1][0] == ['s32_lds'] + (['s32_lds+mixed'] if n > 1 else []) + ['pk16'] * max(0, n - 2)
            assert got[n, 1][1] == (['s32_lds'] + ['s32_lds+mixed'] * 3 if n >= 4 else ['s32_lds'] * n) + ['s32_lds'] * (n % 4 if n >= 4 else 0)
    assert set(got) == {(n, i) for n in (1, 2, 3, 5, 6, 7) for i in (0, 1)}


def test_census_sub_band_exit():
    """the oracle's full_band counter is the number of planted leavers (test_case_is_what_it_plants, case by case); here: how they sit in their items"""
    total = sum(AL.oracle_results()[c['name']][3]['full_band'] for c in CASES)
    assert total >= 8
    for tp in ('', '_transposed'):
        for n in (0, 1, 3, 4):
            t = SIDES['sub_band_exit/%d_of_4_leave%s' % (n, tp)]['trace']
            assert sorted(r['sweep'] for r in t) == ['pk16x4'] * (4 - n) + ['pk16x4+retry'] * n
        # the limit itself: the last insertion that stays and the first that leaves, alone in a search (the 32-bit sweep makes the retry itself)
        stays = {g: SIDES['sub_band_exit/alone_g%d%s' % (g, tp)]['trace'][0]['sweep'] == 's32_lds' for g in (30, 31, 33, 34, 36, 40, 60)}
        assert [g for g in sorted(stays) if stays[g]] == ([30] if tp else [30, 31, 33])
        assert all(SIDES['sub_band_exit/alone_g%d%s' % (g, tp)]['trace'][0]['sweep'] == 's32_lds+full' for g in stays if not stays[g])
    assert sorted(r['sweep'] for r in SIDES['sub_band_exit/long_enough_for_the_chunked_launch']['trace']) == ['pk16x4_chunked'] * 2 + ['pk16x4_chunked+retry'] * 2


def test_census_every_sweep_is_taken():
    names = collections.Counter(r['sweep'] for c in CASES for w in ('score', 'trace') for r in SIDES[c['name']][w] if r['sweep'])
    for sweep in ('pk16', 'pk16_chunked', 's32_lds', 's32_global', 's32_lds+mixed', 's32_global+mixed', 'pk16x4', 'pk16x4_chunked', 'pk16x4+retry',
                  'pk16x4_chunked+retry', 's32_lds+full'):
        assert names[sweep] >= 2, sweep
