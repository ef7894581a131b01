"""The packed traceback sweep (csrc/sw.hip: sw_four_pk16_trace, both instantiations of sw_trace_kernel) against the oracle at the places where its
inner loop can go wrong: the residue cursors that read one step ahead of the table look-ups (the last step of a block, of a chunk and of a pair
then reads the slack of its window), the band-edge masks at both ends of the band, the end-cell counter, items of mixed length, the tails that
take the 32-bit sweep, pairs that are deferred to the full-band launch, and the limit of the 16-bit scores.

Every case is a small search built here (with the builders of tests/align_limit_cases.py) and compared with oracle.search field by field, CIGAR
arena included.  Before the GPU is asked anything, _held() holds the case to what it was built for with the oracle alone: the table is not empty,
every planted pair is reported with more than one CIGAR run (so rule 5a did not settle it and it did reach the traceback sweep), and the sweep
each traced pair must take - from the dispatch arithmetic restated in align_limit_cases.side() - is the one the case names.

Two of the shapes need a word:
  * a sub-band of exactly ONE sixteen-step block holds at most 8 residues on its longest diagonal, fewer than the default seed shapes span (12);
    _tiny() builds it with a seed shape of three letters, and _held() shows that the oracle reports it gapped and traced;
  * a traced pair whose best score is 1: an alignment ends in the first cell that holds the score, and with a score of 1 that is the first matching
    cell - one column, one CIGAR run, settled by rule 5a in the oracle and on the GPU alike, so its score never reaches the sweep as `known`.  The
    lowest score a gapped alignment can have under costs of (match 1, gap 1) is 3 (two columns, a gap, two columns); test_lowest_scores builds
    the search with scores from 1 upwards and holds the whole table to the oracle."""
import functools
import zlib

import numpy as np
import pytest

import align_limit_cases as AL

pytestmark = pytest.mark.gpu

FIELDS = ('q', 't', 'q_start', 'q_end', 't_start', 't_end', 'score', 'nm', 'n_ident', 'aln_len', 'cigar_runs', 'bin', 'cigar_off', 'cells')
W, P_ = AL.W, AL.P_
NT4 = AL.NT4


@pytest.fixture(scope='module')
def ctx():
    from peppan_amd import _native as N
    c = N.Context(0)
    yield c
    c.close()


def _cmp_hits(gh, gc, oh, oc):
    """every field of every hit and the CIGAR arena (the comparison of tests/test_gpu_parity.py, restated)"""
    assert len(gh) == len(oh), (len(gh), len(oh))
    for f in FIELDS:
        assert np.array_equal(gh[f], oh[f]), f
    assert np.array_equal(gc, oc)


# ---------------------------------------------------------------------------------------------------------------- parameter blocks
def _native(case):
    """the block Context.search gets: the protein defaults or nucleotide_params, then what the case sets"""
    from peppan_amd import _native as N
    par = case['params']
    if par['kind'] == 'nucl':
        p = N.nucleotide_params(0., 0.)
    else:
        p = N.default_params(0., 0., 10, 5, dbsize=par.get('dbsize', 5e6), max_evalue=par.get('max_evalue', 1.))
    if 'gap' in par:
        p.gap_open, p.gap_ext = par['gap']
    tab = AL.table(par['table'])
    if tab is not None:
        for x in range(1024):
            p.sub[x] = int(tab[x])
    for x, v in par.get('raise', ()):
        p.sub[x[0] * 32 + x[1]] = v
    if 'seed' in par:                                    # ONE contiguous seed shape of `seed` letters, nothing rejected before the sweeps
        p.n_shapes = 1
        for s in range(4):
            p.weight[s] = par['seed'] if s == 0 else 0
        for i in range(32):
            p.offs[0][i] = i if i < par['seed'] else 0
        p.ungapped_min, p.stage1_min = 1, 0
    return p


def _oracle_side(case):
    """(oracle parameter block, min_scores) that say the same as _native(case)"""
    from oracle import oracle as O
    p = _native(case)
    if case['params']['kind'] == 'nucl':
        ms = [O.min_score(len(s), p.dbsize, p.max_evalue, p.ka_lambda, p.ka_k) for s in case['q']]
    else:
        ms = [O.min_score(len(s), p.dbsize, p.max_evalue) for s in case['q']]
    return O.params_from(p), np.array(ms, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(hits, cigar, stats, trace counters) of the oracle on a case: computed once, shared, never changed"""
    from oracle import oracle as O
    case = CASES[name]
    p, ms = _oracle_side(case)
    O.trace_counts(True)
    h, cg, st = O.search(case['q'], case['t'], p, min_scores=ms)
    tc = O.trace_counts(True)
    for a in (h, cg):
        a.setflags(write=False)
    return h, cg, st, tc


def _l0(case, h):
    """first lane of the sub-band of a reported alignment: from the diagonal it ends on and the band it was found in"""
    end_lane = (int(h['t_end']) - int(h['q_end']) - AL.band_dlo(int(h['bin']))) >> 1
    return AL.sub_band_first_lane(end_lane)


def _held(case):
    """the case does what it was built to do - with the oracle alone"""
    hits, cig, st, tc = _oracle(case['name'])
    assert len(hits) >= 1, case['name']
    by_pair = {(int(h['q']), int(h['t'])): h for h in hits}
    for p in case['pairs']:
        assert (p['q'], p['t']) in by_pair, (case['name'], p['q'], p['t'])
        h = by_pair[p['q'], p['t']]
        if case.get('gapped', True):
            assert int(h['cigar_runs']) > 1, (case['name'], p['q'], p['t'])
            assert (int(h['bin']) == p['bin'] or case.get('any_bin')) and int(h['t_end']) - int(h['q_end']) == p['d_end'], (case['name'], p)
    if 'sweeps' in case:                                 # the sweep of every traced pair, in the length order (align_limit_cases.side)
        assert len(hits) == len(case['pairs']) and tc['traced'] == len(case['pairs']) and tc['gapless'] == 0, (case['name'], len(hits), tc)
        got = [r['sweep'] for r in AL.side(case)['trace']]
        assert sorted(got, key=str) == sorted(case['sweeps']), (case['name'], got)
    if 'sub_blocks' in case:                             # 16-step blocks of every pair's sub-band
        got = sorted(AL.sub_geom(len(case['q'][int(h['q'])]), len(case['t'][int(h['t'])]), int(h['bin']),
                                 (int(h['t_end']) - int(h['q_end']) - AL.band_dlo(int(h['bin']))) >> 1)[2] for h in hits)
        assert got == sorted(case['sub_blocks']), (case['name'], got)
    if 'steps' in case:                                  # in-matrix steps of the pairs' bands: which step of a block is a pair's last
        got = sorted(2 * len(case['q'][p['q']]) - 1 + len(case['t'][p['t']]) - len(case['q'][p['q']]) for p in case['pairs'])
        assert got == sorted(case['steps']), (case['name'], got)
    if 'l0' in case:
        assert sorted(_l0(case, h) for h in hits) == sorted(case['l0']), (case['name'], [_l0(case, h) for h in hits])
    if 'full_band' in case:
        assert tc['full_band'] == case['full_band'], (case['name'], tc)


def _check(ctx, case):
    _held(case)
    oh, oc, ost, _ = _oracle(case['name'])
    ctx.set_query_aa(case['q'])
    ctx.set_ref_aa(case['t'])
    gh, gc, st = ctx.search(_native(case))
    assert (st['candidates'], st['pairs'], st['cells']) == (ost['candidates'], ost['pairs'], ost['cells']), case['name']
    _cmp_hits(gh, gc, oh, oc)


# ---------------------------------------------------------------------------------------------------------------- the builders
def _case(name, **kw):
    extra = {k: kw.pop(k) for k in ('sweeps', 'sub_blocks', 'steps', 'l0', 'full_band', 'gapped') if k in kw}
    c = AL._case(name, **kw)
    c.update(extra)
    return c


W127 = {'raise': (((W, W), 127),)}


def _tiny(name, L, variants, **kw):
    """a query of L tryptophans against itself with g prolines inserted at pos, one target per (pos, g), under W/W = 127 and a seed of three
    letters: 2 * L - 1 + g in-matrix steps, and walking through the insertion (127 + 4 a column) costs more than the gap (11 + g)"""
    c = _case(name, seed=3, steps=[2 * L - 1 + g for _, g in variants], sub_blocks=[(2 * L - 1 + g + 15) // 16 for _, g in variants], **W127, **kw)
    AL._one_query(c, np.full(L, W, np.uint8), variants, lambda n: np.full(n, P_, np.uint8))
    c['any_bin'] = True                                  # tryptophans seed on every diagonal: which of the bands that hold the whole pair nominates it is the seed stage's business
    return c


def _offset_pair(case, rng, L, d1, d2, pos, trail):
    """a query of L residues inside a longer target: d1 residues of leading and `trail` of trailing overhang, the alignment starts on diagonal d1
    and, behind position pos, continues on diagonal d2 (d2 > d1: the target carries d2 - d1 residues more, d2 < d1: it lacks d1 - d2)"""
    base = AL._rand(rng, L)
    body = [base[:pos], AL._rand(rng, d2 - d1), base[pos:]] if d2 > d1 else [base[:pos], base[pos + d1 - d2:]]
    t = np.concatenate([AL._rand(rng, d1)] + body + [AL._rand(rng, trail)]).astype(np.uint8)
    AL._pair(case, base, t, [d1, d2])


def _build():
    out = []
    tr = AL.staging(4000, 0, True)                       # the traceback pass's staging area at its 8 KiB cap

    # ---- block boundaries.  2 * L - 1 + g steps: 16 is the last step of block 1, 17 the first of block 2, 32 / 33 and 48 likewise
    out.append(_tiny('blocks/one_block', 7, [(3, 1), (4, 2), (3, 3), (5, 1)], sweeps=['pk16x4'] * 4))                 # 14, 15, 16, 14 steps
    out.append(_tiny('blocks/first_step_of_block_two', 8, [(3, 2), (5, 2), (4, 3), (2, 3)], sweeps=['pk16x4'] * 4))   # 17, 17, 18, 18
    out.append(_tiny('blocks/two_blocks', 15, [(7, 1), (4, 2), (9, 3), (11, 3)], sweeps=['pk16x4'] * 4))              # 30, 31, 32, 32
    out.append(_tiny('blocks/first_step_of_block_three', 16, [(8, 2), (5, 2), (11, 3), (3, 3)], sweeps=['pk16x4'] * 4))   # 33, 33, 34, 34
    out.append(_tiny('blocks/three_blocks', 23, [(11, 1), (6, 2), (15, 3), (18, 3)], sweeps=['pk16x4'] * 4))          # 46, 47, 48, 48

    # ---- items of mixed length: the lanes of the shorter pairs keep reading the padding of their windows until the longest is through
    c = _case('items/four_unequal_lengths', sweeps=['pk16x4'] * 4)
    rng = AL._rng(c['name'])
    for L, g in ((60, 3), (131, 5), (250, 9), (397, 14)):
        AL._random_pair(c, rng, L, g)
    out.append(c)
    for n in (1, 2, 3, 5, 9):                            # fewer than four selected pairs: the 32-bit sweep; 4 k + 1: packed items and a tail of one
        c = _case('items/%d_selected' % n, sweeps=['pk16x4'] * (n - n % 4) + ['s32_lds'] * (n % 4))
        rng = AL._rng(c['name'])
        for k in range(n):
            AL._random_pair(c, rng, 240 - 11 * k, 4 + k)
        out.append(c)

    # ---- the sub-band at both ends of its band.  A band starts 32 diagonals below a multiple of 64 (align_limit_cases.band_dlo).  An alignment that
    # ends on diagonal 64 k, found in the band of that bin, ends in lane 16: L0 = 0, and its first stretch on diagonal 64 k + g lies g / 2 lanes
    # from the sub-band's last lane (g = 30, 31: IN the last lane, where the F chain of the B step is masked).  One that starts below 64 k and ends
    # on 64 k + r is won by the lower bin's band, where it ends in lane 48 + r / 2: L0 = 32, and a first stretch on diagonal 64 k - 32 lies in the
    # sub-band's first lane, where the H / E chain of the A step is masked
    c = _case('band_ends/l0_is_0', sweeps=['pk16x4'] * 4, l0=[0] * 4)
    rng = AL._rng(c['name'])
    for k, g in ((2, 7), (1, 30), (3, 31), (2, 16)):
        _offset_pair(c, rng, 300, 64 * k + g, 64 * k, 150, 90)
    out.append(c)
    c = _case('band_ends/l0_is_32', sweeps=['pk16x4'] * 4, l0=[32] * 4)
    rng = AL._rng(c['name'])
    for k, s, r in ((2, 5, 4), (1, 32, 4), (3, 31, 0), (2, 12, 20)):
        _offset_pair(c, rng, 300, 64 * k - s, 64 * k + r, 150, 90)
    out.append(c)

    # ---- one pair leaves its sub-band (an insertion of 36 against the 33 that stay, align_limit_cases._sub_band_cases): deferred, retried in the full band
    c = _case('deferred/one_of_four', sweeps=['pk16x4'] * 3 + ['pk16x4+retry'], full_band=1)
    rng = AL._rng(c['name'])
    for k, g in enumerate((36, 30, 33, 30)):
        AL._random_pair(c, rng, 300 + 6 * k, g, pos=150 + 3 * k)
    out.append(c)

    # ---- the chunked form, nucleotide tool.  The staging area of a wavefront is lds_res_bytes = 8192 at its cap; eight windows of two-byte entries
    # share it, 8192 / 16 = 512 entries each; a window holds 8 entries per block and SUB_LANES + 16 = 48 of overlap and slack, so a chunk is
    # (512 - 48) / 8 = 58 blocks (sw_four_pk16_trace: chunk = (lds_res_bytes / 16 - (SUB_LANES + 16)) / 8).  Pairs of more than 57 blocks go to
    # the chunked launch once the longest query + the longest target reach 912 bases.  A pair (L, L + g) has 2 * L - 1 + g steps
    # (_len_for_blocks: L for a given block count): 58 blocks are exactly one chunk, 116 exactly two, and with 59 and 117 the chunk boundary falls in
    # front of the pair's last block, which is then staged and swept alone
    assert (tr['lds_res_bytes'], tr['chunk'], tr['nb_limit']) == (8192, (8192 // 16 - (AL.SUB_LANES + 16)) // 8, 57) and tr['chunk'] == 58
    for label, nb in (('one_chunk', tr['chunk']), ('two_chunks', 2 * tr['chunk']), ('boundary_before_the_last_block', tr['chunk'] + 1),
                      ('two_chunks_and_the_last_block', 2 * tr['chunk'] + 1)):
        c = _case('chunked/' + label, kind='nucl', sweeps=['pk16x4_chunked'] * 4, sub_blocks=[nb] * 4)
        rng = AL._rng(c['name'])
        for g, rem in ((5, 8), (9, 0), (12, 15), (17, 0)):            # rem 0: the pair's last step is the last step of its last block; 15: the first
            AL._random_pair(c, rng, AL._len_for_blocks(nb, g, rem), g, alphabet=NT4)
        out.append(c)

    # ---- the limit of the 16-bit scores: fits16 is min(Lq, Lt) * max_sub + 64 + PK_BIAS < 32767; with max_sub = 127 (W/W raised) 256 residues are
    # the last that fit (256 * 127 + 192 = 32704) and 257 the first that do not (32831): the packed sweep, and the 32-bit sweep of the slow path
    ins = lambda L: [(L // 2 + 5, 7), (L // 3, 3), (2 * L // 3, 11), (L // 2 - 40, 5)]
    for L, sweep in ((256, 'pk16x4'), (257, 's32_lds')):
        assert AL.fits16(L, L + 3, 127) == (L == 256)
        c = _case('fits16/w127_%d' % L, sweeps=[sweep] * 4, **W127)
        AL._one_query(c, AL._w_rich(AL._rng(c['name']), L, 61), ins(L), lambda n: np.full(n, P_, np.uint8))
        out.append(c)
    return {c['name']: c for c in out}


CASES = _build()


@pytest.mark.parametrize('name', sorted(CASES))
def test_case_equals_the_oracle(ctx, name):
    _check(ctx, CASES[name])


def test_lowest_scores(ctx):
    """match 1, everything else -128, gap costs (0, 1), a seed of one letter and an e-value that admits a score of 1: queries of 1 .. 4 tryptophans and
    the query WW.WW against targets that hold them once, and WW.WW against four targets that hold WWWW (two columns, a gap, two columns: score 3, the
    lowest a gapped alignment can have; four of them make an item of the packed sweep).  Scores of 1 are single columns (rule 5a, see the top of the file); the table must be the oracle's all the same"""
    from oracle import oracle as O
    A = AL.A_
    mk = lambda s: np.array([W if ch == 'W' else (P_ if ch == 'P' else A) for ch in s], np.uint8)
    c = _case('lowest_scores', table_='edge', gap=(0, 1), seed=1, dbsize=1., max_evalue=1e30, gapped=False, **{'raise': (((W, W), 1),)})
    c['q'] = [mk('W'), mk('WW'), mk('WWW'), mk('WWPWW'), mk('AWA')]
    c['t'] = [mk('AAWAA'), mk('PWWP'), mk('WWWW'), mk('AWWAWWA'), mk('W'), mk('PWWWW'), mk('WWWWP'), mk('AWWWWA')]
    CASES[c['name']] = c
    p, ms = _oracle_side(c)
    assert int(ms.max()) <= 1
    hits, cig, st, tc = _oracle(c['name'])
    assert 1 in hits['score'].tolist() and len(hits) >= 5
    gapped = [h for h in hits if int(h['cigar_runs']) > 1]
    assert len(gapped) == 4 and all(int(h['score']) == 3 for h in gapped), [(int(h['q']), int(h['t']), int(h['score'])) for h in gapped]      # an item of four for the packed sweep
    _check(ctx, c)


# ---------------------------------------------------------------------------------------------------------------- the randomised sweep
def _families(rng, n, indel):
    """n genes of 60 .. 400 nt in families of 3 .. 6: a random root, members with 8 % substitutions and indels of 1 .. 6 bases at rate `indel` per base"""
    genes = []
    while len(genes) < n:
        root = rng.integers(0, 4, int(rng.integers(60, 401)))
        for _ in range(int(rng.integers(3, 7))):
            m = root.copy()
            sub = rng.random(len(m)) < 0.08
            m[sub] = rng.integers(0, 4, int(sub.sum()))
            parts, at = [], 0
            for pos in np.flatnonzero(rng.random(len(m)) < indel):
                g = int(rng.integers(1, 7))
                if rng.random() < 0.5:
                    parts += [m[at:pos], rng.integers(0, 4, g)]
                    at = pos
                else:
                    parts.append(m[at:pos])
                    at = min(len(m), pos + g)
            parts.append(m[at:])
            m = np.concatenate(parts)
            if 60 <= len(m) <= 400:
                genes.append(m.astype(np.uint8))
    return genes[:n]


RC = np.array([3, 2, 1, 0, 4], dtype=np.uint8)


@pytest.mark.parametrize('tool', ['blastn', 'diamond'])
@pytest.mark.parametrize('part', range(5))
def test_random_small_searches(ctx, tool, part):
    """200 searches in all (2 tools x 5 parts x 20): 40 .. 80 genes, indel rates from 0 to 5 %, seeds fixed by tool, part and number"""
    from peppan_amd import _native as N
    from oracle import oracle as O
    traced = hits_total = 0
    for k in range(20):
        rng = np.random.default_rng(zlib.crc32(('%s/%d/%d' % (tool, part, k)).encode()))
        genes = _families(rng, int(rng.integers(40, 81)), 0.05 * (4 * part + k % 4) / 19.)
        if tool == 'blastn':
            qs, ts = genes, genes + [RC[g[::-1]] for g in genes]
            p = N.nucleotide_params(0., 0.)
            ms = np.array([O.min_score(len(s), p.dbsize, p.max_evalue, p.ka_lambda, p.ka_k) for s in qs], dtype=np.int32)
        else:                                            # the translated search: frame 1 of every gene as the query, its six frames as targets
            nt = [''.join('ACGT'[x] for x in g) for g in genes]
            qs = [O.aa_codes(O.query_frame(s, 11)[1]) for s in nt]
            ts = [O.aa_codes(cc) for s in nt for aa in O.translate_frames(s, range(1, 7), 11) for o, cc in O.ref_chunks(aa)]
            p = N.default_params(0., 0., 10, 5)
            ms = np.array([O.min_score(len(s), p.dbsize, p.max_evalue) for s in qs], dtype=np.int32)
        ctx.set_query_aa(qs)
        ctx.set_ref_aa(ts)
        gh, gc, st = ctx.search(p)
        O.trace_counts(True)
        oh, oc, ost = O.search(qs, ts, O.params_from(p), min_scores=ms)
        tc = O.trace_counts(True)
        _cmp_hits(gh, gc, oh, oc)
        traced += tc['traced'] - tc['gapless']
        hits_total += len(oh)
    assert hits_total >= 20 * 40 and traced >= 100, (hits_total, traced)
