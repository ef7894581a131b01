"""The traceback walk (csrc/trace.hip: walk) against the oracle at the places where its window of code words can go wrong.

A lane of `walk` holds the code words of eight 16-step blocks down from its cell, of four neighbouring diagonals (one unaligned 16-byte load a
block), steps until its cell leaves that window, and the wavefront loads again in rounds.  What can go wrong is therefore a matter of where the
gaps of an alignment lie relative to the window: how far a gap moves the lane sideways (inside the four diagonals, just outside, far outside, in
either direction, with the window's first dword at every offset of the row), how far from the alignment's end it begins (the words and windows are
counted from the end, where the walk starts), how long the stretches between gaps are, how the walk ends, the two row widths, and who shares a
wavefront.

Every case is a small search built here with the builders of tests/align_limit_cases.py and compared with oracle.search field by field, CIGAR
arena included (the comparison of tests/test_gpu_trace_pipeline.py, restated), as given, with the 32-bit sweeps forced and with every buffer of
the traceback stage sized exactly; the three must give the same bytes.  Before the GPU is asked anything, _held() holds the case to what it was
built for with the oracle alone: every planted pair is reported, with exactly the number of CIGAR runs the case planted, and the oracle's
counters say it was traced - or settled by rule 5a where the case says it is gapless."""
import functools
import zlib

import numpy as np
import pytest

import align_limit_cases as AL

pytestmark = pytest.mark.gpu

FIELDS = ('q', 't', 'q_start', 'q_end', 't_start', 't_end', 'score', 'nm', 'n_ident', 'aln_len', 'cigar_runs', 'bin', 'cigar_off', 'cells')
NT4 = AL.NT4
WAYS = (dict(), dict(forced32=True), dict(exact=True))


@pytest.fixture(scope='module')
def ctx():
    from peppan_amd import _native as N
    c = N.Context(0)
    yield c
    c.close()


def _cmp_hits(gh, gc, oh, oc):
    """every field of every hit and the CIGAR arena"""
    assert len(gh) == len(oh), (len(gh), len(oh))
    for f in FIELDS:
        assert np.array_equal(gh[f], oh[f]), f
    assert np.array_equal(gc, oc)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(hits, cigar, stats, trace counters) of the oracle on a case: computed once, shared, never changed"""
    from oracle import oracle as O
    case = CASES[name]
    O.trace_counts(True)
    h, cg, st = O.search(case['q'], case['t'], AL.oracle_params(case), min_scores=AL.min_scores(case))
    tc = O.trace_counts(True)
    for a in (h, cg):
        a.setflags(write=False)
    return h, cg, st, tc


def _held(case):
    """the case does what it was built to do - with the oracle alone"""
    hits, cig, st, tc = _oracle(case['name'])
    by_pair = {(int(h['q']), int(h['t'])): h for h in hits}
    assert len(by_pair) == len(hits), case['name']
    gapless = 0
    for p in case['pairs']:
        assert (p['q'], p['t']) in by_pair, (case['name'], p['q'], p['t'])
        h = by_pair[p['q'], p['t']]
        assert int(h['cigar_runs']) == p['runs'], (case['name'], p['q'], p['t'], int(h['cigar_runs']), p['runs'])
        gapless += p['runs'] == 1
    if case.get('only_planted', True):                   # nothing but the planted pairs: the counters are theirs
        assert len(hits) == len(case['pairs']), (case['name'], len(hits))
        assert tc['traced'] == len(hits) and tc['gapless'] == gapless, (case['name'], tc, gapless)
    else:
        assert tc['traced'] - tc['gapless'] >= len(case['pairs']) - gapless, (case['name'], tc)
    if 'full_band' in case:
        assert tc['full_band'] == case['full_band'], (case['name'], tc)


def _check(ctx, case):
    _held(case)
    oh, oc, ost, _ = _oracle(case['name'])
    ctx.set_query_aa(case['q'])
    ctx.set_ref_aa(case['t'])
    got = []
    for kw in WAYS:
        gh, gc, st = ctx.search(AL.native_params(case, **kw))
        assert (st['candidates'], st['pairs'], st['cells']) == (ost['candidates'], ost['pairs'], ost['cells']), (case['name'], kw)
        _cmp_hits(gh, gc, oh, oc)
        got.append((gh.tobytes(), gc.tobytes()))
    assert got[1] == got[0] and got[2] == got[0], case['name']


# ---------------------------------------------------------------------------------------------------------------- the builders
def _planted(case, rng, L, cuts, lead=0, trail=0, alphabet=AL.AA20, runs=None):
    """a random base of L residues with the indels `cuts` (align_limit_cases._indel_pair: (position in the base, g), g > 0 into the target, g < 0
    into the query), the target with `lead` random residues in front and `trail` behind: the alignment starts on diagonal `lead`.  It is
    expected with one M run per stretch and one run per cut unless `runs` says otherwise"""
    base = AL._rand(rng, L, alphabet)
    q, t, diags = AL._indel_pair(base, cuts, lambda n: AL._rand(rng, n, alphabet))
    t = np.concatenate([AL._rand(rng, lead, alphabet), t, AL._rand(rng, trail, alphabet)]).astype(np.uint8)
    AL._pair(case, q, t, [d + lead for d in diags])
    case['pairs'][-1]['runs'] = 2 * len(cuts) + 1 if runs is None else runs


def _case(name, **kw):
    extra = {k: kw.pop(k) for k in ('full_band', 'only_planted') if k in kw}
    c = AL._case(name, **kw)
    c.update(extra)
    return c


ALTERNATING_20 = [(8 * k + 40, 1 if k % 2 == 0 else -1) for k in range(20)]      # twenty single gaps eight columns apart: 41 runs


def _build():
    out = []

    # ---- gap length against the four diagonals of a window, with the window's first dword at every offset: one gap of 1 .. 9 residues in each
    # direction, 64 columns in front of the alignment's end; `lead` residues of leading overhang put the end diagonal at every residue mod 8
    for lead in range(8):
        c = _case('gap_length/lead_%d' % lead)
        rng = AL._rng(c['name'])
        for g in (1, 2, 3, 4, 5, 6, 7, 8, 9, -1, -2, -3, -4, -5, -6, -7, -8, -9):
            _planted(c, rng, 300, [(300 - 64, g)], lead=lead)
        out.append(c)

    # ---- gap position against words and windows, counted from the alignment's end (the pairs end with their sequences)
    c = _case('gap_position/words_and_windows_from_the_end')
    rng = AL._rng(c['name'])
    for n in (7, 8, 9, 63, 64, 65, 127, 128, 129):
        for g in (1, -2):
            _planted(c, rng, 320, [(320 - n, g)])
    out.append(c)
    # every distance from 56 to 72: the block phase of a pair is a matter of its band, so one of these gaps ends on the last cell of the first
    # window and the next one begins on the first cell of the second
    c = _case('gap_position/every_cell_around_the_first_window_border')
    rng = AL._rng(c['name'])
    for n in range(56, 73):
        for g in (1, -1):
            _planted(c, rng, 320, [(320 - n, g)])
    out.append(c)
    c = _case('gap_position/gaps_fewer_than_eight_cells_apart')
    rng = AL._rng(c['name'])
    _planted(c, rng, 320, [(100, 1), (103, 1), (106, 1), (109, 1)])
    _planted(c, rng, 320, [(150, 1), (155, 2)])
    _planted(c, rng, 320, [(200, -1), (206, -1)])
    _planted(c, rng, 320, [(250, 2), (257, 3)])
    out.append(c)
    c = _case('gap_position/twenty_alternating_gaps_eight_apart')
    rng = AL._rng(c['name'])
    _planted(c, rng, 320, ALTERNATING_20)
    _planted(c, rng, 320, [(8 * k + 40, 2) for k in range(12)])
    for g in (3, -3):                                    # (two bystanders with one gap: four pairs, the packed sweep)
        _planted(c, rng, 320, [(160, g)])
    out.append(c)

    # ---- stretches longer than every buffer: the window is loaded many times in a row down one diagonal, and the walk ends on row 0 and
    # column 0 - cell (0, 0) is the LAST cell of its code word for every pair that starts there (m = 0, asserted below) - or, with a
    # leading overhang, on row 0 in the middle of a word
    c = _case('long_stretches/ends_on_row_and_column_0')
    rng = AL._rng(c['name'])
    for L, cut in ((640, (20, 3)), (667, (20, -2)), (700, (20, 1)), (689, (689 - 10, 2))):
        _planted(c, rng, L, [cut])
    for p in c['pairs']:
        dlo, a0, _ = AL.sub_geom(len(c['q'][p['q']]), len(c['t'][p['t']]), p['bin'], (p['d_end'] - AL.band_dlo(p['bin'])) >> 1)
        assert (0 - a0 + ((0 - 0 - dlo) >> 1)) % 8 == 0, (c['name'], p)
    out.append(c)
    c = _case('long_stretches/ends_on_row_0_inside_a_word')
    rng = AL._rng(c['name'])
    for L, cut, lead in ((640, (20, 3), 3), (655, (20, -2), 5), (700, (690, 1), 9), (671, (300, 2), 14)):
        _planted(c, rng, L, [cut], lead=lead)
    out.append(c)

    # ---- row width 128: the deferred pair of test_gpu_trace_pipeline's deferred/one_of_four (an insertion of 36 among pairs with 30, 33, 30),
    # every pair with a second, short gap 64 columns from its end; the pair that starts on diagonal 0 and ends on 35 leaves its sub-band
    c = _case('row_width/deferred_pair_with_a_short_gap', full_band=1)
    rng = AL._rng(c['name'])
    for k, g in enumerate((36, 30, 33, 30)):
        L = 300 + 6 * k
        _planted(c, rng, L, [(150 + 3 * k, g), (L - 64, -1)])
    out.append(c)
    # ---- fewer than four selected pairs: the 32-bit sweep writes the codes
    for n in (1, 2, 3):
        c = _case('row_width/%d_selected' % n)
        rng = AL._rng(c['name'])
        for k in range(n):
            _planted(c, rng, 240 - 11 * k, [(60, 2 + k), (240 - 11 * k - 65, -1)])
        out.append(c)

    # ---- who shares a wavefront
    for n in (1, 63, 64, 65, 130):
        c = _case('wavefront/%d_pairs' % n)
        rng = AL._rng(c['name'])
        for k in range(n):
            _planted(c, rng, 100 + k % 37, [(30 + k % 41, 1 + k % 5 if k % 2 else -1 - k % 4)])
        out.append(c)
    # rule-5a pairs (the query inside a longer target: one M run), identical pairs (the score pass settles them) and traced pairs take turns in
    # selection order, which is the order of (q, t)
    c = _case('wavefront/three_kinds_of_lanes')
    rng = AL._rng(c['name'])
    for k in range(66):
        if k % 3 == 0:
            _planted(c, rng, 90 + k, [], lead=5 + k % 7, trail=3)
        elif k % 3 == 1:
            _planted(c, rng, 90 + k, [])
        else:
            _planted(c, rng, 90 + k, [(40, 1 + k % 4), (70, -1)])
    out.append(c)
    c = _case('wavefront/one_lane_with_twenty_gaps_among_63_with_one')
    rng = AL._rng(c['name'])
    for k in range(64):
        if k == 31:
            _planted(c, rng, 320, ALTERNATING_20)
        else:
            _planted(c, rng, 100 + k % 29, [(50, 1 + k % 3)])
    out.append(c)

    # ---- the nucleotide tool: four pairs of the chunked launch (a chunk is 58 blocks: 59 and 117 put the chunk boundary in front of the last
    # block), five gaps each - a pair of a thousand columns crosses windows at many more blocks than a protein pair has
    for nb in (59, 117):
        c = _case('nucleotide/chunked_%d_blocks' % nb, table_='nucl1', kind='nucl')
        rng = AL._rng(c['name'])
        for k in range(4):
            gs = [(1, 2, 3, 1, 2), (2, 1, 1, 3, 2), (3, 2, 2, 2, 1), (1, 1, 2, 2, 3)][k]
            L = AL._len_for_blocks(nb, sum(gs), (8, 0, 15, 0)[k])
            _planted(c, rng, L, [((x + 1) * L // 6 + 3 * k, g) for x, g in enumerate(gs)], alphabet=NT4)
        out.append(c)
    return {c['name']: c for c in out}


CASES = _build()


@pytest.mark.parametrize('name', sorted(CASES))
def test_case_equals_the_oracle(ctx, name):
    _check(ctx, CASES[name])


# ---------------------------------------------------------------------------------------------------------------- the randomised sweep
def _families(rng, n, indel):
    """n genes of 300 .. 1500 nt in families of 3 .. 6: a random root, members with 8 % substitutions and indels of 1 .. 6 bases at rate `indel` per base"""
    genes = []
    while len(genes) < n:
        root = rng.integers(0, 4, int(rng.integers(300, 1501)))
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
            if 300 <= len(m) <= 1500:
                genes.append(m.astype(np.uint8))
    return genes[:n]


RC = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
SWEEP = [(tool, k) for tool in ('blastn', 'diamond') for k in range(10)]
_compared = {}                                           # (tool, number) -> (traced and gapped alignments, those with four gaps or more), from the oracle's table


def _random_search(ctx, tool, k):
    from peppan_amd import _native as N
    from oracle import oracle as O
    if (tool, k) in _compared:
        return
    rng = np.random.default_rng(zlib.crc32(('walk/%s/%d' % (tool, k)).encode()))
    genes = _families(rng, int(rng.integers(24, 41)), 0.05 * k / 9.)
    if tool == 'blastn':
        qs, ts = genes, genes + [RC[g[::-1]] for g in genes]
        p = N.nucleotide_params(0., 0.)
        ms = np.array([O.min_score(len(s), p.dbsize, p.max_evalue, p.ka_lambda, p.ka_k) for s in qs], dtype=np.int32)
    else:                                                # the translated search: frame 1 of every gene as the query, its six frames as targets
        nt = [''.join('ACGT'[x] for x in g) for g in genes]
        qs = [O.aa_codes(O.query_frame(s, 11)[1]) for s in nt]
        ts = [O.aa_codes(cc) for s in nt for aa in O.translate_frames(s, range(1, 7), 11) for o, cc in O.ref_chunks(aa)]
        p = N.default_params(0., 0., 10, 5)
        ms = np.array([O.min_score(len(s), p.dbsize, p.max_evalue) for s in qs], dtype=np.int32)
    ctx.set_query_aa(qs)
    ctx.set_ref_aa(ts)
    gh, gc, st = ctx.search(p)
    oh, oc, ost = O.search(qs, ts, O.params_from(p), min_scores=ms)
    _cmp_hits(gh, gc, oh, oc)
    gaps = [int(np.count_nonzero(oc[int(h['cigar_off']):int(h['cigar_off']) + int(h['cigar_runs'])] & 3)) for h in oh]
    _compared[tool, k] = (sum(1 for g in gaps if g >= 1), sum(1 for g in gaps if g >= 4))


@pytest.mark.parametrize('tool,k', SWEEP)
def test_random_search(ctx, tool, k):
    """genes of 300 .. 1 500 nt in families, indel rates from 0 to 5 %, seeds fixed by tool and number"""
    _random_search(ctx, tool, k)


def test_random_searches_compared_enough(ctx):
    """the sweep as a whole (searches that have not run yet in this session run here): enough gapped alignments, and enough with many gaps"""
    for tool, k in SWEEP:
        _random_search(ctx, tool, k)
    gapped = sum(v[0] for v in _compared.values())
    many = sum(v[1] for v in _compared.values())
    assert gapped >= 300 and many >= 50, (gapped, many)
