"""Hand-built cases for the ungapped x-drop pre-filter of the seed stage (K4b, seed_runs_extend): tests/test_seed_extend_cases_host.py runs them
through the oracle alone, tests/test_gpu_seed_extend.py compares the GPU with the oracle on each.

A case is a handful of protein pairs (at most 64 sequences of at most 200 residues).  A pair is a random query and a target that is a copy of
it with substitutions at chosen offsets from the seed position c, so the ungapped score along the seed's diagonal is known residue by residue:

    '='  the query's residue            '~'  another residue of the same letter of the reduced alphabet (the seed survives, the score is low)
    'x'  a residue of another letter of the reduced alphabet (no seed goes through it)

The CORE - offsets 0 .. 14, wide enough for both default seed shapes - matches in the reduced alphabet everywhere except at offset 8, the one
offset neither shape looks at when it starts at c.  It is not kept identical: fifteen identical residues score at least 60 by themselves,
above the default ungapped_min (55) and far above stage1_min (24), so an identical core leaves no edge to put a case on under the default
parameters.  With 'x' at offset 8, at offset -1 and at every third offset outside the core, and nowhere else, the pair has exactly ONE seed position
(both shapes at c; no shape fits anywhere else), so one extension decides the candidate.  Outside the window a case is about, everything is 'x'.

Every edge comes as TWINS that differ by one unit - one point of one residue's score (the pivot: the same offset substituted by two residues
whose scores against the query differ by 1), one offset, or one residue of a sequence's length - and lie on either side of the edge: one twin
yields a candidate per pair, the other none.  A small model of the pre-filter (extension() below, a restatement of ungapped_score in
oracle/align_oracle.c) is used ONLY to draw pairs until one sits on the edge; what the tests assert comes from the oracle:
test_seed_extend_cases_host.py holds every case to the candidate count stated here and the twins to different counts."""
import functools

import numpy as np

from oracle import oracle as O

LETTERS = 'ACDEFGHIKLMNPQRSTVWY'
CODES = [ord(c) - 65 for c in LETTERS]
DEFAULTS = dict(ungapped_min=55, xdrop=12, ext_right=40, ext_left=24, stage1_min=24)
STAGE1_LEN = 16
CORE = 15
PAIRS = 4                               # pairs per case


class Par(object):
    def __init__(self, **kw):
        self.__dict__.update(DEFAULTS)
        self.__dict__.update(kw)

    def overrides(self):
        return {k: getattr(self, k) for k in DEFAULTS}


@functools.lru_cache(maxsize=None)
def _tables():
    p = O.default_params()
    sub = np.array(p.sub[:], dtype=np.int32).reshape(32, 32)
    reduce_ = list(p.reduce[:])
    shapes = [[p.offs[s][i] for i in range(p.weight[s])] for s in range(p.n_shapes)]
    same = {a: [b for b in CODES if b != a and reduce_[b] == reduce_[a]] for a in CODES}
    other = {a: [b for b in CODES if reduce_[b] != reduce_[a]] for a in CODES}
    return sub, reduce_, shapes, same, other


def extension(P, q, t, qpos, tpos, xdrop=None):
    """the pre-filter's verdict on one seed hit.  -> dict: total (-1: stage 1 failed), br, bl, br16 (best after the first 16 residues, or
    where the right side ended before), rise_r / rise_l (index of the residue that made br / bl; -1: none), n_r / n_l (residues scored),
    drop_r / drop_l (the side ended by x-drop, with `fall` = how far below its best)"""
    sub = _tables()[0]
    xd = P.xdrop if xdrop is None else xdrop
    out = dict(total=-1, br=0, bl=0, br16=None, rise_r=-1, rise_l=-1, n_r=0, n_l=0, drop_r=False, drop_l=False, fall_r=0, fall_l=0)
    s = br = k = 0
    while k < P.ext_right and qpos + k < len(q) and tpos + k < len(t):
        if k == STAGE1_LEN:
            out['br16'] = br
            if br < P.stage1_min:
                out.update(br=br, n_r=k)
                return out
        s += int(sub[q[qpos + k], t[tpos + k]])
        k += 1
        if s > br:
            br, out['rise_r'] = s, k - 1
        else:
            out['fall_r'] = max(out['fall_r'], br - s)
            if br - s > xd:
                out['drop_r'] = True
                break
    if out['br16'] is None:
        out['br16'] = br
    out.update(br=br, n_r=k)
    if br < P.stage1_min:
        return out
    s = bl = 0
    k = 1
    while k <= P.ext_left and qpos - k >= 0 and tpos - k >= 0:
        s += int(sub[q[qpos - k], t[tpos - k]])
        if s > bl:
            bl, out['rise_l'] = s, k
        else:
            out['fall_l'] = max(out['fall_l'], bl - s)
            if bl - s > xd:
                out['drop_l'] = True
                k += 1
                break
        k += 1
    out.update(bl=bl, n_l=k - 1, total=br + bl)
    return out


def seed_positions(q, t):
    """(qpos, tpos) of every seed hit of the default shapes between two sequences, each once"""
    _, reduce_, shapes, _, _ = _tables()
    hits = set()
    for offs in shapes:
        keys = {}
        for pos in range(len(q) - offs[-1]):
            k = tuple(reduce_[q[pos + o]] for o in offs)
            if 0xFF not in k:
                keys.setdefault(k, []).append(pos)
        for pos in range(len(t) - offs[-1]):
            k = tuple(reduce_[t[pos + o]] for o in offs)
            for qp in keys.get(k, ()):
                hits.add((qp, pos))
    return sorted(hits)


@functools.lru_cache(maxsize=None)
def _pools():
    """[mode, query residue] -> the residues a target position of that mode is drawn from (padded), and how many they are"""
    _, _, _, same, other = _tables()
    pools, sizes = np.zeros((3, 32, 20), dtype=np.uint8), np.ones((3, 32), dtype=np.int64)
    for a in CODES:
        for m, pool in enumerate(([a], same[a], other[a])):
            pools[m, a, :len(pool)], sizes[m, a] = pool, len(pool)
    return pools, sizes


def verdict(P, q, t):
    """-> (number of candidates of the pair = diagonal bins with a passing hit, the extensions of its hits)"""
    ext = [dict(extension(P, q, t, qp, tp), qpos=qp, tpos=tp) for qp, tp in seed_positions(q, t)]
    bins = set((e['tpos'] - e['qpos'] + (1 << 23)) // 64 for e in ext if P.ungapped_min <= 0 or e['total'] >= P.ungapped_min)
    return len(bins), ext


def layout(right, left, core='~', extra=None, identical=()):
    """offset -> mode.  The core, `right` residues behind it and `left` in front of it follow the single-seed pattern of the module's
    docstring with '=' as the matching mode (core: `core`, '=' at the offsets `identical`); everything else is 'x'.  extra: offsets set afterwards."""
    m = {}
    for o in range(-left, CORE + right):
        inside = 0 <= o < CORE
        m[o] = 'x' if (o == 8 if inside else (o % 3 == 0 or o == -1)) else (core if inside else '=')
    m.update({o: '=' for o in identical if o != 8})
    m.update(extra or {})
    return m


def soften(m, rng):
    """a drawn share of the '=' outside the core becomes '~': the stretch still carries no second seed and scores little"""
    p = rng.random()
    return {o: ('~' if v == '=' and not 0 <= o < CORE and rng.random() < p else v) for o, v in m.items()}


def draw_pair(rng, modes, c, q_len, t_pre=0, q_cut=(0, None), t_cut=(0, None), pivot=None, rises=True):
    """One query and its target(s).  modes: layout(); c: seed position in the query; the target is t_pre random residues and the substituted
    copy; q_cut / t_cut slice the query / the copy afterwards (sequence ends).  pivot: an offset whose target residue is drawn twice, the
    twins' scores there differing by 1 (rises: the higher one is positive) -> (q, t_a, t_b, seed position in q, in t); t_b is None without a pivot."""
    sub, reduce_, _, same, other = _tables()
    pools, sizes = _pools()
    q = np.array(CODES, dtype=np.uint8)[rng.integers(0, len(CODES), q_len)]
    mode = np.full(q_len, 2)                               # 0 '=', 1 '~', 2 'x'
    for o, m in modes.items():
        if 0 <= c + o < q_len:
            mode[c + o] = '=~x'.index(m)
            if m == '~' and not same[int(q[c + o])]:
                q[c + o] = rng.choice([a for a in CODES if same[a]])
    u = rng.random(q_len)                                  # (one draw per position whatever its mode: twins that differ in a mode share the rest)
    t = pools[mode, q, (u * sizes[mode, q]).astype(np.int64)]
    tb = None
    if pivot is not None:
        x = c + pivot
        a = int(q[x])
        pool = ([a] + same[a]) if modes.get(pivot, 'x') in '=~' else other[a]
        twins = [(u, v) for u in pool for v in pool if sub[a, u] - sub[a, v] == 1 and (sub[a, u] > 0) == rises]
        if not twins:
            return None
        u, v = twins[rng.integers(0, len(twins))]
        tb = t.copy()
        t[x], tb[x] = u, v
    pre = np.array(CODES, dtype=np.uint8)[rng.integers(0, len(CODES), t_pre)]
    cut = lambda s: np.ascontiguousarray(np.concatenate([pre, s[t_cut[0]:t_cut[1]]]))
    return np.ascontiguousarray(q[q_cut[0]:q_cut[1]]), cut(t), (cut(tb) if tb is not None else None), c - q_cut[0], c - t_cut[0] + t_pre


def _collect(name, seed, P, draw, accept, n=PAIRS, tries=200000):
    """draws until n twins are accepted.  draw(rng) -> (q, t_a, t_b, qpos, tpos) or two such pairs ((q, t, None, qpos, tpos) each), the first
    the twin that passes; accept(extension of the first's seed, of the second's); both must have that seed and no other"""
    rng = np.random.default_rng(seed)
    got = []
    for _ in range(tries):
        d = draw(rng)
        if d is None:
            continue
        if len(d) == 2:
            (qa, ta, _, qpa, tpa), (qb, tb, _, qpb, tpb) = d
        else:
            qa, ta, tb, qpa, tpa = d
            qb, qpb, tpb = qa, qpa, tpa
        ea, eb = extension(P, qa, ta, qpa, tpa), extension(P, qb, tb, qpb, tpb)
        if not (ea['total'] >= P.ungapped_min > eb['total'] and accept(ea, eb)):
            continue
        if seed_positions(qa, ta) == [(qpa, tpa)] and seed_positions(qb, tb) == [(qpb, tpb)]:
            got.append((qa, ta, qb, tb))
            if len(got) == n:
                break
    assert len(got) == n, 'case builder: %s found %d of %d pairs' % (name, len(got), n)
    mk = lambda role, qs, ts, cand: dict(name='%s/%s' % (name, role), twin=name, par=P.overrides(), q=qs, t=ts, candidates=cand, tool='protein')
    return [mk('pass', [g[0] for g in got], [g[1] for g in got], n), mk('fail', [g[2] for g in got], [g[3] for g in got], 0)]


def _twin_cases():
    D = Par()
    out = []
    some = lambda r: r.choice(CORE, int(r.integers(2, 13)), replace=False)          # core offsets kept identical
    # 1. stage 1: the right side reaches stage1_min with its 16th residue (offset 15) / stays one short of it after 16 residues
    out += _collect('stage1_at_residue_16', 101, D, lambda r: draw_pair(r, layout(40, 24, identical=some(r)), 60, 140, pivot=15),
                    lambda a, b: a['br16'] == D.stage1_min and a['rise_r'] >= 15 and b['br16'] == D.stage1_min - 1 and b['total'] == -1)
    # 2. threshold: br + bl == ungapped_min / ungapped_min - 1; the right side alone reaches it, and only the left side completes it
    out += _collect('threshold_right_alone', 102, D, lambda r: draw_pair(r, soften(layout(int(r.integers(4, 26)), 0, identical=some(r)), r), 60, 140, pivot=int(r.integers(15, 40))),
                    lambda a, b: a['br'] == D.ungapped_min and a['bl'] == 0 and b['total'] == D.ungapped_min - 1)
    out += _collect('threshold_left_completes', 103, D, lambda r: draw_pair(r, soften(layout(int(r.integers(0, 9)), 24, identical=some(r)), r), 60, 140, pivot=-int(r.integers(1, 25))),
                    lambda a, b: a['total'] == D.ungapped_min and a['bl'] > 0 and a['br'] < D.ungapped_min and a['br'] == b['br'] and b['total'] == D.ungapped_min - 1)

    # 3. drop and freeze: the sum falls xdrop + 1 below its best and strongly positive residues follow (they must not count: without the
    #    x-drop the pair would pass); the twin falls exactly xdrop and goes on to pass
    def valley(r):
        v0, v1 = CORE + int(r.integers(0, 6)), CORE + int(r.integers(6, 14))
        return draw_pair(r, layout(40, 0, extra={o: 'x' for o in range(v0, v1)}, identical=some(r)), 60, 140, pivot=v1 - 1, rises=False)

    def fell(a, b, side):
        return a['fall_' + side] == D.xdrop and not a['drop_' + side] and b['drop_' + side] and b['fall_' + side] == D.xdrop + 1
    out += _collect('drop_then_positive_right', 104, D, valley, lambda a, b: fell(a, b, 'r') and a['rise_r'] > b['n_r'])

    def valley_left(r):
        v0, v1 = 1 + int(r.integers(0, 5)), 7 + int(r.integers(0, 8))
        return draw_pair(r, layout(int(r.integers(0, 6)), 24, extra={-o: 'x' for o in range(v0, v1)}, identical=some(r)), 60, 140, pivot=-(v1 - 1), rises=False)
    out += _collect('drop_then_positive_left', 105, D, valley_left, lambda a, b: fell(a, b, 'l') and a['rise_l'] > b['n_l'] and a['br'] == b['br'] < D.ungapped_min)

    # 4. limits: the residue that completes the score is the last one inside the limit (right offset 39, left offset 24) / the first outside
    def at_limit(side, last):
        def draw(r):
            gap = int(r.integers(0, 3))                   # 'x' between the matching stretch and the completing residue
            if side == 'r':
                n = last - CORE - gap
                ident = some(r)
                ma = layout(n, 0, extra={last: '='}, identical=ident)
                mb = layout(n, 0, extra={last: 'x', last + 1: '='}, identical=ident)
            else:
                n = last - 1 - gap
                ma = layout(int(r.integers(0, 5)), n, extra={-last: '='}, identical=some(r))
                mb = dict(ma)
                mb[-last], mb[-last - 1] = 'x', '='
            ma, mb0 = soften(ma, r), mb
            far = (last, last + 1) if side == 'r' else (-last, -last - 1)
            mb = dict(ma)
            mb.update({o: mb0[o] for o in far})
            state = r.bit_generator.state
            a = draw_pair(r, ma, 60, 140)
            r.bit_generator.state = state                 # the twin: the same draws, the completing residue one offset further out
            b = draw_pair(r, mb, 60, 140)
            return (a, b) if np.array_equal(a[0], b[0]) else None
        return draw
    out += _collect('limit_right_39_40', 106, D, at_limit('r', 39), lambda a, b: a['rise_r'] == 39 and a['n_r'] == 40 and not b['drop_r'] and b['n_r'] == 40)
    out += _collect('limit_left_24_25', 107, D, at_limit('l', 24), lambda a, b: a['rise_l'] == 24 and not b['drop_l'] and b['n_l'] == 24 and a['br'] == b['br'])

    # 5. a sequence ends inside a block: the seed within 16 residues of the end / the start of the query / of the target, the other sequence
    #    going on; the completing residue is the sequence's last (first) one, and the twin is one residue shorter there
    def at_end(which, seq):
        def draw(r):
            e = int(r.integers(0 if which == 'end' else 1, 16))        # residues between the core and the end / the start
            if which == 'end':
                m = layout(e, 24, identical=some(r))
                c, n = 60, 60 + CORE + e
                cuts = [(0, n), (0, n - 1)]
            else:
                m = layout(int(r.integers(4, 30)), e, identical=some(r))
                c, n = 60, 60 - e
                cuts = [(n, None), (n + 1, None)]
            state = r.bit_generator.state
            res = []
            for cut in cuts:
                r.bit_generator.state = state
                kw = dict(q_cut=cut) if seq == 'q' else dict(t_cut=cut)
                res.append(draw_pair(r, m, c, 160, **kw))
            return tuple(res)
        return draw

    def ended(which):
        if which == 'end':
            return lambda a, b: a['rise_r'] == a['n_r'] - 1 and a['n_r'] == b['n_r'] + 1 and not a['drop_r'] and not b['drop_r'] and a['n_r'] < CORE + 16
        return lambda a, b: a['rise_l'] == a['n_l'] and a['n_l'] == b['n_l'] + 1 and not a['drop_l'] and not b['drop_l'] and a['n_l'] < 16
    for which in ('end', 'start'):
        for seq in ('q', 't'):
            out += _collect('%s_%s_inside_block' % ({'q': 'query', 't': 'target'}[seq], which), 110 + len(out), D, at_end(which, seq), ended(which))
    return out


def _run_cases():
    """6. a run of several hits of one diagonal bin: the seeds in front fail (stage 1), a later one passes / with the twin none does.  A pair
    is three single-seed stretches on one diagonal, 40 residues apart: two weak ones and, last in target order, a pair of case 2."""
    D = Par()
    rng = np.random.default_rng(120)
    weak = []
    while len(weak) < 2 * PAIRS:
        q, t = draw_pair(rng, layout(0, 0), 12, 40)[:2]
        n, ext = verdict(D, q, t)
        if n == 0 and len(ext) == 1:
            weak.append((q, t))
    strong = _collect('run', 121, D, lambda r: draw_pair(r, layout(int(r.integers(4, 26)), 0, identical=r.choice(CORE, int(r.integers(2, 13)), replace=False)), 12, 70, pivot=int(r.integers(15, 40))),
                      lambda a, b: a['br'] == D.ungapped_min and b['total'] == D.ungapped_min - 1)
    cases = []
    for role, s, cand in (('pass', strong[0], PAIRS), ('fail', strong[1], 0)):
        qs = [np.concatenate([weak[2 * i][0], weak[2 * i + 1][0], s['q'][i]]) for i in range(PAIRS)]
        ts = [np.concatenate([weak[2 * i][1], weak[2 * i + 1][1], s['t'][i]]) for i in range(PAIRS)]
        for q, t in zip(qs, ts):
            n, ext = verdict(D, q, t)
            assert n == (1 if cand else 0) and len(ext) == 3 and len(set(e['tpos'] - e['qpos'] for e in ext)) == 1, 'case builder: run'
        cases.append(dict(name='run_of_hits_later_one_decides/' + role, twin='run_of_hits_later_one_decides', par=D.overrides(), q=qs, t=ts, candidates=cand, tool='protein'))
    return cases


def _parameter_cases():
    """7. parameter sets off the defaults on one set of pairs: the count comes from the oracle alone (the host test holds each to a pre-filter
    that both rejects and accepts).  `tool`: nucleotide = the nucleotide parameter block on a 100-gene set."""
    rng = np.random.default_rng(31)
    qs, ts = [], []
    while len(qs) < 32:                                    # single-seed pairs of every strength, the seed anywhere from the start to the end
        q_len = int(rng.integers(60, 200))
        c = int(rng.integers(0, q_len - CORE))
        m = soften(layout(int(rng.integers(0, 48)), int(rng.integers(0, 48)), identical=rng.choice(CORE, int(rng.integers(0, 13)), replace=False)), rng)
        q, t = draw_pair(rng, m, c, q_len, t_pre=int(rng.integers(0, 3)) * 7)[:2]
        qs.append(q)
        ts.append(t[:200])
    cases = []
    sets = [('ext_37_19', dict(ext_right=37, ext_left=19)), ('ext_9_3', dict(ext_right=9, ext_left=3, stage1_min=20, ungapped_min=30)), ('ext_left_0', dict(ext_left=0)),
            ('ext_48_48', dict(ext_right=48, ext_left=48, ungapped_min=90)), ('xdrop_0', dict(xdrop=0)), ('xdrop_48', dict(xdrop=48, ungapped_min=80)),
            ('stage1_0', dict(stage1_min=0)), ('stage1_is_threshold', dict(stage1_min=55)), ('ungapped_min_0', dict(ungapped_min=0, stage1_min=0))]
    rng = np.random.default_rng(77)
    for i in range(10):                                    # random draws within the ranges pep_search accepts
        um = int(rng.integers(1, 120))
        sets.append(('random_%d' % i, dict(ungapped_min=um, stage1_min=int(rng.integers(0, min(um, 60) + 1)), xdrop=int(rng.integers(0, 49)),
                                           ext_right=int(rng.integers(1, 49)), ext_left=int(rng.integers(0, 49)))))
    for name, kw in sets:
        cases.append(dict(name='params/' + name, twin=None, par=Par(**kw).overrides(), q=qs, t=ts, candidates=None, tool='protein'))
    cases.append(dict(name='params/nucleotide', twin=None, par=None, q=None, t=None, candidates=None, tool='nucleotide'))
    return cases


@functools.lru_cache(maxsize=None)
def cases():
    """every case, twins next to each other: dicts with name, twin (the pair's name, None for the parameter sets), par (overrides of the
    pre-filter's five parameters), q / t (lists of uint8 residue codes), candidates (what the oracle must count; None: not stated), tool"""
    return tuple(_twin_cases() + _run_cases() + _parameter_cases())


def nucleotide_set():
    """the 100-gene nucleotide set of params/nucleotide: base codes of the genes and of their reverse complements (queries, targets)"""
    from peppan_amd import synth
    names, seqs = synth.make_genes(100, 0, seed=9)
    codes = [O.nt_codes(s.decode()) for s in seqs]
    return codes, codes + [(3 - c[::-1]).astype(np.uint8) for c in codes]
