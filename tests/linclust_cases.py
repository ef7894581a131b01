"""Hand-built cases for the clusterer (K9: lc_select, lc_insert, lc_verify, lc_assign of csrc/linclust.hip and the host merge of the gapped stage)
and a restatement of its definition: tests/test_linclust_cases_host.py holds the oracle to the restatement on every case and every case to what
its name says, tests/test_gpu_linclust.py compares the GPU with the oracle on each.

restate() is written from the definition text above oracle_linclust (oracle/align_oracle.c), steps 1, 2, 3 and 4, in numpy and plain Python; it
has no gapped stage (3b), so it equals the oracle exactly where no diagonal that fails without gaps is rescued with gaps.

The case families (a case: name, seqs, min_id, min_cov, base, k, m; every builder draws from a fixed seed):

    witness/   a sequence A and, for EVERY valid window position p of A, a witness: the window between random flanks, short enough to select all
               its own windows and never longer than A.  At min_id = min_cov = 0 the witness of p is a member of A exactly if A selected p, so
               `rep` spells out A's selected set position by position (the selection is otherwise nearly invisible in `rep`)
    limit/     witness sets at the largest k-mer spans pep_linclust accepts
    ladder/    overlapping windows of one random sequence, each accepted by longer ones: the greedy assignment has to wait through a chain of
               20 and more sequences (`depth` of restate()); on the staircase lc_assign needs as many launches (`rounds`)
    ties/      a centre and a slice of it whose overlap and match count sit on, one below and one above the thresholds of step 3; and pairs on
               exact equality that the gapped stage would not accept, so that the ungapped `>=` alone decides them
    repeat/    identical copies, equal lengths in both index orders, sequences of one or a few distinct k-mers (up to m diagonals to one centre)
    shape/     one to five sequences, none with a k-mer, none with a letter, empty ones in between, only the code `base`
    gapped/    one family with indels: the one case the gapped stage takes part in"""
import functools
import math

import numpy as np

M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------- the restatement
def windows(seq, base, k):
    """-> (positions, k-mer values, hashes) of the valid windows of seq: every code < base; value = sum of code[p + i] * base^i; hash =
    splitmix64 finaliser of the value (uint64 arithmetic wraps)"""
    seq = np.asarray(seq, dtype=np.uint8)
    n = len(seq) - k + 1
    if n <= 0:
        z = np.zeros(0, dtype=np.uint64)
        return np.zeros(0, dtype=np.int64), z, z
    bad = np.concatenate([[0], np.cumsum(seq >= base)])
    valid = (bad[k:] - bad[:-k]) == 0
    val = np.zeros(n, dtype=np.uint64)
    w = 1
    for i in range(k):
        val += seq[i:i + n].astype(np.uint64) * np.uint64(w)
        w = (w * base) & M64                                 # (only the weights of invalid windows' letters can wrap)
    pos = np.nonzero(valid)[0]
    val = val[pos]
    h = val.copy()
    h ^= h >> np.uint64(30)
    h *= np.uint64(0xbf58476d1ce4e5b9)
    h ^= h >> np.uint64(27)
    h *= np.uint64(0x94d049bb133111eb)
    h ^= h >> np.uint64(31)
    return pos, val, h


def select(seq, base, k, m):
    """step 1 -> [(position, k-mer value)] of the m smallest (hash, position), in that order"""
    pos, val, h = windows(seq, base, k)
    order = np.lexsort((pos, h))[:m]
    return [(int(pos[i]), int(val[i])) for i in order]


def restate(seqs, min_id, min_cov, base, k, m):
    """-> dict: rep (uint32 per sequence), selected / verified / accepted (the oracle's three totals), failed (diagonals that failed without
    gaps), depth (the longest chain of sequences that wait for an accepted centre in the assignment), rounds (the launches of lc_assign
    that chain costs at most), sel (the selections)"""
    n = len(seqs)
    seqs = [np.asarray(s, dtype=np.uint8) for s in seqs]
    length = [len(s) for s in seqs]
    # 1. selection
    sel = [select(s, base, k, m) for s in seqs]
    # 2. centre of a k-mer: the longest sequence that selected it, the lowest index among equals
    centre = {}
    for s in range(n):
        for _, key in sel[s]:
            c = centre.get(key)
            if c is None or length[s] > length[c]:          # (s ascends: an equal length never replaces)
                centre[key] = s
    # 3. one ungapped verification per distinct (centre, diagonal)
    accepted = [[] for _ in range(n)]
    verified = failed = 0
    for s in range(n):
        seen = set()
        for p, key in sel[s]:
            c = centre[key]
            if c == s:
                continue
            d = next(pc for pc, kc in sel[c] if kc == key) - p
            if (c, d) in seen:
                continue
            seen.add((c, d))
            verified += 1
            x0, x1 = max(0, -d), min(length[s], length[c] - d)
            overlap = x1 - x0
            matches = int((seqs[s][x0:x1] == seqs[c][x0 + d:x1 + d]).sum()) if overlap > 0 else 0
            if overlap > 0 and float(matches) >= min_id * float(overlap) and float(overlap) >= min_cov * float(length[c]) \
                    and float(overlap) >= min_cov * float(length[s]):
                if c not in accepted[s]:
                    accepted[s].append(c)
            else:
                failed += 1
    # 4. greedy assignment in (length descending, index ascending) order
    order = sorted(range(n), key=lambda s: (-length[s], s))
    rank = {s: i for i, s in enumerate(order)}
    members = [[] for _ in range(n)]
    for s in range(n):
        for c in accepted[s]:
            members[c].append(s)
    rep = [None] * n
    for s in order:
        if rep[s] is None:
            rep[s] = s
            for t in members[s]:
                if rep[t] is None:
                    rep[t] = s
    # depth: the longest chain "s waits for an accepted centre".  rounds: the same chain over the centres s cannot decide without - s knows its
    # verdict once every accepted centre ahead of the one it ends under (all of them, if it ends as a representative) is known to be a member
    # and that one to be a representative; that is the number of lc_assign launches when no launch sees its own writes
    chain, wait = [0] * n, [0] * n
    for s in order:
        chain[s] = 1 + max([chain[c] for c in accepted[s]], default=0)
        wait[s] = 1 + max([wait[c] for c in accepted[s] if rep[s] == s or rank[c] <= rank[rep[s]]], default=0)
    return dict(rep=np.array(rep, dtype=np.uint32).reshape(n), selected=sum(len(x) for x in sel), verified=verified, accepted=sum(len(a) for a in accepted),
                failed=failed, depth=max(chain, default=0), rounds=max(wait, default=0), sel=sel)


# ---------------------------------------------------------------------------------------------------------------- builders
def _case(name, seqs, min_id, min_cov, base=4, k=17, m=20, **kw):
    return dict(name=name, seqs=[np.ascontiguousarray(s, dtype=np.uint8) for s in seqs], min_id=float(min_id), min_cov=float(min_cov), base=base, k=k, m=m, **kw)


def _letters(rng, base, n):
    return rng.integers(0, base, n).astype(np.uint8)


WITNESS_PARAMS = [(4, 17, 20), (4, 17, 32), (4, 31, 20), (2, 31, 20), (8, 20, 20), (16, 15, 20), (20, 7, 20), (3, 12, 7), (4, 17, 1)]
WITNESS_SHAPES = [(0, 0), (1, 0), (19, 0), (20, 1), (62, 0), (63, 1), (64, 2), (127, 0), (128, 2), (129, 1), (300, 3)]


def _draw_a(rng, base, k, L, nbad, bad_at=None):
    """a sequence of L codes with nbad codes `base` (where the seed puts them, or at bad_at) whose valid windows hold distinct k-mers"""
    while True:
        a = _letters(rng, base, L)
        a[rng.choice(L, nbad, replace=False) if bad_at is None else bad_at] = base
        val = windows(a, base, k)[1]
        if len(set(val.tolist())) == len(val):
            return a


def _witness(rng, a, p, base, k, n_flank, keys_a):
    """flank + a[p:p + k] + flank: the letters next to the window differ from a's there, and no window but the planted one is a k-mer of a"""
    while True:
        na = int(rng.integers(0, n_flank + 1))
        fa, fb = _letters(rng, base, na), _letters(rng, base, n_flank - na)
        if na and p > 0 and fa[-1] == a[p - 1]:
            fa[-1] = (fa[-1] + 1 + rng.integers(0, base - 1)) % base
        if n_flank - na and p + k < len(a) and fb[0] == a[p + k]:
            fb[0] = (fb[0] + 1 + rng.integers(0, base - 1)) % base
        w = np.concatenate([fa, a[p:p + k], fb])
        pos, val, _ = windows(w, base, k)
        if [int(x) for x, v in zip(pos, val.tolist()) if v in keys_a] == [na]:
            return w


def _witness_set(rng, base, k, m, L, nbad, bad_at=None, a=None, positions=None, n_flank=None):
    a = _draw_a(rng, base, k, L, nbad, bad_at) if a is None else a
    pos, val, _ = windows(a, base, k)
    keys_a = set(val.tolist())
    n_flank = min(m - 1, L - k) if n_flank is None else n_flank
    positions = pos.tolist() if positions is None else positions
    return [a] + [_witness(rng, a, int(p), base, k, n_flank, keys_a) for p in positions], positions


def _witness_cases():
    out = []
    for bi, (base, k, m) in enumerate(WITNESS_PARAMS):
        for si, (extra, nbad) in enumerate(WITNESS_SHAPES):
            rng = np.random.default_rng(9000 + 100 * bi + si)
            seqs, positions = _witness_set(rng, base, k, m, k + extra, nbad)
            out.append(_case('witness/b%d_k%d_m%d/L-k=%d_bad%d' % (base, k, m, extra, nbad), seqs, 0., 0., base, k, m, family='witness', positions=positions))
    # one bad letter next to the stretches of lc_select (npos = 130: 3 positions per lane, stretch j starts at 3j): the last letter before a
    # stretch start, the first letter of a stretch, the last letter of the stretch's first window
    j = 21
    for name, at in (('before_stretch', 3 * j - 1), ('stretch_start', 3 * j), ('first_window_end', 3 * j + 17 - 1)):
        rng = np.random.default_rng(9900 + at)
        seqs, positions = _witness_set(rng, 4, 17, 20, 17 + 129, 1, bad_at=[at])
        out.append(_case('witness/bad_%s_%d' % (name, at), seqs, 0., 0., family='witness', positions=positions))
    return out


def _long_cases():
    """A of 70 000 codes: positions pass 16 bits.  Witnesses for the 20 positions A selects and for 20 it does not - with flanks at
    min_id = 0 like every witness set, and bare (the window alone) at min_id = 1, where a witness is accepted only on the right diagonal"""
    rng = np.random.default_rng(70000)
    a = _draw_a(rng, 4, 17, 70000, 5)
    chosen = sorted(p for p, _ in select(a, 4, 17, 20))
    assert len(chosen) == 20 and sum(p > 65535 for p in chosen) >= 1 and sum(p < 65536 for p in chosen) >= 1, 'case builder: long (the seed must put selected positions on both sides of 2^16)'
    valid = set(windows(a, 4, 17)[0].tolist())
    # not selected: the neighbours of selected positions, a selected position less 2^16, both sides of 2^16, the last window, random ones
    others = []
    for p in [chosen[0] + 1, chosen[-1] - 1, chosen[-1] + 1, chosen[-1] - 65536, 65535, 65536, 69983] + rng.integers(0, 69984, 40).tolist():
        if p in valid and p not in chosen and p not in others and len(others) < 20:
            others.append(int(p))
    assert len(others) == 20, 'case builder: long'
    positions = chosen + sorted(others)
    out = []
    for name, n_flank, min_id in (('flanks', 19, 0.), ('bare', 0, 1.)):
        seqs, _ = _witness_set(rng, 4, 17, 20, 70000, 0, a=a, positions=positions, n_flank=n_flank)
        out.append(_case('witness/long_70000_' + name, seqs, min_id, 0., family='long', positions=positions, chosen=chosen))
    return out


def _limit_cases():
    out = []
    for i, (base, k) in enumerate([(4, 31), (8, 21), (2, 32), (20, 14)]):
        rng = np.random.default_rng(9800 + i)
        seqs, positions = _witness_set(rng, base, k, 20, k + 64, 2)
        out.append(_case('limit/b%d_k%d' % (base, k), seqs, 0., 0., base, k, 20, family='limit', positions=positions))
    return out


def ladder(n=100, step=40, seed=1):
    g = _letters(np.random.default_rng(seed), 4, 6000)
    return [g[step * i:step * i + 1200 - 3 * i] for i in range(n)]


def _ladder_cases():
    out = []
    up = ladder()
    for min_id, min_cov in ((0., 0.), (0.9, 0.5), (0.9, 0.9)):
        out.append(_case('ladder/100_id%g_cov%g' % (min_id, min_cov), up, min_id, min_cov, family='ladder'))
        out.append(_case('ladder/100_reversed_id%g_cov%g' % (min_id, min_cov), up[::-1], min_id, min_cov, family='ladder'))
    out.append(_case('ladder/257_step15_id0.9_cov0.5', ladder(257, 15), 0.9, 0.5, family='ladder'))
    out.append(_case('ladder/257_step15_reversed_id0.9_cov0.5', ladder(257, 15)[::-1], 0.9, 0.5, family='ladder'))
    # a staircase: every window reaches only its next few neighbours, so representatives and members alternate down the whole list and a
    # window's verdict waits for the previous window's - the fixed point of lc_assign needs a launch per step, not only a long chain
    h = _letters(np.random.default_rng(2), 4, 2000)
    stairs = [h[30 * i:30 * i + 120 - i] for i in range(60)]
    out.append(_case('ladder/staircase_60', stairs, 0., 0., family='ladder', rounds_min=20))
    out.append(_case('ladder/staircase_60_reversed', stairs[::-1], 0., 0., family='ladder', rounds_min=20))
    for c in out:
        r = restate(c['seqs'], c['min_id'], c['min_cov'], 4, 17, 20)
        c['depth'], c['rounds'] = r['depth'], r['rounds']
        assert c['depth'] >= 20 and c['rounds'] >= c.get('rounds_min', 0), 'case builder: %s has depth %d, rounds %d' % (c['name'], c['depth'], c['rounds'])
    return out


TIE_LC = (100, 101, 1000)
TIE_ID = (0.9, 0.95, 0.97, 1.0)
TIE_COV = (0.5, 0.8, 0.9)


def tie_grid(min_id, min_cov):
    """-> [(Lc, ovl, matches, which)] of one (min_id, min_cov): ovl one below, at and one above ceil(min_cov * Lc); matches one below, at
    ceil(min_id * ovl) and at its floor (`which` names them; equal numbers once), all in Python doubles"""
    out = []
    for lc in TIE_LC:
        edge = math.ceil(min_cov * lc)
        for ovl in (edge - 1, edge, edge + 1):
            named = (('ceil-1', math.ceil(min_id * ovl) - 1), ('ceil', math.ceil(min_id * ovl)), ('floor', math.floor(min_id * ovl)))
            for mt in sorted(set(v for _, v in named)):
                out.append((lc, ovl, mt, '='.join(w for w, v in named if v == mt)))
    return out


def _tie_pair(rng, lc, ovl, matches, min_id, min_cov, second=False):
    """a centre and a slice of it with ovl - matches substitutions, none within 20 positions of an end (second: but one of them the slice's
    second letter); drawn until the restatement verifies the pair (the two select a common k-mer) once"""
    while True:
        c = _letters(rng, 4, lc)
        start = int(rng.integers(0, lc - ovl + 1))
        s = c[start:start + ovl].copy()
        at = 20 + rng.choice(ovl - 40, ovl - matches - second, replace=False)
        at = np.concatenate([at, [1]]) if second else at
        s[at] = (s[at] + 1 + rng.integers(0, 3, len(at))) % 4
        r = restate([c, s], min_id, min_cov, 4, 17, 20)
        if r['verified'] == 1:
            return c, s


def _tie_cases():
    out = []
    for i, min_id in enumerate(TIE_ID):
        for j, min_cov in enumerate(TIE_COV):
            rng = np.random.default_rng(5000 + 10 * i + j)
            seqs, pairs = [], []
            for lc, ovl, mt, which in tie_grid(min_id, min_cov):
                c, s = _tie_pair(rng, lc, ovl, mt, min_id, min_cov)
                pairs.append(dict(centre=len(seqs), member=len(seqs) + 1, Lc=lc, ovl=ovl, matches=mt, which=which))
                seqs += [c, s]
            out.append(_case('ties/id%g_cov%g' % (min_id, min_cov), seqs, min_id, min_cov, family='ties', pairs=pairs))
    # The pairs above keep their substitutions away from the ends, so the gapped stage would align what the diagonal compared, and a pair on a
    # tie that the ungapped comparison lost would be accepted with gaps all the same.  Here the slice's SECOND letter is substituted: a local
    # alignment starts behind it (+2 - 3 < 0) and spans two letters less - below the coverage the overlap just reaches.  So these pairs are
    # members only through the ungapped comparison itself: `exact` names the comparisons that hold with equality
    rng = np.random.default_rng(5900)
    seqs, pairs = [], []
    for lc, ovl, mt, exact in ((100, 50, 45, ('id', 'cov')), (1000, 500, 450, ('id', 'cov')), (100, 50, 49, ('cov',)), (119, 60, 54, ('id',))):
        c, s = _tie_pair(rng, lc, ovl, mt, 0.9, 0.5, second=True)
        pairs.append(dict(centre=len(seqs), member=len(seqs) + 1, Lc=lc, ovl=ovl, matches=mt, exact=exact))
        seqs += [c, s]
    out.append(_case('ties/exact_and_no_rescue_id0.9_cov0.5', seqs, 0.9, 0.5, family='exact', pairs=pairs))
    return out


def _repeat_cases():
    rng = np.random.default_rng(600)
    out = []
    one = _letters(rng, 4, 200)
    out.append(_case('repeat/40_identical', [one] * 40, 1., 1., family='repeat', verified=39))
    base_seq = _letters(rng, 4, 300)
    variants = []
    for _ in range(6):
        v = base_seq.copy()
        at = rng.choice(300, 6, replace=False)
        v[at] = (v[at] + 1 + rng.integers(0, 3, 6)) % 4
        variants.append(v)
    out.append(_case('repeat/equal_length_variants', variants, 0.9, 0.9, family='repeat'))
    out.append(_case('repeat/equal_length_variants_reversed', variants[::-1], 0.9, 0.9, family='repeat'))
    # two accepted centres of one length, both representatives: the member's first half ends the one, its second half starts the other, and
    # the two share nothing - the lower index takes the member, wherever the three stand (the tie of higher() in lc_assign)
    seqs, triples, rng2 = [], [], np.random.default_rng(601)
    for order in ('abs', 'bas', 'sab', 'asb', 'sba', 'bsa'):
        p1, p2, r1, r2 = (_letters(rng2, 4, n) for n in (100, 100, 200, 200))
        three = dict(a=np.concatenate([r1, p1]), b=np.concatenate([p2, r2]), s=np.concatenate([p1, p2]))
        triples.append({x: len(seqs) + order.index(x) for x in 'abs'})
        seqs += [three[x] for x in order]
    out.append(_case('repeat/two_centres_of_equal_length', seqs, 1., 0.3, family='repeat', triples=triples))
    a = np.zeros(100, dtype=np.uint8)
    acgt =np.tile(np.arange(4, dtype=np.uint8), 30)
    unit = _letters(rng, 4, 23)
    long_ = np.tile(unit, 9)
    # one-key sequences: every selected position of the member is another diagonal to the one centre
    out.append(_case('repeat/A100_A60', [a, a[:60]], 1., 0., family='repeat', verified=20))
    out.append(_case('repeat/ACGT30_ACGT20_less_first', [acgt, acgt[:80][1:]], 1., 0., family='repeat'))
    out.append(_case('repeat/unit23x9_slice', [long_, long_[30:170]], 1., 0., family='repeat'))
    return out


def _shape_cases():
    rng = np.random.default_rng(700)
    s0 = _letters(rng, 4, 240)
    fam = [s0, s0[10:200], s0[40:], s0[:100], _letters(rng, 4, 150)]
    e = np.zeros(0, dtype=np.uint8)
    out = [_case('shape/n%d' % n, fam[:n], 1., 0., family='shape') for n in (1, 3, 4, 5)]
    out.append(_case('shape/all_shorter_than_k', [s0[:16], s0[3:19], s0[:1], s0[50:62], e], 0., 0., family='shape', selected=0))
    out.append(_case('shape/all_empty', [e] * 6, 0.9, 0.9, family='shape', selected=0))
    out.append(_case('shape/empty_between_full', [e, s0, e, e, s0[20:220], e, fam[4], s0[5:90], e], 1., 0., family='shape'))
    out.append(_case('shape/only_code_base', [s0, np.full(90, 4, dtype=np.uint8), s0[30:], np.full(17, 4, dtype=np.uint8)], 1., 0., family='shape'))
    return out


def _gapped_case():
    rng = np.random.default_rng(800)
    top = _letters(rng, 4, 312)
    seqs = [top]
    for i in range(11):
        n = 1 + (i % 12)
        at = int(rng.integers(60, 240))
        v = np.concatenate([top[:at], top[at + n:]]) if i % 2 else np.concatenate([top[:at], _letters(rng, 4, n), top[at:300]])
        sub = rng.choice(len(v), 3, replace=False)
        v[sub] = (v[sub] + 1 + rng.integers(0, 3, 3)) % 4
        seqs.append(v)
    return [_case('gapped/family_of_12', seqs, 0.95, 0.9, family='gapped')]


@functools.lru_cache(maxsize=None)
def cases():
    """every case: dicts with name, seqs (uint8 code arrays), min_id, min_cov, base, k, m, family and what the family's self-checks use"""
    return tuple(_witness_cases() + _long_cases() + _limit_cases() + _ladder_cases() + _tie_cases() + _repeat_cases() + _shape_cases() + _gapped_case())


@functools.lru_cache(maxsize=None)
def restated(name):
    """restate() of the case of that name, computed once"""
    c = next(c for c in cases() if c['name'] == name)
    return restate(c['seqs'], c['min_id'], c['min_cov'], c['base'], c['k'], c['m'])


@functools.lru_cache(maxsize=None)
def oracle_results():
    """name -> (rep, totals) of oracle_linclust on every case, computed once and shared"""
    from oracle import oracle as O
    return {c['name']: O.linclust(c['seqs'], c['min_id'], c['min_cov'], base=c['base'], k=c['k'], m=c['m']) for c in cases()}
