"""What the K21 tests share: the numpy restatement of the neighbour-joining rules of include/peppan_hip.h, the Kimura pair counts in numpy,
bipartition sets of join records and of Newick texts, and the builders of the test matrices.

The restatement is the definition the device is held to bit for bit: float64 throughout, every operation one numpy operation (numpy never fuses a
multiplication into an addition), the row sums added left to right, the arg-min the first smallest Q in row-major order over the live slots.
With a `trace` it also says, round by round, which pairs tied and whether a NaN or the no-usable-Q fallback was met: tests/test_njtree_host.py
holds the tie and overflow matrices of tests/test_gpu_njtree_edges.py (edge_case) to the branches they are meant to reach.

    python tests/njtree_helpers.py > profiles/njtree_vs_reference.txt     how far the restatement is from what rapidnj printed for the committed fixtures"""
import gzip
import json
import os
import sys

import numpy as np


def nj_restated(matrix, trace=None):
    """(node uint32[2 n - 3], length float64[2 n - 3]) of one square matrix, of which the entries with row < column are read.  Sums that overflow are
    legal (the header's rules for +infinity and NaN apply), so numpy's warnings are off in here.

    trace: a list that receives one (m, i, j, n_min, rows_min, any_nan, fallback) per round - the live slots, the list positions joined, how many usable
    pairs (Q below +infinity) attain the smallest Q, the set of list rows i they lie in, whether any Q of the upper triangle is NaN, and whether
    positions 0, 1 were taken for lack of a usable Q.  It changes nothing of what is computed."""
    with np.errstate(all='ignore'):
        return _nj_restated(matrix, trace)


def _nj_restated(matrix, trace):
    n = len(matrix)
    up = np.triu(np.asarray(matrix, dtype=np.float64), 1)
    D = up + up.T
    if n < 2:
        raise ValueError('a tree needs 2 leaves')
    if n == 2:
        return np.array([0, 1], np.uint32), np.array([D[0, 1], D[0, 1]])
    r = np.zeros(n)
    for j in range(n):                                       # left to right from 0.0
        r = r + D[:, j]
    live = list(range(n))
    node = list(range(n))
    out_node, out_len = [], []
    s = 0
    while len(live) > 3:
        m = len(live)
        L = np.array(live)
        Dl, rl = D[np.ix_(L, L)], r[L]
        Q = (float(m - 2) * Dl - rl[:, None]) - rl[None, :]
        upper = np.triu(np.ones((m, m), bool), 1)
        usable = upper & (Q < np.inf)
        masked = np.where(usable, Q, np.inf)
        fallback = not usable.any()
        if not fallback:
            i, j = divmod(int(np.argmin(masked)), m)         # the first smallest: the smaller a, then the smaller b
        else:
            i, j = 0, 1
        if trace is not None:
            ties = usable & (masked == masked[i, j])
            trace.append((m, i, j, int(ties.sum()), set(np.flatnonzero(ties.any(1)).tolist()), bool((np.isnan(Q) & upper).any()), fallback))
        a, b = live[i], live[j]
        dab, ra, rb = D[a, b], r[a], r[b]
        la = 0.5 * dab + (ra - rb) / float(2 * (m - 2))
        out_node += [node[a], node[b]]
        out_len += [la, dab - la]
        ks = np.array([k for k in live if k != a and k != b])
        dak, dbk = D[a, ks].copy(), D[b, ks].copy()
        du = ((dak + dbk) - dab) * 0.5
        r[ks] = ((r[ks] - dak) - dbk) + du
        D[a, ks] = D[ks, a] = du
        r[a] = 0.5 * ((ra + rb) - float(m) * dab)
        node[a] = n + s
        live.pop(j)
        s += 1
    a, b, c = live
    la = 0.5 * ((D[a, b] + D[a, c]) - D[b, c])
    last = [(node[a], la), (node[b], D[a, b] - la), (node[c], D[a, c] - la)]
    if n == 3:                                               # rapidnj prints three leaves in the order 1, 0, 2
        last = [last[1], last[0], last[2]]
    out_node += [x for x, _ in last]
    out_len += [x for _, x in last]
    return np.array(out_node, np.uint32), np.array(out_len, np.float64)


def branches_of_record(node, length, n):
    """[(frozenset of leaf ids below the branch, length)] of a join record, one per entry"""
    below = {k: frozenset([k]) for k in range(n)}
    out = []
    for s in range(max(n - 3, 0)):
        x, y = int(node[2 * s]), int(node[2 * s + 1])
        below[n + s] = below[x] | below[y]
    for k, d in zip(node, length):
        out.append((below[int(k)], float(d)))
    return out


def bipartitions(branches, leaves):
    """the splits of a tree as a set: per branch the side that does not hold the first leaf"""
    leaves = list(leaves)
    everything = frozenset(leaves)
    return {side if leaves[0] not in side else everything - side for side, _ in branches}


def lengths_by_split(branches, leaves):
    """{split: branch length}; the two branches of a two-leaf tree, which share their split, are added"""
    leaves = list(leaves)
    everything = frozenset(leaves)
    out = {}
    for side, d in branches:
        key = side if leaves[0] not in side else everything - side
        out[key] = out.get(key, 0.) + d
    return out


def kimura_counts(codes):
    """codes uint8[n, L] (0 gap, 1..4 = A C G T) -> int32[n (n - 1) / 2, 3]: comparable, transitions, transversions of every pair a < b, row-major"""
    codes = np.asarray(codes)
    out = []
    for a in range(len(codes)):
        for b in range(a + 1, len(codes)):
            x, y = codes[a], codes[b]
            both = (x > 0) & (y > 0)
            differ = both & (x != y)
            ts = differ & ((x + y == 4) & (x != 2) & (y != 2) | (x + y == 6) & (x != 3) & (y != 3))       # A <-> G: 1 + 3, C <-> T: 2 + 4
            out.append((int(both.sum()), int(ts.sum()), int(differ.sum()) - int(ts.sum())))
    return np.array(out, dtype=np.int32).reshape(-1, 3)


def pack_codes(codes):
    """uint8[n, L] of 0..4 -> the .seq store's base-5 packing, uint8[n, ceil(L / 3)] (first third * 25 + second third * 5 + last third)"""
    codes = np.asarray(codes, dtype=np.uint8)
    n, L = codes.shape
    s = -(-L // 3)
    full = np.zeros((n, 3 * s), dtype=np.uint8)
    full[:, :L] = codes
    return full[:, :s] * 25 + full[:, s:2 * s] * 5 + full[:, 2 * s:]


# ---- the rapidnj fixtures (tests/golden/njtree_pd.json.gz, njtree_fa.json.gz)

def load_cases(name):
    with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', name), 'rt') as f:
        return json.load(f)['cases']


def square(upper, n):
    m = np.zeros((n, n))
    m[np.triu_indices(n, 1)] = upper
    return m + m.T


CODE = np.zeros(256, np.uint8)
CODE[[65, 67, 71, 84]] = (1, 2, 3, 4)


def codes_of(case):
    return CODE[np.frombuffer(''.join(case['rows']).encode(), np.uint8).reshape(case['n'], -1)]


def digit_bound(v):
    """half a unit of the fifth significant digit of a printed value"""
    return 0. if v == 0 else 0.5 * 10. ** (np.floor(np.log10(abs(v))) - 4)


def named_branches(matrix, names):
    node, length = nj_restated(matrix)
    return [(frozenset(names[k] for k in side), d) for side, d in branches_of_record(node, length, len(names))]


def against_text(text, matrix, names, parse):
    """the restatement's tree of `matrix` against the text rapidnj printed (parse: njtree.parse_newick): asserts the same leaves and the same splits, all
    2 n - 3 of them -> (worst |difference| of a branch length, worst excess of one over half a unit of the printed value's fifth digit), matched by split"""
    mine = named_branches(matrix, names)
    leaves, branches = parse(text.replace("'", ''))
    n = len(names)
    assert sorted(leaves) == sorted(names) and len(branches) == len(mine) == (2 if n == 2 else 2 * n - 3)
    assert bipartitions(branches, names) == bipartitions(mine, names)
    got, want = lengths_by_split(mine, names), lengths_by_split(branches, names)
    bound = lengths_by_split([(side, digit_bound(d)) for side, d in branches], names)          # (two leaves print their one split twice: the bounds add like the lengths)
    diff = {k: abs(got[k] - want[k]) for k in want}
    return max(diff.values()), max(diff[k] - bound[k] for k in want)


def fixture_report(kimura_distances, parse):
    """per committed case (name, n, worst branch difference, its excess over the digit bound, worst excess of a Kimura distance over the printed quantum 5e-7
    or None): the text of profiles/njtree_vs_reference.txt, and what tests/test_njtree_host.py holds to its allowances"""
    rows = [('pd ' + c['kind'], c['n']) + against_text(c['newick'], square(c['upper'], c['n']), c['names'], parse) + (None,) for c in load_cases('njtree_pd.json.gz')]
    for c in load_cases('njtree_fa.json.gz'):
        counts = kimura_counts(codes_of(c))
        d, undefined = kimura_distances(counts[:, 0], counts[:, 1], counts[:, 2])
        assert not undefined.any()
        off = float(np.abs(d[np.triu_indices(c['n'], 1)] - np.array(c['matrix_upper'])).max()) - 5e-7
        rows.append(('fa', c['n']) + against_text(c['newick'], d, c['names'], parse) + (off,))
    return rows


# ---- case builders

def euclidean(n, seed, dims=6):
    """distances of n random points, rounded to 6 decimals (the form the fixtures store)"""
    rng = np.random.default_rng(seed)
    pts = rng.random((n, dims))
    return np.round(np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)), 6)


def cgav_like(n, seed, genes=300):
    """-log((shared + 0.5) / (presence + 1)) of random allelic profiles with a few lineages, as getDistance makes it"""
    rng = np.random.default_rng(seed)
    founders = rng.integers(1, 6, (4, genes))
    prof = founders[rng.integers(0, 4, n)].copy()
    change = rng.random((n, genes)) < 0.15
    prof[change] = rng.integers(0, 9, int(change.sum()))
    shared = ((prof[:, None, :] == prof[None, :, :]) & (prof[:, None, :] > 0)).sum(-1)
    presence = ((prof[:, None, :] > 0) & (prof[None, :, :] > 0)).sum(-1)
    d = -np.log((shared + 0.5) / (presence + 1.))
    np.fill_diagonal(d, 0.)
    return d


def with_duplicates(n, seed):
    """a Euclidean matrix in which several points coincide: rows are duplicated, Q ties, and the tie-break decides"""
    rng = np.random.default_rng(seed)
    pts = rng.integers(0, 4, (max(2, n // 3), 3)).astype(np.float64)
    pts = pts[rng.integers(0, len(pts), n)]
    return np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))


def tied(n, seed, levels=3):
    """a symmetric matrix of integers 0 .. levels - 1 with a zero diagonal: Q is a small integer, so in most rounds several pairs attain the minimum"""
    rng = np.random.default_rng(seed)
    up = np.triu(rng.integers(0, levels, (n, n)).astype(np.float64), 1)
    return up + up.T


def tied_clades(n, seed, levels=3, fan=2):
    """integers 0 .. levels - 1 again, but an ultrametric: every leaf draws a label of levels - 1 digits below `fan`, and two leaves are as far apart as
    digits remain from the first one they differ in.  Leaves with one label are duplicates, a join of two of them is one more, and so the smallest Q is
    shared by several pairs until a label is down to two leaves: ties in most rounds, where independent draws (tied) tie in about 3 % of them"""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, fan, (n, levels - 1))
    same = np.cumprod(labels[:, None, :] == labels[None, :, :], axis=-1).sum(-1)          # digits of the common prefix
    return (levels - 1 - same).astype(np.float64)


def constant(n, value):
    """every distance off the diagonal is `value`: all Q equal in the first round; at 1e308 every row sum overflows and every Q is NaN"""
    d = np.full((n, n), float(value))
    np.fill_diagonal(d, 0.)
    return d


def planted(n, seed, a, b):
    """euclidean(n, seed) in which a and b all but coincide"""
    d = euclidean(n, seed)
    d[a, b] = d[b, a] = 1e-9
    return d


def one_huge_row(n, seed):
    """euclidean(n, seed) with row and column 0 at 1.5e308: r[0] overflows, so every Q of row 0 is NaN, and every other Q is -infinity"""
    d = euclidean(n, seed)
    d[0, 1:] = d[1:, 0] = 1.5e308
    return d


def chain_parts(m):
    """the workgroups of nj_chain_argmin at m live slots; workgroup (i // 4) % parts has list row i, wavefront i % 4 of it"""
    return min(256, -(-(m - 1) // 4))


# the tie and overflow matrices of tests/test_gpu_njtree_edges.py, by name; tests/test_njtree_host.py proves from the trace that each reaches its branch
TIED_SIZES = (4, 5, 32, 33, 64, 65, 66, 80, 81, 129, 255, 256, 257, 301)
CONSTANT_SIZES = (5, 65, 81, 257)
CGAV12_SIZES = (100, 301)
ALL_NAN_SIZES = (4, 6, 40, 100, 257)
HUGE_ROW_SIZES = (6, 100, 257)
EDGE_BUILDERS = {'tied': lambda n: tied(n, 1),
                 'clades': lambda n: tied_clades(n, 2 if n >= 1026 else 1),       # (seed 2 at 1030 leaves: the first round's ties reach list row 1024)
                 'constant': lambda n: constant(n, 0.25),
                 'cgav12': lambda n: cgav_like(n, 7, genes=12), 'planted': lambda n: planted(n, 1, n - 4, n - 2),
                 'all_nan': lambda n: constant(n, 1e308), 'huge_row': lambda n: one_huge_row(n, 5)}
_edge_cases = {}


def edge_case(kind, n):
    """(matrix, node, length, trace) of EDGE_BUILDERS[kind](n), restated once per process and read-only: both test modules share it"""
    if (kind, n) not in _edge_cases:
        matrix, trace = EDGE_BUILDERS[kind](n), []
        node, length = nj_restated(matrix, trace)
        for a in (matrix, node, length):
            a.setflags(write=False)
        _edge_cases[kind, n] = (matrix, node, length, tuple(trace))
    return _edge_cases[kind, n]


def non_additive(n, seed):
    """random symmetric values that are no metric: neighbour joining gives negative branch lengths"""
    rng = np.random.default_rng(seed)
    d = rng.random((n, n)) ** 3
    d = np.triu(d, 1)
    return d + d.T


def mixed_batch(count=200, seed=2026):
    """`count` matrices of 2 .. 70 leaves: Euclidean ones, and among them an all-zero matrix, matrices with duplicated rows, a non-additive one (negative
    branch lengths) and a CGAV-like one"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 71, count)
    sizes[:8] = (2, 3, 4, 5, 63, 64, 65, 70)
    mats = [euclidean(int(n), seed + k) for k, n in enumerate(sizes)]
    mats[10] = np.zeros((17, 17))
    mats[11] = with_duplicates(33, seed + 1)
    mats[12] = with_duplicates(70, seed + 2)
    mats[13] = with_duplicates(4, seed + 3)
    mats[14] = non_additive(40, seed + 4)
    mats[15] = cgav_like(50, seed + 5)
    return mats


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from peppan_amd.njtree import kimura_distances, parse_newick
    print('the float64 restatement against rapidnj (float32, five printed digits) on the committed fixtures; tests/test_njtree_host.py allows 4 x the worst excess')
    print('case              n   worst |branch difference|   excess over half a unit of the 5th digit   excess of a Kimura distance over 5e-7')
    report = fixture_report(kimura_distances, parse_newick)
    for name, n, diff, excess, dist in report:
        print('%-12s %6d   %.3e                   %10.3e                                 %s' % (name, n, diff, excess, '' if dist is None else '%10.3e' % dist))
    print('worst excess of a branch length: %.3e; of a Kimura distance: %.3e' % (max(r[3] for r in report), max(r[4] for r in report if r[4] is not None)))
