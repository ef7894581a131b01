#!/usr/bin/env python3
"""Generate tests/golden/g29_batchprep.json.gz by IMPORTING the reference's Python (build machine only: needs /root/reference).

    python tests/golden/make_golden_batchprep.py

The same shim as make_golden_divergence.py.  The reference's own filt_genes (PEPPAN.py:525-734) runs, once with `--orthology nj` and once with sbh, on
seeded stores written with its MapBsn: a .tab store of gene tables and a .conflicts store of two members.  Replaced for the run: PEP.pool2 by an object
whose imap_unordered is map and which records what load_conflict and filt_per_group were handed; PEP.filt_per_group by `lambda d: [d[0]]`; PEP.mat_out by
a list.  A trace function on filt_genes' frame (the technique of make_golden_outalleles.py) records genes, used, tmpSet and new_groups at :546, :579,
:595 and :658 of every round.  Only DATA is written: the tables, the conflict lists, the dictionaries handed in, and what was recorded.

The scenario (clust_identity 0.9; conflict kinds as :860 gives them: 0 within one exemplar, else 1 or 2):
  rank 0   hub          whose lists name loci of P, Q and of the rank-1 genes with kinds 1 and 2, so that `used` holds values of both signs afterwards
           P            5 rows, 3 of them in the hub's lists: popped at exactly 0.6 in round 1, back in round 2
           Q            10 rows, 5 in the hub's lists: just under 0.6
           W7, W8       G = 4 with n = 2 G - 1 and n = 2 G rows; W8 has the chain a -> b -> c (b dropped, c stays), one-sided lists, a list that names loci of W7
           CUTL, CUTC   G = 300 x 4 rows: cut < clust_identity; cut >= clust_identity with n <= 6 G
           CUT6         G = 150 x 8 rows: n > 6 G
           FIN          one row per genome, min(col3) = 9000 exactly
           ONE          two rows of one genome, the first names the second: one row left
  rank 1   E            its good rows are in `used` by then: excluded in stage A; X, which `conflicting` pairs with E, is withdrawn with it
           N1, N3, N4   1, 3 and 4 rows negated by `used` values <= 0, and a row zeroed by a value > 0
The generator asserts what the fixture is pinned by: columns 2 and 3 are distinct within every group that takes a sort, so the reference's answer does not
depend on numpy's tie order; the restatement of tests/batchprep_helpers.py equals the recording at every point; every branch of its BRANCHES was taken."""
import gzip, json, os, stat, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'


def build_shim():
    root = tempfile.mkdtemp(prefix='peppan_shim_')
    os.makedirs(os.path.join(root, 'bin'))
    for t in ('mmseqs', 'makeblastdb', 'diamond', 'blastn'):
        p = os.path.join(root, 'bin', t)
        with open(p, 'w') as f:
            f.write('#!/bin/sh\nexit 0\n')
        os.chmod(p, os.stat(p).st_mode | stat.S_IEXEC | stat.S_IXGRP | stat.S_IXOTH)
    for pkg, body in (('numba', 'def jit(*a, **k):\n    if len(a) == 1 and callable(a[0]) and not k:\n        return a[0]\n    return lambda f: f\n'),
                      ('ete3', 'class Tree(object):\n    pass\n')):
        os.makedirs(os.path.join(root, 'py', pkg))
        with open(os.path.join(root, 'py', pkg, '__init__.py'), 'w') as f:
            f.write(body)
    os.makedirs(os.path.join(root, 'cwd'))
    return root


SHIM = build_shim()
os.environ['PATH'] = os.path.join(SHIM, 'bin') + os.pathsep + os.environ['PATH']
sys.path[:0] = [os.path.join(SHIM, 'py'), os.path.join(REF, 'modules'), REF, os.path.dirname(HERE)]
os.chdir(os.path.join(SHIM, 'cwd'))

import numpy as np                       # noqa: E402
if not hasattr(np.lib.npyio, 'format'):  # numpy >= 2 dropped this alias of np.lib.format; the reference's MapBsn spells it the old way
    np.lib.npyio.format = np.lib.format
import PEPPAN as PEP                     # noqa: E402
import batchprep_helpers as H            # noqa: E402

CI = 0.9
LINES = {546: 'start', 579: 'after_a', 595: 'after_b', 658: 'after_c'}
CODE = PEP.filt_genes.__code__


def scenario():
    """-> dict(tab: exemplar -> table, lists: locus -> values, priorities, scores, ortho_groups)"""
    tab, lists, next_locus = {}, {}, [100]

    def gene(ex, genomes, c3, c2=None, base=None):
        """a table: one row per entry of `genomes`; columns 2 and 3 distinct"""
        n = len(genomes)
        if base is not None:
            next_locus[0] = base
        loci = list(range(next_locus[0], next_locus[0] + n))
        next_locus[0] += n + 7
        c2 = c2 or [20000 + 100 * ex + 13 * (n - k) for k in range(n)]
        assert len(set(c2)) == n and len(set(c3)) == n, ex
        tab[ex] = [[ex, g, a, b, b, l, 1] for g, a, b, l in zip(genomes, c2, c3, loci)]
        return loci

    def name(a, b, kind):
        lists.setdefault(a, []).append(b * 10 + kind)

    hub = gene(1, list(range(12)), [9990 - 3 * k for k in range(12)])
    p = gene(2, list(range(5)), [9900 - 5 * k for k in range(5)])
    q = gene(3, list(range(10)), [9800 - 5 * k for k in range(10)])
    for k, l in enumerate(p[:3] + q[:5]):
        name(hub[k], l, 1 + k % 2)
        name(l, hub[k], 1 + k % 2)
    w7 = gene(4, [0, 0, 1, 1, 2, 2, 3], [9700 - 9 * k for k in range(7)])
    name(w7[0], w7[1], 0)                                        # (never walked: 7 < 2 * 4)
    w8 = gene(5, [0, 0, 1, 1, 2, 2, 3, 3], [9650 - 9 * k for k in range(8)], c2=[30000 - 11 * k for k in range(8)])
    name(w8[0], w8[1], 0)                                        # a -> b, one-sided
    name(w8[1], w8[2], 0)                                        # b -> c: b is dropped, c stays
    name(w8[4], w8[5], 0)
    name(w8[5], w8[4], 0)
    name(w8[6], w7[2], 2)                                        # a list that names a locus of another gene
    for ex, G, copies, low in ((6, 300, 4, True), (7, 300, 4, False), (8, 150, 8, False)):
        n = G * copies
        genomes = [k % G for k in range(n)]
        if low:                                                  # the second to fourth copies far below the first: the (3 G)-th largest rs is below 0.9
            c3 = [9999 - k if k < G else 5000 + 3 * G - k for k in range(n)]
        else:                                                    # every copy close to the first: it is above 0.9
            c3 = [9999 - k for k in range(n)]
        gene(ex, genomes, c3, c2=[900000 - 7 * k - ex for k in range(n)], base=30000 - 600 if ex == 8 else None)       # (ex 8 straddles the two members)
    gene(9, list(range(6)), [9000 + 10 * k for k in range(6)])
    one = gene(10, [4, 4], [9500, 9400])
    name(one[0], one[1], 0)
    e = gene(11, list(range(4)), [9500, 9490, 9480, 7000])
    x = gene(12, list(range(4)), [9400 - 3 * k for k in range(4)])
    n1 = gene(13, list(range(8)), [9300 - 3 * k for k in range(8)])
    n3 = gene(14, list(range(9)), [9200 - 3 * k for k in range(9)])
    n4 = gene(15, list(range(11)), [9100 - 3 * k for k in range(11)])
    at = 0
    for l, kind in [(l, 2) for l in e[:3]] + [(n1[1], 1), (n1[5], 2)] + [(l, 1) for l in n3[2:5]] + [(n3[7], 2)] + [(l, 1) for l in n4[1:5]]:
        name(hub[at % 12], l, kind)
        name(l, hub[at % 12], kind)
        at += 1
    del x
    priorities = {ex: [1 if ex >= 11 else 0, ex] for ex in tab}
    scores = {ex: float(sum(r[2] for r in t)) for ex, t in tab.items()}
    scores[1] = max(scores.values()) + 1000.                  # the hub first
    ortho_groups = [[11, 12, -1], [2, 3, 1]]
    return dict(tab=tab, lists=lists, priorities=priorities, scores=scores, ortho_groups=ortho_groups)


def write_stores(S, where):
    with PEP.MapBsn(os.path.join(where, 'g.tab.npz'), 'w') as store:
        for ex, t in S['tab'].items():
            store.save(ex, np.array(t, dtype=np.int64))
    members = sorted(set(r[5] // 30000 for t in S['tab'].values() for r in t))
    with PEP.MapBsn(os.path.join(where, 'g.conflicts.npz'), 'w') as store:
        for m in members:
            off, vals = [30001], []
            for idx in range(30000):
                vals += S['lists'].get(m * 30000 + idx, [])
                off.append(30001 + len(vals))
            store.save(m, np.array(off + vals, dtype=np.int64))
    with open(os.path.join(where, 'clust.fas'), 'w') as f:
        for ex in S['tab']:
            f.write('>%d\n%s\n' % (ex, 'ACGT' * (20 + ex)))


def rows_of(mat):
    return H.recorded(mat)


class RecordingPool(object):
    def __init__(self):
        self.loaded, self.run = [], []

    def imap_unordered(self, fn, items):
        items = list(items)
        if fn is PEP.load_conflict:
            self.loaded.append(sorted(int(i) for _, idss in items for ids in idss for i in ids[:, 0]))
        else:
            self.run.append([[int(d[0][0][0]), int(d[0].shape[0]), bool(d[1]), int(d[2])] for d in items])
        return map(fn, items)


def run_reference(S, orthology, where):
    rounds = []

    def local_trace(frame, event, arg):
        if event == 'line' and frame.f_lineno in LINES:
            L, point = frame.f_locals, LINES[frame.f_lineno]
            if point == 'start':
                rounds.append({})
            rec = dict(genes=[[int(g), float(s)] for g, s in L['genes'].items()], used=[[int(k), int(v)] for k, v in L['used'].items()],
                       new_groups={str(int(g)): rows_of(m) for g, m in L['new_groups'].items()})
            if point != 'start':
                rec['tmpSet'] = {str(int(g)): rows_of(m) for g, m in L['tmpSet'].items()}
            rounds[-1][point] = rec
        return local_trace

    def global_trace(frame, event, arg):
        return local_trace if frame.f_code is CODE else None

    pool = RecordingPool()
    PEP.pool2, PEP.mat_out, PEP.filt_per_group = pool, [], (lambda d: [d[0]])
    PEP.params = dict(clust=os.path.join(where, 'clust.fas'), clust_identity=CI, orthology=orthology, n_thread=2, map_bsn=os.path.join(where, 'g'))
    sys.settrace(global_trace)
    try:
        with PEP.MapBsn(os.path.join(where, 'g.tab.npz')) as groups:
            PEP.filt_genes(groups, np.array(S['ortho_groups']), 'unused.npy', os.path.join(where, 'g.conflicts.npz'), {k: list(v) for k, v in S['priorities'].items()},
                           dict(S['scores']), {'gene%d' % i: i for i in range(max(S['tab']) + 1)})
    finally:
        sys.settrace(None)
    mat_out = [[a, b, int(c), rows_of(m)] for a, b, c, m in PEP.mat_out[:-1]]
    assert PEP.mat_out[-1] == [0, 0, 0, []]
    return dict(rounds=rounds, mat_out=mat_out, loaded=pool.loaded, run=pool.run)


def main():
    S = scenario()
    for ex, t in S['tab'].items():
        assert len(set(r[2] for r in t)) == len(t) and len(set(r[3] for r in t)) == len(t), 'columns 2 and 3 are distinct within a group'
    out = dict(clust_identity=CI, tab={str(k): v for k, v in S['tab'].items()}, lists={str(k): v for k, v in S['lists'].items()},
               priorities={str(k): v for k, v in S['priorities'].items()}, scores={str(k): v for k, v in S['scores'].items()}, ortho_groups=S['ortho_groups'],
               clust_len={str(ex): 4 * (20 + ex) for ex in S['tab']}, runs={})
    seen = {}
    for orthology, mode in (('nj', H.NJ), ('sbh', H.SBH)):
        where = tempfile.mkdtemp(prefix='batchprep_')
        write_stores(S, where)
        rec = run_reference(S, orthology, where)
        out['runs'][orthology] = rec
        assert H.check_run(json.loads(json.dumps(out)), orthology, seen) == len(rec['rounds'])
        print(orthology, len(rec['rounds']), 'rounds,', len(rec['mat_out']), 'pan genes')
    missing = [b for b in H.BRANCHES if not seen.get(b)]
    assert not missing, missing
    print(sorted(seen.items()))
    path = os.path.join(HERE, 'g29_batchprep.json.gz')
    with gzip.GzipFile(path, 'wb', mtime=0) as f:
        f.write(json.dumps(out, separators=(',', ':')).encode())
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
