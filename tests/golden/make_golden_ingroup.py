#!/usr/bin/env python3
"""Generate tests/golden/g21_ingroup.json.gz by IMPORTING the reference's Python (build machine only: needs /root/reference).

    python tests/golden/make_golden_ingroup.py

The same shim as make_golden_divergence.py.  Two kinds of cases, all seeded:
    determine       PEP.determineGroup (PEPPAN.py:1041-1056) on a gIden table (genome, identity, row number), a global_differences dict,
                    min_iden, nSigma and PEP.params['self_id'] -> the bool vector it returns;
    initializing    PEP.initializing2 (PEPPAN.py:1058-1076) on a .tab store written with the reference's MapBsn and a global_differences table
                    saved with np.save, once per parameter set -> per gene the kept table and the score.
Only DATA is written - the tables, the global_differences entries, the parameters and the recorded results - none of the reference's source
text.  The restatement of tests/ingroup_helpers.py classifies the cases, and the conditions the fixture is pinned by are asserted at the end.
"""
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
from ingroup_helpers import edge_variants, gd_object_array, restate, restate_gene, sort_keys   # noqa: E402

PARAMS = [(0.9, 3., 0.005), (0.9, 3., 0.005), (0.95, 2., 0.002), (0.9, 3, 0.005), (0.8, 1., 0.01)]      # (clust_identity, allowed_sigma, self_id); the defaults lead


def pair_table(rng, ids, centre, drop, spread=0.8):
    """bounds near `centre` for the pairs of `ids`, a share `drop` of them left to the default (which lets every row in)"""
    gd = {}
    for i, a in enumerate(ids):
        for b in ids[i + 1:]:
            if rng.random() >= drop:
                gd[(int(a), int(b))] = (round(float(centre * rng.uniform(0.8, 1.6)), 5), round(float(rng.uniform(0.1, spread)), 3))
    return gd


def mixed(rng, n, min_iden, lenient=False, at_threshold=False):
    """repeated genomes, seeds and non-seeds, bounds near 0.02 (lenient: the default for every pair)"""
    cut = int(round((min_iden - 0.02) * 10000))
    genome = rng.integers(0, min(max(2, n // 2), 30), n) + 5
    iden = np.where(rng.random(n) < 0.6, rng.integers(cut, 10001, n), rng.integers(cut - 1500, cut, n))
    iden[0] = 10000
    if at_threshold and n >= 4:
        iden[rng.choice(np.arange(1, n), 3, replace=False)] = (cut - 1, cut, cut + 1)
    gd = {} if lenient else pair_table(rng, sorted(set(genome.tolist())), 0.02, 0.25)
    return genome, iden, gd


def built(rng, n, which):
    """one of the constructed shapes of the GPU edge test (ingroup_helpers.edge_variants), with its own table"""
    from ingroup_helpers import EDGE_GD
    name, genome, iden = [v for v in edge_variants(n, rng) if v[0] == which][0]
    return genome, iden, dict(EDGE_GD)


def main():
    rng = np.random.default_rng(21000)
    plans = []
    for k in range(60):
        n = int(np.exp(rng.uniform(np.log(2), np.log(220))))
        plans.append(('mixed', PARAMS[k % len(PARAMS)], lambda n=n, k=k: mixed(rng, n, PARAMS[k % len(PARAMS)][0])))
    for n in (4, 9, 33, 70, 129, 200):
        plans.append(('threshold', PARAMS[0], lambda n=n: mixed(rng, n, 0.9, at_threshold=True)))
    for n in (6, 50):
        plans.append(('threshold', PARAMS[4], lambda n=n: mixed(rng, n, 0.8, at_threshold=True)))
    for n in (1, 2, 17, 64, 150):
        plans.append(('lenient', PARAMS[0], lambda n=n: mixed(rng, n, 0.9, lenient=True)))
    for which in ('first-out-later-in', 'first-in-later-out', 'seed-behind', 'panel-before'):
        for n in (3, 5, 40, 65, 130, 257, 300):
            plans.append((which, PARAMS[0], lambda n=n, which=which: built(rng, n, which)))
    determine, tally = [], dict(left_out=0, brought_in=0, up=0, down=0, same_genome=0, default=0, at_8800=0)
    for k, (name, (min_iden, sigma, self_id), make) in enumerate(plans):
        genome, iden, gd = make()
        n = len(genome)
        PEP.params = dict(self_id=self_id, allowed_sigma=sigma, clust_identity=min_iden)
        gIden = np.stack([genome, iden, np.arange(n)], axis=1).astype(np.int64)
        with np.errstate(all='ignore'):
            got = PEP.determineGroup(gIden.copy(), dict(gd), min_iden, sigma)
        mine = restate(genome, iden, gd, min_iden, sigma, self_id)
        assert got.dtype == bool and got.tolist() == mine['keep'], (name, n, k)
        for key in ('left_out', 'brought_in', 'up', 'down', 'same_genome', 'default'):
            tally[key] += int(mine[key])
        if min_iden == 0.9 and {8799, 8800, 8801} <= set(iden.tolist()):
            tally['at_8800'] += 1
        determine.append(dict(name='%s_n%d_%d' % (name, n, k), genome=genome.tolist(), iden=iden.tolist(),
                              global_differences=[[a, b, m, s] for (a, b), (m, s) in sorted(gd.items())], min_iden=min_iden, nSigma=sigma, self_id=self_id,
                              ingroup=[int(v) for v in got]))
    print(len(determine), 'determineGroup cases', tally)
    # (0.9 - 0.02) * 10000 is 8800.0 exactly in double arithmetic: a row at 8800 IS a seed, one at 8799 is not
    assert (0.9 - 0.02) * 10000 == 8800.0
    assert len(determine) >= 95
    assert tally['left_out'] * 4 >= len(determine) and tally['brought_in'] * 4 >= len(determine), tally
    assert min(tally[k] for k in ('up', 'down', 'same_genome', 'default')) >= 10 and tally['at_8800'] >= 3, tally

    # ---- initializing2 over a .tab store
    ids = list(range(3, 28))
    gd = pair_table(rng, ids, 0.02, 0.02, spread=0.4)
    np.save('global.npy', gd_object_array(gd), allow_pickle=True)
    sizes = [1, 1, 2, 2, 3, 3, 5, 5, 8, 8, 12, 12, 20, 20, 30, 30, 45, 45, 60, 60, 80, 80, 100, 100, 150, 150, 200, 260, 300, 7, 9, 11, 25, 40, 64, 65, 4, 6, 10, 16]
    tie_sizes = (4, 6, 10, 16)
    tables = {}
    for g, n in enumerate(sizes):
        gene = 100 + 7 * g
        while True:
            t = np.zeros((n, 7), dtype=np.int64)
            t[:, 0] = gene
            t[:, 1] = rng.choice(ids, n)
            t[:, 2] = rng.integers(300, 6000, n) * rng.choice([-1, 1], n)
            t[:, 3] = np.where(rng.random(n) < 0.6, rng.integers(8900, 10001, n), rng.integers(7400, 8900, n))
            t[:, 4] = t[:, 3]
            t[:, 5] = gene * 1000 + np.arange(n)
            t[:, 6] = rng.integers(0, 3, n)
            if n in tie_sizes:                         # two rows that differ in nothing the order, the group or the score can see
                t[1] = t[0]
                t[1, 5] += 1
                t[1, 6] = t[0, 6]
            keys = sort_keys(t.tolist())
            if len(set(keys)) == n - int(n in tie_sizes):
                break
        tables[gene] = t
    with PEP.MapBsn('genes.tab.npz', 'w') as store:
        for gene, t in tables.items():
            store.save(gene, t)
    genes = np.array(sorted(tables))
    runs = []
    for min_iden, sigma, self_id in (PARAMS[0], PARAMS[2]):
        PEP.params = dict(self_id=self_id, allowed_sigma=sigma, clust_identity=min_iden)
        with np.errstate(all='ignore'):
            out = PEP.initializing2(('genes', genes, 'global.npy'))
        assert [int(o[0]) for o in out] == genes.tolist()
        rec, cut = {}, 0
        for gene, kept, score in out:
            t = tables[int(gene)]
            tie = len(t) in tie_sizes
            if not tie:
                want_rows, want_score = restate_gene(t.tolist(), gd, min_iden, sigma, self_id)
                assert np.asarray(kept).tolist() == want_rows and int(score) == want_score, gene
            cut += int(len(kept) < len(t))
            rec[str(int(gene))] = dict(kept=np.asarray(kept).tolist(), score=int(score), tie=tie)
        assert cut >= 8, cut
        runs.append(dict(clust_identity=min_iden, allowed_sigma=sigma, self_id=self_id, genes=rec))
    init = dict(tables={str(g): t.tolist() for g, t in tables.items()}, global_differences=[[a, b, m, s] for (a, b), (m, s) in sorted(gd.items())], runs=runs)
    out = os.path.join(HERE, 'g21_ingroup.json.gz')
    with gzip.GzipFile(out, 'wb', mtime=0) as f:
        f.write(json.dumps(dict(source='PEPPAN.py:1041-1056 (determineGroup), 1058-1076 (initializing2)', determine=determine, initializing=init),
                           separators=(',', ':')).encode())
    print(out, os.path.getsize(out), 'bytes,', len(determine), 'determineGroup cases,', len(tables), 'genes x', len(runs), 'parameter sets')
    assert os.path.getsize(out) < 700 << 10


if __name__ == '__main__':
    main()
