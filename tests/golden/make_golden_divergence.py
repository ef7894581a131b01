#!/usr/bin/env python3
"""Generate tests/golden/g20_divergence.json.gz by IMPORTING the reference's Python (build machine only: needs /root/reference).

    python tests/golden/make_golden_divergence.py

The same shim as make_golden_allele_diff.py.  Every case is a seeded gene group: base-5 packed rows written into a .seq store with the
reference's MapBsn, a genome id per row, `inparalog`, ref_len, a `global_differences` table saved with np.save, and the parameters self_id /
allowed_sigma.  PEP.filt_per_group itself (PEPPAN.py:326-484) runs on it with two spies:
    PEP.compare_seq wrapped          it is called exactly when the reference found the group divergent (:370);
    PEP.subprocess.Popen replaced    by a class that reads the FASTA file named in the command and raises: it is called exactly when the
                                     reference wants a tree, and the >X<row> names are the leaders (:393-415); after three failures the
                                     function returns [mat] (:419-421).
Only DATA is written - packed rows, genomes, inparalog, ref_len, the global_differences entries, the parameters and the three recorded facts
(divergent, tree_asked, leaders) - none of the reference's source text.  The restatement of tests/divergence_helpers.py classifies the
cases, and the conditions the fixture is pinned by are asserted at the end.
"""
import base64, gzip, json, os, stat, sys, tempfile

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
from divergence_helpers import clade, pack_codes, restate   # noqa: E402


class TreeAsked(Exception):
    pass


def reference_facts(case_id, packed, genomes, inparalog, ref_len, gd, self_id, allowed_sigma):
    """run PEP.filt_per_group on one case -> (divergent, tree_asked, leaders)"""
    n = len(packed)
    PEP.params = dict(self_id=self_id, allowed_sigma=allowed_sigma, clust_identity=0.9, orthology='nj', nj='spy {0}')
    seq_file, global_file = 'case%d.seq.npz' % case_id, 'case%d.global.npy' % case_id
    with PEP.MapBsn(seq_file, 'w') as store:
        member = np.empty(n, dtype=object)
        for k in range(n):
            member[k] = packed[k]
        store.save(7, member)
    table = np.empty((len(gd), 2), dtype=object)
    for k, (key, val) in enumerate(sorted(gd.items())):
        table[k, 0], table[k, 1] = key, val
    np.save(global_file, table, allow_pickle=True)
    mat = np.zeros((n, 7), dtype=np.int64)
    mat[:, 1] = genomes
    mat[:, 5] = 7000 + np.arange(n)
    seen = dict(divergent=False, fasta=[])
    real_compare, real_popen = PEP.compare_seq, PEP.subprocess.Popen

    def spy_compare(seqs, diff):
        seen['divergent'] = True
        return real_compare(seqs, diff)

    class SpyPopen(object):
        def __init__(self, cmd, *a, **k):
            with open(cmd[1]) as f:
                seen['fasta'].append([int(line[2:]) for line in f if line.startswith('>X')])
            raise TreeAsked()

    PEP.compare_seq, PEP.subprocess.Popen = spy_compare, SpyPopen
    try:
        res = PEP.filt_per_group([mat, inparalog, ref_len, seq_file, global_file])
    finally:
        PEP.compare_seq, PEP.subprocess.Popen = real_compare, real_popen
        os.unlink(seq_file)
        os.unlink(global_file)
    assert len(res) == 1 and res[0] is mat
    assert len(seen['fasta']) in (0, 3) and all(f == seen['fasta'][0] for f in seen['fasta'])
    return seen['divergent'], bool(seen['fasta']), sorted(seen['fasta'][0]) if seen['fasta'] else []


def all_pairs(genomes, val, drop=None, rng=None):
    ids = sorted(set(int(g) for g in genomes))
    gd = {(a, b): val for i, a in enumerate(ids) for b in ids[i + 1:]}
    if drop:
        for key in list(gd):
            if rng.random() < drop:
                del gd[key]
    return gd


# ---- the recipes: each -> (codes int[n, L], genomes, inparalog, global_differences)
def calm(rng, n, L):
    """one clade, hardly any difference, every genome pair known: not divergent"""
    codes = clade(rng, rng.integers(1, 5, L), n, 0.002, gap=0.03)
    genomes = rng.permutation(n) + 3
    return codes, genomes, bool(rng.integers(0, 2)), all_pairs(genomes, (0.05, 0.5), drop=0.3, rng=rng)


def band(rng, n, L, sigma):
    """one clade whose pairs lie between checkDiv's bound and the distances' bound (allowed_sigma > 1): divergent, mostly no pair beyond"""
    lo, hi = 0.02 * np.exp(0.5 * np.sqrt(sigma)), 0.02 * np.exp(0.5 * sigma)
    codes = clade(rng, rng.integers(1, 5, L), n, np.sqrt(lo * hi) / 2, gap=0.02)
    genomes = rng.permutation(n) + 1
    return codes, genomes, False, all_pairs(genomes, (0.02, 0.5))


def twins(rng, n, L, where, inparalog):
    """near-identical rows of genomes that know nothing of each other (never beyond), and two rows of ONE genome a few columns apart:
    where = 'edge': the first and the last row; 'inner': two middle rows (only an in-paralog sub-group sees them)"""
    anc = rng.integers(1, 5, L)
    codes = np.repeat(anc[None, :], n, axis=0)
    genomes = rng.permutation(n) + 10
    a, b = (0, n - 1) if where == 'edge' else (1, n - 2) if n > 3 else (0, 1)
    cols = rng.choice(L, size=6, replace=False)
    codes[b, cols] = codes[b, cols] % 4 + 1
    genomes[b] = genomes[a]
    return codes, genomes, inparalog, {}


def split(rng, n, L, dup):
    """two clades far apart: a tree is asked for.  dup: the edge rows are strangers to everybody, only same-genome rows across the clades
    (an in-paralog sub-group) make the group divergent"""
    a1 = rng.integers(1, 5, L)
    a2 = clade(rng, a1, 1, 0.25)[0]
    k = n // 2
    codes = np.concatenate([clade(rng, a1, k, 0.003, gap=0.02), clade(rng, a2, n - k, 0.003, gap=0.02)])
    genomes = rng.permutation(n) + 1
    if not dup:
        order = rng.permutation(n)
        return codes[order], genomes[order], bool(rng.integers(0, 2)), all_pairs(genomes, (0.02, 0.5), drop=0.2, rng=rng)
    # rows 0 and n - 1 stay of the first clade with genomes nobody has a bound with; rows 1 and k share a genome across the clades
    codes[n - 1] = clade(rng, a1, 1, 0.003, gap=0.02)[0]
    genomes[k] = genomes[1]
    return codes, genomes, True, {}


def main():
    rng = np.random.default_rng(20200)
    plans = []
    for n in (2, 3, 64, 65, 130):
        plans.append(('calm', n, 300, lambda n=n: calm(rng, n, 300)))
        plans.append(('calm', n, 1002, lambda n=n: calm(rng, n, 1002)))
        for sigma in (3, 5):
            plans.append(('band', n, 600 if n < 130 else 1002, lambda n=n, sigma=sigma: band(rng, n, 600 if n < 130 else 1002, sigma), sigma))
        plans.append(('twins-edge', n, 1002, lambda n=n: twins(rng, n, 1002, 'edge', False)))
        plans.append(('twins-edge-inparalog', n, 1002, lambda n=n: twins(rng, n, 1002, 'edge', True)))
        if n > 3:
            plans.append(('twins-inner-inparalog', n, 1002, lambda n=n: twins(rng, n, 1002, 'inner', True)))
            plans.append(('twins-inner-ignored', n, 1002, lambda n=n: twins(rng, n, 1002, 'inner', False)))
            plans.append(('split-dup', n, 300, lambda n=n: split(rng, n, 300, True)))
        plans.append(('split', n, 300, lambda n=n: split(rng, n, 300, False)))
        plans.append(('split', n, 150, lambda n=n: split(rng, n, 150, False)))
    for n in (6, 12, 17):
        plans.append(('band', n, 1002, lambda n=n: band(rng, n, 1002, 3), 3))
        plans.append(('band', n, 1002, lambda n=n: band(rng, n, 1002, 5), 5))
        plans.append(('twins-inner-inparalog', n, 1002, lambda n=n: twins(rng, n, 1002, 'inner', True)))
        plans.append(('twins-inner-ignored', n, 1002, lambda n=n: twins(rng, n, 1002, 'inner', False)))
        plans.append(('split-dup', n, 300, lambda n=n: split(rng, n, 300, True)))
    cases, classes = [], dict(calm=0, band=0, compatible=0, tree=0, sub_only=0, dup_ignored=0, missing=0)
    for k, plan in enumerate(plans):
        name, n, L, make = plan[:4]
        codes, genomes, inparalog, gd = make()
        sigma = plan[4] if len(plan) > 4 else (1, 3, 5)[k % 3]
        self_id = (0.002, 0.005)[k % 2]
        packed = pack_codes(codes, rng)
        divergent, tree_asked, leaders = reference_facts(k, packed, genomes, inparalog, L, gd, self_id, sigma)
        mine = restate(packed, L, genomes, inparalog, gd, self_id, sigma)
        assert mine['divergent'] == divergent, (name, n)
        assert not tree_asked or (mine['verdict'] == 2 and [g[0] for g in mine['groups']] == leaders), (name, n)
        kind = 'calm' if not divergent else 'band' if mine['verdict'] == 1 else 'tree' if tree_asked else 'compatible'
        classes[kind] += 1
        classes['sub_only'] += int(divergent and not mine['edge_divergent'])
        dups = len(set(genomes.tolist())) < n
        classes['dup_ignored'] += int(dups and not inparalog)
        ids = sorted(set(genomes.tolist()))
        classes['missing'] += int(any((a, b) not in gd for i, a in enumerate(ids) for b in ids[i + 1:]))
        cases.append(dict(name='%s_n%d_L%d_%d' % (name, n, L, k), n=n, ref_len=L, rows=base64.b64encode(packed.tobytes()).decode(), genomes=genomes.tolist(),
                          inparalog=bool(inparalog), global_differences=[[a, b, m, s] for (a, b), (m, s) in sorted(gd.items())], self_id=self_id,
                          allowed_sigma=sigma, divergent=bool(divergent), tree_asked=bool(tree_asked), leaders=leaders, kind=kind))
    print(classes)
    assert len(cases) >= 60
    assert min(classes[c] for c in ('calm', 'band', 'compatible', 'tree')) >= 8, classes
    assert classes['sub_only'] >= 5 and classes['dup_ignored'] >= 5 and classes['missing'] >= 5, classes
    assert {c['self_id'] for c in cases} == {0.002, 0.005} and {c['allowed_sigma'] for c in cases} == {1, 3, 5}
    assert {2, 3, 64, 65, 130} <= {c['n'] for c in cases}
    out = os.path.join(HERE, 'g20_divergence.json.gz')
    with gzip.GzipFile(out, 'wb', mtime=0) as f:
        f.write(json.dumps(dict(source='PEPPAN.py:326-421 (filt_per_group with compare_seq and subprocess.Popen spied on)', cases=cases), separators=(',', ':')).encode())
    print(out, os.path.getsize(out), 'bytes,', len(cases), 'cases')
    assert os.path.getsize(out) < 700 << 10


if __name__ == '__main__':
    main()
