#!/usr/bin/env python3
"""Generate tests/golden/g22_globaldiff.json.gz by IMPORTING the reference's Python (build machine only: needs /root/reference).

    python tests/golden/make_golden_globaldiff.py

The same shim as make_golden_ingroup.py.  Every case is a pair of tables (.clu.npy rows, .bsn.npy rows), a gene -> genome map and nGene; the
reference's get_gene_group makes the groups of them and its get_global_difference (PEPPAN.py:1611-1666) the recorded rows.  Only DATA is written - the
rows, the map, the groups, nGene, and the returned keys and floats (as float.hex() text, which reads back exactly) - none of the reference's source
text.  The restatement of tests/globaldiff_helpers.py classifies the keys, and the conditions the fixture is pinned by are asserted at the end.
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
import globaldiff_helpers as H           # noqa: E402


def random_families(seed, n_families=14, n_genomes=9):
    """families of 2 - 12 genes over genomes -1, 0, 1, ..: a rep with a self row and member rows; some genomes with several copies; bsn rows between
    reps and members, some with a value <= 0"""
    rng = np.random.default_rng(seed)
    genomes = [-1] + list(range(n_genomes - 1))
    genes, clu, bsn, reps, gene = {}, [], [], [], 100
    for f in range(n_families):
        size = int(rng.integers(2, 13))
        members = list(range(gene, gene + size))
        gene += size
        spread = rng.permutation(genomes)[:max(2, int(rng.integers(2, len(genomes))))]
        for k, g in enumerate(members):
            genes[g] = int(spread[k % len(spread)]) if rng.random() < 0.8 else int(rng.choice(spread))
        rep = members[0]
        reps.append(rep)
        clu.append([rep, rep, 10000])
        for g in members[1:]:
            clu.append([rep, g, int(rng.integers(9000, 10001))])
    all_genes = sorted(genes)
    for k in range(3 * n_families):
        r = int(rng.choice(reps))
        family = [g for g in all_genes if r <= g and not any(r < other <= g for other in reps)]
        q = int(rng.choice(all_genes if k % 7 == 0 else family))            # (a row in seven joins two families)
        bsn.append([r, q, int(rng.integers(-200, 9800)) if rng.random() < 0.25 else int(rng.integers(6000, 9900))])
    return genes, clu, bsn


def idle_bsn(genes):
    """the reference cannot index with an empty bsn table: one row between two genes of one genome, which no selected group holds"""
    genes[900001] = genes[900002] = 0
    return [[900001, 900002, 5000]]


def star(m=40):
    """one rep and m - 1 members, a genome each"""
    genes = {1000 + k: k for k in range(m)}
    clu = [[1000, 1000, 10000]] + [[1000, 1000 + k, 9990 - 37 * k] for k in range(1, m)]
    return genes, clu, idle_bsn(genes)


def chain():
    """rep 1 gathers 2 and 3, rep 4 takes 1 (popped as q), then 1 returns as r and starts from [1]; 5 absorbs itself twice"""
    genes = {1: 0, 2: 1, 3: 2, 4: 3, 5: 4, 6: 5, 7: 0, 8: 1}
    clu = [[1, 2, 9800], [1, 3, 9700], [4, 1, 9600], [1, 6, 9500], [5, 5, 10000], [5, 5, 9900], [5, 7, 9400], [1, 8, 9300]]
    return genes, clu, idle_bsn(genes)


def bsn_after_pop():
    """clu: 10 gathers 11, 12; 20 gathers 21.  bsn: (10, 20) pops 20's list, the next (10, 20) meets [20] alone; (10, 10) pops 10's own list, the next row of
    10 starts from [10]; rows between two genes of one genome (dropped) and rows with a value <= 0 (filtered)"""
    genes = {10: 0, 11: 1, 12: 2, 20: 3, 21: 0, 30: 1, 31: 1, 32: 4}
    clu = [[10, 10, 10000], [10, 11, 9900], [10, 12, 9850], [20, 20, 10000], [20, 21, 9700], [30, 31, 9650], [30, 32, 9640]]
    bsn = [[10, 20, 8800], [10, 20, 8700], [20, 10, 8600], [10, 30, 0], [10, 30, -5], [30, 11, 8500], [10, 10, 8400], [10, 21, 8300], [11, 31, 8200], [30, 31, 8100]]
    return genes, clu, bsn


def exact_counts():
    """group (1, 2) in genomes 10 and 11; bsn rows from gene 1 to single genes: 1, 5, 8, 60, 128 and 300 of them in genomes 20 .. 25"""
    genes, bsn, gene = {1: 10, 2: 11}, [], 100
    clu = [[1, 1, 10000], [1, 2, 9500]]
    for genome, count in ((20, 1), (21, 5), (22, 8), (23, 60), (24, 128), (25, 300)):
        for k in range(count):
            genes[gene] = genome
            bsn.append([1, gene, 9900 - 13 * k - genome])
            gene += 1
    return genes, clu, bsn


def ties():
    """seven groups of the same shape (two single-copy genomes, no further gene) and one better one: nGene = 3 cuts inside the tie, so the sha1 key decides"""
    genes, clu, gene = {}, [], 500
    for f in range(7):
        genes[gene], genes[gene + 1] = 2 * f, 2 * f + 1
        clu += [[gene, gene, 10000], [gene, gene + 1, 9000 + 100 * f]]
        gene += 2
    for k in range(3):
        genes[gene + k] = 20 + k
    clu += [[gene, gene, 10000], [gene, gene + 1, 9950], [gene, gene + 2, 9940]]
    return genes, clu, idle_bsn(genes)


def nothing():
    """no group with two single-copy genomes"""
    genes = {1: 0, 2: 0, 3: 1, 4: -1, 5: -1}
    return genes, [[1, 1, 10000], [1, 2, 9900], [3, 3, 10000], [4, 5, 9800]], [[1, 3, 500], [1, 3, -1]]


def big(seed):
    """one group: two single-copy genomes and 150 genes in each of two further genomes, in random order, as a star"""
    rng = np.random.default_rng(seed)
    genomes = [0, 1] + [2] * 150 + [3] * 150
    order = rng.permutation(len(genomes))
    genes = {7000 + k: genomes[int(o)] for k, o in enumerate(order)}
    clu = [[7000, 7000, 10000]] + [[7000, 7000 + k, int(rng.integers(8000, 10001))] for k in range(1, len(genomes))]
    return genes, clu, idle_bsn(genes)


def run_case(name, genes, clu, bsn, nGene):
    prefix = os.path.join(SHIM, 'cwd', name.replace(' ', '_'))
    np.save(prefix + '.npy', np.array(clu, dtype=np.int64).reshape(-1, 3))
    np.save(prefix + '.bsn.npy', np.array(bsn, dtype=np.int64).reshape(-1, 3))
    groups = PEP.get_gene_group(prefix + '.clu', prefix + '.bsn.npy')
    out = PEP.get_global_difference(groups, prefix + '.clu', prefix + '.bsn.npy', genes, nGene)
    rows = [[[int(k[0]), int(k[1])], float(v[0]).hex(), float(v[1]).hex()] for k, v in out.tolist()] if out.size else []
    return dict(name=name, nGene=nGene, clu=clu, bsn=bsn, genes=sorted(genes.items()), groups=[[int(g), [int(x) for x in m]] for g, m in groups.items()],
                shape=list(out.shape), rows=rows)


def last_bit_differs(case):
    """does some key's mean differ in its last bits both from a plain running sum and from one pairwise sum over the whole list"""
    c = dict(case, geneInGenomes=dict(case['genes']), geneGroups={np.int64(g): [np.int64(x) for x in m] for g, m in case['groups']})
    sel_clu, sel_bsn = H.select_rows(c['geneGroups'], c['clu'], c['bsn'], c['geneInGenomes'], c['nGene'])
    events, arena, _ = H.walk(sel_clu, sel_bsn, c['geneInGenomes'])
    table = H.log_table()
    for codes in H.items_by_key(events, arena).values():
        x = table[np.array(codes)]
        if len(x) > H.BUFFER:
            m, plain = H.numpy_sum(x) / len(x), np.float64(0.)
            for v in x:
                plain = plain + v
            if len({H.tail(s, 0.)[0] for s in (m, plain / len(x), H.pairwise(x) / len(x))}) == 3:         # (in the recorded number, exp of the mean)
                return True
    return False


def main():
    cases = [run_case('families %d' % s, *random_families(s), 1000) for s in (11, 12)]
    cases += [run_case('star', *star(), 1000), run_case('chain', *chain(), 1000), run_case('bsn after pop', *bsn_after_pop(), 1000),
              run_case('exact counts', *exact_counts(), 1000), run_case('ties', *ties(), 3), run_case('nothing', *nothing(), 1000)]
    for seed in range(100, 140):
        case = run_case('big', *big(seed), 1000)
        if last_bit_differs(case):
            print('big: seed %d' % seed)
            break
    else:
        raise SystemExit('no seed with a last-bit difference')
    cases.append(case)
    path = os.path.join(HERE, 'g22_globaldiff.json.gz')
    with gzip.GzipFile(path, 'wb', mtime=0) as f:
        f.write(json.dumps(dict(cases=cases), separators=(',', ':')).encode())
    # ---- what the fixture is pinned by
    loaded = H.load_cases()
    counts = []
    for c in loaded:
        rows, n = H.restated(c['geneGroups'], c['clu'], c['bsn'], c['geneInGenomes'], c['nGene'])
        assert H.same_rows([[k, v] for k, v in rows], c['rows']), c['name']
        assert c['shape'] == ((len(rows), 2) if rows else (0, 0)), (c['name'], c['shape'])
        counts += n
        print('%-14s %4d clu rows, %3d bsn rows, %3d keys, largest %d' % (c['name'], len(c['clu']), len(c['bsn']), len(rows), max(n) if n else 0))
    for lo, hi in ((1, 1), (2, 7), (8, 8), (9, 127), (128, 128), (129, 8192), (8193, 1 << 40), (16385, 1 << 40)):
        assert any(lo <= n <= hi for n in counts), (lo, hi)
    by_name = {c['name']: c for c in loaded}
    # (ties: the group of three genomes and two of the seven tied groups of two)
    assert by_name['nothing']['shape'] == (0, 0) and len({g for k, _ in by_name['ties']['rows'] for g in k}) == 3 + 2 * 2
    assert any(k[0] == -1 for c in loaded for k, _ in c['rows']) and all(len(c['rows']) >= 10 for c in loaded if c['name'].startswith('families'))
    assert any(v <= 0 for c in loaded for v in c['bsn'][:, 2]) and any(r == q for c in loaded for r, q, _ in c['clu'])
    print('%s: %d bytes, %d cases' % (path, os.path.getsize(path), len(cases)))


if __name__ == '__main__':
    main()
