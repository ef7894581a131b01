#!/usr/bin/env python3
"""Generate tests/golden/njtree_pd.json.gz and tests/golden/njtree_fa.json.gz by RUNNING the reference's bundled rapidnj (build machine only).

    python tests/golden/make_golden_njtree.py <directory of the reference checkout>

njtree_pd.json.gz: per case a distance matrix as its upper triangle with at most 6 decimals (Euclidean distances of seeded random points; one case of
-log distances as getDistance makes them) and the text `rapidnj -i pd` prints for it (PEPPAN_parser.py:168).  njtree_fa.json.gz: per case an alignment over
ACGT- (seeded: every row a mutated copy of a random earlier row, 1 - 20 % substitutions; 3 - 8 % of the columns hold gaps in some rows), the text
`rapidnj -i fa -t d` prints for it (PEPPAN.py:19, 409-417) and the upper triangle of the matrix `-o m` prints.  Sizes 2, 3, 4, 5, 8, 17, 33, 64, 65, 100.
Only DATA is written: inputs and what the binary printed.

rapidnj computes in float32.  A case in which the float64 restatement of tests/njtree_helpers.py finds another topology is a near-tie of two joins: its
seed is stepped until both agree, and the seed that was used is recorded with the case.  An alignment with a pair Kimura's distance is undefined for is
stepped over in the same way (rapidnj prints a fixed value there, which this project does not restate)."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from njtree_helpers import against_text, cgav_like, euclidean, kimura_counts      # noqa: E402
from peppan_amd.njtree import kimura_distances, parse_newick                                                        # noqa: E402

SIZES = (2, 3, 4, 5, 8, 17, 33, 64, 65, 100)
LETTERS = np.frombuffer(b'-ACGT', dtype=np.uint8)


def run(rapidnj, args, text, suffix):
    with tempfile.NamedTemporaryFile('w', suffix=suffix, delete=False) as f:
        f.write(text)
    try:
        return subprocess.run([rapidnj] + args + [f.name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, check=True).stdout
    finally:
        os.unlink(f.name)


def same_topology(text, matrix, names):
    try:
        against_text(text, matrix, names, parse_newick)
    except AssertionError:
        return False
    return True


def pd_case(rapidnj, n, seed, kind):
    while True:
        m = np.round(cgav_like(n, seed) if kind == 'cgav' else euclidean(n, seed), 6)
        names = ['G%d' % k for k in range(n)]
        text = '%d\n' % n + ''.join('%s %s\n' % (names[k], ' '.join('%.6f' % x for x in m[k])) for k in range(n))
        tree = run(rapidnj, ['-i', 'pd'], text, '.pd')
        if same_topology(tree, m, names):
            return {'n': n, 'seed': seed, 'kind': kind, 'names': names, 'upper': [float('%.6f' % x) for x in m[np.triu_indices(n, 1)]], 'newick': tree}
        seed += 1000


def alignment(n, seed, columns=300):
    rng = np.random.default_rng(seed)
    rows = [rng.integers(1, 5, columns)]
    for k in range(1, n):
        row = rows[int(rng.integers(0, k))].copy()
        hit = rng.random(columns) < rng.uniform(0.01, 0.20)
        row[hit] = (row[hit] - 1 + rng.integers(1, 4, int(hit.sum()))) % 4 + 1
        rows.append(row)
    codes = np.array(rows, dtype=np.uint8)
    gap_cols = np.flatnonzero(rng.random(columns) < rng.uniform(0.03, 0.08))
    for c in gap_cols:
        codes[rng.random(n) < 0.3, c] = 0
    return codes


def fa_case(rapidnj, n, seed):
    while True:
        codes = alignment(n, seed)
        names = ['X%d' % (3 * k) for k in range(n)]
        counts = kimura_counts(codes)
        d, undefined = kimura_distances(counts[:, 0], counts[:, 1], counts[:, 2])
        fasta = ''.join('>%s\n%s\n' % (name, LETTERS[row].tobytes().decode()) for name, row in zip(names, codes))
        if not undefined.any():
            tree = run(rapidnj, ['-i', 'fa', '-t', 'd'], fasta, '.fa')
            if same_topology(tree, d, names):
                lines = run(rapidnj, ['-i', 'fa', '-t', 'd', '-o', 'm'], fasta, '.fa').split('\n')[1:n + 1]
                printed = np.array([[float(x) for x in line.split('\t')[1].split()] for line in lines])
                assert [line.split('\t')[0] for line in lines] == names and printed.shape == (n, n)
                return {'n': n, 'seed': seed, 'names': names, 'rows': [LETTERS[row].tobytes().decode() for row in codes], 'newick': tree,
                        'matrix_upper': [float(x) for x in printed[np.triu_indices(n, 1)]]}
        seed += 1000


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rapidnj = os.path.join(sys.argv[1], 'dependencies', 'rapidnj')
    pd = [pd_case(rapidnj, n, 100 + n, 'euclidean') for n in SIZES] + [pd_case(rapidnj, 50, 150, 'cgav')]
    fa = [fa_case(rapidnj, n, 200 + n) for n in SIZES]
    for name, cases in (('njtree_pd.json.gz', pd), ('njtree_fa.json.gz', fa)):
        with open(os.path.join(HERE, name), 'wb') as raw, gzip.GzipFile(fileobj=raw, mode='wb', mtime=0) as f:
            f.write(json.dumps({'cases': cases}, separators=(',', ':')).encode())
        print(name, os.path.getsize(os.path.join(HERE, name)), 'bytes; seeds', [c['seed'] for c in cases])


if __name__ == '__main__':
    main()
