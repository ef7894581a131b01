"""K21 (neighbour-joining trees, csrc/njtree.hip) measured on one GPU, beside the reference's bundled rapidnj on the CPU of a machine that has it.

    python tools/njtree_rate.py reference <reference checkout> <out.txt>     rapidnj's times (no GPU): the 2 000-leaf matrix, a sample of the small
                                                                             alignments, the cost of one Popen of the binary
    python tools/njtree_rate.py gpu <out.txt> [reference times.txt]          K21's times on one MI355X (pep_set_timing 2); the reference's lines,
                                                                             when given, are copied in below them (profiles/njtree_rate.txt)

Inputs, the same in both modes (seeded): one CGAV-like -log matrix of 2 000 leaves (PEPPAN_parser.py:168), and 20 000 alignments of 2 - 200 rows x 300
columns over ACGT-, every row a copy of a root with 2 - 10 % substitutions and 1 % gaps (the tags of PEPPAN.py:393-398, one tree per group, :409-417).
Reported: HIP-event kernel times, the wall time of the library calls (Context.kimura_pairs, Context.nj_trees: checks, copies, kernels) and of
njtree.trees_of_rows - gene_trees behind its read of the .seq store: counts, logarithms on the host, trees, text.  No threshold: a tool, not a test."""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
os.environ.setdefault('PEPPAN_LOG', '0')
import numpy as np                                                         # noqa: E402
import njtree_helpers as H                                                 # noqa: E402

BIG, GROUPS, COLUMNS, SAMPLE_EVERY = 2000, 20000, 300, 40
LETTERS = np.frombuffer(b'-ACGT', dtype=np.uint8)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def big_matrix(genes=1000):
    """-log((shared + 0.5) / (presence + 1)) of BIG allelic profiles of a few lineages, as getDistance makes it (H.cgav_like, counted in slabs of rows)"""
    rng = np.random.default_rng(21)
    founders = rng.integers(1, 6, (8, genes))
    prof = founders[rng.integers(0, 8, BIG)].copy()
    change = rng.random((BIG, genes)) < 0.15
    prof[change] = rng.integers(0, 9, int(change.sum()))
    d = np.zeros((BIG, BIG))
    for a in range(0, BIG, 50):
        slab = prof[a:a + 50, None, :]
        shared = ((slab == prof[None, :, :]) & (slab > 0)).sum(-1)
        presence = ((slab > 0) & (prof[None, :, :] > 0)).sum(-1)
        d[a:a + 50] = -np.log((shared + 0.5) / (presence + 1.))
    np.fill_diagonal(d, 0.)
    return d


def alignments():
    """-> list of uint8[n, COLUMNS] codes 0..4"""
    rng = np.random.default_rng(22)
    out = []
    for n in rng.integers(2, 201, GROUPS):
        codes = np.repeat(rng.integers(1, 5, COLUMNS)[None, :], int(n), axis=0).astype(np.uint8)
        hit = rng.random(codes.shape) < rng.uniform(0.02, 0.10)
        codes[hit] = (codes[hit] - 1 + rng.integers(1, 4, int(hit.sum()))) % 4 + 1
        codes[rng.random(codes.shape) < 0.01] = 0
        out.append(codes)
    return out


def reference(ref_dir, out_path):
    rapidnj = os.path.join(ref_dir, 'dependencies', 'rapidnj')
    tmp = tempfile.mkdtemp(prefix='njtree_rate_')

    def timed(args, text, name, repeat=1):
        path = os.path.join(tmp, name)
        with open(path, 'w') as f:
            f.write(text)
        best = []
        for _ in range(repeat):
            t0 = time.perf_counter()
            p = subprocess.Popen([rapidnj] + args + [path], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
            p.communicate()
            best.append(time.perf_counter() - t0)
        os.unlink(path)
        return float(np.median(best))

    say('# the reference\'s bundled rapidnj on the CPU machine that has it (%d CPUs), Popen + communicate as PEPPAN.py:416 does it' % os.cpu_count())
    spawn = timed(['-i', 'pd'], '2\nA 0 0.3\nB 0.3 0\n', 'two.pd', repeat=21)
    say('one Popen of rapidnj on a 2-leaf matrix (the per-spawn cost): median of 21: %.2f ms' % (1e3 * spawn))
    m = big_matrix()
    text = '%d\n' % BIG + ''.join('G%d %s\n' % (k, ' '.join('%.6f' % x for x in row)) for k, row in enumerate(m))
    say('rapidnj -i pd on the %d-leaf matrix (reading its %.0f MB of text included): median of 3: %.3f s' % (BIG, len(text) / 1e6, timed(['-i', 'pd'], text, 'big.pd', repeat=3)))
    groups = alignments()[::SAMPLE_EVERY]
    t0 = time.perf_counter()
    for k, codes in enumerate(groups):
        timed(['-i', 'fa', '-t', 'd'], ''.join('>X%d\n%s\n' % (r, LETTERS[row].tobytes().decode()) for r, row in enumerate(codes)), 'g.fa')
    took = time.perf_counter() - t0
    say('rapidnj -i fa -t d, one spawn per alignment, every %dth of the %d alignments (%d of them, temporary file written as :411-414 do): %.2f s = %.2f ms per tree; '
        'EXTRAPOLATED to all %d: %.0f s on one core' % (SAMPLE_EVERY, GROUPS, len(groups), took, 1e3 * took / len(groups), GROUPS, took * SAMPLE_EVERY))
    os.rmdir(tmp)
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def gpu(out_path, reference_path):
    from peppan_amd import _native as N, njtree as NJ, orthofilter as OF
    with N.Context(0) as ctx:
        ctx.set_timing(2)
        OF._CONTEXTS[(os.getpid(), 0)] = ctx                                             # njtree's calls go through this context
        say('# K21 on one MI355X, pep_set_timing 2; PEP_NJ_BLOCK_LEAVES %d' % N.NJ_BLOCK_LEAVES)
        m = big_matrix()
        ctx.nj_trees([H.euclidean(300, 1)])                                              # warm-up: the chain's kernels are loaded
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            (node, length), = ctx.nj_trees([m])
            walls.append(time.perf_counter() - t0)
        say('one matrix of %d leaves (launch chain, %d launches): HIP events %.1f ms; Context.nj_trees wall, median of 3: %.1f ms (upload of %.0f MB included)'
            % (BIG, 2 * (BIG - 3) + 3, ctx.call_times(N.CALL_NJ_TREES, total=True)[0][1], 1e3 * float(np.median(walls)), m.nbytes / 1e6))
        groups = alignments()
        packed = [H.pack_codes(c) for c in groups]
        n = np.array([len(c) for c in groups])
        rows = np.concatenate([p.reshape(-1) for p in packed])
        row_off = np.arange(int(n.sum()) + 1, dtype=np.uint64) * np.uint64(packed[0].shape[1])
        row_len = np.full(int(n.sum()), COLUMNS, np.uint32)
        starts = np.concatenate([[0], np.cumsum(n)])
        index = [np.arange(a, b, dtype=np.uint32) for a, b in zip(starts[:-1], starts[1:])]
        pairs = int((n * (n - 1) // 2).sum())
        say('%d alignments of 2 - 200 rows x %d columns: %d rows, %d pairs, %.0f MB of matrices' % (GROUPS, COLUMNS, n.sum(), pairs, 8e-6 * float((n * n).sum())))
        ctx.kimura_pairs(rows, row_off, row_len, index[:50])
        t0 = time.perf_counter()
        counts = ctx.kimura_pairs(rows, row_off, row_len, index)
        wall = time.perf_counter() - t0
        say('  Context.kimura_pairs: HIP events bit planes %.2f ms + pairs %.2f ms; wall %.3f s (%.0f MB of counts to the host)' % (tuple(ctx.call_times(N.CALL_KIMURA_PAIRS, total=True)[0][:2]) + (wall, 12e-6 * pairs)))
        dist = [NJ.kimura_distances(c[:, 0], c[:, 1], c[:, 2])[0] for c in counts]
        t0 = time.perf_counter()
        trees = ctx.nj_trees(dist)
        wall = time.perf_counter() - t0
        say('  Context.nj_trees: HIP events one-workgroup kernels %.1f ms; wall %.3f s = %.1f us per tree' % (ctx.call_times(N.CALL_NJ_TREES, total=True)[0][0], wall, 1e6 * wall / GROUPS))
        del counts, dist, trees
        names = [['X%d' % k for k in range(int(k))] for k in n]
        t0 = time.perf_counter()
        texts = NJ.trees_of_rows(rows, row_off, row_len, index, names)
        wall = time.perf_counter() - t0
        say('  njtree.trees_of_rows (gene_trees behind its read of the .seq store: counts, logarithms, trees, text): %.3f s = %.1f us per tree; %d groups without a tree'
            % (wall, 1e6 * wall / GROUPS, sum(t is None for t in texts)))
        OF._CONTEXTS.pop((os.getpid(), 0))
    if reference_path:
        with open(reference_path) as f:
            lines.extend(f.read().rstrip('\n').split('\n'))
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    if len(sys.argv) >= 4 and sys.argv[1] == 'reference':
        reference(sys.argv[2], sys.argv[3])
    elif len(sys.argv) >= 3 and sys.argv[1] == 'gpu':
        gpu(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        sys.exit(__doc__)
