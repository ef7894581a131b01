"""K25 (the tree cutting of filt_per_group, csrc/treecut.hip) measured on one GPU, beside its numpy restatement on one thread of the same machine.

    python tools/treecut_rate.py <out.txt> [groups]

Inputs (seeded), the workload of profiles/njtree_rate.txt: 20 000 trees of 2 - 200 leaves, and one tree of 2 000 leaves.  Every tree is a random binary
tree over one to three clades; W0 lies beyond W1 between the clades and below it within them, so a tree of one clade needs no cut (the test of :438 ends
it) and the others need one or two; the share is printed.  Reported: HIP-event kernel times (pep_set_timing 2), the wall time of the library call
(Context.tree_cuts: checks, copies, kernels), the numpy restatement per tree over every 400th tree, and orthofilter.filt_per_groups as a whole over the
groups of tests/golden/g28_treecut.json.gz (a .seq store of 20 000 groups is not built here).  No threshold: a tool, not a test."""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
os.environ.setdefault('PEPPAN_LOG', '0')
import numpy as np                                                         # noqa: E402
import treecut_helpers as H                                                # noqa: E402

BIG, SAMPLE_EVERY = 2000, 400
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def make_tree(rng, n, k):
    clusters = H.split_evenly(n, min(k, n))
    sides, lengths = H.tree_of_clusters(rng, clusters, n)
    W0, W1 = H.dyadic_matrices(rng, clusters, n)
    return dict(sides=sides, lengths=lengths, W0=W0, W1=W1, strong=np.ones(n, bool), cap=3000)


def run(ctx, trees, path=0):
    t0 = time.perf_counter()
    res = ctx.tree_cuts([H.sets_of(t['sides']) for t in trees], [t['lengths'] for t in trees], [t['W0'] for t in trees], [t['W1'] for t in trees],
                        [t['strong'] for t in trees], 3000, path)
    return res, time.perf_counter() - t0


def main():
    out, groups = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 20000
    from peppan_amd import _native as N, orthofilter
    rng = np.random.default_rng(25)
    t0 = time.perf_counter()
    sizes = rng.integers(2, 201, groups)
    trees = [make_tree(rng, int(n), int(k)) for n, k in zip(sizes, rng.integers(1, 4, groups))]
    big = make_tree(rng, BIG, 3)
    say('# K25 on one MI355X, pep_set_timing 2; PEP_NJ_BLOCK_LEAVES %d, PEP_CUT_ROUND %d (inputs built in %.0f s)' % (N.NJ_BLOCK_LEAVES, N.CUT_ROUND, time.perf_counter() - t0))
    with N.Context(0) as ctx:
        ctx.set_timing(2)
        run(ctx, trees[:50])                                               # (the first call of a context allocates)
        sets_time = time.perf_counter()
        res, wall = run(ctx, trees)
        del sets_time
        cuts = np.array([r[2] for r in res])
        say('%d trees of 2 - 200 leaves: %d leaves, %.0f MB per matrix; %.1f %% need one or more cuts (%d cuts in all, %d ties)' % (
            groups, int(sizes.sum()), float((sizes.astype(np.int64) ** 2).sum()) * 8 / 1e6, 100. * (cuts > 0).mean(), int(cuts.sum()), sum(r[3] for r in res)))
        say('  Context.tree_cuts: HIP events preparation + one-workgroup kernel %.1f ms; wall %.3f s = %.1f us per tree (bit sets packed in numpy included)' % (
            ctx.call_times(N.CALL_TREE_CUT, total=True)[0][0], wall, wall / groups * 1e6))
        res_big, wall_big = run(ctx, [big])
        res_big, wall_big = run(ctx, [big])
        say('one tree of %d leaves (launch chain, %d cuts): HIP events %.1f ms; Context.tree_cuts wall %.1f ms (upload of %d MB included)' % (
            BIG, res_big[0][2], ctx.call_times(N.CALL_TREE_CUT, total=True)[0][1], wall_big * 1e3, 2 * BIG * BIG * 8 // 1000000))
    sample = list(range(0, groups, SAMPLE_EVERY))
    t0 = time.perf_counter()
    for k in sample:
        want = H.cut_restated(**trees[k])
        assert H.same_result(res[k], want) is None, k
    spent = time.perf_counter() - t0
    say('the numpy restatement, one thread of the same machine, every %dth tree (%d of them, each equal to the device bit for bit): %.2f s = %.1f ms per tree; '
        'EXTRAPOLATED to all %d: %.0f s' % (SAMPLE_EVERY, len(sample), spent, spent / len(sample) * 1e3, groups, spent / len(sample) * groups))
    t0 = time.perf_counter()
    want = H.cut_restated(**big)
    say('the numpy restatement of the %d-leaf tree: %.1f s (equal to the device: %s)' % (BIG, time.perf_counter() - t0, H.same_result(res_big[0], want) is None))
    golden = H.load_golden()
    with tempfile.TemporaryDirectory() as folder:
        store, to_run, gds, params = H.golden_store(golden, folder)
        by = H.golden_by_params(golden)
        for key, idx in by.items():
            orthofilter.filt_per_groups(store, [to_run[k] for k in idx], gds[key], params[key])
        t0 = time.perf_counter()
        for key, idx in by.items():
            orthofilter.filt_per_groups(store, [to_run[k] for k in idx], gds[key], params[key])
        say('orthofilter.filt_per_groups (verdicts, trees, cuts) over the %d groups of the golden fixture, %d rows, in %d calls: %.1f ms' % (
            len(to_run), sum(len(t[0]) for t in to_run), len(by), (time.perf_counter() - t0) * 1e3))
        orthofilter.close()
    with open(out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
