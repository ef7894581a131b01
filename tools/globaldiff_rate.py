"""K22 (genome-pair identity statistics, csrc/globaldiff.hip) measured on one GPU, beside the reference's own get_global_difference on one CPU thread.

    python tools/globaldiff_rate.py reference <out.txt>                     the reference's function (no GPU; needs the reference checkout that
                                                                             tests/golden/make_golden_globaldiff.py imports) on a sample small enough to finish
    python tools/globaldiff_rate.py gpu <out.txt> [reference times.txt]     K22's times on one MI355X (pep_set_timing 2); the reference's lines, when
                                                                             given, are copied in below them (profiles/globaldiff_rate.txt)

Inputs (seeded): `groups` star clusters of single-copy genes over G genomes - a rep with its self row and G - 1 members, one gene per genome, identities
9000 .. 10000 - and one bsn row per group.  Such a group emits (G + 1) (G + 2) / 2 items, so 1 000 groups come to 1.26e8 items at G = 500 and 2.0e9 at
G = 2 000, which is within the item limit of one call (2^32).  The reference's sample is 20 groups at G = 200.
Reported: HIP-event kernel times, the wall time of the library call (Context.global_diff: checks, uploads, kernels, read-back) and of the whole
globaldiff.get_global_difference (selection, files, walk, K22, tail).  No threshold: a tool, not a test."""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
os.environ.setdefault('PEPPAN_LOG', '0')
import numpy as np                                                         # noqa: E402

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def stars(groups, G, seed=22):
    """-> (geneGroups with numpy int64 keys, clu int64[groups * G, 3], bsn int64[groups, 3], geneInGenomes)"""
    rng = np.random.default_rng(seed)
    genes = np.arange(groups * G, dtype=np.int64).reshape(groups, G)
    clu = np.stack([np.repeat(genes[:, :1], G, axis=1), genes, rng.integers(9000, 10001, (groups, G))], axis=-1).reshape(-1, 3)
    clu[::G, 2] = 10000
    bsn = np.stack([genes[:, 0], genes[:, G - 1], rng.integers(6000, 9000, groups)], axis=-1)
    genome = np.tile(np.arange(G), groups)
    geneInGenomes = dict(zip(genes.reshape(-1).tolist(), genome.tolist()))
    geneGroups = {np.int64(row[0]): [np.int64(g) for g in row] for row in genes}
    return geneGroups, clu, bsn, geneInGenomes


def write_tables(folder, clu, bsn):
    np.save(os.path.join(folder, 'rate.npy'), clu)
    np.save(os.path.join(folder, 'rate.bsn.npy'), bsn)
    return os.path.join(folder, 'rate.clu'), os.path.join(folder, 'rate.bsn.npy')


def reference(out_path):
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    here = os.getcwd()
    import make_golden_globaldiff as M                                     # (builds the shim and imports the reference's PEPPAN)
    os.chdir(here)
    groups, G = 20, 200
    geneGroups, clu, bsn, geneInGenomes = stars(groups, G)
    with tempfile.TemporaryDirectory() as tmp:
        clu_file, bsn_file = write_tables(tmp, clu, bsn)
        t0 = time.perf_counter()
        out = M.PEP.get_global_difference(geneGroups, clu_file, bsn_file, geneInGenomes, 1000)
        took = time.perf_counter() - t0
    items = groups * ((G + 1) * (G + 2) // 2)
    say('# the reference\'s get_global_difference on one CPU thread (%d CPUs in the machine), numpy %s' % (os.cpu_count(), np.__version__))
    say('%d groups at G = %d: %d items, %d keys: %.2f s = %.2f us per item' % (groups, G, items, len(out), took, 1e6 * took / items))
    for n_groups, genomes in ((1000, 500), (1000, 2000)):
        n = n_groups * ((genomes + 1) * (genomes + 2) // 2)
        say('EXTRAPOLATED by the item count to %d groups at G = %d (%.3g items): %.0f s; not measured' % (n_groups, genomes, n, took / items * n))
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def gpu(out_path, reference_path):
    from peppan_amd import _native as N, globaldiff as GD, orthofilter as OF
    with N.Context(0) as ctx:
        ctx.set_timing(2)
        OF._CONTEXTS[(os.getpid(), 0)] = ctx                                             # globaldiff's calls go through this context
        say('# K22 on one MI355X, pep_set_timing 2; chunks of %d items; the item limit of one call is %d, so G = 2000 (%.3g items) fits and is measured as asked'
            % (N.GDIFF_CHUNK_ITEMS, N.GDIFF_MAX_ITEMS, 1000 * (2001 * 2002 // 2)))
        table = GD.log_table()
        ctx.global_diff([[0, 2, 0, 2, 5, 0]], [0, 1], 2, table)                          # warm-up: the kernels are loaded
        for groups, G in ((20, 200), (1000, 500), (1000, 2000)):
            geneGroups, clu, bsn, geneInGenomes = stars(groups, G)
            genes = np.arange(groups * G, dtype=np.int64)
            t0 = time.perf_counter()
            events, arena, genomes = N.global_diff_walk(clu, bsn, genes, np.tile(np.arange(G), groups))
            walk = time.perf_counter() - t0
            items = int((events[:, 1] * events[:, 3]).sum())
            t0 = time.perf_counter()
            g1, g2, n, mean, var = ctx.global_diff(events, arena, len(genomes), table)
            wall = time.perf_counter() - t0
            ms = ctx.call_times(N.CALL_GLOBAL_DIFF, total=True)[0]
            say('%d groups at G = %d: %d rows, %d items, %d keys, largest %d' % (groups, G, len(events), items, len(n), int(n.max())))
            say('  host walk (pep_global_diff_walk, %d arena entries): %.3f s' % (len(arena), walk))
            say('  Context.global_diff: HIP events counting %.1f ms + chunks %.1f ms + sums %.1f ms = %.1f ms (%.2f ns per item); wall %.3f s'
                % (ms[0], ms[1], ms[2], sum(ms), 1e6 * sum(ms) / items, wall))
            with tempfile.TemporaryDirectory() as tmp:
                clu_file, bsn_file = write_tables(tmp, clu, bsn)
                t0 = time.perf_counter()
                out = GD.get_global_difference(geneGroups, clu_file, bsn_file, geneInGenomes, 1000)
                whole = time.perf_counter() - t0
            assert len(out) == len(n)
            say('  globaldiff.get_global_difference (selection, files, walk, K22, tail): %.3f s = %.2f ns per item' % (whole, 1e9 * whole / items))
            del events, arena, out
        OF._CONTEXTS.pop((os.getpid(), 0))
    if reference_path:
        with open(reference_path) as f:
            lines.extend(f.read().rstrip('\n').split('\n'))
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    if len(sys.argv) >= 3 and sys.argv[1] == 'reference':
        reference(sys.argv[2])
    elif len(sys.argv) >= 3 and sys.argv[1] == 'gpu':
        gpu(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        sys.exit(__doc__)
