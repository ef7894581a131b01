"""K26 (the front half of a round of filt_genes, csrc/batchprep.hip) measured on one GPU, beside its plain-Python restatement on one thread of the same machine.

    python tools/batchprep_rate.py <out.txt> [commit] [genes] [genomes]

Inputs (seeded): one round of 500 genes over 2 000 genomes; two thirds of the genes have one row per genome, one third 2 - 4 copies per genome.  A tenth of
the copies name another copy of their genome in the same table (kind 0, both ways), one row in a hundred a locus of the next gene (kind 2); `used` holds
one locus in twenty, half of them with a value <= 0.  The tables go into a .tab store and the lists into a .conflicts store of 30 000 loci per member.
Reported: HIP-event kernel times of stages A and C (pep_set_timing 2), the wall time of the three library calls (checks, copies, kernels), of
paralogfilter.prepare_batch as a whole (stores read, layout, A, B, C, the matrices gathered), and of the plain-Python restatement (tests/batchprep_helpers.py)
per row over every 25th gene, extrapolated.  No threshold: a tool, not a test."""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
os.environ.setdefault('PEPPAN_LOG', '0')
import numpy as np                                                         # noqa: E402
import batchprep_helpers as H                                              # noqa: E402

SAMPLE_EVERY, CI = 25, 0.9
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def make_round(rng, n_genes, n_genomes):
    """-> (tables: list of int64[n, 7], lists: locus -> list of values, used: locus -> value)"""
    tables, lists, locus0 = [], {}, 0
    for g in range(n_genes):
        copies = int(rng.integers(2, 5)) if g % 3 == 2 else 1
        n = n_genomes * copies
        t = np.zeros((n, 7), np.int64)
        t[:, 0], t[:, 1] = g + 1, np.tile(np.arange(n_genomes), copies)
        t[:, 2] = rng.permutation(n) * 3 + 50000
        t[:, 3] = 9999 - rng.permutation(n) % 3000 - np.repeat(np.arange(copies), n_genomes) * 400
        t[:, 4], t[:, 5], t[:, 6] = t[:, 3], locus0 + rng.permutation(n), 1
        if copies > 1:
            for r in np.flatnonzero(rng.random(n) < 0.1).tolist():
                other = (r + n_genomes) % n
                lists.setdefault(int(t[r, 5]), []).append(int(t[other, 5]) * 10)
                lists.setdefault(int(t[other, 5]), []).append(int(t[r, 5]) * 10)
        for r in np.flatnonzero(rng.random(n) < 0.01).tolist():
            lists.setdefault(int(t[r, 5]), []).append((locus0 + n + int(rng.integers(0, n_genomes))) * 10 + 2)
        tables.append(t)
        locus0 += n
    loci = rng.choice(locus0, locus0 // 20, replace=False)
    used = {int(l): (0 if k % 2 else 7000 + 1000) for k, l in enumerate(loci.tolist())}
    return tables, lists, used, locus0


def write_stores(folder, tables, lists, n_loci):
    from peppan_amd.mapbsn import MapBsn
    with MapBsn(os.path.join(folder, 'r.tab.npz'), 'w') as store:
        for t in tables:
            store.save(int(t[0, 0]), t)
    with MapBsn(os.path.join(folder, 'r.conflicts.npz'), 'w') as store:
        for m in range(n_loci // 30000 + 2):
            off, vals = [30001], []
            for idx in range(30000):
                vals += lists.get(m * 30000 + idx, [])
                off.append(30001 + len(vals))
            store.save(m, np.array(off + vals, dtype=np.int64))


def main():
    out = sys.argv[1]
    commit = sys.argv[2] if len(sys.argv) > 2 else 'unknown'
    n_genes, n_genomes = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else (500, 2000)
    from peppan_amd import _native as N, paralogfilter
    rng = np.random.default_rng(26)
    t0 = time.perf_counter()
    tables, lists, used, n_loci = make_round(rng, n_genes, n_genomes)
    n_rows = sum(len(t) for t in tables)
    n_loci += n_genomes                                                    # (the last gene's lists name loci behind it)
    say('# K26 on one MI355X, pep_set_timing 2, the working tree on commit %s; PEP_PREP_LDS_ROWS %d (inputs built in %.0f s)' % (commit, N.PREP_LDS_ROWS, time.perf_counter() - t0))
    say('%d genes x %d genomes: %d rows (%d genes of one row per genome, %d of 2 - 4), %d conflict values in %d lists, %d loci in `used`' % (
        n_genes, n_genomes, n_rows, sum(1 for t in tables if len(t) == n_genomes), sum(1 for t in tables if len(t) > n_genomes), sum(len(v) for v in lists.values()), len(lists), len(used)))
    M = np.concatenate(tables)
    gene_off = np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.uint64)
    state = paralogfilter._used_state(used, n_loci)
    lens = np.array([len(lists.get(l, ())) for l in M[:, 5].tolist()], np.int64)
    flat = np.array([v for l in M[:, 5].tolist() for v in lists.get(l, ())], np.int64)
    with N.Context(0) as ctx:
        ctx.set_timing(2)
        ctx.batch_screen(gene_off, M[:, 3], M[:, 5], state, (CI - 0.02) * 10000)                      # (the first call of a context allocates)
        t0 = time.perf_counter()
        out3, out4, present, excluded = ctx.batch_screen(gene_off, M[:, 3], M[:, 5], state, (CI - 0.02) * 10000)
        wall_a, ms_a = time.perf_counter() - t0, ctx.call_times(N.CALL_BATCH_SCREEN, total=True)[0][0]
        M[:, 3], M[:, 4] = out3, out4
        keep = M[:, 3] != 0
        owner = np.repeat(np.arange(n_genes), np.diff(gene_off.astype(np.int64)))
        A, a_off = M[keep], np.concatenate([[0], np.cumsum(np.bincount(owner[keep], minlength=n_genes))]).astype(np.uint64)
        a_lens = lens[keep]
        start = np.concatenate([[0], np.cumsum(lens)])[:-1][keep]
        cfl_off, cfl = paralogfilter._csr(flat, start, a_lens)
        t0 = time.perf_counter()
        col3, popped = N.batch_unsure_walk(a_off, A[:, 3], A[:, 5], cfl_off, cfl, n_loci)
        wall_b = time.perf_counter() - t0
        A[:, 3] = col3
        keep = A[:, 3] > 0
        a_owner = np.repeat(np.arange(n_genes), np.diff(a_off.astype(np.int64)))
        Cm, c_off = A[keep], np.concatenate([[0], np.cumsum(np.bincount(a_owner[keep], minlength=n_genes))]).astype(np.uint64)
        cfl_off, cfl = paralogfilter._csr(flat, start[keep], a_lens[keep])
        res = {}
        for name, path in (('auto', N.PREP_AUTO), ('workspace', N.PREP_WS)):
            ctx.batch_prune(N.PREP_NJ, c_off, Cm[:, 1], Cm[:, 2], Cm[:, 3], Cm[:, 4], Cm[:, 5], cfl_off, cfl, n_loci, CI, 10000 * CI, path)
            t0 = time.perf_counter()
            res[name] = ctx.batch_prune(N.PREP_NJ, c_off, Cm[:, 1], Cm[:, 2], Cm[:, 3], Cm[:, 4], Cm[:, 5], cfl_off, cfl, n_loci, CI, 10000 * CI, path)
            res[name + '_time'] = (time.perf_counter() - t0, ctx.call_times(N.CALL_BATCH_PRUNE, total=True)[0][0])
        assert all(np.array_equal(a, b) for a, b in zip(res['auto'][:4], res['workspace'][:4]))
    out_off, rows, inparalog, final, n_ties = res['auto']
    say('stage A, Context.batch_screen: HIP events %.2f ms; wall %.1f ms; %d genes excluded' % (ms_a, wall_a * 1e3, int(excluded.sum())))
    say('stage B, pep_batch_unsure_walk (host C++, one thread): wall %.1f ms; %d genes popped' % (wall_b * 1e3, int(popped.sum())))
    say('stage C, Context.batch_prune over %d rows: HIP events %.2f ms (genes up to %d rows in LDS) / %.2f ms (every gene in the workspace, identical output); wall %.1f ms; '
        '%d rows left, %d genes final, %d to_run, %d ties' % (len(Cm), res['auto_time'][1], N.PREP_LDS_ROWS, res['workspace_time'][1], res['auto_time'][0] * 1e3, len(rows),
                                                            int(final.sum()), n_genes - int(final.sum()), n_ties))
    with tempfile.TemporaryDirectory() as folder:
        t0 = time.perf_counter()
        write_stores(folder, tables, lists, n_loci)
        say('(stores written in %.0f s)' % (time.perf_counter() - t0))
        genes = [((g + 1) * 1000, float(n_genes - g)) for g in range(n_genes)]
        params = dict(clust_identity=CI, orthology='nj')
        for _ in range(2):
            t0 = time.perf_counter()
            got = paralogfilter.prepare_batch(os.path.join(folder, 'r.tab.npz'), os.path.join(folder, 'r.conflicts.npz'), genes, used, {}, params)
            wall = time.perf_counter() - t0
        paralogfilter.close()
    say('paralogfilter.prepare_batch as a whole (the stores read and inflated, layout, A, B, C, the matrices gathered), second call: %.2f s = %.2f us per row' % (wall, wall / n_rows * 1e6))
    # the restatement on a sample: stage A and C per gene (stage B is sequential over the round: the sample takes the popped flags as given)
    sample = list(range(0, n_genes, SAMPLE_EVERY))
    t0 = time.perf_counter()
    threshold, sample_rows, equal = (CI - 0.02) * 10000, 0, True
    for g in sample:
        table = tables[g].tolist()
        sample_rows += len(table)
        mine, _, ex = H.screen(table, used, threshold)
        mine = [r for r in mine if r[3] != 0]
        gene = (g + 1) * 1000
        if ex:
            equal = equal and got.status[gene] == 'excluded'
            continue
        cfl_g = {r[5]: lists[r[5]] for r in mine if r[5] in lists}
        popped_g = H.unsure_walk([0], {0: mine}, {0: cfl_g})                # (this gene alone: what the round's used2 adds is not in the sample)
        if got.status[gene] == 'popped' or popped_g:
            continue
        mine = [r for r in mine if r[3] > 0]
        rows_g, inpar_g, final_g, _ = H.prune(mine, cfl_g, H.NJ, CI, 10000 * CI)
        equal = equal and got.mats[gene].tolist() == [mine[i] for i in rows_g] and got.status[gene] == ('final' if final_g else 'to_run')
    spent = time.perf_counter() - t0
    say('the plain-Python restatement, one thread of the same machine, every %dth gene (%d genes, %d rows; equal to prepare_batch where the round\'s used2 leaves them alone: %s): '
        '%.2f s = %.2f us per row; EXTRAPOLATED to all %d rows: %.0f s' % (SAMPLE_EVERY, len(sample), sample_rows, equal, spent, spent / sample_rows * 1e6, n_rows, spent / sample_rows * n_rows))
    with open(out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
