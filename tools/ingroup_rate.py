"""K17 (in-group rows and gene scores of `initializing`, csrc/ingroup.hip) measured on one GPU, beside a vectorised numpy form of the restatement.
    python tools/ingroup_rate.py [out.txt] [genes]
The batch is shaped like the mapping's gene table: `genes` genes (10 000) x 500 genomes with one to three rows per genome, about 85 % of the rows at
or above the identity threshold, a global_differences table of all genome pairs, and one worst-case gene of 16 384 rows, half of them rows below the
threshold that no seed lets in.  Reported: the HIP-event times of ingroup_pairs and ingroup_finish (pep_set_timing 2), the wall time of the host
prologue alone (pep_gene_ingroups_check: the checks, first[] and the work list) and its share of the call, the wall time of Context.gene_ingroups,
the worst-case gene alone, and in the same process the wall time of the numpy form, asserted equal.  One warm-up call, then the median of the repeats.
The code measured is named by the parent commit (when git metadata is there) and the SHA-1 of the sources of the stage.  The lines are appended to the
file named (profiles/ingroup_rate.txt is this tool's output).  A tool, not a test."""
import hashlib, os, socket, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('PEPPAN_LOG', '0')
import numpy as np                                                         # noqa: E402
from peppan_amd import _native as N, orthofilter as OF                     # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
n_genes = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
GENOMES, SELF_ID, SIGMA, THR = 500, 0.005, 3., (0.9 - 0.02) * 10000
SOURCES = ('peppan_amd/csrc/ingroup.hip', 'peppan_amd/csrc/gdtable.h', 'peppan_amd/csrc/common.h', 'peppan_amd/_native.py')
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def code_id():
    h = hashlib.sha1()
    for f in SOURCES:
        with open(os.path.join(ROOT, f), 'rb') as src:
            h.update(src.read())
    try:
        parent = 'parent commit ' + subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        parent = 'tree without git metadata'
    return '%s, sources of the stage (%s) sha1 %s' % (parent, ' '.join(os.path.basename(f) for f in SOURCES), h.hexdigest()[:12])


def make_batch(rng):
    gd = {(a, b): (float(rng.uniform(0.015, 0.03)), float(rng.uniform(0.1, 0.5))) for a in range(GENOMES) for b in range(a + 1, GENOMES)}
    genome, iden, score, lens = [], [], [], []
    for _ in range(n_genes):
        g = np.repeat(np.arange(GENOMES), rng.integers(1, 4, GENOMES))
        g = g[rng.permutation(len(g))]
        i = np.where(rng.random(len(g)) < 0.85, rng.integers(8800, 10001, len(g)), rng.integers(8000, 8800, len(g)))
        i[0] = 10000
        genome.append(g); iden.append(i); score.append(rng.integers(-5000, 5000, len(g))); lens.append(len(g))
    g = rng.integers(0, GENOMES, 16384)
    i = np.where(np.arange(16384) % 2 == 0, rng.integers(8800, 10001, 16384), rng.integers(1000, 2000, 16384))      # 1 - 2000 / 8800 = 0.77 > every bound
    genome.append(g); iden.append(i); score.append(rng.integers(-5000, 5000, 16384)); lens.append(16384)
    return (np.concatenate(genome).astype(np.uint32), np.concatenate(iden).astype(np.int32), np.concatenate(score).astype(np.int64),
            np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), gd)


def numpy_form(genome, iden, score, gene_off, den):
    """the restatement with one matrix per gene: rows below the threshold against the seeds in front of them"""
    keep, total = np.zeros(len(genome), bool), np.zeros(len(gene_off) - 1, np.int64)
    for g in range(len(gene_off) - 1):
        lo, hi = int(gene_off[g]), int(gene_off[g + 1])
        G, I = genome[lo:hi].astype(np.int64), iden[lo:hi].astype(np.float64)
        seed = I >= THR
        s, t = np.flatnonzero(seed), np.flatnonzero(~seed)
        raw = seed.copy()
        for c in range(0, len(t), 1024):
            tt = t[c:c + 1024]
            ss = s[s < tt[-1]]
            ok = ((1. - I[tt][:, None] / I[ss][None, :]) / den[G[tt][:, None], G[ss][None, :]] < 1) & (ss[None, :] < tt[:, None])
            raw[tt] = ok.any(axis=1)
        _, first, inverse = np.unique(G, return_index=True, return_inverse=True)
        k = raw[first[inverse]]
        keep[lo:hi] = k
        total[g] = np.abs(score[lo:hi][first][raw[first]]).sum()
    return keep, total


def median_of(f, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = f()
        times.append(time.perf_counter() - t0)
    return res, float(np.median(times)), min(times), max(times)


def main():
    rng = np.random.default_rng(17)
    genome, iden, score, gene_off, gd = make_batch(rng)
    table = OF.gd_table(gd, SELF_ID, SIGMA)
    den = np.full((GENOMES, GENOMES), np.nan)
    for (a, b), row in zip(gd, table.vals):            # gd was made in sorted key order
        den[a, b] = den[b, a] = row[2]
    np.fill_diagonal(den, SELF_ID)
    say('# ingroup_rate on %s, %s' % (socket.gethostname(), code_id()))
    say('%d genes x %d genomes (1 - 3 rows per genome) + one gene of 16 384 rows: %d rows, %d genome pairs in the table, %.0f %% seeds'
        % (n_genes, GENOMES, len(genome), len(table.keys), 100 * float((iden >= THR).mean())))
    with N.Context(0) as ctx:
        ctx.gene_ingroups(genome, iden, score, gene_off, table, SELF_ID, THR)          # warm-up: the buffers grow once
        ctx.set_timing(2)
        ctx.gene_ingroups(genome, iden, score, gene_off, table, SELF_ID, THR)
        ms, moved = ctx.gene_ingroups_times()
        ctx.set_timing(0)
        say('  HIP events: ingroup_pairs %.3f ms, ingroup_finish %.3f ms; %d bytes to the host' % (ms[0], ms[1], moved))
        (keep, total), wall, lo, hi = median_of(lambda: ctx.gene_ingroups(genome, iden, score, gene_off, table, SELF_ID, THR), 5)
        _, pro, _, _ = median_of(lambda: N.gene_ingroups_check(genome, iden, score, gene_off, table, SELF_ID, THR), 5)
        say('  Context.gene_ingroups wall: median %.1f ms (min %.1f, max %.1f) over 5 calls; the host prologue alone (checks, first[], work list) %.1f ms = %.0f %% of the call'
            % (1e3 * wall, 1e3 * lo, 1e3 * hi, 1e3 * pro, 100 * pro / wall))
        w0 = int(gene_off[-2])
        ctx.set_timing(2)
        ctx.gene_ingroups(genome[w0:], iden[w0:], score[w0:], [0, len(genome) - w0], table, SELF_ID, THR)
        say('  the worst-case gene alone (16 384 rows, 8 192 of them below the threshold and let in by nobody): ingroup_pairs %.3f ms' % ctx.gene_ingroups_times()[0][0])
        ctx.set_timing(0)
    t0 = time.perf_counter()
    want_keep, want_total = numpy_form(genome, iden, score, gene_off, den)
    t1 = time.perf_counter()
    assert np.array_equal(keep, want_keep) and np.array_equal(total, want_total)
    say('  numpy form of the restatement (one thread, one matrix per gene: rows below the threshold x seeds): %.2f s, equal to the device in every row and score; %d of %d rows kept'
        % (t1 - t0, int(keep.sum()), len(keep)))
    say('  ratio numpy form / Context.gene_ingroups: %.0f x' % ((t1 - t0) / wall))
    if out_path:
        with open(out_path, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
