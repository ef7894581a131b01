"""K16 (divergence verdicts of gene groups, csrc/divergence.hip) measured on one GPU beside the path it replaces.
    python tools/group_verdict_rate.py [out.txt]
The 500-group batch of tools/allele_diff_rate.py (same seed and shapes: n log-uniform 20..2 000, ref_len 300..3 000) in a .seq store, with a
divergence per group, genomes and a global_differences table drawn so that roughly 80 / 15 / 5 % of the groups come out as verdict 0 / 1 / 2
(the shares that came out are printed).  Reported: HIP-event times of the four kernels (pep_set_timing 2), bytes_to_host, the wall time of
orthofilter.group_verdicts(detail=True), and beside it, in the same process, the path a caller had before K16: group_differences(edge=True,
full=True) followed by the host float layer (the vectorised checkDiv and distances_from_diff) - which must produce the same verdicts, and that
is asserted.  One warm-up call of each, then the median of 5 with min and max.  The lines are appended to the file named
(profiles/group_verdict_rate.txt is this tool's output).  A tool, not a test."""
import os, shutil, socket, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
os.environ.setdefault('PEPPAN_LOG', '0')
import numpy as np                                                         # noqa: E402
from divergence_helpers import clade, pack_codes                           # noqa: E402
from peppan_amd import _native as N, orthofilter as OF                     # noqa: E402
from peppan_amd.mapbsn import MapBsn                                       # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
lines = []
SELF_ID, SIGMA, GENOMES = 0.002, 5, 2000


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, repeats=5):
    fn()                                        # warm-up: code objects loaded, workspaces and pinned staging areas grown
    t, res = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), min(t), max(t), res


def host_verdict(diffX, diff, genomes, gd):
    """the float layer on the host, vectorised, from K15's two squares (what a caller of group_differences had to do)"""
    n = len(genomes)
    if n < 2:
        return 0
    for row in (0, n - 1):
        other = np.arange(n) != row
        mut, aln = diffX[row, other, 0].astype(np.float64), diffX[row, other, 1].astype(np.float64)
        _, den_x, _ = OF._gd_of_pairs(gd, np.full(n - 1, genomes[row]), genomes[other], aln)
        if np.any(mut / aln / den_x > 1):
            break
    else:
        return 0                                # (the batch has no in-paralog group)
    distances = OF.distances_from_diff(diff.astype(np.float64), genomes, gd)
    return 2 if np.any(distances[:, :, 0] > distances[:, :, 1]) else 1


say('# group_verdict_rate on %s' % socket.gethostname())
rng = np.random.default_rng(15)
sizes = np.exp(rng.uniform(np.log(20), np.log(2000), 500)).astype(int)
lens = rng.integers(300, 3001, 500)
den_x, den = 0.02 * np.exp(0.5 * np.sqrt(SIGMA)), 0.02 * np.exp(0.5 * SIGMA)
aim = rng.choice(3, size=500, p=[0.8, 0.15, 0.05])
groups, genomes = [], []
for n, L, a in zip(sizes, lens, aim):
    level = (0.004, np.sqrt(den_x * den), 0.004)[a]
    codes = clade(rng, rng.integers(1, 5, int(L)), int(n), level / 2, gap=0.05)
    if a == 2:
        codes[int(n) // 2:] = clade(rng, rng.integers(1, 5, int(L)), int(n) - int(n) // 2, 0.002, gap=0.05)      # a second clade far away
    groups.append(pack_codes(codes, rng))
    genomes.append(rng.permutation(GENOMES)[:int(n)])
gd_dict = {(a, b): (0.02, 0.5) for a in range(GENOMES) for b in range(a + 1, GENOMES) if (a * 7 + b) % 10}      # 90 % of the genome pairs are known
t0 = time.perf_counter()
gd = OF.gd_table(gd_dict, SELF_ID, SIGMA)
say('gd_table of %d keys (host, once per run of the pipeline): %.2f s' % (len(gd.keys), time.perf_counter() - t0))
tmp = tempfile.mkdtemp(prefix='k16_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None)
try:
    path = os.path.join(tmp, 'b.seq.npz')
    rows = [r for p in groups for r in p]
    with MapBsn(path, 'w') as store:
        for m in range(0, len(rows), 1000):
            member = np.empty(len(rows[m:m + 1000]), dtype=object)
            for k, r in enumerate(rows[m:m + 1000]):
                member[k] = r
            store.save(m // 1000, member)
    to_run, at = [], 0
    for p, g, L in zip(groups, genomes, lens):
        mat = np.zeros((len(p), 6), dtype=np.int64)
        mat[:, 1], mat[:, 5] = g, np.arange(at, at + len(p))
        at += len(p)
        to_run.append((mat, False, int(L)))
    params = dict(self_id=SELF_ID, allowed_sigma=SIGMA)
    with N.Context(0) as ctx:
        OF._CONTEXTS[(os.getpid(), 0)] = ctx
        t0 = time.perf_counter()
        OF._read_groups(path, [t[0] for t in to_run], lens)
        read_s = time.perf_counter() - t0
        ctx.set_timing(2)
        OF.group_verdicts(path, to_run, gd, params)
        ms, moved = [], []
        for _ in range(5):
            res = OF.group_verdicts(path, to_run, gd, params)
            a, b = ctx.group_verdicts_totals()
            ms.append(a)
            moved.append(b)
        ctx.set_timing(0)
        ms = np.median(np.array(ms), axis=0)
        verdicts = np.array([v.verdict for v in res])
        shares = np.bincount(verdicts, minlength=3) / 5.
        say('500-group batch (n log-uniform 20..2 000, ref_len 300..3 000), %d rows, %.1f MB packed, %d genomes: verdict 0 / 1 / 2 = %.1f / %.1f / %.1f %%' % (
            len(rows), sum(len(r) for r in rows) / 1e6, GENOMES, shares[0], shares[1], shares[2]))
        say('  HIP events, summed over the library calls of one batch: allele_planes %.3f ms, verdict_edge %.3f ms, verdict_pairs %.3f ms, verdict_leaders %.3f ms' % tuple(ms))
        say('  bytes_to_host: %d (one byte per group and one word per library call; the rest is the triangles and leaders of the %d verdict-2 groups)' % (moved[-1], int((verdicts == 2).sum())))
        new_s, lo, hi, res = timed(lambda: OF.group_verdicts(path, to_run, gd, params))
        say('  orthofilter.group_verdicts(detail=True) over the .seq store: median %.3f s (min %.3f, max %.3f) of 5; reading the store alone %.3f s' % (new_s, lo, hi, read_s))
        light_s, lo, hi, _ = timed(lambda: OF.group_verdicts(path, to_run, gd, params, detail=False))
        say('  ... with detail=False: median %.3f s (min %.3f, max %.3f)' % (light_s, lo, hi))

        def old_path():
            return [host_verdict(diffX, diff, g, gd) for (diffX, diff), g in zip(OF.iter_group_differences(path, [t[0] for t in to_run], lens), genomes)]
        old_s, lo, hi, old = timed(old_path)
        assert np.array_equal(np.array(old), verdicts), 'the two paths disagree on a verdict'
        say('  the path before K16 in the same process: group_differences(edge=True, full=True) + the host float layer (vectorised checkDiv, distances_from_diff), '
            'the same 500 verdicts (asserted equal): median %.2f s (min %.2f, max %.2f) of 5' % (old_s, lo, hi))
        dominated = 'reading the store' if read_s > 0.5 * new_s else 'not the store read (%.0f %% of it): the host side of the verdict-2 groups (float64 squares, distances, incompatible) and the tables of the call' % (100 * read_s / new_s)
        say('  the new path is dominated by %s' % dominated)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'a') as f:
        f.write('\n'.join(lines) + '\n\n')
