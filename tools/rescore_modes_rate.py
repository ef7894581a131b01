"""Rescoring modes 2 and 3 (K7's codon grid, csrc/rescore.hip: k7_table<2>, k7_table<3>) measured on one GPU beside the path they replace.
    python tools/rescore_modes_rate.py [out.txt] [--hits N] [--gpu-only]
A table shaped like the hot call's: 70 000 hits of about 1 000 columns - 2 000 genes of 900 .. 1 100 nt against mutated copies of them on either strand,
every hit with 0 .. 3 gap runs of 1 .. 6 bases (fixed seed).  Reported per mode, in one process: the wall time of RunBlast._rescore_table through the GPU
(upload of the table, k7_table, float end), and beside it the host walk it took before K7 counted these modes - rescore_alignments fed by the same
function through a context object without rescore_codons, which is that path unchanged.  The two must give identical identity and score arrays, and that
is asserted.  One warm-up call and the median of 5 for the GPU route, one call of the host walk (seconds, and gigabytes of temporaries).  --gpu-only leaves the
host walk out: for a run under `rocprofv3 --kernel-trace --stats`, whose table gives the kernel's own time.  The lines are appended to the file named
(profiles/rescore_modes_rate.txt is this tool's output).  A tool, not a test."""
import os, socket, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('PEPPAN_LOG', '0')
import numpy as np                                                         # noqa: E402
from peppan_amd import _native as N, uberBlast as UB                       # noqa: E402
from peppan_amd.hittable import HitTable                                   # noqa: E402

import argparse                                                            # noqa: E402
_p = argparse.ArgumentParser()
_p.add_argument('out', nargs='?')
_p.add_argument('--hits', type=int, default=70000)
_p.add_argument('--gpu-only', action='store_true')
_a = _p.parse_args()
out_path, n_hits, gpu_only = _a.out, _a.hits, _a.gpu_only
lines = []
COMP = bytes.maketrans(b'ACGT', b'TGCA')


def say(text):
    print(text, flush=True)
    lines.append(text)


def make_table(rng, n_genes, n_hits):
    genes, copies = [], []
    for j in range(n_genes):
        g = rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), int(rng.integers(900, 1101)))
        c = g.copy()
        hit = np.flatnonzero(rng.random(len(c)) < (0.01, 0.05, 0.1, 0.2)[j % 4])
        c[hit] = rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), len(hit))
        genes.append(g.tobytes())
        copies.append(c.tobytes().translate(COMP)[::-1] if j % 2 else c.tobytes())
    q, qs, qe, ss, se, c_off, c_runs, arena = [], [], [], [], [], [], [], []
    for k in range(n_hits):
        j = int(rng.integers(0, n_genes))
        L = len(genes[j])
        gaps = [(int(rng.integers(1, 7)), int(rng.integers(1, 3))) for _ in range(int(rng.integers(0, 4)))]
        room = L - 40 - sum(g for g, _ in gaps)
        cuts = np.sort(rng.integers(1, room, len(gaps))).tolist()
        runs, at = [], 0
        for (g, op), cut in zip(gaps, cuts):
            if cut > at:
                runs.append(((cut - at) << 2) | 0)
            runs.append((g << 2) | op)
            at = cut
        runs.append(((room - at) << 2) | 0)
        qa = sum(w >> 2 for w in runs if w & 3 != 2)
        ra = sum(w >> 2 for w in runs if w & 3 != 1)
        a, b = int(rng.integers(0, L - qa + 1)), int(rng.integers(0, L - ra + 1))
        q.append(j); qs.append(a + 1); qe.append(a + qa)
        lo, hi = b + 1, b + ra
        ss.append(L - lo + 1 if j % 2 else lo); se.append(L - hi + 1 if j % 2 else hi)
        c_off.append(len(arena)); c_runs.append(len(runs))
        arena += runs
    return genes, copies, [np.array(x, dtype=np.int64) for x in (q, qs, qe, ss, se, c_off, c_runs)], np.array(arena, dtype=np.uint32)


class HostWalk(object):
    """a context object without rescore_codons: _rescore_table then takes the host walk, rescore_alignments, as it did for modes 2 / 3 before"""


def same(a, b):
    return a.shape == b.shape and bool(np.all((a == b) | ((a != a) & (b != b))))


say('# rescore_modes_rate on %s' % socket.gethostname())
rng = np.random.default_rng(23)
t0 = time.perf_counter()
genes, copies, (q, qs, qe, ss, se, c_off, c_runs), arena = make_table(rng, 2000, n_hits)
q_names, r_names = ['g%04d' % j for j in range(len(genes))], ['c%04d' % j for j in range(len(copies))]
lens = np.array([len(g) for g in genes], dtype=np.int64)
columns = int(sum(int(w) >> 2 for w in arena.tolist() if w & 3 != 2))
say('%d hits, %d runs, %.1f M columns (%.0f per hit), %d genes of 900 .. 1 100 nt; made in %.1f s' % (n_hits, len(arena), columns / 1e6, columns / float(n_hits), len(genes),
                                                                                                    time.perf_counter() - t0))
rb = UB.RunBlast()
rb.qrySeq = {n: s.decode() for n, s in zip(q_names, genes)}
rb.refSeq = {n: s.decode() for n, s in zip(r_names, copies)}
z = np.zeros(n_hits)


def table():
    return HitTable(list(q_names), list(r_names), q, q, z, z, z, z, qs, qe, ss, se, z, z, lens[q], lens[q], arena, c_off, c_runs, rid=np.arange(n_hits))


with N.Context(0) as ctx:
    for mode in (3, 2):
        rb.table_id = 11
        rb._rescore_table(None, None, table(), mode, None, 11, cut=False, ctx=ctx)          # warm-up: sequences uploaded, code object loaded, workspaces grown
        t = []
        for _ in range(5):
            T = table()
            t0 = time.perf_counter()
            new = rb._rescore_table(None, None, T, mode, None, 11, cut=False, ctx=ctx)
            t.append(time.perf_counter() - t0)
        gpu_s = float(np.median(t))
        say('mode %d  _rescore_table through the GPU (table upload + k7_table<%d> + float end): median %.4f s (min %.4f, max %.4f) of 5' % (mode, mode, gpu_s, min(t), max(t)))
        if gpu_only:
            continue
        T = table()
        t0 = time.perf_counter()
        with np.errstate(all='ignore'):
            old = rb._rescore_table(None, None, T, mode, None, 11, cut=False, ctx=HostWalk())
        host_s = time.perf_counter() - t0
        assert same(old.iden, new.iden) and same(old.score, new.score), 'the two paths disagree'
        say('mode %d  the host walk it replaces (rescore_alignments over the same table, same process), identical iden and score (asserted): %.2f s once  ->  %.0f x'
            % (mode, host_s, host_s / gpu_s))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'a') as f:
        f.write('\n'.join(lines) + '\n\n')
