"""K20 (the counting loops of PEPPAN_parser, csrc/parser.hip) measured on one GPU, beside a numpy form of the reference's own loops on one thread.
    python tools/parser_rate.py [out.txt] [genomes] [genes] [orders] [core genes]
Defaults: BASELINE's largest configuration - 2 000 genomes, a pan-genome of 50 000 genes walked in 1 000 orders (writeCurve), and 2 000 profiles of 3 000 core
genes (getDistance).  The presence matrix has a core / shell / cloud mix, printed with the result: 6 % of the genes in 99 to 100 % of the genomes, 8 % at a
frequency drawn evenly from 15 to 95 %, 86 % at 0.15 u^3 (u even in 0..1; never below one genome).  The profiles carry alleles 1 .. 40 skewed to the low numbers,
2 % of the entries absent (0).  Reported per function: the HIP-event time of the kernel (pep_set_timing 2), the wall time of the library call (Context method:
checks, copies both ways, kernel), the wall time of the whole host function from arrays (orders by shuffling, bit packing, library call; recoding, library call,
-log) and of its parts, and the text writers.  One warm-up call, then the median of 3.  Beside it the reference's loops in numpy on one thread of the same box, at
a reduced number of orders / of rows, asserted equal to the device there, with the extrapolation to the full size stated as one.  The code measured is named by
the parent commit (when git metadata is there) and the SHA-1 of the sources of the stage.  The lines are appended to the file named
(profiles/parser_rate.txt is this tool's output).  A tool, not a test."""
import hashlib, os, socket, subprocess, sys, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
os.environ.setdefault('PEPPAN_LOG', '0')
import numpy as np                                                         # noqa: E402
from peppan_amd import _native as N, panparser as PP                       # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
GENOMES = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
GENES = int(sys.argv[3]) if len(sys.argv) > 3 else 50000
ORDERS = int(sys.argv[4]) if len(sys.argv) > 4 else 1000
CORE = int(sys.argv[5]) if len(sys.argv) > 5 else 3000
CPU_ORDERS, CPU_ROWS = 2, 40
SOURCES = ('peppan_amd/csrc/parser.hip', 'peppan_amd/csrc/common.h', 'peppan_amd/panparser.py', 'peppan_amd/_native.py')
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


def median_of(f, repeats=3):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = f()
        times.append(time.perf_counter() - t0)
    return res, float(np.median(times))


def make_presence(rng):
    kind = rng.random(GENES)
    freq = np.where(kind < 0.06, rng.uniform(0.99, 1.0, GENES), np.where(kind < 0.14, rng.uniform(0.15, 0.95, GENES), 0.15 * rng.random(GENES) ** 3))
    P = rng.random((GENOMES, GENES), dtype=np.float32) < freq[None, :].astype(np.float32)
    empty = np.flatnonzero(~P.any(0))
    P[rng.integers(0, GENOMES, len(empty)), empty] = True                   # every gene of a pan-genome is in some genome
    return P


def numpy_curves(P, orders):
    """the loop of writeCurve in its own shape: a counter per gene, two sums over all genes per step"""
    members = [np.flatnonzero(row) for row in P]
    curves = np.zeros([len(P), len(orders), 2], dtype=int)
    for t, order in enumerate(orders):
        genes = np.zeros(P.shape[1], dtype=int)
        for k, g in enumerate(order):
            genes[members[g]] += 1
            curves[k, t, :] = (np.sum(genes >= 1), np.sum(genes >= (k + 1)))
    return curves


def numpy_rows(profiles, rows):
    """the first `rows` rows of getDistance's loop in its own shape -> their (shared, presence) counts against the rows behind them"""
    contents = profiles > 0
    out = []
    for i in range(rows):
        p, c, j = profiles[i], contents[i], i + 1
        out.append((np.sum((p == profiles[j:]) & (contents[j:] * c), 1), np.sum(contents[j:] * c, 1)))
    return out


def main():
    rng = np.random.default_rng(20)
    say('# parser_rate on %s, %s' % (socket.gethostname(), code_id()))
    # ---- writeCurve
    P = make_presence(rng)
    per_gene = P.sum(0) / float(GENOMES)
    say('writeCurve: %d genomes x %d genes x %d orders; genes in >= 99 %% of the genomes %d, in 15 .. 99 %% %d, below 15 %% %d; %.0f genes per genome; %d words per bit row, matrix %.1f MB'
        % (GENOMES, GENES, ORDERS, int((per_gene >= 0.99).sum()), int(((per_gene >= 0.15) & (per_gene < 0.99)).sum()), int((per_gene < 0.15).sum()), P.sum(1).mean(),
           (GENES + 63) // 64, GENOMES * ((GENES + 63) // 64) * 8 / 1e6))
    np.random.seed(20)
    orders, t_shuffle = median_of(lambda: PP.shuffled_orders(GENOMES, ORDERS))
    bits, t_pack = median_of(lambda: N.pack_presence(P))
    with N.Context(0) as ctx:
        ctx.rarefaction_curves(bits, GENES, orders)                            # warm-up: the buffers grow once
        ctx.set_timing(2)
        ctx.rarefaction_curves(bits, GENES, orders)
        ms, _, up, down = ctx.parser_times()
        ctx.set_timing(0)
        steps = GENOMES * ORDERS
        say('  HIP events: rarefaction %.3f ms = %.2f ns per step of a walk, %.0f GB/s of bit-row words read; %d bytes to the device, %d bytes to the host'
            % (ms, 1e6 * ms / steps, steps * ((GENES + 63) // 64) * 8 / ms / 1e6, up, down))
        curves, wall = median_of(lambda: ctx.rarefaction_curves(bits, GENES, orders))
        _, c_wall = median_of(lambda: N.rarefaction_curves_check(bits, GENES, orders))
        say('  Context.rarefaction_curves wall: median %.1f ms over 3 calls; its host checks alone (rarefaction_curves_check): %.1f ms' % (1e3 * wall, 1e3 * c_wall))
    _, whole = median_of(lambda: PP._curves_of(P, ORDERS, None, None))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        _, t_text = median_of(lambda: PP.curve_text(curves, GENOMES, np.mean(P.sum(1)), GENES))
    say('  whole function from the presence matrix (orders, packing, library call): median %.2f s; of it %d shuffles %.3f s, bit packing %.3f s, the library call %.3f s; '
        'the text of the file (three curve fits, sorted table) %.3f s more' % (whole, ORDERS, t_shuffle, t_pack, wall, t_text))
    t0 = time.perf_counter()
    want = numpy_curves(P, orders[:CPU_ORDERS])
    cpu = time.perf_counter() - t0
    assert np.array_equal(want, curves[:, :CPU_ORDERS]), 'the numpy form and the device disagree'
    say('  numpy form of the reference\'s loop, one thread, %d orders (equal to the device in every entry): %.1f us per step; EXTRAPOLATED to %d orders: %.0f s = %.0f x the whole '
        'function, %.0f x the library call' % (CPU_ORDERS, 1e6 * cpu / (CPU_ORDERS * GENOMES), ORDERS, cpu / CPU_ORDERS * ORDERS, cpu / CPU_ORDERS * ORDERS / whole,
                                             cpu / CPU_ORDERS * ORDERS / wall))
    PP.close()
    # ---- getDistance
    skew = np.minimum((40 * rng.random((GENOMES, CORE)) ** 2).astype(np.int64) + 1, 40)
    profiles = np.where(rng.random((GENOMES, CORE)) < 0.02, 0, skew)
    say('getDistance: %d profiles x %d genes, alleles 1 .. 40, %.1f %% absent' % (GENOMES, CORE, 100. * (profiles == 0).mean()))
    with N.Context(0) as ctx:
        as32 = PP._as_int32(profiles)
        ctx.profile_pairs(as32)
        ctx.set_timing(2)
        ctx.profile_pairs(as32)
        _, ms, up, down = ctx.parser_times()
        ctx.set_timing(0)
        pairs = GENOMES * (GENOMES - 1) // 2
        say('  HIP events: profile_pairs %.3f ms = %.1f G comparisons per second of kernel time; %d bytes to the device, %d bytes to the host' % (ms, pairs * CORE / ms / 1e6, up, down))
        (shared, presence), wall = median_of(lambda: ctx.profile_pairs(as32))
        say('  Context.profile_pairs wall (copies, kernel, mirroring the triangle): median %.1f ms over 3 calls' % (1e3 * wall))
    dist, whole = median_of(lambda: PP.getDistance(profiles))
    _, t_log = median_of(lambda: PP.distances_of(shared, presence))
    _, t_text = median_of(lambda: PP.dist_text(['genome%04d' % k for k in range(GENOMES)], dist), 1)
    say('  whole function getDistance (int64 profiles to int32, library call, -log): median %.3f s; of it -log on the counts %.3f s; the text of the .dist file %.2f s more'
        % (whole, t_log, t_text))
    rows = min(CPU_ROWS, GENOMES - 1)
    t0 = time.perf_counter()
    want = numpy_rows(profiles, rows)
    cpu = time.perf_counter() - t0
    for i, (s, p) in enumerate(want):
        assert np.array_equal(s, shared[i, i + 1:]) and np.array_equal(p, presence[i, i + 1:]), 'the numpy form and the device disagree'
    done = sum(GENOMES - 1 - i for i in range(rows))
    say('  numpy form of the reference\'s loop, one thread, the first %d rows = %d pairs (equal to the device in every count): %.2f us per pair; EXTRAPOLATED to all %d pairs: %.1f s '
        '= %.0f x the whole function, %.0f x the library call' % (rows, done, 1e6 * cpu / done, pairs, cpu / done * pairs, cpu / done * pairs / whole, cpu / done * pairs / wall))
    PP.close()
    if out_path:
        with open(out_path, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
