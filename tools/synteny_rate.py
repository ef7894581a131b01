"""K18 (neighbourhood paralog splitting, csrc/synteny.hip) measured on one GPU, beside a vectorised numpy form of the restatement.
    python tools/synteny_rate.py [out.txt] [genomes]
The batch is shaped like the paralogous names of a pan-genome: one two-copy family over `genomes` genomes (2 000: 4 000 members, 8 x 10^6 pairs) whose copies
sit at two neighbourhoods, lists of six ids with a few of them replaced by shared noise codes, and 3 000 small families of 2 to 40 members.  Reported: the
HIP-event times of the count pass, the scans and the emit pass (pep_set_timing 2), the wall time of Context.synteny_pairs, of the host walk (synteny_walk) and
of resolve_groups as a whole, pairs per second, the large family alone, and in the same process the wall time of the numpy form (one incidence-matrix product
per group), asserted equal pair for pair.  One warm-up call, then the median of the repeats.  The code measured is named by the parent commit (when git metadata
is there) and the SHA-1 of the sources of the stage.  The lines are appended to the file named (profiles/synteny_rate.txt is this tool's output).  A tool,
not a test."""
import hashlib, os, socket, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('PEPPAN_LOG', '0')
import numpy as np                                                         # noqa: E402
from peppan_amd import _native as N, synteny as SY                         # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
GENOMES = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
SMALL, NN = 3000, 2
SOURCES = ('peppan_amd/csrc/synteny.hip', 'peppan_amd/csrc/scan.hip', 'peppan_amd/csrc/common.h', 'peppan_amd/synteny.py', 'peppan_amd/_native.py')
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


def family(rng, genomes, copies, loci, noise=0.05, pool=8):
    """`copies` members in each of `genomes` genomes, each at one of `loci` neighbourhoods of six codes; a code is replaced by shared noise with probability `noise`"""
    n = genomes * copies
    genome = np.repeat(np.arange(genomes), copies)
    locus = (np.arange(n) % copies + rng.integers(0, loci, genomes).repeat(copies)) % loci
    codes = 1000 + 100 * locus[:, None] + np.arange(6)[None, :]
    swap = rng.random((n, 6)) < noise
    codes = np.where(swap, rng.integers(10, 10 + pool, (n, 6)), codes)
    return genome, [np.unique(row) for row in codes]


def make_batch(rng):
    groups = [(0, np.arange(2 * GENOMES), ) + family(rng, GENOMES, 2, 2)]
    for g in range(SMALL):
        genomes = int(rng.integers(1, 21))
        genome, lists = family(rng, genomes, 2, int(rng.integers(1, 4)), noise=0.1)
        groups.append((g + 1, np.arange(len(genome)), genome, lists))
    return groups


def numpy_form(genome, lists, nn):
    """the restatement with one incidence-matrix product per group -> (has, dc, conf [., 2], walk [., 2])"""
    n = len(genome)
    codes, inverse = np.unique(np.concatenate(lists) if n else np.zeros(0, np.int64), return_inverse=True)
    length = np.array([len(a) for a in lists], dtype=np.int64)
    X = np.zeros((n, max(len(codes), 1)), dtype=np.float32)
    X[np.repeat(np.arange(n), length), inverse.reshape(-1)] = 1
    C = (X @ X.T).astype(np.int64)
    pad = 6 - np.minimum(6, length)
    d = 3 * nn - (3 * C + np.maximum(pad[:, None], pad[None, :]) + 1)
    m, k = np.triu_indices(n, 1)
    d, flag = d[m, k], genome[m] != genome[k]
    conflict = ~flag & (d > 0)
    if not conflict.any():
        return False, 0, np.zeros((0, 2), np.uint32), np.zeros((0, 2), np.uint32)
    dc = int(d[conflict].min())
    w = np.flatnonzero(d < dc)
    w = w[np.lexsort((k[w], m[w], flag[w], d[w]))]
    return True, dc, np.stack([m[conflict], k[conflict]], 1).astype(np.uint32), np.stack([m[w], k[w]], 1).astype(np.uint32)


def median_of(f, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = f()
        times.append(time.perf_counter() - t0)
    return res, float(np.median(times)), min(times), max(times)


def tables(groups):
    n = [len(g[1]) for g in groups]
    lists = [a for g in groups for a in g[3]]
    member_off = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
    nb_off = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.uint64)
    return member_off, np.concatenate([g[2] for g in groups]).astype(np.uint32), nb_off, np.concatenate(lists).astype(np.uint32)


def main():
    rng = np.random.default_rng(18)
    groups = make_batch(rng)
    T = tables(groups)
    n = np.array([len(g[1]) for g in groups], dtype=np.int64)
    pairs = int((n * (n - 1) // 2).sum())
    say('# synteny_rate on %s, %s' % (socket.gethostname(), code_id()))
    say('one family of %d members (%d pairs) + %d families of 2 .. 40 members: %d members, %d pairs, nNeighbor %d' % (n[0], n[0] * (n[0] - 1) // 2, SMALL, n.sum(), pairs, NN))
    with N.Context(0) as ctx:
        ctx.synteny_pairs(*T, NN)                                              # warm-up: the buffers grow once
        ctx.set_timing(2)
        ctx.synteny_pairs(*T, NN)
        ms, moved = ctx.synteny_times()
        ctx.set_timing(0)
        say('  HIP events: synteny_count + synteny_mask %.3f ms, scans + offsets %.3f ms, synteny_emit %.3f ms = %.0f million pairs per second of kernel time; %d bytes to the host'
            % (ms[0], ms[1], ms[2], pairs / ms.sum() / 1e3, moved))
        (has, dc, conf_off, conf, walk_off, walk), wall, lo, hi = median_of(lambda: ctx.synteny_pairs(*T, NN), 5)
        say('  Context.synteny_pairs wall: median %.1f ms (min %.1f, max %.1f) over 5 calls: %d conflict pairs, %d walked pairs' % (1e3 * wall, 1e3 * lo, 1e3 * hi, len(conf), len(walk)))
        (verdict, comps), w_wall, _, _ = median_of(lambda: N.synteny_walk(T[0], conf_off, conf, walk_off, walk), 5)
        say('  synteny_walk (host C++) wall: median %.1f ms; verdicts none / refused / partition: %d / %d / %d'
            % (1e3 * w_wall, int((verdict == 0).sum()), int((verdict == 1).sum()), int((verdict == 2).sum())))
        big = tables(groups[:1])
        ctx.set_timing(2)
        ctx.synteny_pairs(*big, NN)
        ms1 = ctx.synteny_times()[0]
        ctx.set_timing(0)
        say('  the family of %d members alone: count %.3f ms, scans %.3f ms, emit %.3f ms' % (n[0], ms1[0], ms1[1], ms1[2]))
    _, r_wall, _, _ = median_of(lambda: SY.resolve_groups([g for g in groups], NN), 3)
    SY.close()
    say('  resolve_groups wall (lists from sets, planner, device, walk, dictionaries): median %.2f s = %.1f million pairs per second' % (r_wall, pairs / r_wall / 1e6))
    t0 = time.perf_counter()
    for g, (_, _, genome, lists) in enumerate(groups):
        h, d, c, w = numpy_form(genome, lists, NN)
        assert h == bool(has[g]) and d == int(dc[g]), g
        assert np.array_equal(c, conf[conf_off[g]:conf_off[g + 1]]) and np.array_equal(w, walk[walk_off[g]:walk_off[g + 1]]), g
    t1 = time.perf_counter()
    say('  numpy form of the restatement (one thread, one incidence-matrix product and one lexsort per group): %.2f s, equal to the device in every pair and its place' % (t1 - t0))
    say('  ratio numpy form / (Context.synteny_pairs + synteny_walk): %.0f x' % ((t1 - t0) / (wall + w_wall)))
    if out_path:
        with open(out_path, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
