"""K15 (pairwise allele differences of gene groups, csrc/allelediff.hip) measured on one GPU, beside the numpy formulation on the CPUs.
    python tools/allele_diff_rate.py one   [out.txt]     one group of 2 000 rows x 1 002 nt
    python tools/allele_diff_rate.py batch [out.txt]     a batch shaped like a `to_run` list: 500 groups, n log-uniform 20..2 000, ref_len 300..3 000
Per shape: HIP-event times of allele_planes and allele_diff (pep_set_timing 2), wall time of Context.allele_diff with the copy back and the share of
it that is the output's way back (timed inside the library), wall time of the two drop-ins with their int64 expansion; for `batch` also the wall time
of group_differences over a .seq store against decode + numpy over the same store.  One warm-up call of every shape, then the median of the repeats.
The CPU side is the NUMPY formulation of tests/allele_diff_helpers.py on the CPUs granted to this process - NOT numba, which is not installed here;
the reference runs its two kernels through numba, which will be faster than numpy by a factor nobody has measured.  Every numpy job is ONE group whose
row blocks are spread over the threads, so the threads are loaded evenly whatever the group sizes are.  For `batch` numpy runs on every 20th group,
one group after the other, and its time is EXTRAPOLATED to the whole batch by n^2 x ref_len (decoding by n x ref_len); the line says so.
The code measured is named by the parent commit (when git metadata is there) and the SHA-1 of the sources of the stage, because the tool runs on trees
that are not committed yet.  The lines are appended to the file named (profiles/allele_diff_rate.txt is this tool's output).  A tool, not a test."""
import hashlib, os, socket, subprocess, sys, tempfile, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
os.environ.setdefault('PEPPAN_LOG', '0')
import numpy as np                                                         # noqa: E402
from allele_diff_helpers import counts, decode_rows, numpy_tri_edge, random_group  # noqa: E402
from peppan_amd import _native as N, orthofilter as OF                     # noqa: E402
from peppan_amd.configure import effective_cpus                            # noqa: E402
from peppan_amd.mapbsn import MapBsn, decodeSeq                            # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else 'one'
out_path = sys.argv[2] if len(sys.argv) > 2 else None
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def code_id():
    h = hashlib.sha1()
    for f in ('peppan_amd/csrc/allelediff.hip', 'peppan_amd/csrc/grouptable.h', 'peppan_amd/csrc/common.h', 'peppan_amd/_native.py', 'peppan_amd/orthofilter.py'):
        with open(os.path.join(ROOT, f), 'rb') as src:
            h.update(src.read())
    try:
        head = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
        dirty = subprocess.check_output(['git', '-C', ROOT, 'status', '--porcelain', '--untracked-files=no'], stderr=subprocess.DEVNULL).decode().strip()
        head = 'commit %s%s' % (head, ' + uncommitted changes' if dirty else '')
    except Exception:
        head = 'tree without git metadata'
    return '%s, sources of the stage (allelediff.hip grouptable.h common.h _native.py orthofilter.py) sha1 %s' % (head, h.hexdigest()[:12])


def median_wall(fn, repeats):
    fn()                                        # warm-up: code objects loaded, workspaces and pinned staging areas grown
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), min(t), max(t)


def table(groups, lens):
    rows = np.concatenate([p.reshape(-1) for p in groups])
    sizes = np.concatenate([np.full(len(p), p.shape[1], dtype=np.int64) for p in groups])
    row_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    row_len = np.concatenate([np.full(len(p), L, dtype=np.uint32) for p, L in zip(groups, lens)])
    starts = np.concatenate([[0], np.cumsum([len(p) for p in groups])])
    return rows, row_off, row_len, [np.arange(a, b, dtype=np.uint32) for a, b in zip(starts[:-1], starts[1:])]


def kernel_and_call(ctx, tab, repeats, label):
    packed, row_off, row_len, index = tab
    out_bytes = sum(4 * (len(g) * (len(g) - 1) + 4 * len(g)) for g in index)
    ctx.set_timing(2)
    ctx.allele_diff(packed, row_off, row_len, index, 3, out_budget=1 << 31)
    ev = []
    for _ in range(repeats):
        ctx.allele_diff(packed, row_off, row_len, index, 3, out_budget=1 << 31)
        ev.append(ctx.allele_diff_times())
    ctx.set_timing(0)
    planes, pairs = float(np.median([e[0] for e in ev])), float(np.median([e[1] for e in ev]))
    back = []
    wall, lo, hi = median_wall(lambda: (ctx.allele_diff(packed, row_off, row_len, index, 3, out_budget=1 << 31), back.append(ctx.allele_diff_times()[2])), repeats)
    back = float(np.median(back[1:]))
    checks, _, _ = median_wall(lambda: ctx.allele_diff(packed, row_off, row_len, index, 0), repeats)      # host checks only (there the bytes are checked on the host): no kernel, no output
    say('%s: %d rows, %.1f MB packed in, %.1f MB out (both modes)' % (label, len(row_len), len(packed) / 1e6, out_bytes / 1e6))
    say('  HIP events (newest library call of the batch when the wrapper splits it): allele_planes %.3f ms, allele_diff %.3f ms' % (planes, pairs))
    say('  Context.allele_diff wall, copy back included: median %.1f ms (min %.1f, max %.1f) over %d calls; the same call with no mode bit set '
        '(host checks only, with the byte check the kernel otherwise makes; nothing uploaded) %.1f ms' % (wall * 1e3, lo * 1e3, hi * 1e3, repeats, checks * 1e3))
    share = back / 1e3 / wall
    say('  output copy (device to the buffer of the caller, host wall time inside the library, one library call): %.1f ms = %.0f %% of the call%s' % (
        back, 100 * share, ' - above 80 %: the obvious follow-up is a consumer that reduces on the device instead of shipping n^2 pairs (not built here)' if share > 0.8 else
        '; the rest is uploads, host checks, the work list and making the result views'))
    return wall


def numpy_group(seqs, pool, block=64):
    """numpy_tri_edge of ONE group with its row blocks spread over the pool's threads (numpy releases the GIL inside its loops)"""
    n = seqs.shape[0]

    def rows(a0):
        first = a0 // 512 * 512
        sq = np.concatenate([counts(seqs[a0:a0 + block], seqs[b0:b0 + 512]) for b0 in range(first, n, 512)], axis=1)
        return [sq[a - a0, a + 1 - first:] for a in range(a0, min(a0 + block, n))]
    tri = [t for part in pool.map(rows, range(0, n, block)) for t in part]
    return (np.concatenate(tri) if tri else np.zeros((0, 2), np.int64)), counts(seqs[[0, n - 1]], seqs)


cpus = effective_cpus()
threads = min(cpus, 16)
say('# allele_diff_rate %s on %s, %s, %d CPUs granted' % (what, socket.gethostname(), code_id(), cpus))
rng = np.random.default_rng(15)
with N.Context(0) as ctx:
    OF._CONTEXTS[(os.getpid(), 0)] = ctx
    if what == 'one':
        n, L = 2000, 1002
        p = random_group(rng, n, L, gap=0.05, div=0.04)
        kernel_and_call(ctx, table([p], [L]), 9, 'one group 2 000 x 1 002')
        seqs = decode_rows(p, L)
        w, lo, hi = median_wall(lambda: OF.compare_seq(seqs, np.zeros((n, n, 2), dtype=np.int64)), 5)
        say('  drop-in compare_seq (host packing + GPU + int64[n, n, 2] expansion): median %.1f ms (min %.1f, max %.1f)' % (w * 1e3, lo * 1e3, hi * 1e3))
        w, lo, hi = median_wall(lambda: OF.compare_seqX(seqs, np.zeros((n, n, 2), dtype=np.int64)), 5)
        say('  drop-in compare_seqX: median %.1f ms (min %.1f, max %.1f)' % (w * 1e3, lo * 1e3, hi * 1e3))
        t0 = time.perf_counter()
        want = numpy_tri_edge(seqs)
        one = time.perf_counter() - t0
        with ThreadPoolExecutor(threads) as pool:
            numpy_group(seqs[:256], pool)
            t0 = time.perf_counter()
            got = numpy_group(seqs, pool)
            many = time.perf_counter() - t0
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        say('  numpy formulation (NOT numba: numba is not installed on this box) for both functions: %.2f s on one thread, %.2f s with the row blocks on %d threads' % (one, many, threads))
    else:
        sizes = np.exp(rng.uniform(np.log(20), np.log(2000), 500)).astype(int)
        lens = rng.integers(300, 3001, 500)
        groups = [random_group(rng, int(n), int(L), gap=0.05, div=0.04) for n, L in zip(sizes, lens)]
        tab = table(groups, lens)
        kernel_and_call(ctx, tab, 3, '500-group batch (n log-uniform 20..2 000, ref_len 300..3 000)')
        tmp = tempfile.mkdtemp(prefix='k15_', dir='/dev/shm' if os.path.isdir('/dev/shm') else None)
        try:
            path = os.path.join(tmp, 'b.seq.npz')
            mats, at = [], 0
            rows = [r for p in groups for r in p]
            with MapBsn(path, 'w') as store:
                for m in range(0, len(rows), 1000):
                    member = np.empty(len(rows[m:m + 1000]), dtype=object)
                    for k, r in enumerate(rows[m:m + 1000]):
                        member[k] = r
                    store.save(m // 1000, member)
            for p in groups:
                mat = np.zeros((len(p), 6), dtype=np.int64)
                mat[:, 5] = np.arange(at, at + len(p))
                mats.append(mat)
                at += len(p)

            def gpu_path():
                for diffX, diff in OF.iter_group_differences(path, mats, lens):
                    pass
            t0 = time.perf_counter()
            gpu_path()
            first = time.perf_counter() - t0
            t0 = time.perf_counter()
            gpu_path()
            gpu_s = time.perf_counter() - t0
            say('  group_differences over the .seq store (%d members; store read, one batch, both int64 squares per group made and dropped): %.2f s '
                '(first call %.2f s)' % ((len(rows) + 999) // 1000, gpu_s, first))
            OF.compare_seq(decode_rows(groups[0], int(lens[0])), np.zeros((len(groups[0]),) * 2 + (2,), dtype=np.int64))       # warm-up
            decoded = [decode_rows(p, int(L)) for p, L in zip(groups, lens)]
            for fn, name in ((OF.compare_seq, 'compare_seq'), (OF.compare_seqX, 'compare_seqX')):
                t0 = time.perf_counter()
                for seqs in decoded:
                    fn(seqs, np.zeros((len(seqs), len(seqs), 2), dtype=np.int64))
                say('  drop-in %s, one call per group over the 500 groups (host packing + GPU + int64[n, n, 2] made and filled), one pass: %.2f s' % (name, time.perf_counter() - t0))
            del decoded
            pick = list(range(0, 500, 20))
            t0 = time.perf_counter()
            with MapBsn(path) as conn:
                members = {}
                jobs = []
                for k in pick:
                    ids = mats[k][:, 5].tolist()
                    for i in ids:
                        if i // 1000 not in members:
                            members[i // 1000] = conn.get(i // 1000)
                    packed = np.array([members[i // 1000][i % 1000] for i in ids])
                    seqs = np.array([45, 65, 67, 71, 84], dtype=np.uint8)[decodeSeq(packed)][:, :int(lens[k])]
                    seqs[seqs == 45] = 0
                    jobs.append(seqs)
            decode_s = time.perf_counter() - t0
            with ThreadPoolExecutor(threads) as pool:
                numpy_group(jobs[0], pool)
                t0 = time.perf_counter()
                for seqs in jobs:
                    numpy_group(seqs, pool)
                np_s = time.perf_counter() - t0
            work, rows_work = sizes.astype(float) ** 2 * lens, sizes.astype(float) * lens
            scale, rows_scale = work.sum() / work[pick].sum(), rows_work.sum() / rows_work[pick].sum()
            cpu_s = decode_s * rows_scale + np_s * scale
            say('  decode + numpy formulation (NOT numba: numba is not installed on this box), every 20th group, one group after the other with its row blocks on %d '
                'threads: store read + decode %.2f s (one thread), numpy %.2f s' % (threads, decode_s, np_s))
            say('  EXTRAPOLATED to the 500 groups - numpy by n^2 x ref_len (x %.1f), decode by n x ref_len (x %.1f), assuming the sample\'s rate holds: %.0f s' % (scale, rows_scale, cpu_s))
            say('  ratio decode + numpy (extrapolated) / group_differences (measured) for the 500-group batch: %.0f x' % (cpu_s / gpu_s))
        finally:
            import shutil
            shutil.rmtree(tmp, ignore_errors=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'a') as f:
        f.write('\n'.join(lines) + '\n\n')
