"""K19 (the gene structure of predictions, csrc/genestruct.hip) measured on one GPU, beside two single-thread forms of the same function.
    python tools/genestruct_rate.py [out.txt] [predictions]
The batch is shaped like the intact predictions of write_output: 16 contigs of 2.2 Mb carry genes back to back (an open reading frame of 0.9 to 1.5 kb behind 60
nucleotides, half of them on the reverse strand, 5 % with an early stop codon), and 2 x 10^6 predictions name them in the contig form - the window [s2 - 1, e2) of
the contig, 1.0 to 1.6 kb, the frame list [0] for nine in ten.  Reported: the HIP-event time of the kernel (pep_set_timing 2), the wall time of
Context.gene_structure with its host prologue timed through gene_structure_check, the wall time of gene_structures as a whole with its parts, and the bytes each way.
One warm-up call, then the median of the repeats (5 for the library call, 3 for gene_structures).  Beside it, on a sample of 20 000 of the same items and one thread:
the plain-loop restatement of tests/genestruct_helpers.py and a numpy form (peppan_amd.configure.transeq with marked starts + str.find, the reference's own shape),
both asserted equal to the device on the sample.  The code measured is named by the parent commit (when git metadata is there) and the SHA-1 of the sources of the
stage.  The lines are appended to the file named (profiles/genestruct_rate.txt is this tool's output).  A tool, not a test."""
import hashlib, os, socket, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
os.environ.setdefault('PEPPAN_LOG', '0')
import numpy as np                                                         # noqa: E402
from peppan_amd import _native as N, genestruct as GS                      # noqa: E402
from peppan_amd.configure import transeq                                   # noqa: E402
from genestruct_helpers import rc, restate                                 # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
PREDICTIONS = int(sys.argv[2]) if len(sys.argv) > 2 else 2000000
CONTIGS, CONTIG_LEN, SAMPLE, LEAD = 16, 2200000, 20000, 60
SOURCES = ('peppan_amd/csrc/genestruct.hip', 'peppan_amd/csrc/common.h', 'peppan_amd/genestruct.py', 'peppan_amd/_native.py')
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


def make_contigs(rng):
    """-> ({name: str}, genes [(contig, s2, e2, strand, orf length, intact)])"""
    sense = np.array([[a, b, c] for a in b'ACGT' for b in b'ACGT' for c in b'ACGT' if bytes([a, b, c]) not in (b'TAA', b'TAG', b'TGA')], dtype=np.uint8)
    contigs, genes = {}, []
    for c in range(CONTIGS):
        name = 'contig%02d' % c
        seq = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, CONTIG_LEN)].copy()
        at = 500
        while at + 1800 < CONTIG_LEN:
            codons = int(rng.integers(300, 501))
            orf = sense[rng.integers(0, len(sense), codons)].copy()
            orf[0] = np.frombuffer((b'ATG', b'ATG', b'GTG', b'TTG')[int(rng.integers(0, 4))], dtype=np.uint8)
            orf[-1] = np.frombuffer((b'TAA', b'TAG', b'TGA')[int(rng.integers(0, 3))], dtype=np.uint8)
            intact = rng.random() >= 0.05
            if not intact:
                orf[int(rng.integers(30, codons // 2))] = np.frombuffer(b'TAA', dtype=np.uint8)
            lead = sense[rng.integers(0, len(sense), LEAD // 3)]
            tail = int(rng.integers(40, 100))
            window = np.concatenate([lead.reshape(-1), orf.reshape(-1), seq[at + LEAD + 3 * codons:at + LEAD + 3 * codons + tail]])
            strand = '+-'[int(rng.integers(0, 2))]
            if strand == '-':
                window = np.frombuffer(rc(window.tobytes().decode()).encode(), dtype=np.uint8)
            seq[at:at + len(window)] = window
            genes.append((name, at + 1, at + len(window), strand, 3 * codons, intact))
            at += len(window) + int(rng.integers(0, 40))
        contigs[name] = seq.tobytes().decode()
    return contigs, genes


def make_items(rng, genes):
    pick = rng.integers(0, len(genes), PREDICTIONS)
    several = rng.random(PREDICTIONS) < 0.1
    items = []
    for pid, (g, more) in enumerate(zip(pick.tolist(), several.tolist())):
        name, s2, e2, strand, orf, intact = genes[g]
        pred = [''] * 16
        pred[5], pred[11], pred[12], pred[14] = name, strand, orf, [0, 1, 2] if more else [0]
        s, e = (s2 + LEAD, e2) if strand == '+' else (s2, e2 - LEAD)
        items.append([pid, pred, None, s, e, s2, e2, LEAD, int(orf * 0.2 + 0.01), 11])
    return items


def numpy_form(item):
    """determineGeneStructure in the reference's own shape: the vectorised transeq of this package with marked starts, then str.find / str.rfind"""
    pid, pred, seq, s, e, s2, e2, lp, allowed_vary, gtable = item
    cds, cdss = 'CDS', []
    a, b = lp // 3, (lp + allowed_vary) // 3
    for frame, aa in zip(pred[14], transeq({'n': seq}, transl_table=gtable, markStarts=True, frame=','.join(str(f + 1) for f in pred[14]))['n']):
        if (len(seq) - frame) % 3 > 0:
            aa = aa[:-1]
        cds = 'CDS'
        s0, s1 = aa.find('M', a, b), aa.rfind('M', 0, a)
        start = s0 if s0 >= 0 else s1
        if start < 0:
            cds, start = 'nostart', a
        stop = aa.find('X', start)
        while 0 <= stop < b:
            s0 = aa.find('M', stop, b)
            if s0 < 0:
                break
            start, stop = s0, aa.find('X', s0)
        if stop < 0:
            cds = 'nostop'
        elif (stop - start + 1) * 3 < pred[12] - allowed_vary:
            cds = 'premature_stop:{0:.2f}%'.format((stop - start + 1) * 300 / pred[12])
        if cds == 'CDS':
            if pred[11] == '+':
                return pid, cds, s2 + start * 3 + frame, s2 + stop * 3 + 2 + frame
            return pid, cds, e2 - stop * 3 - 2 - frame, e2 - start * 3 - frame
        cdss.append(cds)
        if frame > 0:
            cds = cdss[0].replace('premature_stop', 'frameshift') if cdss[0].find('premature_stop') >= 0 else 'frameshift'
    return pid, cds, s, e


def median_of(f, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = f()
        times.append(time.perf_counter() - t0)
    return res, float(np.median(times)), min(times), max(times)


def main():
    rng = np.random.default_rng(19)
    contigs, genes = make_contigs(rng)
    items = make_items(rng, genes)
    n = len(items)
    win = np.array([it[6] - it[5] + 1 for it in items])
    say('# genestruct_rate on %s, %s' % (socket.gethostname(), code_id()))
    say('%d predictions over %d genes on %d contigs of %d nt: windows %d .. %d nt (mean %.0f), %.1f %% of the genes intact, frame list [0] for %.1f %%, strand - for %.1f %%'
        % (n, len(genes), CONTIGS, CONTIG_LEN, win.min(), win.max(), win.mean(), 100. * np.mean([g[5] for g in genes]), 100. * np.mean([len(it[1][14]) == 1 for it in items]),
           100. * np.mean([it[1][11] == '-' for it in items])))
    # the library's tables, as gene_structures makes them
    names = sorted(contigs)
    index = {k: i for i, k in enumerate(names)}
    nt = ''.join(contigs[k] for k in names).encode()
    seq_off = np.concatenate([[0], np.cumsum([len(contigs[k]) for k in names])]).astype(np.uint64)
    T = (seq_off, np.array([index[it[1][5]] for it in items], np.uint32), np.array([it[5] - 1 for it in items], np.uint64), win.astype(np.uint32),
         np.array([sum(2 << f for f in it[1][14]) | (it[1][11] == '-') for it in items], np.uint8), np.array([it[7] for it in items], np.uint32),
         np.array([it[8] for it in items], np.uint32), np.array([it[1][12] for it in items], np.uint32))
    with N.Context(0) as ctx:
        ctx.gene_structure(nt, *T)                                             # warm-up: the buffers grow once
        ctx.set_timing(2)
        ctx.gene_structure(nt, *T)
        ms, up, down = ctx.gene_structure_times()
        ctx.set_timing(0)
        say('  HIP events: gene_structure %.3f ms = %.0f million predictions per second of kernel time, %.1f GB/s of window bytes; %d bytes to the device, %d bytes to the host'
            % (ms, n / ms / 1e3, win.sum() / ms / 1e6, up, down))
        (frame, start_aa, stop_aa, kind), wall, lo, hi = median_of(lambda: ctx.gene_structure(nt, *T), 5)
        _, c_wall, _, _ = median_of(lambda: N.gene_structure_check(*T), 5)
        say('  Context.gene_structure wall: median %.1f ms (min %.1f, max %.1f) over 5 calls; its host prologue alone (gene_structure_check): median %.1f ms'
            % (1e3 * wall, 1e3 * lo, 1e3 * hi, 1e3 * c_wall))
        say('  outcomes: frame 0 / 1 / 2 / none: %s; first tried frame CDS / nostart / nostop / premature_stop: %s'
            % (' / '.join(str(int((frame == f).sum())) for f in (0, 1, 2, -1)), ' / '.join(str(int((kind == k).sum())) for k in range(4))))
    got, g_wall, g_lo, g_hi = median_of(lambda: GS.gene_structures(items, genomes=contigs), 3)
    _, r_wall, _, _ = median_of(lambda: GS.results(items, frame, start_aa, stop_aa, kind), 3)
    GS.close()
    say('  gene_structures wall (columns from the items, contigs to bytes, device, tuples): median %.2f s (min %.2f, max %.2f) over 3 calls = %.2f us per prediction; '
        'of it results() - coordinates, texts, tuples - %.2f s, the library call %.2f s, the rest reading the items into columns'
        % (g_wall, g_lo, g_hi, 1e6 * g_wall / n, r_wall, wall))
    # one thread, a sample of the same items with their windows as strings
    sample = rng.choice(n, min(SAMPLE, n), replace=False)
    with_seq = []
    for k in sample.tolist():
        it = list(items[k])
        w = contigs[it[1][5]][it[5] - 1:it[6]]
        it[2] = w if it[1][11] == '+' else rc(w)
        with_seq.append(it)
    t0 = time.perf_counter()
    mine = [restate(it)[0] for it in with_seq]
    t1 = time.perf_counter()
    theirs = [numpy_form(it) for it in with_seq]
    t2 = time.perf_counter()
    assert mine == [got[k] for k in sample.tolist()], 'the restatement and the device disagree on the sample'
    assert theirs == mine, 'the numpy form and the device disagree on the sample'
    say('  on a SAMPLE of %d of these items, one thread, windows sliced beforehand: the plain-loop restatement %.1f us per prediction, the numpy form (transeq with marked '
        'starts + str.find) %.1f us per prediction; both equal to the device in every tuple of the sample' % (len(sample), 1e6 * (t1 - t0) / len(sample), 1e6 * (t2 - t1) / len(sample)))
    say('  ratio numpy form / gene_structures per prediction: %.0f x; numpy form / Context.gene_structure: %.0f x' % ((t2 - t1) / len(sample) / (g_wall / n), (t2 - t1) / len(sample) / (wall / n)))
    if out_path:
        with open(out_path, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
