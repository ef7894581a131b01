"""K24 (the allele pass of write_output: csrc/outalleles.hip, peppan_amd/outalleles.py) measured on one GPU, beside the plain-Python restatement of the same pass.
    python tools/outalleles_rate.py [out.txt] [genomes] [genes]
The table is shaped like write_output's at PEPPAN.py:1390: `genomes` (400) genomes of one contig each carry `genes` (5 000) genes of 870 - 930 nt, 100 nt apart,
half of them on the reverse strand, each one of eight alleles of its gene (the first is the gene's representative); one prediction per gene and genome, in the
order of contig and start - 2 x 10^6 rows.  Reported: the HIP-event time of each K24 launch (pep_set_timing 2), the wall time of Context.out_alleles (the whole
call and the plan alone) with its host prologue timed through out_alleles_check, and the wall time of allele_pass as a whole with its parts - the tables made
from the Python objects, K24, K19 (which is sent the contigs a second time), the dictionary and the texts of columns 13 and 15.  One warm-up call, then the median
of the repeats (5 for the library call, 3 for allele_pass).  Beside it, on the rows of the first genomes (10^5 rows) and one thread: the restatement of
tests/outalleles_helpers.py with tests/genestruct_helpers.py as its determineGeneStructure, asserted equal to allele_pass on those rows in every column and in
the dictionary.  The code measured is named by the parent commit (when git metadata is there) and the SHA-1 of the sources of the stage.  The lines are appended
to the file named (profiles/outalleles_rate.txt is this tool's output).  A tool, not a test."""
import hashlib, os, socket, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
os.environ.setdefault('PEPPAN_LOG', '0')
import numpy as np                                                         # noqa: E402
from peppan_amd import _native as N, outalleles as OA                      # noqa: E402
import outalleles_helpers as H                                             # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
GENOMES = int(sys.argv[2]) if len(sys.argv) > 2 else 400
GENES = int(sys.argv[3]) if len(sys.argv) > 3 else 5000
ALLELES, GAP, SLOT, SAMPLE_ROWS = 8, 100, 1030, 100000
SOURCES = ('peppan_amd/csrc/outalleles.hip', 'peppan_amd/csrc/sha1.h', 'peppan_amd/csrc/sort.hip', 'peppan_amd/csrc/common.h', 'peppan_amd/outalleles.py',
           'peppan_amd/genestruct.py', 'peppan_amd/_native.py')
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


COMPLEMENT = np.full(256, ord('N'), np.uint8)
for a, b in zip(b'ACGT', b'TGCA'):
    COMPLEMENT[a] = b


def make_inputs(rng):
    """-> (table, genomes, encodes, clust_ref)"""
    sense = np.array([[a, b, c] for a in b'ACGT' for b in b'ACGT' for c in b'ACGT' if bytes([a, b, c]) not in (b'TAA', b'TAG', b'TGA', b'ATG', b'GTG', b'TTG')], dtype=np.uint8)
    lengths = 3 * rng.integers(290, 311, GENES)                                # 870 .. 930
    variants = np.zeros((GENES, ALLELES, SLOT - GAP), np.uint8)
    for g in range(GENES):
        codons = int(lengths[g]) // 3
        orf = sense[rng.integers(0, len(sense), codons)].copy()
        orf[0], orf[-1] = np.frombuffer(b'ATG', np.uint8), np.frombuffer(b'TAA', np.uint8)
        for v in range(ALLELES):
            text = orf.copy()
            for k in rng.integers(1, codons - 1, v).tolist():                  # allele v differs from the representative in v codons
                text[k] = sense[int(rng.integers(0, len(sense)))]
            variants[g, v, :3 * codons] = text.reshape(-1)
    encodes, clust_ref, genomes, names = {}, {}, {}, []
    for g in range(GENES):
        names.append('gene%05d' % g)
        encodes[names[g]] = g + 1
        clust_ref[g + 1] = variants[g, 0, :int(lengths[g])].tobytes().decode()
    rows = []
    letters = np.frombuffer(b'ACGT', np.uint8)
    for c in range(GENOMES):
        contig = 'genome%04d' % c
        encodes[contig] = GENES + 1 + c
        block = letters[rng.integers(0, 4, (GENES, SLOT))]
        pick = rng.integers(0, ALLELES, GENES)
        minus = rng.random(GENES) < 0.5
        for g in range(GENES):
            n = int(lengths[g])
            text = variants[g, pick[g], :n]
            block[g, GAP:GAP + n] = COMPLEMENT[text[::-1]] if minus[g] else text
        genomes[GENES + 1 + c] = (contig, block.reshape(-1).tobytes().decode())
        clen = GENES * SLOT
        for g in range(GENES):
            n = int(lengths[g])
            s = g * SLOT + GAP + 1
            rows.append([names[g], 1, len(rows) + 1, contig, '', contig, 99.5, 1, n, s, s + n - 1, '-' if minus[g] else '+', n, clen, [0], 'CDS', ''])
    return rows, genomes, encodes, clust_ref


def median_of(f, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = f()
        times.append(time.perf_counter() - t0)
    return res, float(np.median(times)), min(times), max(times)


def main():
    rng = np.random.default_rng(24)
    t0 = time.perf_counter()
    rows, genomes, encodes, clust_ref = make_inputs(rng)
    table = H.as_object_table(rows)
    n = len(table)
    say('# outalleles_rate on %s, %s' % (socket.gethostname(), code_id()))
    say('%d predictions: %d genes of 870 - 930 nt x %d genomes of one contig of %d nt, %d alleles per gene, strand - for half (inputs made in %.0f s)'
        % (n, GENES, GENOMES, GENES * SLOT, ALLELES, time.perf_counter() - t0))
    T, t_wall, _, _ = median_of(lambda: OA.tables(table, genomes, encodes, clust_ref, 0.8), 1)
    say('  tables (names to indices, integer columns, the arena of %.2f GB): %.2f s' % (len(T.nt) / 1e9, t_wall))
    ctx = OA._context(None)
    args = (T.nt, T.contig_off, T.seed_contig, T.rows)
    ctx.out_alleles(*args)                                                     # warm-up: the buffers grow once
    ctx.set_timing(2)
    plan, first, rank, tflag = ctx.out_alleles(*args)
    ms = ctx.call_times(N.CALL_OUT_ALLELES, total=True)[0]
    ctx.set_timing(0)
    spans = plan[:, 5].astype(np.int64)
    say('  HIP events: plan %.3f ms, digest %.3f ms (%.1f GB/s of allele bytes), classes %.3f ms, comparison %.3f ms, sort %.3f ms, ranks %.3f ms; sum %.3f ms = %.1f million '
        'predictions per second of kernel time' % (ms[0], ms[1], spans.sum() / ms[1] / 1e6, ms[2], ms[3], ms[4], ms[5], sum(ms), n / sum(ms) / 1e3))
    _, wall, lo, hi = median_of(lambda: ctx.out_alleles(*args), 5)
    _, p_wall, _, _ = median_of(lambda: ctx.out_alleles(None, *args[1:], plan_only=True), 5)
    _, c_wall, _, _ = median_of(lambda: N.out_alleles_check(*args[1:]), 5)
    say('  Context.out_alleles wall (%.2f GB of contigs and %d B per row up, %d B per row back): median %.0f ms (min %.0f, max %.0f) over 5 calls; the plan alone: median %.0f ms; '
        'the host prologue alone (out_alleles_check): median %.0f ms' % (len(T.nt) / 1e9, 4 * N.OUTA_COLS, 4 * N.OUTA_PLAN_COLS + 9, 1e3 * wall, 1e3 * lo, 1e3 * hi, 1e3 * p_wall, 1e3 * c_wall))
    say('  classes: %d distinct alleles and %d seeds met again among %d rows; intact %d, fragment %d, structural variation %d'
        % (int((first == np.arange(n)).sum()), int(np.unique(T.rows[first == -1, N.OUTA_GENE]).size), n, int((plan[:, 0] == 2).sum()), int((plan[:, 0] == 1).sum()),
           int((plan[:, 0] == 3).sum())))
    parts_of = []

    def whole():
        work, timing = table.copy(), {}
        alleles = OA.allele_pass(work, genomes, encodes, clust_ref, 0.8, 11, timing=timing)
        parts_of.append(timing)
        print('  (an allele_pass call: %s)' % ', '.join('%s %.1f s' % kv for kv in timing.items()), flush=True)
        return work, alleles

    whole()                                                                    # warm-up of K19's buffers
    (work, alleles), a_wall, a_lo, a_hi = median_of(whole, 3)
    parts = {k: float(np.median([t[k] for t in parts_of[1:]])) for k in parts_of[-1]}
    say('  allele_pass wall: median %.1f s (min %.1f, max %.1f) over 3 calls = %.2f us per prediction; of it tables %.1f s, K24 calls %.1f s (two rounds: the plan alone, then the '
        'whole call), K19 calls with their columns and result tuples %.1f s (the contigs go up a second time there), dictionary and texts %.1f s: Python holds %.0f %% of the call'
        % (a_wall, a_lo, a_hi, 1e6 * a_wall / n, parts['tables'], parts['k24'], parts['k19'], parts['texts'], 100. * (parts['tables'] + parts['texts']) / a_wall))
    OA.close()
    # one thread, the rows of the first genomes
    m = min(n, SAMPLE_ROWS) // GENES * GENES or n
    sample = [list(r) for r in rows[:m]]
    t0 = time.perf_counter()
    r_alleles, _ = H.restate(sample, genomes, encodes, clust_ref, 0.8, 11)
    t1 = time.perf_counter()
    # the same rows alone through allele_pass: equal in every column and in the dictionary
    sub = H.as_object_table(rows[:m])
    s_alleles = OA.allele_pass(sub, genomes, encodes, clust_ref, 0.8, 11)
    OA.close()
    assert [[int(v) if isinstance(v, (int, np.integer)) else v for v in r] for r in sub.tolist()] == sample, 'the restatement and allele_pass disagree on the sample'
    assert [(g, list(a.items())) for g, a in s_alleles.items()] == [(g, list(a.items())) for g, a in r_alleles.items()], 'the dictionaries disagree on the sample'
    say('  on the first %d rows, one thread: the plain-Python restatement (dictionaries of strings, determineGeneStructure restated in loops) %.1f us per prediction; '
        'equal to allele_pass on those rows in every column and in the dictionary' % (m, 1e6 * (t1 - t0) / m))
    say('  ratio restatement / allele_pass per prediction: %.0f x; restatement / Context.out_alleles: %.0f x' % ((t1 - t0) / m / (a_wall / n), (t1 - t0) / m / (wall / n)))
    if out_path:
        with open(out_path, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
