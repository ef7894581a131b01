"""K23 (the GFF front end: csrc/cdsgenes.hip, peppan_amd/gffgenes.py) measured on one GPU, and the reference's iter_readGFF on the same files on a CPU.
    python tools/gffgenes_rate.py [out.txt] [genomes]                on a machine with a GPU
    python tools/gffgenes_rate.py [out.txt] [genomes] reference      where the reference checkout of the golden generators is (no GPU needed)
A seeded synthetic genome set: per genome 5 contigs of 1 Mb carrying about 5 000 genes back to back (an open reading frame of 200 to 400 codons, half of
them on the reverse strand, 4 % without a stop, with an inner stop or out of frame), written as GFF3 with its FASTA part in lines of 70.  The default, 8
genomes = 40 Mb and 40 000 CDS, runs in well under a minute.
GPU mode reports the HIP-event time of each launch (pep_set_timing 2), the wall time of Context.cds_genes for the whole set in one call, of readGFF as a
whole and of the host parse alone (read_gff_file over the files); one warm-up, then the median of 5 (3 for readGFF).  Reference mode imports the
reference's Python under the shim of tests/golden/make_golden_synteny.py, times PEPPAN.iter_readGFF file by file on one core of THIS machine's CPU and says
so in its line; BASELINE.md's 1.5 s per example genome is the same function on real annotations.  The same seed gives the same files in both modes (their
SHA-1 is printed).  The code measured is named by the parent commit (when git metadata is there) and the SHA-1 of the sources of the stage.  The lines are
appended to the file named (profiles/gffgenes_rate.txt is this tool's output).  A tool, not a test."""
import hashlib, os, socket, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
os.environ.setdefault('PEPPAN_LOG', '0')
import numpy as np                                                         # noqa: E402

args = [a for a in sys.argv[1:] if a != 'reference']
REFERENCE = 'reference' in sys.argv[1:]
out_path = os.path.abspath(args[0]) if args else None
GENOMES = int(args[1]) if len(args) > 1 else 8
CONTIGS, CONTIG_LEN = 5, 1000000
PARAMS = dict(min_cds=120., incompleteCDS='')
SOURCES = ('peppan_amd/csrc/cdsgenes.hip', 'peppan_amd/csrc/codonclass.h', 'peppan_amd/csrc/sha1.h', 'peppan_amd/csrc/common.h', 'peppan_amd/gffgenes.py',
           'peppan_amd/_native.py')
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
COMPLEMENT[[ord(c) for c in 'ACGT']] = [ord(c) for c in 'TGCA']


def genome_text(rng, g):
    sense = np.array([[a, b, c] for a in b'ACGT' for b in b'ACGT' for c in b'ACGT' if bytes([a, b, c]) not in (b'TAA', b'TAG', b'TGA')], dtype=np.uint8)
    rows, fasta, n_genes = ['##gff-version 3'], ['##FASTA'], 0
    for c in range(CONTIGS):
        seq = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, CONTIG_LEN)].copy()
        at = 200
        while at + 1400 < CONTIG_LEN:
            codons = int(rng.integers(200, 401))
            orf = sense[rng.integers(0, len(sense), codons)].copy()
            orf[0] = np.frombuffer((b'ATG', b'ATG', b'GTG', b'TTG')[int(rng.integers(0, 4))], dtype=np.uint8)
            orf[-1] = np.frombuffer((b'TAA', b'TAG', b'TGA')[int(rng.integers(0, 3))], dtype=np.uint8)
            flaw = rng.random()
            if flaw < 0.015:
                orf[-1] = sense[5]
            elif flaw < 0.03:
                orf[codons // 2] = np.frombuffer(b'TAA', dtype=np.uint8)
            gene = orf.reshape(-1)[:-1] if 0.03 <= flaw < 0.04 else orf.reshape(-1)
            strand = '+-'[int(rng.integers(0, 2))]
            if strand == '-':
                gene = COMPLEMENT[gene][::-1]
            seq[at:at + len(gene)] = gene
            n_genes += 1
            rows.append('contig%d\tsynth\tgene\t%d\t%d\t.\t%s\t.\tID=gene_%05d;locus_tag=G%d_%05d' % (c, at + 1, at + len(gene), strand, n_genes, g, n_genes))
            rows.append('contig%d\tsynth\tCDS\t%d\t%d\t.\t%s\t0\tID=cds_%05d;Parent=gene_%05d;locus_tag=G%d_%05d;product=hypothetical protein'
                        % (c, at + 1, at + len(gene), strand, n_genes, n_genes, g, n_genes))
            at += len(gene) + int(rng.integers(20, 120))
        text = seq.tobytes().decode()
        fasta.append('>contig%d' % c)
        fasta += [text[k:k + 70] for k in range(0, len(text), 70)]
    return '\n'.join(rows + fasta) + '\n', n_genes


def median_of(f, repeats):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = f()
        times.append(time.perf_counter() - t0)
    return res, float(np.median(times)), min(times), max(times)


def main():
    rng = np.random.default_rng(23)
    where = tempfile.mkdtemp(prefix='gffgenes_rate_')
    files, n_genes, digest = [], 0, hashlib.sha1()
    for g in range(GENOMES):
        text, n = genome_text(rng, g)
        files.append(os.path.join(where, 'genome%03d.gff' % g))
        with open(files[-1], 'w') as out:
            out.write(text)
        digest.update(text.encode())
        n_genes += n
    size = sum(os.path.getsize(f) for f in files)
    say('# gffgenes_rate%s on %s, %s' % (' (reference mode)' if REFERENCE else '', socket.gethostname(), code_id()))
    say('%d genomes of %d contigs of %d nt, %d CDS (%.0f per genome), %.1f MB of GFF text, sha1 of the files %s; min_cds %g, incompleteCDS %r, table 11'
        % (GENOMES, CONTIGS, CONTIG_LEN, n_genes, n_genes / GENOMES, size / 1e6, digest.hexdigest()[:12], PARAMS['min_cds'], PARAMS['incompleteCDS']))
    if REFERENCE:
        sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
        import make_golden_synteny as shimmed                                  # the shim: stub packages and tools, the reference on sys.path
        PEP = shimmed.PEP
        PEP.params.update(PARAMS)
        times, kept = [], 0
        for f in files:
            t0 = time.perf_counter()
            seq, cds = PEP.iter_readGFF([f, 'CDS', 11])
            times.append(time.perf_counter() - t0)
            kept += sum(1 for v in cds.values() if v[6])
        say('  the reference\'s iter_readGFF, one file after another on ONE CORE OF THIS MACHINE\'S CPU (the build machine, not the GPU machine): median %.2f s per genome '
            '(min %.2f, max %.2f), %.1f s for the set = %.0f us per CDS; %d of %d CDS kept.  BASELINE.md: 1.5 s per example genome (6.0 s for four, 20 915 CDS)'
            % (float(np.median(times)), min(times), max(times), sum(times), 1e6 * sum(times) / n_genes, kept, n_genes))
    else:
        from peppan_amd import _native as N, gffgenes as GG
        parsed, p_wall, p_lo, p_hi = median_of(lambda: [GG.read_gff_file(f, 'CDS', 11, **PARAMS) for f in files], 3)
        say('  host parse alone (read_gff_file over the files: lines, names, contigs to upper-cased bytes, windows): median %.2f s (min %.2f, max %.2f) = %.3f s per genome'
            % (p_wall, p_lo, p_hi, p_wall / GENOMES))
        tables = GG._tables(parsed)
        call = lambda ctx: ctx.cds_genes(*tables, GG._min_cds(PARAMS['min_cds']), GG._mask(PARAMS['incompleteCDS']))
        with N.Context(0) as ctx:
            call(ctx)                                                              # warm-up: the buffers grow once
            ctx.set_timing(2)
            code, _ = call(ctx)
            ms = ctx.call_times(N.CALL_CDS_GENES, total=True)[0]
            ctx.set_timing(0)
            nt = int(tables[4].sum())
            kept_nt = int(tables[4][code == 0].sum())
            say('  HIP events: cds_verdict %.3f ms = %.0f million CDS per second, %.1f GB/s of window bytes; cds_digest %.3f ms for the %d kept = %.1f GB/s of hashed bytes'
                % (ms[0], len(code) / ms[0] / 1e3, nt / ms[0] / 1e6, ms[1], int((code == 0).sum()), kept_nt / ms[1] / 1e6))
            _, wall, lo, hi = median_of(lambda: call(ctx), 5)
            say('  Context.cds_genes wall, the whole set in one call (%.1f MB of contigs and %d windows up, 21 B per CDS back): median %.1f ms (min %.1f, max %.1f)'
                % (len(tables[0]) / 1e6, len(code), 1e3 * wall, 1e3 * lo, 1e3 * hi))
            say('  the CDS go to cds_digest in file order, not sorted by length: that launch is %.0f %% of the call' % (100 * ms[1] / (1e3 * wall)))
            say('  codes 0 .. 5: %s' % ' / '.join(str(int((code == k).sum())) for k in range(6)))
        (seq, cds), r_wall, r_lo, r_hi = median_of(lambda: GG.readGFF(files, 'CDS', 11, PARAMS), 3)
        GG.close()
        say('  readGFF as a whole (parse, one library call, texts and records of %d genes): median %.2f s (min %.2f, max %.2f) = %.3f s per genome, %.1f us per CDS; '
            'of it the host parse %.0f %%, the library call %.0f %%' % (len(cds), r_wall, r_lo, r_hi, r_wall / GENOMES, 1e6 * r_wall / n_genes, 100 * p_wall / r_wall, 100 * wall / r_wall))
    for f in files:
        os.remove(f)
    os.rmdir(where)
    if out_path:
        with open(out_path, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
