#!/usr/bin/env python3
"""Generate tests/golden/g26_gffgenes.json.gz by IMPORTING the reference's Python (build machine only: needs /root/reference).

    python tests/golden/make_golden_gffgenes.py

The shim is make_golden_synteny.py's, imported from there.  Seeded synthetic GFF texts and FASTA gene files go through the reference's iter_readGFF
(PEPPAN.py:117-182), checkPseu (:992-1010) and addGenes (:1013-1021).  Only DATA is written - the file texts, the parameters, and the returned
dictionaries (digests as decimal strings) - none of the reference's source text.  The restatement of tests/gffgenes_helpers.py is run over every case,
and the conditions the fixture is pinned by are asserted at the end.
"""
import gzip, json, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_synteny as SHIMMED    # noqa: E402  (builds the shim, puts the reference on sys.path, changes into the shim's working directory)

PEP = SHIMMED.PEP
np = SHIMMED.np
import gffgenes_helpers as H             # noqa: E402

STOPS = ('TAA', 'TAG', 'TGA')
PROBED = [('ATG', '', 11, 4), ('ATG', 'e', 11, 0), ('GTGAAATGA', '', 11, 0), ('GTGAAATGA', '', 4, 4), ('ATGAAATA', 'f', 11, 0), ('ATGAAA-', 'f', 11, 4),
          ('ATGAAAT-', 'f', 11, 4), ('ATGA-ATAA', '', 11, 0), ('ATG-NATAA', '', 11, 0), ('ATGANATAA', '', 11, 5), ('ATGANATAA', 'i', 11, 0),
          ('TAAAAATAA', 's', 11, 5), ('TAAAAATAA', 'si', 11, 0), ('A', 'f', 11, 3), ('A', 'fs', 11, 0)]


def dna(rng, n):
    return ''.join(rng.choice(list('ACGT'), n).tolist())


def body(rng, n_codons):
    out = []
    while len(out) < n_codons:
        c = dna(rng, 3)
        if c not in STOPS:
            out.append(c)
    return ''.join(out)


def gene(rng, kind):
    start, stop, n = str(rng.choice(['ATG', 'GTG', 'TTG'])), str(rng.choice(['TAA', 'TAG'])), int(rng.integers(12, 80))
    if kind == 'ok':
        return start + body(rng, n) + stop
    if kind == 'short':
        return start + body(rng, 2) + stop
    if kind == 'shift':
        return start + body(rng, n) + 'C' * int(rng.integers(1, 3)) + stop
    if kind == 'nostart':
        return 'CCC' + body(rng, n) + stop
    if kind == 'nostop':
        return start + body(rng, n) + 'CCC'
    if kind == 'inner':
        return start + body(rng, n // 2) + 'TAG' + body(rng, n // 2) + stop
    if kind == 'tga':
        return start + body(rng, n // 2) + 'TGA' + body(rng, n // 2) + 'TAA'
    if kind == 'tga_end':
        return start + body(rng, n) + 'TGA'
    if kind == 'iupac':
        return start + body(rng, n // 2) + 'ARG' + body(rng, n // 2) + stop
    if kind == 'gap':
        return start + body(rng, n // 2) + 'A-G' + body(rng, n // 2) + stop
    raise ValueError(kind)


KINDS = ['ok', 'short', 'shift', 'nostart', 'nostop', 'inner', 'tga', 'tga_end', 'iupac', 'gap', 'ok']


def genome_text(rng, n_contigs=2):
    """contigs with one gene of every kind on both strands, random spacers between them; some lines lower case, blanks inside lines, a comment line inside
    the FASTA part; features of a missing contig, with start = 0, end < start and an end beyond the contig, on both strands"""
    lines, fasta = ['##gff-version 3'], ['##FASTA']
    serial = 0
    for c in range(n_contigs):
        text = dna(rng, int(rng.integers(20, 60)))
        for kind in KINDS:
            for strand in '+-':
                g = gene(rng, kind)
                start = len(text) + 1
                text += g if strand == '+' else H.rc(g).replace('N', '-') if kind == 'gap' else H.rc(g)
                serial += 1
                lines.append('ctg%d\tsynth\tgene\t%d\t%d\t.\t%s\t.\tID=gene%d;locus_tag=L%04d' % (c, start, len(text), strand, serial, serial))
                lines.append('ctg%d\tsynth\tCDS\t%d\t%d\t.\t%s\t0\tID=cds%d;Parent=gene%d;locus_tag=L%04d' % (c, start, len(text), strand, serial, serial, serial))
                text += dna(rng, int(rng.integers(0, 40)))
        for strand in '+-':
            for start, end in ((0, 90), (200, 100), (len(text) - 50, len(text) + 500), (-40, -4)):
                serial += 1
                lines.append('ctg%d\tsynth\tCDS\t%d\t%d\t.\t%s\t0\tID=edge%d' % (c, start, end, strand, serial))
        fasta.append('>ctg%d some description' % c)
        for at in range(0, len(text), 70):
            row = text[at:at + 70]
            if at % 280 == 70:
                row = row.lower()
            if at % 350 == 140:
                row = row[:30] + ' ' + row[30:50] + '\t' + row[50:] + '  '
            fasta.append(row)
            if at == 140:
                fasta.append('# a comment between sequence lines')
    for strand in '+-':
        serial += 1
        lines.append('nowhere\tsynth\tCDS\t10\t99\t.\t%s\t0\tID=lost%d' % (strand, serial))
    return '\n'.join(lines + fasta) + '\n'


def parser_text(rng):
    ctg1, ctg2 = 'ATG' + body(rng, 30) + 'TAA' + dna(rng, 30), dna(rng, 10) + 'GTG' + body(rng, 20) + 'TAG'
    rows = [
        'c1\ts\tgene\t1\t96\t.\t+\t.\tID=g1;Name=fromGene',
        'c1\ts\tCDS\t1\t96\t.\t+\t0\tID=x1;Parent=g1;Name=ownName',                    # Parent resolves in front of Name
        'c1\ts\tCDS\t1\t96\t.\t+\t0\tID=x2;Parent=unknown;Name=byName',                # an unknown Parent: Name
        'c1\ts\tCDS\t1\t96\t.\t+\t0\tID=byId;note=none',                               # ID alone
        'c1\ts\tCDS\t1\t96\t.\t+\t0\tID=x3;old_locus_tag=OLD7;locus_tag=NEW7',         # a substring search: the old tag comes first
        'c1\ts\tCDS\t1\t96\t.\t+\t0\tID=x4;Parent=g1;locus_tag=TAG4;Name=n4',          # locus_tag in front of everything
        'c1\ts\tmRNA\t1\t96\t.\t+\t.\tID=m1;Parent=g1',                                # records m1 -> fromGene
        'c1\ts\tCDS\t4\t96\t.\t+\t0\tID=x5;Parent=m1',
        'c1\ts\texon\t1\t96\t.\t+\t.\tID=e1;Parent=nobody',                            # records e1 -> e1
        'c1\ts\tCDS\t1\t96\t.\t+\t0\tParent=e1',
        'c1\ts\tCDS\t7\t96\t.\t+\t0\tID=again;locus_tag=TAG4',                         # a second line of a name, same contig: ignored
        'c2\ts\tCDS\t11\t76\t.\t+\t0\tID=split;locus_tag=TWO',
        'c2\ts\tCDS\t1\t9\t.\t+\t0\tID=split2;locus_tag=TWO',                          # ... on the same contig
        'c1\ts\tCDS\t1\t96\t.\t+\t0\tID=split3;locus_tag=TWO',                         # ... and on another
        'c2\ts\tCDS\t11\t40\t.\t-\t0\tID=minus1;locus_tag=MINUS',                      # two lines of a '-' gene: the first alone
        'c2\ts\tCDS\t50\t76\t.\t-\t0\tID=minus2;locus_tag=MINUS',
        'short\tline',
        '',
        'c1\ts\tCDS\t1\t96\t.\t.\t0\tID=nostrand',                                     # a strand that is not '-' reads forward
    ]
    return '\n'.join(['##gff-version 3'] + rows + ['##FASTA', '>c1', ctg1[:50], ctg1[50:], '>c2 second', ctg2]) + '\n'


def rows_of(d):
    return [[k, v[:5] + [str(v[5]), v[6]]] for k, v in d.items()]


def run_read(name, entry, gtable, min_cds, incomplete, feature='CDS'):
    PEP.params['min_cds'], PEP.params['incompleteCDS'] = min_cds, incomplete
    case = dict(name=name, entry=entry, feature=feature, gtable=gtable, min_cds=min_cds, incomplete=incomplete, seq=None, cds=None, error=None)
    try:
        seq, cds = PEP.iter_readGFF([entry, feature, gtable])
        case['seq'], case['cds'] = [[k, v] for k, v in seq.items()], rows_of(cds)
    except AssertionError:
        case['error'] = 'AssertionError'
    return case


def run_genes(name, gene_file, gtable, min_cds, incomplete):
    PEP.params['min_cds'], PEP.params['incompleteCDS'] = min_cds, incomplete
    before = {'old:gene': ['old.fna', '', 0, 0, '+', 12345678901234567890123, 'ATGAAATAA']}
    genes, error = {k: list(v) for k, v in before.items()}, None
    try:
        assert PEP.addGenes(genes, gene_file, gtable) is genes
    except IndexError:
        error = 'IndexError'
    return dict(name=name, gene_file=gene_file, gtable=gtable, min_cds=min_cds, incomplete=incomplete, before=rows_of(before), genes=rows_of(genes), error=error)


def pseu(text, incomplete, gtable, min_cds):
    PEP.params['min_cds'], PEP.params['incompleteCDS'] = min_cds, incomplete
    try:
        return [text, incomplete, gtable, min_cds, int(PEP.checkPseu('n', text, gtable))]
    except IndexError:
        return [text, incomplete, gtable, min_cds, 'IndexError']


def main():
    rng = np.random.default_rng(26)
    files = {'synth.gff': genome_text(rng), 'second.v2.gff': genome_text(rng, 1), 'zipped.gff.gz': genome_text(rng, 1), 'names.gff': parser_text(rng)}
    pair = genome_text(rng, 1)
    files['pair.gff'], files['pair.fna'] = pair[:pair.index('##FASTA')], pair[pair.index('##FASTA'):]
    files['twice.gff'] = '##FASTA\n>c1\nACGT\n>c2\nAC\n>c1 again\nGG\n'
    files['nameless.gff'] = 'c1\ts\tgene\t1\t9\t.\t+\t.\tID=g1\nc1\ts\tCDS\t1\t9\t.\t+\t0\tnote=nothing;Parent=g9\n##FASTA\n>c1\nATGAAATAA\n'
    files['extra.fna'] = ('>ok first\nATG' + body(rng, 20) + 'TAA\n>short\nATGAAATAA\n>lower\natg' + body(rng, 12).lower() + 'tag\n# a comment\n>blanks\nGTG' + body(rng, 6)
                          + ' ' + body(rng, 6) + '\n\t' + body(rng, 3) + 'TAA  \n>nostart\nCCC' + body(rng, 15) + 'TAA\n>dup\nATGCCCTAA\n>dup\nTTG' + body(rng, 14) + 'TAG\n')
    files['hollow.fna'] = '>one\nATG' + body(rng, 11) + 'TAA\n>nothing\n>after\nATG' + body(rng, 11) + 'TAA\n'
    os.makedirs('fixture_files', exist_ok=True)
    os.chdir('fixture_files')
    H.write_files(dict(files=files), '.')

    read = []
    for entry in ('synth.gff', 'second.v2.gff'):
        for incomplete, gtable, min_cds in (('', 11, 30), ('sife', 11, 30), ('f', 4, 30), ('', 11, 0), ('se', 11, 120.)):
            read.append(run_read('%s %r %d %r' % (entry, incomplete, gtable, min_cds), entry, gtable, min_cds, incomplete))
    read += [run_read('gz', 'zipped.gff.gz', 11, 30, ''), run_read('pair', 'pair.gff,pair.fna', 11, 30, 'e'), run_read('pair table 4', 'pair.gff,pair.fna', 4, 0, ''),
             run_read('names', 'names.gff', 11, 0, 'sife'), run_read('names by gene', 'names.gff', 11, 30, '', feature='gene'),
             run_read('duplicate contig', 'twice.gff', 11, 30, ''), run_read('nameless feature', 'nameless.gff', 11, 30, '')]
    genes = [run_genes('extra', 'extra.fna', 11, 30, ''), run_genes('extra sife', 'extra.fna', 11, 0, 'sife'), run_genes('two files', 'extra.fna,,hollow.fna', 4, 30, 's'),
             run_genes('hollow', 'hollow.fna,extra.fna', 11, 0, ''), run_genes('none', '', 11, 30, '')]
    designed = ['ATGAAATAA', 'ATGAAATGA', 'CCCAAATAA', 'ATGTAAAAATAG', 'ATGAAACCC', 'ATGAAATA', 'ATGAAATAAC', 'ATGA-ATAA', 'ATGANATAA', 'TAA', 'TGA', 'AT', '-', 'N', '',
                'ATG' + 'AAA' * 70 + 'TAA', 'ATG' + 'AAA' * 62 + 'TGA' + 'AAA' * 3 + 'TAA']
    cases = [pseu(t, m, g, 0) for t in designed for m in H.MASKS for g in (11, 4)]
    cases += [pseu(t, m, g, 0) for t, m, g, _ in PROBED] + [pseu(t, '', 11, k) for t in ('ATGAAATAA', '') for k in (9, 10, 9.5, -1)]
    path = os.path.join(HERE, 'g26_gffgenes.json.gz')
    with gzip.GzipFile(path, 'wb', mtime=0) as f:
        f.write(json.dumps(dict(files=files, read=read, genes=genes, pseu=cases), separators=(',', ':')).encode())

    # ---- what the fixture is pinned by
    fx = H.load()
    for t, m, g, want in PROBED:
        assert [t, m, g, 0, want] in fx['pseu'], (t, m, g)
    assert {frozenset(c[1]) for c in fx['pseu']} == {frozenset(m) for m in H.MASKS} and len(set(H.MASKS)) == 16 and {c[2] for c in fx['pseu']} == {4, 11}
    assert {c[4] for c in fx['pseu']} == {0, 1, 2, 3, 4, 5, 'IndexError'}
    for t, m, g, k, want in fx['pseu']:
        try:
            got = H.check_pseu(t, g, k, m)
        except IndexError:
            got = 'IndexError'
        assert got == want, (t, m, g, k, got, want)
    codes = {'+': set(), '-': set()}
    for c in fx['read']:
        try:
            got = H.read_gff(c['entry'], c['feature'], c['gtable'], c['min_cds'], c['incomplete'])
            assert c['error'] is None and got[0] == c['seq'] and got[1] == c['cds'] and list(got[1]) == list(c['cds']) and list(got[0]) == list(c['seq']), c['name']
            for v in c['cds'].values():
                if v[4] in codes:
                    codes[v[4]].add(min(v[5], 7) if v[6] == '' else 0)
        except AssertionError:
            assert c['error'] == 'AssertionError', c['name']
    assert codes['+'] == codes['-'] == set(range(7)), codes
    assert {c['gtable'] for c in fx['read']} == {4, 11} and [c['name'] for c in fx['read'] if c['error']] == ['duplicate contig', 'nameless feature']
    by = {c['name']: c for c in fx['read']}
    names = by['names']['cds']
    assert list(names) == ['names:' + n for n in ('fromGene', 'byName', 'byId', 'OLD7', 'TAG4', 'e1', 'TWO', 'MINUS', 'nostrand')], list(names)
    assert names['names:TAG4'][2:4] == [1, 96] and names['names:TWO'][1:4] == ['names:c2', 11, 76] and names['names:MINUS'][2:4] == [11, 40]
    assert names['names:fromGene'][2] == 1 and len(names['names:MINUS'][6]) == 30 and names['names:nostrand'][6] == names['names:byId'][6] != ''
    assert list(by['names by gene']['cds']) == ['names:fromGene']
    synth = by["synth.gff '' 11 30"]
    assert any(ch.islower() for ch in fx['files']['synth.gff'].split('##FASTA')[1]) and any(ch in 'R-' for v in synth['seq'].values() for ch in v[1])
    assert '\n# a comment' in fx['files']['synth.gff'].split('##FASTA')[1] and ' ' in fx['files']['synth.gff'].split('>ctg0')[1].split('\n', 1)[1]
    assert all(v[1] == v[1].upper() and ' ' not in v[1] and '#' not in v[1] for v in synth['seq'].values())
    edges = {(v[2], v[3]) for v in synth['cds'].values()}
    assert any(s == 0 for s, e in edges) and any(e < s for s, e in edges) and any(v[3] > len(synth['seq'][v[1]][1]) for v in synth['cds'].values() if v[1] in synth['seq'])
    assert any(v[1] not in synth['seq'] and v[5] == 6 for v in synth['cds'].values())
    assert by['pair']['seq'] and all(v[0] == 'pair.gff' for v in by['pair']['seq'].values()) and any(v[6] for v in by['pair']['cds'].values())
    assert by['gz']['seq'] and any(v[6] for v in by['gz']['cds'].values()) and all(k.startswith('second:') for k in by["second.v2.gff '' 11 30"]['cds'])
    for c in fx['genes']:
        filled, error = dict((k, list(v)) for k, v in c['before'].items()), None
        try:
            H.add_genes(filled, c['gene_file'], c['gtable'], c['min_cds'], c['incomplete'])
        except IndexError:
            error = 'IndexError'
        assert error == c['error'] and filled == c['genes'] and list(filled) == list(c['genes']), c['name']
    assert [c['error'] for c in fx['genes']] == [None, None, None, 'IndexError', None] and 'hollow:one' in fx['genes'][3]['genes'] and 'hollow:after' not in fx['genes'][3]['genes']
    assert 'extra:dup' in fx['genes'][0]['genes'] and fx['genes'][0]['genes']['extra:dup'][6].startswith('TTG')
    print('%s: %d bytes; %d read cases, %d gene-file cases, %d checkPseu cases' % (path, os.path.getsize(path), len(read), len(genes), len(cases)))


if __name__ == '__main__':
    main()
