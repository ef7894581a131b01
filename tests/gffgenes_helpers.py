"""K23's rules in plain Python, for the tests: the GFF front end of the reference (iter_readGFF PEPPAN.py:117-182, checkPseu :992-1010, addGenes :1013-1021)
restated from its behaviour, one character and one codon at a time, with nothing of the package under test in it.  The fixture
(tests/golden/g26_gffgenes.json.gz, made by tests/golden/make_golden_gffgenes.py from the reference's own functions) holds the restatement to the reference;
the GPU tests hold the library to the restatement where the fixture has no case.  Everything is integers and text: every comparison is ==."""
import gzip
import hashlib
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'g26_gffgenes.json.gz')
LETTERS = 'sife'
MASKS = [''.join(l for k, l in enumerate(LETTERS) if m >> k & 1) for m in range(16)]
STARTS, STOPS = ('ATG', 'GTG', 'TTG'), ('TAA', 'TAG', 'TGA')
PAIR = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A', 'N': 'N'}


def rc(text):
    return ''.join(PAIR.get(ch, 'N') for ch in reversed(text.upper()))


def marked(text, gtable):
    """the frame-1 translation with marked starts, as far as checkPseu looks at it: M, X, '-' or 'o' per codon; a partial last codon counts"""
    out = []
    for at in range(0, len(text), 3):
        codon = text[at:at + 3]
        if '-' in codon:
            out.append('-')
        elif len(codon) < 3 or any(ch not in 'ACGT' for ch in codon):
            out.append('X')
        elif codon in STARTS:
            out.append('M')
        elif codon in STOPS and not (codon == 'TGA' and gtable == 4):
            out.append('X')
        else:
            out.append('o')
    return ''.join(out)


def check_pseu(text, gtable, min_cds, incomplete):
    """-> 0 .. 5; IndexError where the reference raises it (no codon at all)"""
    if len(text) < min_cds:
        return 1
    if len(text) % 3 and 'f' not in incomplete:
        return 2
    aa = marked(text.upper(), gtable)
    if not aa:
        raise IndexError('no codon')
    if aa[0] != 'M' and 's' not in incomplete:
        return 3
    if aa[-1] != 'X' and 'e' not in incomplete:
        return 4
    if 'X' in aa[:-1] and 'i' not in incomplete:
        return 5
    return 0


def sha1_int(text):
    return int(hashlib.sha1(text.encode('ascii')).hexdigest(), 16)


def attribute(attr, key):
    """the first non-empty value behind `key=` anywhere in the attribute column (a substring search: old_locus_tag= holds locus_tag=), up to the next ';'"""
    at = attr.find(key + '=')
    while at >= 0:
        value = attr[at + len(key) + 1:].split(';')[0]
        if value:
            return value
        at = attr.find(key + '=', at + 1)
    return None


def lines_of(fname):
    if fname.lower().endswith('gz'):
        with gzip.open(fname, 'rt') as fin:
            return fin.readlines()
    with open(fname) as fin:
        return fin.readlines()


def read_gff(entry, feature, gtable, min_cds, incomplete):
    """one entry of the file list -> (seq, cds) as iter_readGFF returns them; AssertionError for a duplicate contig and for a feature without a name"""
    fnames = entry.split(',')
    prefix = os.path.basename(fnames[0]).split('.')[0]
    seq, first_line, ids = {}, {}, {}
    for fn in fnames:
        contig = None
        for line in lines_of(fn):
            if line[:1] == '#':
                continue
            if line[:1] == '>':
                contig = prefix + ':' + line[1:].split()[0]
                assert contig not in seq, 'duplicate contig'
                seq[contig] = [fnames[0], '']
            elif contig is not None:
                seq[contig][1] += ''.join(line.split()).upper()
            else:
                cols = line.strip().split('\t')
                if len(cols) < 3:
                    continue
                name = attribute(cols[8], 'locus_tag')
                if name is None and attribute(cols[8], 'Parent') in ids:
                    name = ids[attribute(cols[8], 'Parent')]
                if name is None:
                    name = attribute(cols[8], 'Name')
                if name is None:
                    name = attribute(cols[8], 'ID')
                if cols[2] == feature:
                    assert name is not None, 'feature without a name'
                    first_line.setdefault(prefix + ':' + name, [fnames[0], prefix + ':' + cols[0], int(cols[3]), int(cols[4]), cols[6]])
                elif attribute(cols[8], 'ID') is not None:
                    ids[attribute(cols[8], 'ID')] = name
    cds = {}
    for gene, (fname, contig, start, end, strand) in first_line.items():
        code, text = 6, ''
        if contig in seq:
            text = seq[contig][1][start - 1:end]
            if strand == '-':
                text = rc(text)
            try:
                code = check_pseu(text, gtable, min_cds, incomplete)
            except IndexError:
                code = 6
        cds[gene] = [fname, contig, start, end, strand, code, ''] if code else [fname, contig, start, end, strand, sha1_int(text), text]
    return seq, cds


def fasta_records(fname):
    records, name = {}, None
    for line in lines_of(fname):
        if line[:1] == '>':
            name = line[1:].split()[0]
            records[name] = ''
        elif line[:1] != '#':
            records[name] += ''.join(line.split()).upper()
    return records


def add_genes(genes, gene_file, gtable, min_cds, incomplete):
    """addGenes (:1013-1021); IndexError escapes with the records in front of it already in genes"""
    for gfile in gene_file.split(','):
        if not gfile:
            continue
        prefix = os.path.basename(gfile).split('.')[0]
        for name, text in fasta_records(gfile).items():
            if not check_pseu(text, gtable, min_cds, incomplete):
                genes[prefix + ':' + name] = [gfile, '', 0, 0, '+', sha1_int(text), text]
    return genes


# ---- the fixture
def load():
    with gzip.open(GOLDEN, 'rt') as fin:
        fx = json.load(fin)
    for case in fx['read'] + fx['genes']:
        for rows in ('cds', 'genes', 'before'):
            if case.get(rows) is not None:
                case[rows] = {k: v[:5] + [int(v[5]), v[6]] for k, v in case[rows]}
        if case.get('seq') is not None:
            case['seq'] = dict(case['seq'])
    return fx


def write_files(fx, where):
    """the fixture's files under `where` (the recorded names are relative: run with `where` as the working directory)"""
    for name, text in fx['files'].items():
        path = os.path.join(where, name)
        if name.endswith('.gz'):
            with gzip.open(path, 'wt') as out:
                out.write(text)
        else:
            with open(path, 'w', newline='') as out:
                out.write(text)
