"""The front end of ortho(): the gene dictionary every later stage starts from (PEPPAN.py:1844-1845).

    readGFF(fnames, feature, gtable, params)       PEPPAN.py:117-191    drop-in: (seq, cds), the reference's two dictionaries
    addGenes(genes, gene_file, gtable, params)     PEPPAN.py:1013-1021  drop-in
    read_gff_file(fname, feature, ...)             the host parse of one (possibly comma-joined) file: contigs, and one window per gene
    cds_verdicts(seqs, strands, gtable, ...)       checkPseu (:992-1010) and the digest for callers that hold their own sequences

The reference cuts every CDS out of its contig, reverse-complements it character by character, translates it through numpy arrays per character and
hashes it, one Python round per gene (1.5 s per genome).  Here the host reads the lines and resolves the names; K23 (csrc/cdsgenes.hip,
Context.cds_genes, include/peppan_hip.h) judges every window and digests the kept ones straight from the contig bytes, all files of a batch in one
call; the texts of the kept genes are slices of the contigs made here.  There is no CPU fallback: a missing library or GPU raises PepError.  The context is
orthofilter's cached one (one per process and device; close() releases it).

What the reference does and this reproduces: the FIRST line of a gene name is the gene, every later line of that name is ignored (the elif of :158 is
never true), so a gene is one window contig[start - 1 : end] with Python's slice semantics (start = 0 and end < start give nothing, an end beyond the
contig is clipped); a gene whose contig is missing, or whose window is empty while min_cds <= 0, gets code 6 (:179-180) and is decided here.
The one deviation: a file with a character outside ASCII raises ValueError (str.upper() may change lengths there).
"""
import math
import os
import re
from collections import namedtuple

import numpy as np

from . import _native as N
from .configure import readFasta, uopen
from .orthofilter import _context, close

__all__ = ['readGFF', 'addGenes', 'read_gff_file', 'cds_verdicts', 'close']

GffFile = namedtuple('GffFile', 'fname contigs genes')        # genes: [(name, contig, start, end, strand, (offset, length) or None = code 6)]

_LOCUS, _PARENT, _NAME, _ID = (re.compile(key + r'=([^;]+)') for key in ('locus_tag', 'Parent', 'Name', 'ID'))
_RC = bytes(b'TGCATGCA'[b'ACGTacgt'.index(c)] if c in b'ACGTacgt' else ord('N') for c in range(256))       # rc(): A <-> T, C <-> G, anything else N
DEFAULT_BATCH_BYTES = 256 << 20


def _mask(incompleteCDS):
    return sum(bit for letter, bit in N.CDS_ALLOW.items() if letter in incompleteCDS)


def _min_cds(min_cds):
    """len < min_cds for the integer lengths below 2^31 <=> len < this"""
    return max(0, min(int(math.ceil(min_cds)), N.CDS_MAX_WINDOW))


def _found(pattern, text):
    m = pattern.search(text)
    return m.group(1) if m else None


def read_gff_file(fname, feature='CDS', gtable=11, min_cds=0, incompleteCDS=''):
    """One entry of the reference's file list - `a.gff`, or `a.gff,b.fna` - parsed as :121-165 do -> GffFile(fname, contigs, genes).  fname: the first
    name of the list; contigs: {'prefix:name': upper-cased ASCII bytes} with prefix = basename(fname) up to its first dot; genes: per gene name, in the
    order of their first lines, (name, contig, start, end, strand, window) with window = (0-based offset, length) as slice(start - 1, end).indices gives
    them, or None where the reference ends in its code 6: the contig is missing, or the window is empty and min_cds <= 0."""
    fnames = fname.split(',')
    first = fnames[0]
    prefix = os.path.basename(first).split('.')[0]
    pieces, found, ids = {}, {}, {}
    for fn in fnames:
        with uopen(fn) as fin:
            cur = None
            for line in fin:
                if not line.isascii():
                    raise ValueError('%s: a character outside ASCII' % fn)
                if line.startswith('#'):
                    continue
                if line.startswith('>'):
                    cname = '%s:%s' % (prefix, line[1:].strip().split()[0])
                    if cname in pieces:
                        raise AssertionError('Error: duplicated sequence name %s' % cname.split(':', 1)[1])
                    cur = pieces[cname] = []
                elif cur is not None:
                    cur.extend(line.strip().split())
                else:
                    part = line.strip().split('\t')
                    if len(part) <= 2:
                        continue
                    attr = part[8]
                    name = _found(_LOCUS, attr)
                    if name is None:
                        name = ids.get(_found(_PARENT, attr))
                    if name is None:
                        name = _found(_NAME, attr)
                    if name is None:
                        name = _found(_ID, attr)
                    if part[2] == feature:
                        if name is None:
                            raise AssertionError('Error: CDS has no name. %s' % line)
                        gname = '%s:%s' % (prefix, name)
                        if gname not in found:                                     # the first line of a name is the gene
                            found[gname] = ('%s:%s' % (prefix, part[0]), int(part[3]), int(part[4]), part[6])
                    else:
                        own = _found(_ID, attr)
                        if own is not None:
                            ids[own] = name
    contigs = {cname: ''.join(p).upper().encode('ascii') for cname, p in pieces.items()}
    genes = []
    for gname, (cname, start, end, strand) in found.items():
        window = None
        if cname in contigs:
            lo, hi, _ = slice(start - 1, end).indices(len(contigs[cname]))
            window = (lo, max(0, hi - lo))
            if window[1] == 0 and min_cds <= 0:
                window = None
        genes.append((gname, cname, start, end, strand, window))
    return GffFile(first, contigs, genes)


def _digest_ints(digests):
    """uint8[n, 20] -> n Python ints, by the conversion pipeline.gene_hashes uses"""
    if len(digests) == 0:
        return []
    from .hittable import _pyrows
    digests = np.ascontiguousarray(digests)
    return _pyrows().pep_digest_ints(digests.ctypes.data, len(digests), 20)


def _text(contig, lo, n, rev):
    piece = contig[lo:lo + n]
    return (piece.translate(_RC)[::-1] if rev else piece).decode('ascii')


def _tables(files):
    """the windows of parsed files as Context.cds_genes takes them: (arena, contig_off, contig, win_off, win_len, strand), the genes without a window left out"""
    arena, contig_off, contig, win_off, win_len, strand = [], [0], [], [], [], []
    for f in files:
        index = {}
        for cname, text in f.contigs.items():
            index[cname] = len(arena)
            arena.append(text)
            contig_off.append(contig_off[-1] + len(text))
        for g in f.genes:
            if g[5] is not None:
                contig.append(index[g[1]])
                win_off.append(g[5][0])
                win_len.append(g[5][1])
                strand.append(g[4] == '-')
    return (b''.join(arena), np.array(contig_off, np.uint64), np.array(contig, np.uint32), np.array(win_off, np.uint64), np.array(win_len, np.uint32),
            np.array(strand, np.uint8))


def _batch(files, gtable, min_cds, incompleteCDS, device, seq, cds):
    """the files of one batch: one library call for all their windows, then the two dictionaries' entries in file order"""
    tables = _tables(files)
    code, ints = np.zeros(0, np.uint8), []
    if len(tables[2]):
        code, digest = _context(device).cds_genes(*tables, _min_cds(min_cds), _mask(incompleteCDS), table4=gtable == 4)
        ints = _digest_ints(digest)
    verdict = iter(zip(code.tolist(), ints))
    for f in files:
        for cname, text in f.contigs.items():
            seq[cname] = [f.fname, text.decode('ascii')]
        for gname, cname, start, end, strand, window in f.genes:
            c, h = next(verdict) if window is not None else (6, 0)
            if c:
                cds[gname] = [f.fname, cname, start, end, strand, c, '']
            else:
                cds[gname] = [f.fname, cname, start, end, strand, h, _text(f.contigs[cname], window[0], window[1], strand == '-')]


def readGFF(fnames, feature, gtable, params, device=None, batch_bytes=DEFAULT_BATCH_BYTES):
    """PEPPAN.py:117-191 -> (seq, cds): seq['prefix:contig'] = [file, sequence], cds['prefix:gene'] = [file, 'prefix:contig', start, end, strand,
    the SHA-1 of the sequence as an integer, the sequence] for a kept gene and [.., code 1 - 6, ''] for a dropped one.  params: min_cds and incompleteCDS
    are read.  The files are taken in the order given (the reference's pool returns them in any order; with two files that share a prefix the later one
    counts here).  Files are parsed one after another and sent in batches: a batch is closed in front of the file that would take its contigs beyond
    batch_bytes (default 256 MiB, some fifty bacterial genomes: far below the device's memory, large enough that the call's fixed cost does not show)."""
    if not isinstance(fnames, list):
        fnames = [fnames]
    min_cds, incomplete = params['min_cds'], params['incompleteCDS']
    seq, cds = {}, {}
    files, size = [], 0
    for fn in fnames:
        f = read_gff_file(fn, feature, gtable, min_cds, incomplete)
        n = sum(len(t) for t in f.contigs.values())
        if files and size + n > batch_bytes:
            _batch(files, gtable, min_cds, incomplete, device, seq, cds)
            files, size = [], 0
        files.append(f)
        size += n
    if files:
        _batch(files, gtable, min_cds, incomplete, device, seq, cds)
    return seq, cds


def _upper_ascii(s, k):
    s = s.encode('utf-8') if isinstance(s, str) else bytes(s)
    if not s.isascii():
        raise ValueError('sequence %d: a character outside ASCII' % k)
    return s.upper()


def cds_verdicts(seqs, strands, gtable, min_cds, incompleteCDS, device=None):
    """checkPseu (:992-1010) for sequences the caller holds -> (codes uint8[n], digests uint8[n, 20]).  seqs: str or bytes, upper-cased here as checkPseu
    does; strands[k] '-' (or 1): sequence k is a window of a contig as it stands there and is judged and digested as its reverse complement, anything else:
    as given.  codes: 0 kept, 1 - 5 checkPseu's, 6 for an empty sequence with min_cds <= 0 (where checkPseu raises IndexError); digests:
    hashlib.sha1(text).digest() of the kept, zeros for the others."""
    texts = [_upper_ascii(s, k) for k, s in enumerate(seqs)]
    rev = [s == '-' or s == 1 for s in strands]
    if len(rev) != len(texts):
        raise ValueError('cds_verdicts: one strand per sequence')
    codes, digests = np.full(len(texts), 6, np.uint8), np.zeros((len(texts), 20), np.uint8)
    sent = [k for k, t in enumerate(texts) if len(t) or min_cds > 0]
    if sent:
        lens = [len(texts[k]) for k in sent]
        got = _context(device).cds_genes(b''.join(texts[k] for k in sent), np.concatenate([[0], np.cumsum(lens)]), np.arange(len(sent)), np.zeros(len(sent), np.uint64),
                                         lens, [rev[k] for k in sent], _min_cds(min_cds), _mask(incompleteCDS), table4=gtable == 4)
        codes[sent], digests[sent] = got
    return codes, digests


def addGenes(genes, gene_file, gtable, params, device=None):
    """PEPPAN.py:1013-1021: every record of the (comma-joined) FASTA files that checkPseu keeps becomes genes['prefix:name'] = [file, '', 0, 0, '+',
    digest, sequence]; -> genes.  An empty record with min_cds <= 0 raises IndexError where the reference does: the records in front of it are in genes."""
    min_cds, incomplete = params['min_cds'], params['incompleteCDS']
    for gfile in gene_file.split(','):
        if gfile == '':
            continue
        prefix = os.path.basename(gfile).split('.')[0]
        records = list(readFasta(gfile).items())
        for k, (name, s) in enumerate(records):
            if not s.isascii():
                raise ValueError('%s: a character outside ASCII' % gfile)
        broken = next((k for k, (name, s) in enumerate(records) if not s and min_cds <= 0), None)
        if broken is not None:
            records = records[:broken]
        codes, digests = cds_verdicts([s for name, s in records], ['+'] * len(records), gtable, min_cds, incomplete, device)
        kept = np.flatnonzero(codes == 0)
        for k, h in zip(kept.tolist(), _digest_ints(digests[kept])):
            name, s = records[k]
            genes['%s:%s' % (prefix, name)] = [gfile, '', 0, 0, '+', h, s]
        if broken is not None:
            raise IndexError('string index out of range')
    return genes
