"""The per-prediction step of write_output: `determineGeneStructure` (PEPPAN.py:1193-1229, called at :1468 through pool2.imap_unordered), which
translates the window around every intact prediction in up to three frames and looks for its start and stop codon.

    determine_gene_structure    PEPPAN.py:1193-1229   drop-in for one item
    gene_structures             the same for a list of items, one GPU call per translation table

The reference builds numpy arrays per character and a Python string per frame (transeq with markStarts), then runs a handful of find / rfind
calls - one Python call per prediction, and predictions number genes x genomes.  K19 (csrc/genestruct.hip, Context.gene_structure) classifies
the codons of every tried frame on the device and carries the search as a small forward-only state, one wavefront per prediction, integers
only; it returns the frame that gave a CDS with its start and stop codon, or the outcome of the first tried frame.  Coordinates and texts -
the one float is the percentage in a text, formatted by the reference's own expression - are made here.  There is no CPU fallback: a missing
library or GPU raises PepError.  The context is orthofilter's cached one (one per process and device; close() releases it).
"""
import numpy as np

from . import _native as N
from .orthofilter import _context, close

__all__ = ['determine_gene_structure', 'gene_structures', 'close']

_FRAME_LISTS = {(0,): 2, (1,): 4, (2,): 8, (0, 1): 6, (0, 2): 10, (1, 2): 12, (0, 1, 2): 14}      # pred[14] -> bits 1-3 of the flag byte


def _frame_bits(frames, k):
    bits = _FRAME_LISTS.get(tuple(int(f) for f in frames))
    if bits is None:
        raise ValueError('item %d: the tried frames must be an ascending non-empty subset of 0, 1, 2, not %r' % (k, list(frames)))
    return bits


def _as_bytes(seq):
    """a sequence as ASCII bytes, one byte per character (a character outside ASCII becomes '?', which translates to X as it does in the reference)"""
    return seq if isinstance(seq, (bytes, bytearray)) else seq.encode('ascii', 'replace')


def results(items, frame, start_aa, stop_aa, kind):
    """What determineGeneStructure returns for `items`, from the four arrays Context.gene_structure gave for them -> [(pid, cds, start, stop)].
    A frame that gave a CDS: its codons as genome coordinates (:1219-1222).  None: (s, e) and the text of the FIRST tried frame - nostart, nostop,
    premature_stop:..% - when the last tried frame is 0, else frameshift, or frameshift:..% for a premature first frame (:1225-1228)."""
    out = []
    for item, f, a, z, k in zip(items, frame.tolist(), start_aa.tolist(), stop_aa.tolist(), kind.tolist()):
        pid, pred, _, s, e, s2, e2 = item[:7]
        if f >= 0:
            if pred[11] == '+':
                out.append((pid, 'CDS', s2 + a * 3 + f, s2 + z * 3 + 2 + f))
            else:
                out.append((pid, 'CDS', e2 - z * 3 - 2 - f, e2 - a * 3 - f))
            continue
        if k == 0:
            raise ValueError('item %r: a first tried frame that is a CDS cannot come without its frame' % (pid,))
        cds = N.GENESTRUCT_KINDS[k]
        if k == 3:
            cds = 'premature_stop:{0:.2f}%'.format((z - a + 1) * 300 / pred[12])
        if pred[14][-1] > 0:
            cds = cds.replace('premature_stop', 'frameshift') if k == 3 else 'frameshift'
        out.append((pid, cds, s, e))
    return out


def gene_structures(items, genomes=None, contig_key=None, device=None):
    """determineGeneStructure for a list of the reference's toRun entries [pid, pred, seq, s, e, s2, e2, lp, allowed_vary, gtable] (:1465); of pred
    the strand pred[11], the reference length pred[12] and the tried frames pred[14] are read.  -> [(pid, cds, start, stop)] in the order of items.
    genomes is None: the window of an item is its own seq (already reverse-complemented for '-', as :1449 leaves it).
    genomes given (key -> sequence, str or bytes): the window is [s2 - 1, e2) of genomes[key], read backward and complemented on the device for '-';
    seq is not read and may be None.  The key is pred[5], or contig_key[pred[5]] / contig_key(pred[5]) when contig_key is given (write_output:
    genomes={k: v[1] for k, v in genomes.items()}, contig_key=encodes).  Items of table 4 and of the other tables go in one library call each."""
    items = list(items)
    n = len(items)
    if n == 0:
        return []
    flags = np.array([_frame_bits(it[1][14], k) for k, it in enumerate(items)], dtype=np.uint8)
    columns = []
    for name, values in (('lp', [it[7] for it in items]), ('allowed_vary', [it[8] for it in items]), ('ref_len', [it[1][12] for it in items])):
        col = np.array(values)
        if col.dtype.kind not in 'iu' or (col < 0).any() or (col >= 1 << 32).any():
            raise ValueError('%s must be integers in [0, 2^32)' % name)
        columns.append(col.astype(np.uint32))
    if (columns[2] == 0).any():
        raise ValueError('item %d: pred[12] is 0' % int(np.flatnonzero(columns[2] == 0)[0]))
    table4 = np.array([it[9] == 4 for it in items], dtype=bool)
    if genomes is None:
        seqs = [_as_bytes(it[2]) for it in items]
        win_len = np.array([len(s) for s in seqs], dtype=np.int64)
        seq_index = np.arange(n, dtype=np.int64)
        win_off = np.zeros(n, dtype=np.int64)
    else:
        keys = [it[1][5] for it in items]
        if contig_key is not None:
            keys = [contig_key(k) for k in keys] if callable(contig_key) else [contig_key[k] for k in keys]
        index = {}
        seq_index = np.array([index.setdefault(k, len(index)) for k in keys], dtype=np.int64)
        seqs = [_as_bytes(genomes[k]) for k in index]
        win_off = np.array([it[5] for it in items], dtype=np.int64) - 1
        win_len = np.array([it[6] for it in items], dtype=np.int64) - win_off
        flags |= np.array([it[1][11] != '+' for it in items], dtype=np.uint8)
        if (win_off < 0).any() or (win_len < 0).any():
            raise ValueError('item %d: [s2 - 1, e2) is no window' % int(np.flatnonzero((win_off < 0) | (win_len < 0))[0]))
    if (win_len >= N.GENESTRUCT_MAX_WINDOW).any():
        raise ValueError('item %d: a window of 2^31 nucleotides or more' % int(np.flatnonzero(win_len >= N.GENESTRUCT_MAX_WINDOW)[0]))
    frame, kind = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    start_aa, stop_aa = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    ctx = _context(device)
    for t4 in (False, True):
        part = np.flatnonzero(table4 == t4)
        if not len(part):
            continue
        if genomes is None:
            nt = b''.join([seqs[k] for k in part]) if len(part) < n else b''.join(seqs)
            seq_off = np.concatenate([[0], np.cumsum(win_len[part])])
            which = np.arange(len(part))
        else:
            used, which = np.unique(seq_index[part], return_inverse=True)
            nt = b''.join([seqs[k] for k in used])
            seq_off = np.concatenate([[0], np.cumsum([len(seqs[k]) for k in used])])
        got = ctx.gene_structure(nt, seq_off, which, win_off[part], win_len[part], flags[part], columns[0][part], columns[1][part], columns[2][part], table4=t4)
        frame[part], start_aa[part], stop_aa[part], kind[part] = got
    return results(items, frame, start_aa, stop_aa, kind)


def determine_gene_structure(data, device=None):
    """PEPPAN.py:1193-1229 on the GPU: data = [pid, pred, seq, s, e, s2, e2, lp, allowed_vary, gtable] -> (pid, cds, start, stop)"""
    return gene_structures([data], device=device)[0]
