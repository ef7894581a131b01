"""The allele pass of write_output (PEPPAN.py:1391-1472): for every prediction the reference cuts the predicted region out of its contig, reverse-complements
it character by character on '-', uses the string as a dictionary key to number the alleles of its gene, works out the window determineGeneStructure is
to look at and, in batches of 10 000 rows, writes that function's results back into the table.

    allele_pass     PEPPAN.py:1391-1472   drop-in: mutates the prediction table as the reference does, returns the alleles dictionary
    allele_ids      the array-level call under it: plan, class first rows, ranks and 't' flags for plain arrays
    tables          the prediction table and its dictionaries as those arrays

K24 (csrc/outalleles.hip, Context.out_alleles, include/peppan_hip.h) plans every row, digests every allele in place, groups equal ones, compares
their bytes and ranks the classes of every gene on the device; K19 (Context.gene_structure) judges the windows.  What stays here: names to indices, the
reference's float expressions (float64, evaluated once per distinct value), one slice per DISTINCT allele for the dictionary, and the texts of columns 13 and
15, made by the reference's own format expressions in a Python loop over the rows.

The reference's write-back after every batch shows through in one place only: a '-' row at the head of a batch looks back at rows whose column 9 is already
updated.  So a table of more than one batch takes two rounds - the plan alone and K19 for every row but those heads, then the whole K24 call with the updated
column 9 and K19 for the heads - instead of one launch per 10 000 rows.  There is no CPU fallback: a missing library or GPU raises PepError.  The context
is orthofilter's cached one (one per process and device; close() releases it).
"""
import math

import numpy as np

from . import _native as N
from .genestruct import _frame_bits, results as _structure_results
from .orthofilter import _context, close

__all__ = ['allele_pass', 'allele_ids', 'tables', 'close']


class _Complement(dict):
    def __missing__(self, key):
        return 'N'


_RC = _Complement({ord(a): b for a, b in zip('ATGCN', 'TACGN')})


def rc(seq):
    """modules/configure.py:152-154 without the per-character join"""
    return seq.upper()[::-1].translate(_RC)


def _ascii(seq, what):
    """a sequence as bytes, one per character: the device compares bytes where the reference compares characters, so anything else is refused"""
    if isinstance(seq, (bytes, bytearray)):
        return bytes(seq)
    try:
        return seq.encode('ascii')
    except UnicodeEncodeError:
        raise ValueError('%s holds a character outside ASCII' % what)


def _int_column(prediction, k, misc):
    col = np.array(prediction[:, k].tolist())
    if col.dtype.kind not in 'iu':                                   # (a misc_feature row may hold anything: the reference never reads its numbers)
        col = np.array([0 if m else v for v, m in zip(prediction[:, k].tolist(), misc.tolist())])
        if col.dtype.kind not in 'iu':
            raise ValueError('column %d of the prediction table must hold integers' % k)
    return col.astype(np.int64)


class Tables(object):
    """what `tables` made: nt, contig_off, seed_contig, rows for Context.out_alleles; gene_names, seeds and seeded (the alleles dictionary's keys in order, the
    representative each starts with or None, and whether it has one); contig_seqs (the contigs as given, None where no row reads one); no_key (per row: the name whose look-up at :1461
    raises KeyError, or None); sv_ref (per row: the representative's length of :1461-1462, 0 for none)"""


def tables(prediction, genomes, encodes, clust_ref, pseudogene):
    """the object table as it stands at PEPPAN.py:1390 and the dictionaries write_output was given -> Tables"""
    n = len(prediction)
    T = Tables()
    names, kinds, contigs = prediction[:, 0].tolist(), prediction[:, 15].tolist(), prediction[:, 5].tolist()
    misc = np.array([k == 'misc_feature' for k in kinds], dtype=bool)
    noname = np.array([g == '' for g in names], dtype=bool)
    skipped = misc | noname
    rows = np.zeros((n, N.OUTA_COLS), np.int64)
    # ---- the allele sets of :1391-1398, in order of first appearance ('' too, as the reference does)
    gene_index = {}
    rows[:, N.OUTA_GENE] = [0 if m else gene_index.setdefault(g, len(gene_index)) for g, m in zip(names, misc.tolist())]
    T.gene_names = list(gene_index)
    seeds = [clust_ref[encodes[g]] if g in encodes and encodes[g] in clust_ref else None for g in T.gene_names]
    T.seeded = [s is not None for s in seeds]
    T.seeds = seeds
    # ---- contigs: one index per name; the bytes of those a row that is not skipped reads
    contig_index = {}
    rows[:, N.OUTA_CONTIG] = [contig_index.setdefault(c, len(contig_index)) for c in contigs]
    read = np.zeros(len(contig_index), bool)
    read[rows[~skipped, N.OUTA_CONTIG]] = True
    T.contig_seqs = [genomes[encodes[c]][1] if read[k] else None for c, k in contig_index.items()]
    parts = [_ascii(s, 'contig %r' % c) if s is not None else b'' for c, s in zip(contig_index, T.contig_seqs)]
    seed_contig = np.full(len(seeds), -1, np.int64)
    for g, s in enumerate(seeds):
        if s is not None:
            seed_contig[g] = len(parts)
            parts.append(_ascii(s, 'the representative of %r' % T.gene_names[g]))
    T.nt = b''.join(parts)
    T.contig_off = np.concatenate([[0], np.cumsum([len(p) for p in parts], dtype=np.uint64)]).astype(np.uint64)
    T.seed_contig = seed_contig
    # ---- the integer columns
    strands, second = prediction[:, 11].tolist(), prediction[:, 4].tolist()
    rows[:, N.OUTA_FLAGS] = misc * N.OUTA_MISC + noname * N.OUTA_NONAME + np.array([bool(x) for x in second], dtype=bool) * N.OUTA_SECONDARY + \
        np.array([x != '+' for x in strands], dtype=bool) * N.OUTA_MINUS
    for col, k in ((N.OUTA_S, 9), (N.OUTA_E, 10), (N.OUTA_PART, 1), (N.OUTA_QS, 7), (N.OUTA_QE, 8), (N.OUTA_REFLEN, 12), (N.OUTA_CLEN, 13)):
        rows[:, col] = _int_column(prediction, k, misc)
    rows[misc, N.OUTA_S:] = 0                                          # (a row without a name is still somebody's neighbour: its columns 9 and 10 are read)
    # ---- the two float expressions, in float64, once per distinct value
    vary = {int(v): int(int(v) * (1 - pseudogene) + 0.01) for v in np.unique(rows[~skipped, N.OUTA_REFLEN]).tolist()}                   # :1408
    rows[~skipped, N.OUTA_VARY] = [vary[v] for v in rows[~skipped, N.OUTA_REFLEN].tolist()]
    sv = {}
    for g in T.gene_names:
        p = g.rsplit('/', 2)[0]                                       # :1460
        if p not in encodes:
            sv[g] = (0, 0, p)
        elif encodes[p] in clust_ref:                                 # len(seq2) < pseudogene * len(ref)  <=>  len(seq2) < ceil(pseudogene * len(ref))
            ref_len = len(clust_ref[encodes[p]])
            sv[g] = (min(max(int(math.ceil(pseudogene * ref_len)), 0), 2 ** 31 - 1), ref_len, None)
        else:
            sv[g] = (0, 0, None)
    per_row = [sv[g] if not sk else (0, 0, None) for g, sk in zip(names, skipped.tolist())]
    rows[:, N.OUTA_SVMIN] = [x[0] for x in per_row]
    T.sv_ref = [x[1] for x in per_row]
    T.no_key = [x[2] for x in per_row]
    T.rows = rows
    return T


def allele_ids(nt, contig_off, seed_contig, rows, look9=None, key_bits=0, plan_only=False, device=None):
    """K24 for plain arrays, as include/peppan_hip.h states it (Context.out_alleles names the arguments)
    -> (plan int32[n, 6]: class, s2, e2, lp, a, len; first int32[n]: the first row of the row's class, -1 the seed, -2 a skipped row; rank uint32[n];
    tflag uint8[n]); with plan_only the plan and three None"""
    return _context(device).out_alleles(nt, contig_off, seed_contig, rows, look9=look9, plan_only=plan_only, key_bits=key_bits)


def _structures(ctx, T, prediction, plan, which, gtable):
    """determineGeneStructure (K19) for the rows `which` of the table, their windows taken from the plan -> [(pid, cds, start, stop)]"""
    if not len(which):
        return []
    rows = T.rows[which]
    flags = np.array([_frame_bits(prediction[i][14], i) for i in which.tolist()], dtype=np.uint8) | ((rows[:, N.OUTA_FLAGS] & N.OUTA_MINUS) != 0).astype(np.uint8)
    s2, e2, lp = plan[which, 1].astype(np.int64), plan[which, 2].astype(np.int64), plan[which, 3]
    got = ctx.gene_structure(T.nt, T.contig_off, rows[:, N.OUTA_CONTIG], s2 - 1, e2 - s2 + 1, flags, lp, rows[:, N.OUTA_VARY], rows[:, N.OUTA_REFLEN], table4=gtable == 4)
    items = [(i, prediction[i], None, s, e, a, b) for i, s, e, a, b in zip(which.tolist(), rows[:, N.OUTA_S].tolist(), rows[:, N.OUTA_E].tolist(), s2.tolist(), e2.tolist())]
    return _structure_results(items, *got)


def allele_pass(prediction, genomes, encodes, clust_ref, pseudogene, gtable, device=None, timing=None):
    """PEPPAN.py:1391-1472 on the GPU.  prediction: the 17-column object table as it stands at :1390, in that row order; it is mutated as the reference
    mutates it (columns 9, 10, 13 and 15).  -> alleles, the reference's dict of dicts gene -> {sequence: id}, both levels in its insertion order.
    A KeyError of the reference (:1461, a name without its '/n' suffix that `encodes` lacks) is raised before anything is written; a row the library
    refuses (include/peppan_hip.h lists them) raises PepError naming it.  timing (optional dict): receives the seconds spent in 'tables', 'k24',
    'k19' and 'texts'."""
    import time
    clock = [time.perf_counter()]

    def lap(name):
        now = time.perf_counter()
        if timing is not None:
            timing[name] = timing.get(name, 0.) + now - clock[0]
        clock[0] = now

    n = len(prediction)
    if n == 0:
        return {}
    T = tables(prediction, genomes, encodes, clust_ref, pseudogene)
    lap('tables')
    ctx = _context(device)
    rows = T.rows
    index = np.arange(n)
    heads = (index >= N.OUTA_BATCH) & (index % N.OUTA_BATCH < 5) & ((rows[:, N.OUTA_FLAGS] & N.OUTA_MINUS) != 0)
    two_rounds = bool(heads.any())
    # round 1: every row but the heads, none of which sees an updated neighbour
    if two_rounds:
        plan = ctx.out_alleles(None, T.contig_off, T.seed_contig, rows, plan_only=True)[0]
    else:
        plan, first, rank, tflag = ctx.out_alleles(T.nt, T.contig_off, T.seed_contig, rows)
    intact = np.isin(plan[:, 0], (N.OUTA_INTACT, N.OUTA_STRUCTVAR))
    missing = np.flatnonzero(intact & np.array([k is not None for k in T.no_key], dtype=bool) & ~heads)
    if len(missing):
        raise KeyError(T.no_key[int(missing[0])])
    lap('k24')
    done = _structures(ctx, T, prediction, plan, np.flatnonzero((plan[:, 0] == N.OUTA_INTACT) & ~heads), gtable)
    lap('k19')
    if two_rounds:
        # round 2: the heads look back at column 9 as round 1 left it; the numbering takes every row in its place
        look9 = rows[:, N.OUTA_S].copy()
        for pid, cds, start, stop in done:
            look9[pid] = start
        plan, first, rank, tflag = ctx.out_alleles(T.nt, T.contig_off, T.seed_contig, rows, look9=look9)
        late = np.flatnonzero(heads & np.isin(plan[:, 0], (N.OUTA_INTACT, N.OUTA_STRUCTVAR)))
        for i in late.tolist():
            if T.no_key[i] is not None:
                raise KeyError(T.no_key[i])
        lap('k24')
        done += _structures(ctx, T, prediction, plan, np.flatnonzero(heads & (plan[:, 0] == N.OUTA_INTACT)), gtable)
        lap('k19')
    # ---- the dictionary: one slice per distinct allele, in the reference's insertion order
    alleles = {g: ({s: str(1)} if s is not None else {}) for g, s in zip(T.gene_names, T.seeds)}
    klass, ids = plan[:, 0].tolist(), [None] * n
    for i, (r, t) in enumerate(zip(rank.tolist(), tflag.tolist())):
        if klass[i] != N.OUTA_SKIPPED:
            ids[i] = 't{0}'.format(r) if t else str(r)
    contig_of, minus = rows[:, N.OUTA_CONTIG].tolist(), ((rows[:, N.OUTA_FLAGS] & N.OUTA_MINUS) != 0).tolist()
    for i in np.flatnonzero(first == index).tolist():
        a, length = int(plan[i, 4]), int(plan[i, 5])
        seq = T.contig_seqs[contig_of[i]][a:a + length]
        alleles[prediction[i][0]][rc(seq) if minus[i] else seq] = ids[i]
    # ---- the texts, by the reference's expressions (:1406-1412, :1416, :1462, :1467-1472), column 13 from the row's own coordinates before they move
    lengths = plan[:, 5].tolist()
    for i, pred in enumerate(prediction):
        k = klass[i]
        if k == N.OUTA_SKIPPED:
            pred[13] = '{0}:{1}:{2}-{3}:{4}-{5}'.format(pred[0], 't0', pred[7], pred[8], pred[9], pred[10])
            continue
        if pred[4]:
            map_tag = '{0}:({1}){2}:{3}-{4}:{5}-{6}'.format(pred[0], pred[4].rsplit(':', 1)[-1], '{0}', pred[7], pred[8], pred[9], pred[10])
        else:
            map_tag = '{0}:{1}:{2}-{3}:{4}-{5}'.format(pred[0], '{0}', pred[7], pred[8], pred[9], pred[10])
        pred[13] = map_tag.format(ids[i])
        if k == N.OUTA_FRAGMENT:
            pred[15] = 'pseudogene=' + 'fragment:{0:.2f}%'.format((pred[10] - pred[9] + 1) * 100 / pred[12])
        elif k == N.OUTA_STRUCTVAR:
            pred[15] = 'pseudogene=' + 'structural_variation:{0:.2f}%'.format(100. * lengths[i] / T.sv_ref[i])
    for pid, cds, start, stop in done:
        pred = prediction[pid]
        pred[9:11] = start, stop
        if cds != 'CDS':
            pred[15] = 'pseudogene=' + cds
    lap('texts')
    return alleles
