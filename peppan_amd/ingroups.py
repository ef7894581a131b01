"""The step of ortho() in front of the paralog filter: `initializing` (PEPPAN.py:1078-1093), which decides for every gene of the .tab store which
of its matches are "in group" and what the gene scores.

    determine_group     PEPPAN.py:1041-1056   drop-in for determineGroup
    gene_ingroups       PEPPAN.py:1058-1076   what initializing2 returns for a list of per-gene tables, in GPU batches
    initializing        PEPPAN.py:1078-1093   over a .tab store: the filtered tables written back, {gene: score} returned

determineGroup walks the rows of a gene in order and tests, for every row at or above the identity threshold, the rows behind it that are not
in yet - a Python lambda per row.  Only rows at or above the threshold ever act as sources and the flags only grow, so the walk is a test per
row without an order; K17 (csrc/ingroup.hip, Context.gene_ingroups) evaluates it for all genes of a batch in one submission.  The row order
(:1069) and the rescaled identity (:1070) are the reference's own numpy expressions, evaluated per gene on the host: the order is an unstable
sort of float keys, and its tie order is numpy's business.  The one transcendental depends on the genome pair alone and comes from
orthofilter.gd_table, K16's table.  There is no CPU fallback: a missing library or GPU raises PepError.  The context is orthofilter's cached
one (one per process and device; orthofilter.close() releases it).
"""
import shutil

import numpy as np

from . import _native as N
from .mapbsn import MapBsn
from .orthofilter import GdTable, _context, close, gd_table

__all__ = ['determine_group', 'gene_ingroups', 'initializing', 'close']

BATCH_ROWS = 1 << 22
GENES_PER_ROUND = 10000


def _threshold(min_iden):
    return (min_iden - 0.02) * 10000


def _table_of(global_differences, self_id, allowed_sigma):
    if isinstance(global_differences, GdTable):
        if global_differences.allowed_sigma != allowed_sigma:
            raise ValueError('the GdTable was made with allowed_sigma %r, not %r' % (global_differences.allowed_sigma, allowed_sigma))
        return global_differences
    return gd_table(global_differences, self_id, allowed_sigma)


def _checked_columns(genome, iden):
    """genome ids and identities as the library takes them; ValueError for what does not fit"""
    if len(genome) and (genome.min() < 0 or genome.max() >= 1 << 32):
        raise ValueError('genome ids must fit 32 bits')
    if len(iden) and (iden.min() < 0 or iden.max() > N.INGROUP_MAX_IDEN):
        raise ValueError('column 4 (identity) must lie in [0, 2^31), found %d .. %d' % (iden.min(), iden.max()))
    return genome.astype(np.uint32), iden.astype(np.int32)


def determine_group(gIden, global_differences, min_iden, nSigma, self_id, device=None):
    """PEPPAN.py:1041-1056 on the GPU.  gIden: int[n, 3] = (genome, identity, row number 0 .. n-1) in the order of :1069;
    global_differences: the dict (g1, g2) -> (mean, sigma), the saved [k, 2] object array, or a GdTable made with allowed_sigma = nSigma;
    self_id: what the reference reads from its module-wide params.  -> bool[n]"""
    gIden = np.asarray(gIden)
    if gIden.ndim != 2 or gIden.shape[1] != 3:
        raise ValueError('gIden must be [n, 3], not %s' % (gIden.shape,))
    gIden = gIden.astype(np.int64)
    n = gIden.shape[0]
    if not np.array_equal(gIden[:, 2], np.arange(n)):
        raise ValueError('column 2 of gIden must number the rows 0 .. n-1')
    if n == 0:
        return np.zeros(0, dtype=bool)
    gd = _table_of(global_differences, self_id, nSigma)
    genome, iden = _checked_columns(gIden[:, 0], gIden[:, 1])
    keep, _ = _context(device).gene_ingroups(genome, iden, np.zeros(n, np.int64), [0, n], gd, self_id, _threshold(min_iden))
    return keep


def _ordered(matches):
    """a table of two rows and more as :1069-1070 leave it: rows by falling 1000 * |score| / max |score| + column 3, column 4 rescaled to the first row"""
    matches = matches[np.argsort(-(1000 * np.abs(matches.T[2]) / np.max(np.abs(matches.T[2])) + matches.T[3]))]
    matches.T[4] = (10000 * matches.T[3] / matches[0, 3]).astype(int)
    return matches


def gene_ingroups(tables, global_differences, params, device=None, batch_rows=BATCH_ROWS):
    """What initializing2 (PEPPAN.py:1058-1076) returns for the tables of a list of genes, as the .tab store holds them (int64[n, >= 5]: column 1
    genome, 2 score, 3 and 4 identity).  params: clust_identity, allowed_sigma, self_id.  -> per gene (matches, score): the rows in group, in the
    order of :1069 with column 4 rescaled (:1070), and the sum of |score| over the first kept row of every genome (:1074).  A table of one row
    passes through untouched with matches[0, 2] as its score (:1066-1068); an empty one raises ValueError.  One GPU batch per batch_rows rows."""
    self_id, sigma = params['self_id'], params['allowed_sigma']
    gd = _table_of(global_differences, self_id, sigma)
    thr = _threshold(params['clust_identity'])
    out = [None] * len(tables)
    todo, rows = [], 0

    def flush():
        if not todo:
            return
        genome, iden = _checked_columns(np.concatenate([m[:, 1] for _, m in todo]), np.concatenate([m[:, 4] for _, m in todo]))
        gene_off = np.concatenate([[0], np.cumsum([len(m) for _, m in todo])])
        keep, score = _context(device).gene_ingroups(genome, iden, np.concatenate([m[:, 2] for _, m in todo]), gene_off, gd, self_id, thr)
        for (k, m), lo, hi, s in zip(todo, gene_off[:-1], gene_off[1:], score):
            out[k] = (m[keep[lo:hi]], s)
        del todo[:]

    for k, matches in enumerate(tables):
        matches = np.asarray(matches)
        if len(matches) == 0:
            raise ValueError('gene %d of the list has an empty table' % k)
        if len(matches) == 1:
            out[k] = (matches, matches[0, 2])
            continue
        if rows and rows + len(matches) > batch_rows:
            flush()
            rows = 0
        todo.append((k, _ordered(matches)))
        rows += len(matches)
    flush()
    return out


def initializing(bsn_file, global_file, params, device=None, batch_rows=BATCH_ROWS):
    """PEPPAN.py:1078-1093: every gene of <bsn_file>.tab.npz, in sorted order and 10 000 genes at a time, through gene_ingroups; the filtered
    tables go to <bsn_file>.tmp.npz, which then replaces the .tab store.  global_file: what get_global_difference saved (:1666).
    -> {int(gene): score}"""
    gd = gd_table(np.load(global_file, allow_pickle=True), params['self_id'], params['allowed_sigma'])
    gene_scores = {}
    with MapBsn(bsn_file + '.tab.npz') as conn, MapBsn(bsn_file + '.tmp.npz', 'w') as conn2:
        genes = sorted(conn.keys())
        for ite in range(0, len(genes), GENES_PER_ROUND):
            part = genes[ite:ite + GENES_PER_ROUND]
            for gene, (data, score) in zip(part, gene_ingroups([conn.get(g) for g in part], gd, params, device, batch_rows)):
                gene_scores[int(gene)] = score
                conn2.save(gene, data)
    shutil.move(bsn_file + '.tmp.npz', bsn_file + '.tab.npz')
    return gene_scores
