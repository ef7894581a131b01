"""The integer layer of the paralog filter (filt_genes -> filt_per_group, PEPPAN.py:326-484): pairwise allele differences of gene groups.

    compare_seq, compare_seqX   PEPPAN.py:296-316   drop-ins for the reference's two numba kernels
    group_differences           PEPPAN.py:330-333 + :346 + :370 for a whole `to_run` list (:624-626) in one GPU batch
    group_verdicts              PEPPAN.py:335-392: what filt_per_group decides from those differences, decided on the GPU (K16); per-pair data
                                comes back only for the groups that go on to the tree test
    group_trees                 PEPPAN.py:393-417: the neighbour-joining tree text of those groups (K21, njtree.py)
    cut_groups                  PEPPAN.py:424-482: the trees cut at their incompatible branches (K25, treecut.py), the list of matrices of every group
    filt_per_groups             all of filt_per_group for a whole `to_run` list: the drop-in for the imap_unordered of :626
    gd_table, distances_from_diff, incompatible_of   the host halves of it (the exp() per genome pair; :371-380; :400-406)

Both counts are sums over columns, so the rows never leave the base-5 packing of the .seq store (mapbsn.encodeSeq): K15
(csrc/allelediff.hip, Context.allele_diff) turns the packed bytes into bit planes and counts with population counts.  The float layer
of filt_per_group up to the decision to build a tree is K16 (csrc/divergence.hip, Context.group_verdicts); the tree text is K21 (njtree.py);
the cutting of the tree is K25 (treecut.py), which needs no ete3.  Not here: `--orthology ml` (FastTree), and the reference's choice where two
different branches tie exactly in both sort keys of :458, which depends on ete3's rooting - such ties are counted, see DESIGN.md section 8.
There is no CPU fallback.
The drop-ins and group_differences share one cached context per process and device; close() releases it.
"""
import collections
import os

import numpy as np

from . import _native as N
from .mapbsn import MapBsn

__all__ = ['compare_seq', 'compare_seqX', 'group_differences', 'iter_group_differences', 'pack_rows', 'close',
           'group_verdicts', 'group_trees', 'cut_groups', 'mats_of_cut', 'filt_per_groups', 'gd_table', 'distances_from_diff', 'incompatible_of', 'GdTable', 'GroupVerdict']

_CODE = np.full(256, 255, dtype=np.uint8)
_CODE[[0, 65, 67, 71, 84]] = (0, 1, 2, 3, 4)

_CONTEXTS = {}


def _context(device=None):
    """one context per (process, device), made on first use (HIP state does not survive fork()) and kept until close(): its grow-only
    device workspaces stay as large as the largest call made them (bit planes and output: up to 2 GiB each)"""
    key = (os.getpid(), int(device or 0))
    if key not in _CONTEXTS:
        _CONTEXTS[key] = N.Context(key[1])
    return _CONTEXTS[key]


def close():
    """destroy the contexts this module made in this process and free their device memory; the next call makes a new one"""
    for key in [k for k in _CONTEXTS if k[0] == os.getpid()]:
        _CONTEXTS.pop(key).close()


def pack_rows(seqs):
    """uint8[n, L] of 0 / ASCII A C G T -> uint8[n, ceil(L / 3)] in the .seq store's packing (first third * 25 + second third * 5 + last
    third, mapbsn.encodeSeq row by row).  ValueError for any other byte."""
    seqs = np.asarray(seqs)
    if seqs.dtype != np.uint8:
        raise TypeError('seqs must be uint8, not %s' % seqs.dtype)
    if seqs.ndim != 2:
        raise ValueError('seqs must be [n, L], not %d-dimensional' % seqs.ndim)
    codes = _CODE[seqs]
    if codes.size and codes.max() == 255:
        bad = int(seqs[codes == 255][0])
        raise ValueError('seqs holds byte %d: only 0 and the ASCII codes of A, C, G, T are comparable' % bad)
    n, L = codes.shape
    s = -(-L // 3)
    full = np.zeros((n, 3 * s), dtype=np.uint8)
    full[:, :L] = codes
    return full[:, :s] * 25 + full[:, s:2 * s] * 5 + full[:, 2 * s:]


def _run(seqs, diff, mode, device):
    """checks of the drop-ins' arguments (no device needed), then one group through K15 -> (tri, edge)"""
    seqs = np.asarray(seqs)
    packed = pack_rows(seqs)
    if not isinstance(diff, np.ndarray) or diff.dtype != np.int64:
        raise TypeError('diff must be an int64 array')
    n, s = packed.shape
    if diff.shape != (n, n, 2):
        raise ValueError('diff must be [n, n, 2] for n = %d rows, not %s' % (n, diff.shape))
    if n == 0:
        return None, None
    row_off = np.arange(n + 1, dtype=np.uint64) * np.uint64(s)
    row_len = np.full(n, seqs.shape[1], dtype=np.uint32)
    return _context(device).allele_diff(packed, row_off, row_len, [np.arange(n, dtype=np.uint32)], mode, out_budget=1 << 31)[0]


def _fill_upper(diff, tri):
    """packed upper triangle (row-major pairs a < b) -> diff[a, a+1:]"""
    n, at = diff.shape[0], 0
    for a in range(n - 1):
        diff[a, a + 1:] = tri[at:at + n - a - 1]
        at += n - a - 1
    return diff


def compare_seq(seqs, diff, device=None):
    """PEPPAN.py:296-305 on the GPU: for rows a < b, diff[a, b] = (mismatches + 1, comparable columns + 2); every other cell of the
    caller's int64[n, n, 2] stays as passed.  seqs: uint8[n, L] with 0 for a column that does not count and the ASCII code of A, C, G, T
    otherwise - what the reference's caller always passes (:332-333 zero everything else); any other byte raises ValueError naming it."""
    tri, _ = _run(seqs, diff, 1, device)
    if tri is not None:
        _fill_upper(diff, tri)
    return diff


def compare_seqX(seqs, diff, device=None):
    """PEPPAN.py:307-316 on the GPU: diff[a, b] = (mismatches + 1, comparable columns + 2) for a = first and last row against EVERY row b,
    a itself included; every other cell stays as passed.  Input as for compare_seq."""
    _, edge = _run(seqs, diff, 2, device)
    if edge is not None:
        diff[0] = edge[0]
        diff[-1] = edge[1]
    return diff


def _read_groups(seq_store, mats, ref_lens):
    """the packed rows of the groups' loci (column 5 of every table: member id // 1000, row id % 1000 of the store, PEPPAN.py:331), as they lie
    in the store -> (packed, row_off, row_len, one array of row indices per group)"""
    own = not isinstance(seq_store, MapBsn)
    store = MapBsn(seq_store) if own else seq_store
    try:
        members, rows, row_len, groups = {}, [], [], []
        for mat, ref_len in zip(mats, ref_lens):
            ids = [int(i) for i in np.asarray(mat)[:, 5].tolist()] if len(mat) else []
            s = -(-int(ref_len) // 3)
            first = len(rows)
            for i in ids:
                m = i // 1000
                if m not in members:
                    members[m] = store.get(m)
                row = np.asarray(members[m][i % 1000], dtype=np.uint8)
                if row.shape != (s,):
                    raise ValueError('locus %d holds %s packed bytes, a gene of %d nt needs %d' % (i, row.shape, int(ref_len), s))
                rows.append(row)
                row_len.append(int(ref_len))
            groups.append(np.arange(first, len(rows), dtype=np.uint32))
    finally:
        if own:
            store.close()
    packed = np.concatenate(rows) if rows else np.zeros(0, np.uint8)
    row_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    return packed, row_off, np.array(row_len, dtype=np.uint32), groups


def iter_group_differences(seq_store, mats, ref_lens, edge=True, full=True, device=None, out_budget=1 << 30):
    """group_differences as a generator: the GPU batch runs on the first next(); the int64 squares are made one group at a time"""
    packed, row_off, row_len, groups = _read_groups(seq_store, mats, ref_lens)
    mode = (1 if full else 0) | (2 if edge else 0)
    res = _context(device).allele_diff(packed, row_off, row_len, groups, mode, out_budget=out_budget) if mode else [(None, None)] * len(groups)
    for g, (tri, strip) in zip(groups, res):
        n = len(g)
        diffX = diff = None
        if edge:
            diffX = np.zeros((n, n, 2), dtype=np.int64)
            if n:
                diffX[0], diffX[-1] = strip[0], strip[1]
        if full:
            diff = np.zeros((n, n, 2), dtype=np.int64)
            if n > 1:
                _fill_upper(diff, tri)
        yield diffX, diff


def group_differences(seq_store, mats, ref_lens, edge=True, full=True, device=None, out_budget=1 << 30):
    """The GPU-first form of PEPPAN.py:330-333 + :346 + :370 for a list of gene groups (the `to_run` list of filt_genes, :624-626).

    seq_store: the .seq store (MapBsn or its path); mats: the groups' tables, column 5 = locus id (member id // 1000, row id % 1000 of
    the store, :331); ref_lens: the exemplar length of every group.  The packed rows go from the store to ONE Context.allele_diff batch
    without being decoded on the host.  -> per group (diffX, diff): what compare_seqX / compare_seq return for zero-filled int64[n, n, 2]
    (None for the one not asked for: edge=False / full=False)."""
    return list(iter_group_differences(seq_store, mats, ref_lens, edge, full, device, out_budget))


GdTable = collections.namedtuple('GdTable', 'keys vals default self_id allowed_sigma')


def gd_table(global_differences, self_id, allowed_sigma):
    """The host half of K16: the one transcendental of checkDiv / distances (PEPPAN.py:341, :378) depends on the genome pair alone, so it is
    evaluated here, with numpy as the reference writes it, once per entry of global_differences and once for the default (0.5, 0.6) of a
    missing pair (:340, :377).  global_differences: the dict (g1, g2) -> (mean, sigma) or the [k, 2] object array get_global_difference saves
    (:1666; dict(np.load(...)) at :328).  -> GdTable: keys uint64[k] = g1 << 32 | g2 ascending, vals float64[k, 3] = (gd0,
    gd0 * exp(gd1 * sqrt(allowed_sigma)), gd0 * exp(gd1 * allowed_sigma)), default float64[3].  A key with g1 > g2 can never be looked up
    (the reference sorts the pair, :340) and is left out."""
    if not (np.isfinite(self_id) and self_id > 0):
        raise ValueError('self_id must be finite and > 0, not %r' % (self_id,))
    if not (np.isfinite(allowed_sigma) and allowed_sigma >= 0):
        raise ValueError('allowed_sigma must be finite and >= 0, not %r' % (allowed_sigma,))
    if not isinstance(global_differences, dict):
        global_differences = dict(global_differences)
    items = [(int(k[0]), int(k[1]), float(v[0]), float(v[1])) for k, v in global_differences.items() if k[0] <= k[1]]
    if any(g1 < 0 or g2 >= 1 << 32 for g1, g2, _, _ in items):
        raise ValueError('genome ids must fit 32 bits')
    items.sort()
    gd0 = np.array([i[2] for i in items] + [0.5], dtype=np.float64)
    gd1 = np.array([i[3] for i in items] + [0.6], dtype=np.float64)
    vals = np.stack([gd0, gd0 * np.exp(gd1 * np.sqrt(allowed_sigma)), gd0 * np.exp(gd1 * allowed_sigma)], axis=1)
    if not (np.isfinite(vals).all() and (vals > 0).all()):
        raise ValueError('global_differences holds a pair whose bound is not finite and > 0')
    keys = np.array([(i[0] << 32) | i[1] for i in items], dtype=np.uint64)
    return GdTable(keys, np.ascontiguousarray(vals[:-1]), vals[-1].copy(), float(self_id), allowed_sigma)


def _gd_of_pairs(gd, ga, gb, aln):
    """(gd0, checkDiv's denominator, the distances' denominator) of every pair: genome ids ga, gb and aln, arrays of one shape"""
    lo, hi = np.minimum(ga, gb).astype(np.uint64), np.maximum(ga, gb).astype(np.uint64)
    key = (lo << np.uint64(32)) | hi
    at = np.searchsorted(gd.keys, key)
    hit = at < len(gd.keys)
    hit[hit] = gd.keys[at[hit]] == key[hit]
    vals = np.concatenate([gd.vals, gd.default[None, :]])
    row = np.where(hit, at, len(gd.keys))
    same = ga == gb
    own = np.maximum(gd.self_id, 2.0 / aln)
    return np.where(same, own, vals[row, 0]), np.where(same, own, vals[row, 1]), np.where(same, own, vals[row, 2])


def distances_from_diff(diff, genomes, gd):
    """PEPPAN.py:371-380 by elementwise numpy: diff float64[n, n, 2] with its upper triangle filled (compare_seq's), the genome id of every row
    (column 1 of the group's table), gd from gd_table -> distances float64[n, n, 2], symmetric, zero on the diagonal."""
    diff = np.asarray(diff, dtype=np.float64)
    n = diff.shape[0]
    genomes = np.asarray(genomes).astype(np.int64)
    distances = np.zeros((n, n, 2), dtype=np.float64)
    a, b = np.triu_indices(n, 1)
    mut, aln = diff[a, b, 0], diff[a, b, 1]
    gd0, _, den = _gd_of_pairs(gd, genomes[a], genomes[b], aln)
    d = mut / aln / den
    distances[a, b, 0] = distances[b, a, 0] = d / gd0
    distances[a, b, 1] = distances[b, a, 1] = 1 / gd0
    return distances


def incompatible_of(distances, groups):
    """PEPPAN.py:400-406 with the reference's own expression (the order of a float sum is numpy's business) -> (incompatible float64[n, n, 2],
    needs_tree: whether the reference goes on to build a tree, :406-407)"""
    incompatible = np.zeros(shape=distances.shape, dtype=float)
    for i1, g1 in enumerate(groups):
        for i2 in range(i1 + 1, len(groups)):
            g2 = groups[i2]
            incompatible[g2[0], g1[0], :] = incompatible[g1[0], g2[0], :] = np.sum(distances[g1][:, g2, :], (0, 1))
    return incompatible, not bool(np.all(incompatible[:, :, 0] <= incompatible[:, :, 1]))


def group_trees(seq_store, to_run_groups, verdicts, device=None, digits=5):
    """PEPPAN.py:393-417 behind group_verdicts: the tree text of every group that goes on to the tree test, by K21 (njtree.gene_trees, which see)"""
    from .njtree import gene_trees
    return gene_trees(seq_store, to_run_groups, verdicts, device, digits)


class GroupVerdict(object):
    """verdict: 0 not divergent (the reference returns [mat] at :368), 1 divergent but no pair beyond its bound (:484), 2 a pair beyond (:383).
    For verdict 2 and detail=True also diff, groups, distances, incompatible, needs_tree; None otherwise."""
    __slots__ = ('verdict', 'diff', 'groups', 'distances', 'incompatible', 'needs_tree')

    def __init__(self, verdict):
        self.verdict = verdict
        self.diff = self.groups = self.distances = self.incompatible = self.needs_tree = None


def group_verdicts(seq_store, to_run_groups, global_differences, params, detail=True, device=None, out_budget=1 << 30):
    """filt_per_group (PEPPAN.py:326-407) up to its decision to build a tree, for a whole `to_run` list (:624) in one GPU batch.

    seq_store: the .seq store (MapBsn or its path); to_run_groups: per group (mat, inparalog, ref_len, ...) as filt_genes collects them
    (column 1 of mat = genome id, column 5 = locus id); global_differences: the dict, the saved [k, 2] object array, or a GdTable;
    params: self_id and allowed_sigma.  -> one GroupVerdict per group.  The packed rows go from the store to ONE Context.group_verdicts
    batch; the device decides every verdict, and per-pair data comes back only for verdict 2 (when detail): diff float64[n, n, 2] as :370
    leaves it, groups as :383-392 leave them, distances (:371-380, by distances_from_diff on the host) and incompatible / needs_tree
    (:400-406).  The tree and its cutting (:409-482) are group_trees and cut_groups; filt_per_groups runs all three."""
    gd = global_differences if isinstance(global_differences, GdTable) else gd_table(global_differences, params['self_id'], params['allowed_sigma'])
    mats = [np.asarray(t[0]) for t in to_run_groups]
    packed, row_off, row_len, groups = _read_groups(seq_store, mats, [t[2] for t in to_run_groups])
    genomes = [m[:, 1].astype(np.int64) if len(m) else np.zeros(0, np.int64) for m in mats]
    if any(len(g) and (g.min() < 0 or g.max() >= 1 << 32) for g in genomes):
        raise ValueError('genome ids must fit 32 bits')
    inparalog = np.array([1 if t[1] else 0 for t in to_run_groups], dtype=np.uint8)
    res = _context(device).group_verdicts(packed, row_off, row_len, groups, genomes, inparalog, gd, gd.self_id, detail=detail, out_budget=out_budget)
    out = []
    for genome, (verdict, tri, leader) in zip(genomes, res):
        v = GroupVerdict(verdict)
        if tri is not None:
            n = len(leader)
            v.diff = _fill_upper(np.zeros((n, n, 2), dtype=np.float64), tri)
            order = np.argsort(leader, kind='stable')
            cuts = np.flatnonzero(np.diff(leader[order])) + 1
            v.groups = [part.tolist() for part in np.split(order, cuts)]
            v.distances = distances_from_diff(v.diff, genome, gd)
            v.incompatible, v.needs_tree = incompatible_of(v.distances, v.groups)
        out.append(v)
    return out


def mats_of_cut(mat, groups, leaves, part, n_parts):
    """PEPPAN.py:474-482: the matrices of one group from the partition of its tree's leaves.  groups: as :383-392 leave them (g[0] the leader); leaves: the
    leader rows in the order of `part`; part[i]: the component of leaves[i] in the order of the reference's queue, -1 for a dropped leaf.  Component by
    component the rows of its leaders' groups, sorted; `mat` itself for a component that holds every leaf."""
    members = {int(g[0]): g for g in groups}
    mats = []
    for q in range(int(n_parts)):
        tips = [int(a) for a, p in zip(leaves, part) if p == q]
        if len(tips) < len(groups):
            mats.append(mat[sorted(nn for a in tips for nn in members.get(a, []))])
        else:
            mats.append(mat)
    return mats


def cut_groups(to_run_groups, verdicts, texts, params, cap=3000, path=0, device=None, detail=False):
    """PEPPAN.py:424-482 behind group_trees for a whole `to_run` list in ONE K25 batch (treecut.cut_trees, which see): per group the list of matrices
    filt_per_group returns.  verdicts: group_verdicts' (detail=True); texts: group_trees'; params: clust_identity.  A group without a tree text - verdict 0
    or 1, no incompatible pair of leaders, or a tree that failed - gives [mat] (:368, :407, :419-421, :484).  detail=True: (that list, per group the
    treecut.CutResult or None)."""
    from .treecut import cut_trees
    if not (len(to_run_groups) == len(verdicts) == len(texts)):
        raise ValueError('cut_groups: one verdict and one text (or None) per group')
    wanted = [k for k, text in enumerate(texts) if text is not None]
    bound = (params['clust_identity'] - 0.02) * 10000
    leaders = [[int(g[0]) for g in verdicts[k].groups] for k in wanted]
    strong = [np.asarray(to_run_groups[k][0])[lead, 4].astype(np.float64) >= bound for k, lead in zip(wanted, leaders)]
    cuts = cut_trees([texts[k] for k in wanted], [verdicts[k].incompatible for k in wanted], leaders, strong, cap, path, device)
    out, found = [[t[0]] for t in to_run_groups], [None] * len(to_run_groups)
    for k, c in zip(wanted, cuts):
        out[k] = mats_of_cut(to_run_groups[k][0], verdicts[k].groups, c.leaves, c.part, c.n_parts)
        found[k] = c
    return (out, found) if detail else out


def filt_per_groups(seq_store, to_run, global_differences, params, device=None):
    """The drop-in for `pool.imap_unordered(filt_per_group, to_run)` (PEPPAN.py:626) with `--orthology nj`: group_verdicts, group_trees, cut_groups.

    seq_store, to_run, global_differences: as for group_verdicts (to_run: per group (mat, inparalog, ref_len, ...)); params: self_id, allowed_sigma,
    clust_identity and orthology.  -> (per group, in the order given, the list of matrices filt_per_group returns; n_ties: how often two different
    branches tied exactly in both sort keys of :458, where the reference's choice depends on ete3's rooting and this project's own rule decided).
    orthology 'ml' sends every tree of fewer than 500 tags to FastTree (:415), which is not restated: NotImplementedError when such a group is met."""
    orthology = params.get('orthology', 'nj')
    if orthology not in ('nj', 'ml', 'sbh'):
        raise ValueError('filt_per_groups: orthology is nj, ml or sbh, not %r' % (orthology,))
    verdicts = group_verdicts(seq_store, to_run, global_differences, params, detail=True, device=device)
    if orthology == 'ml':                                # (sbh never reaches filt_per_group: filt_genes is not run for it)
        for k, v in enumerate(verdicts):
            if v.verdict == 2 and v.needs_tree and len(v.groups) < 500:
                raise NotImplementedError('filt_per_groups: group %d has %d tags, and --orthology ml builds the tree of fewer than 500 tags with FastTree '
                                          '(PEPPAN.py:415), which is not restated; only rapidnj (nj) is' % (k, len(v.groups)))
    texts, _ = group_trees(seq_store, to_run, verdicts, device)
    out, found = cut_groups(to_run, verdicts, texts, params, device=device, detail=True)
    return out, sum(c.n_ties for c in found if c is not None)
