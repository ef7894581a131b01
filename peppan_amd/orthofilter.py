"""The integer layer of the paralog filter (filt_genes -> filt_per_group, PEPPAN.py:326-484): pairwise allele differences of gene groups.

    compare_seq, compare_seqX   PEPPAN.py:296-316   drop-ins for the reference's two numba kernels
    group_differences           PEPPAN.py:330-333 + :346 + :370 for a whole `to_run` list (:624-626) in one GPU batch

Both counts are sums over columns, so the rows never leave the base-5 packing of the .seq store (mapbsn.encodeSeq): K15
(csrc/allelediff.hip, Context.allele_diff) turns the packed bytes into bit planes and counts with population counts.  The float layer
of filt_per_group (checkDiv, distances, the tree) is not here: see DESIGN.md section 8.  There is no CPU fallback.
The drop-ins and group_differences share one cached context per process and device; close() releases it.
"""
import os

import numpy as np

from . import _native as N
from .mapbsn import MapBsn

__all__ = ['compare_seq', 'compare_seqX', 'group_differences', 'iter_group_differences', 'pack_rows', 'close']

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


def iter_group_differences(seq_store, mats, ref_lens, edge=True, full=True, device=None, out_budget=1 << 30):
    """group_differences as a generator: the GPU batch runs on the first next(); the int64 squares are made one group at a time"""
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
    mode = (1 if full else 0) | (2 if edge else 0)
    res = _context(device).allele_diff(packed, row_off, np.array(row_len, dtype=np.uint32), groups, mode, out_budget=out_budget) if mode else [(None, None)] * len(groups)
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
