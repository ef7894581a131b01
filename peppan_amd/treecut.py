"""The tree cutting of filt_per_group (PEPPAN.py:424-482) without ete3: K25 (csrc/treecut.hip, include/peppan_hip.h) at the level of arrays.

    cut_trees           a batch of trees - Newick texts or parse_newick's branches - with their `incompatible` arrays -> per tree the partition of the leaves
    branch_sets         the branches of one tree as the bit sets of leaves K25 reads

The reference walks an ete3 tree; read closely its lines compute on the unrooted tree (the header says why), so the device works on bit sets of leaves.
What is not restated is the reference's choice at an exact tie of (key, ic0) between two different bipartitions, which depends on ete3's rooting: K25's
own rule decides there, and every such tie is counted in n_ties.  There is no CPU fallback.  The context is orthofilter's cached one.
"""
import collections

import numpy as np

from . import _native as N
from .njtree import parse_newick
from .orthofilter import _context

__all__ = ['CutResult', 'cut_trees', 'branch_sets']

# leaves: the leader rows in the order of the tree's leaves (ascending); part[i]: the component of leaves[i] in the reference's output order, -1 dropped;
# log_where [n_cuts, 2]: component and lowest inducing branch (in the order of the branches given); log_val [n_cuts, 4]: s0, s1, m, key
CutResult = collections.namedtuple('CutResult', 'leaves part n_parts n_cuts n_ties log_where log_val')


def _leaf_id(name):
    """the integer behind a leaf name: X<leader> as filt_per_group writes it (PEPPAN.py:413), or the number itself (:424-426 strip the X)"""
    name = str(name)
    return int(name[1:] if name[:1] == 'X' else name)


def branch_sets(names, branches, leaves):
    """parse_newick's (leaf names, [(frozenset of names below, length)]) -> (uint64[B, words] bit sets over the positions of `leaves`, float64[B] lengths).
    `leaves`: the ascending leader rows; every name must be one of them and each must be named once."""
    where = {int(a): i for i, a in enumerate(leaves)}
    ids = [_leaf_id(x) for x in names]
    if sorted(ids) != sorted(where):
        raise ValueError('cut_trees: the tree names leaves %s, the leaders are %s' % (sorted(ids)[:8], sorted(where)[:8]))
    at = {name: where[i] for name, i in zip(names, ids)}
    words = (len(leaves) + 63) // 64
    sets = np.zeros((len(branches), words), dtype=np.uint64)
    for e, (below, _) in enumerate(branches):
        pos = np.fromiter((at[x] for x in below), dtype=np.int64, count=len(below))
        np.bitwise_or.at(sets[e], pos >> 6, np.uint64(1) << (pos & 63).astype(np.uint64))
    return sets, np.array([float(d) for _, d in branches], dtype=np.float64)


def cut_trees(texts_or_branches, incompatibles, leaders, strong, cap=N.CUT_DEFAULT_CAP, path=N.CUT_AUTO, device=None):
    """PEPPAN.py:424-482 for a batch of trees in one K25 call.

    texts_or_branches[k]: the tree text (names X<leader> or <leader>, a length on every branch: njtree.newick's) or what parse_newick made of it;
    incompatibles[k]: float64[n, n, 2] of :400-404 over all rows of the group; leaders[k]: the leader rows g[0], the tree's leaves; strong[k]: per leader,
    in the order of leaders[k], whether mat[leader, 4] >= (clust_identity - 0.02) * 10000 (:469); cap: the reference's 3000 iterations per component;
    path: _native.CUT_AUTO / CUT_BLOCK / CUT_CHAIN.  -> one CutResult per tree.  An empty batch is legal."""
    if not (len(texts_or_branches) == len(incompatibles) == len(leaders) == len(strong)):
        raise ValueError('cut_trees: one tree, one incompatible array, one list of leaders and one of strong flags per tree')
    if not len(leaders):
        return []
    sets, lengths, w0, w1, flags, leaves_of = [], [], [], [], [], []
    for tree, inc, lead, st in zip(texts_or_branches, incompatibles, leaders, strong):
        lead = np.asarray(lead, dtype=np.int64).reshape(-1)
        order = np.argsort(lead, kind='stable')
        leaves = lead[order]
        names, branches = parse_newick(tree) if isinstance(tree, str) else tree
        s, d = branch_sets(names, branches, leaves)
        inc = np.asarray(inc, dtype=np.float64)
        sets.append(s)
        lengths.append(d)
        w0.append(np.ascontiguousarray(inc[np.ix_(leaves, leaves)][:, :, 0]))
        w1.append(np.ascontiguousarray(inc[np.ix_(leaves, leaves)][:, :, 1]))
        flags.append(np.asarray(st).astype(bool).reshape(-1)[order])
        leaves_of.append(leaves)
    res = _context(device).tree_cuts(sets, lengths, w0, w1, flags, cap, path)
    return [CutResult(leaves, *r) for leaves, r in zip(leaves_of, res)]
