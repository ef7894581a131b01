"""Neighbour-joining trees without an external binary: the two places where the reference shells out to rapidnj.

    nj_trees            rapidnj itself (PEPPAN.py:416, PEPPAN_parser.py:168)   a batch of distance matrices -> join records, on the GPU (K21b)
    newick              its output with the quotes stripped, as both call sites strip them (PEPPAN.py:417, PEPPAN_parser.py:168)
    parse_newick        a small reader of that text, for callers without ete3
    kimura_distances    the distance `rapidnj -i fa -t d` makes of an alignment (PEPPAN.py:19), host float64 from K21a's integer counts
    gene_trees          PEPPAN.py:393-417 for a whole `to_run` list: the tree text of every group filt_per_group would build a tree for
    (panparser.writeCGAV writes <prefix>_CGAV.nwk through nj_trees and newick when rapidnj is not installed)

K21 (csrc/njtree.hip, include/peppan_hip.h) does the integer and the quadratic part: Context.kimura_pairs counts per pair of rows the comparable
columns, the transitions and the transversions over K15's bit planes, Context.nj_trees joins every matrix of a batch - one workgroup per tree up to
PEP_NJ_BLOCK_LEAVES leaves, a chain of launches per tree beyond.  Its arithmetic is stated in the header, in float64; rapidnj computes in float32 and
prints five significant digits, so branch lengths agree to that and topologies agree except at near-ties (profiles/njtree_vs_reference.txt).  There is
no CPU fallback.  The context is orthofilter's cached one.

Deviation from rapidnj, on purpose: a pair of rows with no shared column, or so far apart that Kimura's logarithm has no argument, gets one fixed
value from rapidnj (0.478556 where it was probed) and a tree is built on it; here such a pair is undefined, kimura_distances marks it, and gene_trees
gives the group no tree - the caller then does what PEPPAN.py:419-421 do when the tree fails and keeps the group whole.

Cutting the tree (PEPPAN.py:424-482, ete3 there) is K25: treecut.py, orthofilter.cut_groups.  Not here: FastTree."""
import collections

import numpy as np

from .orthofilter import _context, _read_groups

__all__ = ['NjTree', 'nj_trees', 'newick', 'parse_newick', 'kimura_distances', 'square_of', 'gene_trees', 'trees_of_rows']

NjTree = collections.namedtuple('NjTree', 'node length n')


def nj_trees(matrices, device=None):
    """one NjTree per square distance matrix (entries with row < column are read): node uint32[2 n - 3] and length float64[2 n - 3] as
    include/peppan_hip.h states them - per join the two joined node ids (leaves 0 .. n - 1, join s makes node n + s) and their branch lengths, then the
    last three nodes; n = 2: two entries.  An empty list is legal."""
    matrices = list(matrices)
    if not matrices:
        return []
    return [NjTree(node, length, len(m)) for m, (node, length) in zip(matrices, _context(device).nj_trees(matrices))]


def newick(tree, names, digits=5):
    """the text rapidnj prints for the tree, quotes stripped (PEPPAN.py:417, PEPPAN_parser.py:168 strip them): names unquoted, lengths as '%.{digits}g', the
    trifurcation of the last three nodes outermost - ((a:..,b:..):..,c:..,d:..); -, children in the order of the tree's arrays.  No trailing newline."""
    n = tree.n
    if len(names) != n:
        raise ValueError('newick: %d names for %d leaves' % (len(names), n))
    fmt = '%%s:%%.%dg' % digits
    text = {k: str(name) for k, name in enumerate(names)}
    node, length = [int(x) for x in tree.node], [float(x) for x in tree.length]
    for s in range(max(n - 3, 0)):
        text[n + s] = '(%s,%s)' % (fmt % (text.pop(node[2 * s]), length[2 * s]), fmt % (text.pop(node[2 * s + 1]), length[2 * s + 1]))
    first = 2 * max(n - 3, 0)
    return '(%s);' % ','.join(fmt % (text.pop(k), d) for k, d in zip(node[first:], length[first:]))


def parse_newick(text):
    """a Newick text with a length on every branch, names unquoted -> (leaf names in the order of the text, [(frozenset of the leaf names below the
    branch, length)] for every branch, in the order the branches close).  Enough for the trees newick writes and rapidnj prints."""
    text = text.strip()
    if not text.endswith(';'):
        raise ValueError('parse_newick: no closing ;')
    leaves, branches, at = [], [], 0

    def subtree():
        nonlocal at
        if text[at] == '(':
            below = set()
            while True:
                at += 1                                   # ( or ,
                child = subtree()
                if text[at] != ':':
                    raise ValueError('parse_newick: no branch length at %d' % at)
                end = at + 1
                while text[end] not in ',);':
                    end += 1
                branches.append((frozenset(child), float(text[at + 1:end])))
                at = end
                below |= child
                if text[at] == ')':
                    at += 1
                    return below
                if text[at] != ',':
                    raise ValueError('parse_newick: , or ) expected at %d' % at)
        end = at
        while text[end] not in ':,();':
            end += 1
        if end == at:
            raise ValueError('parse_newick: a name expected at %d' % at)
        leaves.append(text[at:end])
        at = end
        return {leaves[-1]}

    subtree()
    if text[at] != ';':
        raise ValueError('parse_newick: text behind the tree at %d' % at)
    return leaves, branches


def square_of(tri, n=None):
    """a packed upper triangle (row-major pairs a < b, as K15 and K21a write them) -> the symmetric [n, n] array with a zero diagonal"""
    tri = np.asarray(tri)
    if n is None:
        n = int(round((1 + np.sqrt(1 + 8 * len(tri))) / 2))
    if n * (n - 1) // 2 != len(tri):
        raise ValueError('square_of: %d entries are no triangle of %d rows' % (len(tri), n))
    out = np.zeros((n, n), dtype=tri.dtype)
    a, b = np.triu_indices(n, 1)
    out[a, b] = out[b, a] = tri
    return out


def kimura_distances(comparable, transitions, transversions):
    """Kimura's two-parameter distance as `rapidnj -i fa -t d` makes it (PEPPAN.py:19), float64 on the host from K21a's counts: with P = transitions /
    comparable and Q = transversions / comparable, d = -0.5 * log((1 - 2 P - Q) * sqrt(1 - 2 Q)).  The counts: packed triangles (1-D, made square here) or
    square arrays, of which the entries with row < column are read.  -> (d float64[n, n] with a zero diagonal, undefined bool[n, n]): a pair is undefined - and its d is nan - when comparable == 0,
    1 - 2 P - Q <= 0 or 1 - 2 Q <= 0.  rapidnj prints one fixed value for such pairs; this project does not restate it (see the module's text)."""
    cmp, ts, tv = (np.asarray(x) for x in (comparable, transitions, transversions))
    if cmp.ndim == 1:
        d, undefined = _kimura_of_pairs(cmp, ts, tv)
        return square_of(d), square_of(undefined)
    a, b = np.triu_indices(len(cmp), 1)
    d, undefined = _kimura_of_pairs(cmp[a, b], ts[a, b], tv[a, b])
    return square_of(d, len(cmp)), square_of(undefined, len(cmp))


def _kimura_of_pairs(cmp, ts, tv):
    """kimura_distances over flat arrays of pairs -> (d with nan where undefined, undefined)"""
    cmp, ts, tv = cmp.astype(np.float64), ts.astype(np.float64), tv.astype(np.float64)
    some = cmp > 0
    safe = np.where(some, cmp, 1.)
    P, Q = ts / safe, tv / safe
    u, v = 1 - 2 * P - Q, 1 - 2 * Q
    undefined = ~(some & (u > 0) & (v > 0))
    d = -0.5 * np.log(np.where(undefined, 1., u) * np.sqrt(np.where(undefined, 1., v)))
    d[undefined] = np.nan
    return d, undefined


def gene_trees(seq_store, to_run_groups, verdicts, device=None, digits=5):
    """The tree text of filt_per_group (PEPPAN.py:393-417 with the reference's default `--orthology nj`, :19) for a whole `to_run` list in two GPU batches.

    seq_store, to_run_groups: as for orthofilter.group_verdicts; verdicts: what it returned for them (detail=True).  For every group of verdict 2 with
    needs_tree the rows of the leaders g[0] of verdict.groups are the reference's tags (:393-398; code 0 is '-', which Kimura's distance skips pairwise):
    ONE Context.kimura_pairs batch over them, the logarithms on the host, ONE Context.nj_trees batch, then newick with the names X<leader> (:413).
    -> (texts, n_undefined): per group the tree text, or None for a group that needs no tree and for a group with an undefined pair (kimura_distances) -
    the caller then returns [mat] as :419-421 do when the tree fails; n_undefined counts the latter."""
    if len(verdicts) != len(to_run_groups):
        raise ValueError('gene_trees: one verdict per group')
    wanted = [k for k, v in enumerate(verdicts) if v.verdict == 2 and v.needs_tree]           # (needs_tree: two leaders at least, :400-406)
    texts = [None] * len(verdicts)
    if not wanted:
        return texts, 0
    leaders = [[int(g[0]) for g in verdicts[k].groups] for k in wanted]
    mats = [np.asarray(to_run_groups[k][0])[lead] for k, lead in zip(wanted, leaders)]
    packed, row_off, row_len, groups = _read_groups(seq_store, mats, [to_run_groups[k][2] for k in wanted])
    made = trees_of_rows(packed, row_off, row_len, groups, [['X%d' % a for a in lead] for lead in leaders], device, digits)
    for k, text in zip(wanted, made):
        texts[k] = text
    return texts, sum(text is None for text in made)


def trees_of_rows(packed, row_off, row_len, groups, names, device=None, digits=5):
    """gene_trees behind its read of the .seq store: rows and groups as for Context.kimura_pairs, per group the names of its rows -> per group the tree text,
    None for a group with an undefined pair"""
    texts = [None] * len(groups)
    if not len(groups):
        return texts
    counts = _context(device).kimura_pairs(packed, row_off, row_len, groups)
    ends = np.cumsum([len(c) for c in counts])
    flat = np.concatenate(counts)
    d, undefined = _kimura_of_pairs(flat[:, 0], flat[:, 1], flat[:, 2])          # the logarithms of the whole batch at once
    dist, usable = [], []
    for k, (a, b) in enumerate(zip(ends - [len(c) for c in counts], ends)):
        if not undefined[a:b].any():
            usable.append(k)
            dist.append(square_of(d[a:b], len(groups[k])))
    for k, tree in zip(usable, nj_trees(dist, device)):
        texts[k] = newick(tree, names[k], digits)
    return texts
