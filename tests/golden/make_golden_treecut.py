#!/usr/bin/env python3
"""Generate tests/golden/g28_treecut.json.gz by IMPORTING the reference's Python (build machine only: needs /root/reference).

    python tests/golden/make_golden_treecut.py

The shim of make_golden_divergence.py, with two differences.  subprocess.Popen is replaced by a class that reads the FASTA file the reference wrote and
RETURNS a tree text - the one K21 makes of those rows: Kimura's distances and the neighbour joining of tests/njtree_helpers.py, which the device equals bit
for bit, printed by peppan_amd.njtree.newick.  And the `ete3` the reference imports is this project's own small stand-in, written from scratch below: it
implements only what PEPPAN.py:417-482 call (the constructor from Newick, get_leaves, get_leaf_names, get_midpoint_outgroup, set_outgroup, get_children,
iter_descendants('postorder'), is_leaf, is_root, up, detach, delete(preserve_branch_length=True), name, dist), after ete3's documented behaviour.  Real
ete3 cannot be run where this project is built.

PEP.filt_per_group itself (PEPPAN.py:326-484) runs on every case, TWICE: with the stand-in's midpoint rooting and rooted at an arbitrary other branch.  The
two runs must return the same matrices - the evidence for the claim of include/peppan_hip.h that the rooting shows only at exact ties - and the
numpy restatement of tests/treecut_helpers.py must return them too.  Only DATA is written: the case's inputs, the tree text and the rows of each returned
matrix - none of the reference's source text.

Two kinds of case.  Dyadic: ref_len 1022 without gaps, every genome pair at (2^-5, 0) and self_id 2^-5, so that distances[:, :, 0] is the integer mut and
[:, :, 1] is 32: every sum is exact in any order and no margin is needed.  Float: general parameters and gaps; there the restatement reports how close any
ic0 came to 1 and any runner-up to the winner, and both must exceed 1e-9 (L^2 * 2^-52 = 1.5e-11 at 256 leaves, times about 60).  Every case has n_ties == 0.
"""
import base64, gzip, json, os, stat, sys, tempfile, time

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'

ETE3_STAND_IN = r'''
"""a stand-in for the few ete3 calls PEPPAN.py:417-482 make; ROOTING chooses what get_midpoint_outgroup returns"""
ROOTING = 'midpoint'


class Tree(object):
    def __init__(self, newick=None):
        self.name, self.dist, self.up, self.children = '', 0.0, None, []
        if newick is not None:
            text = newick.strip()
            if not text.endswith(';'):
                raise ValueError('no closing ;')
            at = self._read(text, 0)
            if text[at] != ';':
                raise ValueError('text behind the tree')
            self.dist = 0.0

    def _read(self, text, at):
        if text[at] == '(':
            while True:
                child = Tree()
                child.up = self
                self.children.append(child)
                at = child._read(text, at + 1)
                if text[at] == ')':
                    at += 1
                    break
                if text[at] != ',':
                    raise ValueError(', or ) expected')
        end = at
        while text[end] not in ':,();':
            end += 1
        self.name = text[at:end]
        at = end
        if text[at] == ':':
            end = at + 1
            while text[end] not in ',);':
                end += 1
            self.dist = float(text[at + 1:end])
            at = end
        return at

    def get_children(self):
        return self.children

    def is_leaf(self):
        return not self.children

    def is_root(self):
        return self.up is None

    def iter_descendants(self, strategy='levelorder'):
        assert strategy == 'postorder'
        for child in self.children:
            for node in child.iter_descendants('postorder'):
                yield node
            yield child

    def get_leaves(self):
        return [self] if self.is_leaf() else [leaf for child in self.children for leaf in child.get_leaves()]

    def get_leaf_names(self):
        return [leaf.name for leaf in self.get_leaves()]

    def _root(self):
        node = self
        while node.up is not None:
            node = node.up
        return node

    def _farthest(self, leaves_only):
        """(node, distance) of the node farthest from self over the whole tree"""
        best, seen, todo = (self, 0.0), {id(self)}, [(self, 0.0)]
        while todo:
            node, d = todo.pop()
            if d > best[1] and (node.is_leaf() or not leaves_only):
                best = (node, d)
            near = [(c, c.dist) for c in node.children] + ([(node.up, node.dist)] if node.up is not None else [])
            for other, step in near:
                if id(other) not in seen:
                    seen.add(id(other))
                    todo.append((other, d + step))
        return best

    def get_midpoint_outgroup(self):
        root = self._root()
        if ROOTING != 'midpoint':
            # an arbitrary other branch: the last internal node below the root, else the last leaf
            nodes = list(root.iter_descendants('postorder'))
            inner = [n for n in nodes if not n.is_leaf() and n.up is not root]
            return inner[-1] if inner else nodes[-2] if len(nodes) > 1 else None
        a, _ = root._farthest(True)
        _, span = a._farthest(False)
        half, walked, node = span / 2.0, 0.0, a
        while node is not None:
            walked += node.dist
            if walked > half:
                break
            node = node.up
        return node

    def set_outgroup(self, outgroup):
        """self stays the root object; its two children become the outgroup and the rest of the tree, the outgroup's branch split evenly between them"""
        root = self
        if outgroup is root or outgroup.up is None:
            raise ValueError('cannot set the root as outgroup')
        if outgroup.up is root and len(root.children) == 2:
            return
        # the tree as an undirected graph, without the subtree below the outgroup; a root of two children is no node of it, any other root becomes a plain node
        plain = None
        if len(root.children) != 2:
            plain = Tree()
            plain.name = root.name
        alias = lambda node: plain if node is root else node
        near = {}

        def link(x, y, d):
            near.setdefault(id(x), []).append((y, d))
            near.setdefault(id(y), []).append((x, d))

        todo = list(root.children)
        if plain is None:
            link(root.children[0], root.children[1], root.children[0].dist + root.children[1].dist)
        while todo:
            node = todo.pop()
            if node.up is not root or plain is not None:
                link(node, alias(node.up), node.dist)
            if node is not outgroup:
                todo.extend(node.children)
        start, = [y for y, _ in near[id(outgroup)]]
        half = outgroup.dist / 2.0 if (outgroup.up is not root or plain is not None) else near[id(outgroup)][0][1] / 2.0
        # hang everything but the outgroup below `start`
        seen, todo = {id(outgroup), id(start)}, [start]
        while todo:
            node = todo.pop()
            node.children = []
            for other, d in near[id(node)]:
                if id(other) not in seen:
                    seen.add(id(other))
                    other.up, other.dist = node, d
                    node.children.append(other)
                    todo.append(other)
        root.children = [outgroup, start]
        outgroup.up = start.up = root
        outgroup.dist = start.dist = half
        root.up, root.dist = None, 0.0

    def detach(self):
        if self.up is not None:
            self.up.children.remove(self)
            self.up = None
        return self

    def delete(self, prevent_nondicotomic=True, preserve_branch_length=False):
        """the node leaves the tree, its children join its parent; like ete3's, the node itself keeps its list of children, and a parent left with one
        child is deleted in turn.  The reference goes on using a deleted node as the root of its component (:463-468), which this keeps possible"""
        parent = self.up
        if parent is not None:
            if preserve_branch_length:
                if len(self.children) == 1:
                    self.children[0].dist += self.dist
                elif len(self.children) > 1:
                    parent.dist += self.dist
            for c in self.children:
                parent.children.append(c)
                c.up = parent
            parent.children.remove(self)
            self.up = None
        if prevent_nondicotomic and parent is not None and len(parent.children) < 2:
            parent.delete(prevent_nondicotomic=False, preserve_branch_length=preserve_branch_length)
'''


def build_shim():
    root = tempfile.mkdtemp(prefix='peppan_shim_')
    os.makedirs(os.path.join(root, 'bin'))
    for t in ('mmseqs', 'makeblastdb', 'diamond', 'blastn'):
        p = os.path.join(root, 'bin', t)
        with open(p, 'w') as f:
            f.write('#!/bin/sh\nexit 0\n')
        os.chmod(p, os.stat(p).st_mode | stat.S_IEXEC | stat.S_IXGRP | stat.S_IXOTH)
    for pkg, body in (('numba', 'def jit(*a, **k):\n    if len(a) == 1 and callable(a[0]) and not k:\n        return a[0]\n    return lambda f: f\n'),
                      ('ete3', ETE3_STAND_IN)):
        os.makedirs(os.path.join(root, 'py', pkg))
        with open(os.path.join(root, 'py', pkg, '__init__.py'), 'w') as f:
            f.write(body)
    os.makedirs(os.path.join(root, 'cwd'))
    return root


SHIM = build_shim()
os.environ['PATH'] = os.path.join(SHIM, 'bin') + os.pathsep + os.environ['PATH']
sys.path[:0] = [os.path.join(SHIM, 'py'), os.path.join(REF, 'modules'), REF, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
os.chdir(os.path.join(SHIM, 'cwd'))

import numpy as np                       # noqa: E402
if not hasattr(np.lib.npyio, 'format'):  # numpy >= 2 dropped this alias of np.lib.format; the reference's MapBsn spells it the old way
    np.lib.npyio.format = np.lib.format
import ete3                              # noqa: E402  (the stand-in)
import PEPPAN as PEP                     # noqa: E402
import njtree_helpers as NJ              # noqa: E402
import treecut_helpers as H              # noqa: E402
from divergence_helpers import clade, pack_codes, pair_counts, restate   # noqa: E402
from peppan_amd import njtree, orthofilter, treecut                      # noqa: E402

CODE_OF = {'-': 0, 'A': 1, 'C': 2, 'G': 3, 'T': 4}
CLUST_IDENTITY = 0.9


def text_of_fasta(path):
    """the tree text K21 makes of the FASTA file the reference wrote, or None when a pair has no defined distance"""
    names, rows = [], []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith('>'):
                names.append(line[1:])
            elif line:
                rows.append([CODE_OF[c] for c in line])
    counts = NJ.kimura_counts(np.array(rows, dtype=np.uint8))
    d, undefined = njtree._kimura_of_pairs(counts[:, 0], counts[:, 1], counts[:, 2])
    if undefined.any():
        return None
    node, length = NJ.nj_restated(njtree.square_of(d, len(names)))
    return njtree.newick(njtree.NjTree(node, length, len(names)), names)


def reference_run(case_id, packed, mat, inparalog, ref_len, gd, self_id, allowed_sigma, rooting):
    """PEP.filt_per_group on one case -> (the rows of each returned matrix, the tree text it was given or None, seconds spent behind the tree text)"""
    n = len(packed)
    PEP.params = dict(self_id=self_id, allowed_sigma=allowed_sigma, clust_identity=CLUST_IDENTITY, orthology='nj', nj='spy {0}')
    ete3.ROOTING = rooting
    seq_file, global_file = 'case%d.seq.npz' % case_id, 'case%d.global.npy' % case_id
    with PEP.MapBsn(seq_file, 'w') as store:
        member = np.empty(n, dtype=object)
        for k in range(n):
            member[k] = packed[k]
        store.save(7, member)
    table = np.empty((len(gd), 2), dtype=object)
    for k, (key, val) in enumerate(sorted(gd.items())):
        table[k, 0], table[k, 1] = key, val
    np.save(global_file, table, allow_pickle=True)
    seen = dict(text=None, t0=None)
    real_popen = PEP.subprocess.Popen

    class SpyPopen(object):
        def __init__(self, cmd, *a, **k):
            seen['text'] = text_of_fasta(cmd[1])
            if seen['text'] is None:
                raise ValueError('undefined distance')

        def communicate(self):
            seen['t0'] = time.perf_counter()
            return seen['text'], ''

    PEP.subprocess.Popen = SpyPopen
    try:
        res = PEP.filt_per_group([mat, inparalog, ref_len, seq_file, global_file])
        spent = time.perf_counter() - seen['t0'] if seen['t0'] is not None else 0.
    finally:
        PEP.subprocess.Popen = real_popen
        os.unlink(seq_file)
        os.unlink(global_file)
    for m in res:
        assert np.array_equal(m, mat[m[:, 6]])
    return [m[:, 6].tolist() for m in res], seen['text'], spent


def restated_run(packed, mat, inparalog, ref_len, gd, self_id, allowed_sigma, text, report):
    """the same through this project's host layers and the numpy restatement of K25"""
    n = len(packed)
    if text is None:
        return [list(range(n))]
    mine = restate(packed, ref_len, mat[:, 1], inparalog, gd, self_id, allowed_sigma)
    _, mut, aln = pair_counts(packed, ref_len)
    diff = np.zeros((n, n, 2))
    diff[:, :, 0], diff[:, :, 1] = np.array(mut, dtype=float), np.array(aln, dtype=float)
    distances = orthofilter.distances_from_diff(diff, mat[:, 1], orthofilter.gd_table(gd, self_id, allowed_sigma))
    incompatible, needs_tree = orthofilter.incompatible_of(distances, mine['groups'])
    assert needs_tree
    leaves = np.array([g[0] for g in mine['groups']])
    names, branches = njtree.parse_newick(text)
    sets, lengths = treecut.branch_sets(names, branches, leaves)
    strong = mat[leaves, 4].astype(np.float64) >= (CLUST_IDENTITY - 0.02) * 10000
    inc = incompatible[np.ix_(leaves, leaves)]
    cut = H.cut_restated(H.sides_of(sets, len(leaves)), lengths, inc[:, :, 0], inc[:, :, 1], strong, report=report)
    report['n_ties'], report['n_cuts'], report['leaves'] = cut['n_ties'], cut['n_cuts'], len(leaves)
    return [[int(r) for r in m[:, 6]] for m in orthofilter.mats_of_cut(mat, mine['groups'], leaves, cut['part'], cut['n_parts'])]


def make_case(rng, sizes, L, far, near, sub, gap, weak):
    """clades of the given sizes, `far` apart; within a clade sub-clusters `near` apart whose rows differ by `sub` (<= 1 %: they share a leader);
    weak: the clades whose rows all score below the clust_identity bound"""
    anc = rng.integers(1, 5, L)
    rows, iden = [], []
    for c, size in enumerate(sizes):
        top = clade(rng, anc, 1, far)[0]
        left = size
        while left > 0:
            k = int(min(left, rng.integers(1, 4)))
            mid = clade(rng, top, 1, near)[0]
            rows.append(clade(rng, mid, k, sub, gap=gap))
            iden += [int(rng.integers(8000, 8700)) if c in weak else int(rng.integers(8900, 9900)) for _ in range(k)]
            left -= k
    codes = np.concatenate(rows)
    order = rng.permutation(len(codes))
    return codes[order], np.array(iden)[order]


def main():
    rng = np.random.default_rng(2828)
    plans = []
    for sizes, weak in (((3, 3), ()), ((4, 5, 3), ()), ((6, 2, 4, 5), (1,)), ((2, 7), (0,)), ((8, 8, 8), ()), ((5, 4, 6, 3, 4), (3,)), ((12, 9), ()), ((3, 3, 3, 3, 3, 3), (2, 4)),
                        ((1, 1), ()), ((1, 2, 1), ()), ((10, 14, 9, 11), ())):
        plans.append(('dyadic', sizes, weak))
    for sizes, weak in (((3, 4), ()), ((5, 4, 4), ()), ((6, 3, 5, 4), (2,)), ((9, 7), (1,)), ((4, 4, 4, 4, 4), ()), ((2, 2), ()), ((11, 8, 10), ())):
        plans.append(('float', sizes, weak))
    plans.append(('calm', (6,), ()))
    cases, spent, n_cut, n_dropped = [], 0., 0, 0
    for k, (kind, sizes, weak) in enumerate(plans):
        if kind == 'dyadic':
            L, gap, self_id, sigma = 1022, 0., 2.0 ** -5, 3
            codes, iden = make_case(rng, sizes, L, 0.09, 0.02, 0.002, gap, weak)
            val = (2.0 ** -5, 0.0)
        elif kind == 'float':
            L, gap, self_id, sigma = int(rng.integers(300, 700)), 0.02, 0.005, 3
            codes, iden = make_case(rng, sizes, L, 0.2, 0.03, 0.003, gap, weak)
            val = (0.02, 0.5)
        else:
            L, gap, self_id, sigma = 300, 0.02, 0.005, 3
            codes, iden = clade(rng, rng.integers(1, 5, L), sizes[0], 0.002, gap=0.02), np.full(sizes[0], 9500)
            val = (0.05, 0.5)
        n = len(codes)
        genomes = rng.permutation(n) + 1
        gd = {(int(a), int(b)): val for a in sorted(genomes) for b in sorted(genomes) if a < b}
        inparalog = bool(k % 2)
        packed = pack_codes(codes, rng)
        mat = np.zeros((n, 7), dtype=np.int64)
        mat[:, 1], mat[:, 4], mat[:, 5], mat[:, 6] = genomes, iden, 7000 + np.arange(n), np.arange(n)
        returned, text, t = reference_run(k, packed, mat, inparalog, L, gd, self_id, sigma, 'midpoint')
        other, text2, _ = reference_run(k, packed, mat, inparalog, L, gd, self_id, sigma, 'other')
        assert text == text2
        assert returned == other, ('the rooting shows', kind, sizes, returned, other)
        spent += t
        report = {}
        mine = restated_run(packed, mat, inparalog, L, gd, self_id, sigma, text, report)
        assert mine == returned, (kind, sizes, mine, returned)
        if text is not None:
            assert report['n_ties'] == 0, (kind, sizes)
            if kind == 'float' and report['scored']:
                assert report['ic0_margin'] > 1e-9 and report['gap'] > 1e-9, (kind, sizes, report)
            n_cut += report['n_cuts'] > 0
            n_dropped += sum(len(m) for m in returned) < n
        assert (text is None) == (kind == 'calm'), (kind, sizes)
        print('%-7s %-22s n %3d leaves %3s cuts %2s returned %s' % (kind, sizes, n, report.get('leaves', '-'), report.get('n_cuts', '-'), [len(m) for m in returned]))
        cases.append(dict(name='%s_%s_%d' % (kind, 'x'.join(map(str, sizes)), k), kind=kind, n=n, ref_len=L, rows=[base64.b64encode(r.tobytes()).decode() for r in packed],
                          genomes=genomes.tolist(), identity=iden.tolist(), inparalog=inparalog, global_differences=[[a, b, m, s] for (a, b), (m, s) in sorted(gd.items())],
                          self_id=self_id, allowed_sigma=sigma, clust_identity=CLUST_IDENTITY, text=text, returned=returned))
    assert n_cut >= 12 and n_dropped >= 3, (n_cut, n_dropped)
    out = os.path.join(HERE, 'g28_treecut.json.gz')
    with gzip.GzipFile(out, 'wb', mtime=0) as f:
        f.write(json.dumps(dict(source='PEPPAN.py:326-484 (filt_per_group over a stand-in for ete3, rooted two ways; subprocess.Popen returns the tree text of K21)',
                                cases=cases), separators=(',', ':')).encode())
    print(out, os.path.getsize(out), 'bytes,', len(cases), 'cases,', n_cut, 'with cuts,', n_dropped, 'with dropped rows')
    print('the reference\'s lines behind the tree text (:417-482) with the stand-in, all cases, one thread of the build machine: %.1f ms' % (spent * 1000))
    assert os.path.getsize(out) < 700 << 10


if __name__ == '__main__':
    main()
