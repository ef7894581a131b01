#!/usr/bin/env python3
"""Generate tests/golden/g22_synteny.json.gz by IMPORTING the reference's Python (build machine only: needs /root/reference).

    python tests/golden/make_golden_synteny.py

The same shim as make_golden_ingroup.py, with PEP.pool2 replaced by an object whose imap_unordered is map.  Two kinds of cases, all seeded:
    groups      PEP.ite_synteny_resolver (PEPPAN.py:1097-1151) on (grp_tag, ids, co_genomes, neighbors, nNeighbor) -> what it returns;
    runs        PEP.synteny_resolver (PEPPAN.py:1153-1191) on a Prediction file -> the text of <prefix>.synteny.Prediction.
Only DATA is written - the inputs and the recorded results - none of the reference's source text.  The restatement of tests/synteny_helpers.py
is held to every case, and the conditions the fixture is pinned by are asserted at the end.
"""
import gzip, json, os, stat, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'


def build_shim():
    root = tempfile.mkdtemp(prefix='peppan_shim_')
    os.makedirs(os.path.join(root, 'bin'))
    for t in ('mmseqs', 'makeblastdb', 'diamond', 'blastn'):
        p = os.path.join(root, 'bin', t)
        with open(p, 'w') as f:
            f.write('#!/bin/sh\nexit 0\n')
        os.chmod(p, os.stat(p).st_mode | stat.S_IEXEC | stat.S_IXGRP | stat.S_IXOTH)
    for pkg, body in (('numba', 'def jit(*a, **k):\n    if len(a) == 1 and callable(a[0]) and not k:\n        return a[0]\n    return lambda f: f\n'),
                      ('ete3', 'class Tree(object):\n    pass\n')):
        os.makedirs(os.path.join(root, 'py', pkg))
        with open(os.path.join(root, 'py', pkg, '__init__.py'), 'w') as f:
            f.write(body)
    os.makedirs(os.path.join(root, 'cwd'))
    return root


SHIM = build_shim()
os.environ['PATH'] = os.path.join(SHIM, 'bin') + os.pathsep + os.environ['PATH']
sys.path[:0] = [os.path.join(SHIM, 'py'), os.path.join(REF, 'modules'), REF, os.path.dirname(HERE)]
os.chdir(os.path.join(SHIM, 'cwd'))

import numpy as np                       # noqa: E402
if not hasattr(np.lib.npyio, 'format'):  # numpy >= 2 dropped this alias of np.lib.format; the reference's MapBsn spells it the old way
    np.lib.npyio.format = np.lib.format
import PEPPAN as PEP                     # noqa: E402
from synteny_helpers import locus_group, parse_prediction, record_of, restate, same_record   # noqa: E402


class SerialPool(object):
    imap_unordered = staticmethod(map)


PEP.pool2 = SerialPool()


def group_plans(rng):
    """(name, nNeighbor, maker) of every recorded group"""
    plans = []
    # the smallest conflict distance at each of 1 .. 5 (nNeighbor 2): full lists against lists of 6, 5, 4, 3, 2 ids that share nothing
    for short, dc in ((6, 5), (5, 4), (4, 3), (3, 2), (2, 1)):
        for k in range(7):
            n = int(rng.integers(4, 16))
            plans.append(('dc%d' % dc, 2, lambda n=n, short=short: locus_group(rng, n, max(2, n // 3), 3, sizes=(6, short), noise=0., drop=0.)))
    # shared noise codes: merges the walk tries and has to skip
    for k in range(30):
        n = int(rng.integers(5, 40))
        plans.append(('noise', 2, lambda n=n: locus_group(rng, n, max(2, n // 4), int(rng.integers(2, 5)), sizes=(6, 6, 7), noise=0.25, pool=4, drop=0.05)))
    # a stray member of a genome of its own that shares nothing: refused splits
    for k in range(20):
        n = int(rng.integers(3, 14))
        plans.append(('stray', 2, lambda n=n, k=k: locus_group(rng, n, 2, 2, sizes=((6,), (7,), (9,), (6, 7, 9))[k % 4], noise=0., drop=0., stray=1 + k % 2)))
    # no conflict at all: every member in a genome of its own, or one neighbourhood shared by all
    for k in range(10):
        n = int(rng.integers(2, 12))
        plans.append(('apart', 2, lambda n=n: (list(range(n)), locus_group(rng, n, 1, 3, sizes=(6,), noise=0.1)[1])))
    for k in range(10):
        n = int(rng.integers(2, 12))
        plans.append(('one-locus', 2, lambda n=n: locus_group(rng, n, 3, 1, sizes=(6, 7), noise=0., drop=0.)))
    # list sizes: empty lists, 7, 9 and 20 and more ids
    for sizes in ((0, 6), (0, 1, 6), (7,), (9,), (20, 24), (6, 40), (0, 7, 9, 22)):
        for k in range(3):
            n = int(rng.integers(4, 20))
            plans.append(('lists', 2, lambda n=n, sizes=sizes: locus_group(rng, n, max(2, n // 3), 3, sizes=sizes, noise=0.1, pool=5, drop=0.05)))
    # nNeighbor 1 and 3
    for nn in (1, 3):
        for k in range(12):
            n = int(rng.integers(3, 24))
            plans.append(('nn%d' % nn, nn, lambda n=n, k=k: locus_group(rng, n, max(2, n // 3), 3, sizes=((6,), (5, 6), (6, 7, 9), (3, 6))[k % 4], noise=0.15 * (k % 3), pool=4,
                                                                  stray=k % 2)))
    # plain random groups
    for k in range(20):
        n = int(rng.integers(2, 40))
        plans.append(('random', 2, lambda n=n: locus_group(rng, n, int(rng.integers(1, 6)), int(rng.integers(1, 6)), sizes=(0, 3, 5, 6, 6, 6, 7, 9), noise=0.2, pool=6, drop=0.1,
                                                            stray=int(rng.integers(0, 2)))))
    # large groups: more than one chunk of 64 members, one beyond 256
    for n in (65, 70, 96, 128, 130, 260):
        plans.append(('large', 2, lambda n=n: locus_group(rng, n, 12, 5, sizes=(6, 6, 7), noise=0.08, pool=6, drop=0.03)))
    return plans


def make_run(rng, genomes, variant):
    """the text of a Prediction table: per genome one or two contigs with a backbone of shared genes, the family P at two neighbourhoods of
    every genome, Q/2 likewise (a name that ends in /digits), S twice in ONE genome and nowhere else (a group of one genome), one id that spans two
    rows, and one id that no row carries"""
    rows, gid = [], 0
    for g in range(genomes):
        genome = 'G%02d' % g
        order = ['b%02d' % k for k in range(24)]
        extra = [('P', 3), ('P', 15), ('Q/2', 8), ('Q/2', 20)]
        if g == 1:
            extra += [('S', 5), ('S', 6)]
        if variant == 2 and g % 2 == 0:
            extra += [('P', 22)]                    # a third copy at a third neighbourhood
        for name, at in sorted(extra, key=lambda e: -e[1]):
            order.insert(at, name)
        if variant == 1 and g == 2:
            order = order[:10] + order[14:]          # a deletion next to a copy: a shorter neighbourhood
        pos = 100
        for k, name in enumerate(order):
            contig = '%s_c%d' % (genome, 1 if k < 18 or variant == 0 else 2)
            gid += 1
            if (g, k) == (0, 4):
                gid += 1                            # a gap: this id is carried by no row
            length = int(rng.integers(300, 1500))
            parts = [(pos, pos + length)]
            if (g, k) == (1, 9) or (variant == 2 and (g, k) == (3, 3)):
                cut = pos + length // 2             # one id in two rows
                parts = [(pos, cut - 10), (cut + 10, pos + length)]
            for a, b in parts:
                s, e = (a, b) if rng.random() < 0.5 else (b, a)
                rows.append([name, int(rng.integers(1, 5)), gid, genome, '%s_%04d' % (genome, k), contig, int(rng.integers(8000, 10001)) / 100., 1, abs(b - a) + 1, s, e,
                             abs(b - a) + 1, int(rng.integers(0, 3)), int(rng.integers(100, 3000)), '%dM' % (abs(b - a) + 1)])
            pos += length + int(rng.integers(20, 300))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    assert len({tuple(str(v) for v in r[1:]) for r in rows}) == len(rows)
    return ''.join('\t'.join(str(v) for v in r) + '\n' for r in rows)


def main():
    rng = np.random.default_rng(22000)
    groups, tally = [], dict(none=0, refused=0, partition=0, skipped=0, n65=0, n257=0)
    dcs, nns, list_sizes = {}, set(), set()
    for k, (name, nn, make) in enumerate(group_plans(rng)):
        genome, lists = make()
        n = len(genome)
        ids = np.cumsum(rng.integers(1, 4, n)).astype(np.int64)
        tag = int(rng.integers(1, 5000))
        got = PEP.ite_synteny_resolver([tag, ids, np.array(genome, dtype=np.int64), [set(a) for a in lists], nn])
        rec = record_of(got)
        mine, detail = restate(tag, ids.tolist(), genome, lists, nn)
        assert same_record(rec, mine), (name, k, rec, mine)
        tally[rec['verdict']] += 1
        tally['skipped'] += int(detail['skipped'] > 0)
        tally['n65'] += int(n >= 65)
        tally['n257'] += int(n >= 257)
        if detail['has'] and nn == 2:
            dcs[detail['dc']] = dcs.get(detail['dc'], 0) + 1
        nns.add(nn)
        list_sizes |= {len(a) for a in lists}
        groups.append(dict(name='%s_n%d_%d' % (name, n, k), tag=tag, ids=ids.tolist(), genomes=[int(g) for g in genome], neighbors=[[int(v) for v in a] for a in lists],
                           nNeighbor=nn, returned=rec))
    print(len(groups), 'groups', tally, 'dc', sorted(dcs.items()), 'list sizes', sorted(list_sizes))
    assert len(groups) >= 150
    assert min(tally['none'], tally['refused'], tally['partition'], tally['skipped']) >= 15, tally
    assert all(dcs.get(d, 0) >= 5 for d in (1, 2, 3, 4, 5)), dcs
    assert nns == {1, 2, 3}
    assert {0, 6, 7, 9} <= list_sizes and max(list_sizes) >= 20
    assert tally['n65'] >= 5 and tally['n257'] >= 1, tally

    runs = []
    for variant, genomes in enumerate((4, 5, 6)):
        text = make_run(rng, genomes, variant)
        with open('run%d.Prediction' % variant, 'w') as f:
            f.write(text)
        out = PEP.synteny_resolver('run%d' % variant, 'run%d.Prediction' % variant, 2)
        with open(out) as f:
            after = f.read()
        before_names, after_names = {r[0] for r in parse_prediction(text)}, {r[0] for r in parse_prediction(after)}
        assert 'Q/2/0.1' in after_names and 'P/0.1' in after_names and 'S' in after_names and not any(n.startswith('S/') for n in after_names), sorted(after_names - before_names)
        runs.append(dict(nNeighbor=2, prediction=text, synteny_prediction=after))
        print('run', variant, len(parse_prediction(text)), 'rows, new names', sorted(after_names - before_names))
    out = os.path.join(HERE, 'g22_synteny.json.gz')
    with gzip.GzipFile(out, 'wb', mtime=0) as f:
        f.write(json.dumps(dict(source='PEPPAN.py:1097-1151 (ite_synteny_resolver), 1153-1191 (synteny_resolver)', groups=groups, runs=runs), separators=(',', ':')).encode())
    print(out, os.path.getsize(out), 'bytes')
    assert os.path.getsize(out) < 700 << 10


if __name__ == '__main__':
    main()
