"""An independent restatement of ite_synteny_resolver (PEPPAN.py:1097-1151) in plain Python loops, one pair at a time, the loader of the
g22 fixture recorded from the reference's own functions (tests/golden/make_golden_synteny.py), and seeded group makers.  Shares no code with
peppan_amd.

The restatement, without the reference's sort of all pairs: for members m < k of a group, c = |N_m & N_k|,
    s = 3 c + max(6 - min(6, |N_m|), 6 - min(6, |N_k|), 0) + 1,  d = 3 nNeighbor - s,  flag = genomes differ.
A pair is a conflict iff the genomes are equal and d > 0.  With dc the smallest d of a conflict pair, the reference's walk reads exactly the
pairs with d < dc, in the order (d, flag, m, k), and merges the components of their ends unless a conflict pair joins the in-conflict
members of the two."""
import gzip
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
G22 = os.path.join(HERE, 'golden', 'g22_synteny.json.gz')

SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 300)         # members per group of the GPU edge test
LIST_SIZES = (0, 1, 6, 7, 8, 9, 40)                          # ids per neighbour list


def load_g22():
    with gzip.open(G22, 'rb') as f:
        return json.loads(f.read().decode())


def pair_distance(a, b, nNeighbor):
    """d of one pair from two ascending lists, an element at a time"""
    c = 0
    for x in a:
        for y in b:
            if x == y:
                c += 1
    la = len(a) if len(a) < 6 else 6
    lb = len(b) if len(b) < 6 else 6
    pad = max(6 - la, 6 - lb, 0)
    return 3 * nNeighbor - (3 * c + pad + 1)


def restate_pairs(genome, lists, nNeighbor):
    """-> dict(has, dc, conf [(m, k)] ascending, walk [(m, k)] in the order (d, flag, m, k), d_min: the smallest d of any pair)"""
    n = len(genome)
    every, conf = [], []
    for m in range(n):
        for k in range(m + 1, n):
            d = pair_distance(lists[m], lists[k], nNeighbor)
            flag = 1 if genome[m] != genome[k] else 0
            every.append((d, flag, m, k))
            if flag == 0 and d > 0:
                conf.append((m, k, d))
    if not conf:
        return dict(has=False, dc=0, conf=[], walk=[], d_min=min([e[0] for e in every], default=0))
    dc = min(c[2] for c in conf)
    walk = [e for e in every if e[0] < dc]
    walk.sort()
    return dict(has=True, dc=dc, conf=[(m, k) for m, k, _ in conf], walk=[(m, k) for _, _, m, k in walk], d_min=min(e[0] for e in every))


def restate_walk(n, conf, walk):
    """-> (verdict 0 none / 1 refused / 2 partition, [(root, [members])] in the order of the roots or None, merges skipped)"""
    if not conf:
        return 0, None, 0
    pair = set()
    hot = set()
    for m, k in conf:
        pair.add((m, k))
        pair.add((k, m))
        hot.add(m)
        hot.add(k)
    tag = list(range(n))
    A = {i: ([i] if i in hot else []) for i in range(n)}
    B = {i: ([] if i in hot else [i]) for i in range(n)}
    skipped = 0
    for m, k in walk:
        ti, tj = tag[m], tag[k]
        if ti == tj:
            continue
        clash = False
        for x in A[ti]:
            for y in A[tj]:
                if (x, y) in pair:
                    clash = True
        if clash:
            skipped += 1
            continue
        for x in A[tj] + B[tj]:
            tag[x] = ti
        A[ti] = A[ti] + A.pop(tj)
        B[ti] = B[ti] + B.pop(tj)
    for t in A:
        if not A[t]:
            return 1, None, skipped
    return 2, [(t, A[t] + B[t]) for t in sorted(A)], skipped


def restate(grp_tag, ids, co_genomes, neighbors, nNeighbor):
    """what ite_synteny_resolver returns, in the fixture's form -> (record, details): record = dict(verdict, tag, parts [[root id, [ids]]])"""
    lists = [sorted(int(v) for v in nb) for nb in neighbors]
    P = restate_pairs([int(g) for g in co_genomes], lists, nNeighbor)
    verdict, comps, skipped = restate_walk(len(ids), P['conf'], P['walk'])
    rec = dict(verdict=('none', 'refused', 'partition')[verdict], tag=None if verdict == 0 else grp_tag,
               parts=None if verdict != 2 else [[int(ids[t]), [int(ids[x]) for x in c]] for t, c in comps])
    P['skipped'] = skipped
    return rec, P


def record_of(returned):
    """the value ite_synteny_resolver (the reference's or peppan_amd's) returned, in the fixture's form"""
    tag, parts = returned
    if tag is None:
        assert parts is None
        return dict(verdict='none', tag=None, parts=None)
    if parts is None:
        return dict(verdict='refused', tag=int(tag), parts=None)
    return dict(verdict='partition', tag=int(tag), parts=[[int(k), [int(x) for x in v]] for k, v in parts.items()])


def same_record(a, b):
    """equal as the caller sees them: the dictionary's entries (their order is not observable: :1181 sorts the lists), the lists in order"""
    return a['verdict'] == b['verdict'] and a['tag'] == b['tag'] and \
        (a['parts'] is None) == (b['parts'] is None) and (a['parts'] is None or sorted(a['parts']) == sorted(b['parts']))


def case_inputs(c):
    """a recorded case -> (grp_tag, ids int64[], co_genomes int64[], [set], nNeighbor) as the reference takes them"""
    return c['tag'], np.array(c['ids'], dtype=np.int64), np.array(c['genomes'], dtype=np.int64), [set(nb) for nb in c['neighbors']], c['nNeighbor']


def flat(groups):
    """[(genome[], [list])] -> (member_off, genome, nb_off, nb) of one library call"""
    member_off, genome, nb_off, nb = [0], [], [0], []
    for g, lists in groups:
        genome += [int(v) for v in g]
        for a in lists:
            nb += [int(v) for v in a]
            nb_off.append(len(nb))
        member_off.append(len(genome))
    return (np.array(member_off, dtype=np.uint64), np.array(genome, dtype=np.uint32), np.array(nb_off, dtype=np.uint64), np.array(nb, dtype=np.uint32))


def locus_group(rng, n, n_genomes, n_loci, sizes=(6,), noise=0.1, pool=6, stray=0, drop=0.):
    """A group shaped like a paralogous family: every member sits at one of n_loci neighbourhoods (a set of codes of its own) in one of
    n_genomes genomes; its list is the locus's first `size` codes (size drawn from `sizes`), each dropped with probability `drop` or replaced
    by one of `pool` shared noise codes with probability `noise`.  `stray` further members share nothing with anybody and have a genome of
    their own.  -> (genome list, [ascending list])"""
    genome, lists = [], []
    for _ in range(n):
        locus = int(rng.integers(0, n_loci))
        size = int(sizes[int(rng.integers(0, len(sizes)))])
        own = []
        for t in range(size):
            r = rng.random()
            if r < drop:
                continue
            own.append(int(rng.integers(0, pool)) + 10 if r < drop + noise else 1000 + 100 * locus + t)
        genome.append(int(rng.integers(0, n_genomes)))
        lists.append(sorted(set(own)))
    for k in range(stray):
        genome.append(n_genomes + k)
        lists.append([50000 + 100 * k + t for t in range(int(sizes[0]))])
    return genome, lists


def parse_prediction(text):
    """Prediction text -> rows of fields (strings)"""
    return [line.split('\t') for line in text.split('\n') if line]


def prediction_columns(text):
    """-> (rows, name, gid, genome, contig, start) of a Prediction text, columns as split_names takes them"""
    rows = parse_prediction(text)
    start = [min(float(r[9]), float(r[10])) for r in rows]
    return rows, [r[0] for r in rows], [int(r[2]) for r in rows], [r[3] for r in rows], [r[5] for r in rows], start


def expected_names(text_in, text_out):
    """the name the reference gave every row of text_in, found in text_out by the row's other columns (unique in the fixture)"""
    after = {tuple(r[1:]): r[0] for r in parse_prediction(text_out)}
    rows = parse_prediction(text_in)
    assert len(after) == len(rows)
    return [after[tuple(r[1:])] for r in rows]
