"""What the K22 tests share: the restatement of get_global_difference (PEPPAN.py:1611-1666) as include/peppan_hip.h cuts it - the group selection
as the reference writes it, the dictionary walk into events over an append-only arena, the items of an event, numpy's sum restated operation by
operation, the host tail - and the reader of tests/golden/g22_globaldiff.json.gz (made by tests/golden/make_golden_globaldiff.py from the reference's own
function).  Nothing here calls the library; np.mean is used nowhere, so that test_globaldiff_host.py can hold the restated sum to the recorded results."""
import gzip
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE_SIZE, BUFFER, LEAF = 10050, 8192, 128


def log_table():
    """element i is the reference's np.log(1.005 - np.array(data) / 10000.) of a value i, whatever the length of data"""
    return np.log(1.005 - np.arange(TABLE_SIZE) / 10000.)


# ---- numpy's sum
def pairwise(v):
    """numpy's pairwise sum of a float64 vector (the inner loop of np.add.reduce over one buffer)"""
    n = len(v)
    if n < 8:
        r = np.float64(0.)
        for x in v:
            r = r + x
        return r
    if n <= LEAF:
        r = v[:8].copy()
        i = 8
        while i + 8 <= n:
            r = r + v[i:i + 8]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for x in v[i:]:
            res = res + x
        return res
    h = n // 2
    h -= h % 8
    return pairwise(v[:h]) + pairwise(v[h:])


def numpy_sum(x):
    """np.mean's sum of a float64 vector: the buffers of 8192 elements summed pairwise, their sums added left to right from 0.0"""
    s = np.float64(0.)
    for k in range(0, len(x), BUFFER):
        s = s + pairwise(x[k:k + BUFFER])
    return s


def two_means(x):
    """(m, v) of the header: m = S(x) / n, v = S((x - m) * (x - m)) / n"""
    x = np.asarray(x, dtype=np.float64)
    m = numpy_sum(x) / np.float64(len(x))
    d = x - m
    return m, numpy_sum(d * d) / np.float64(len(x))


def tail(m, v):
    """PEPPAN.py:1663-1665 as written"""
    mean_diff = min(max(m, np.log(0.02)), np.log(0.5))
    sigma = min(max(np.sqrt(v), np.log(1.6)), np.log(2.4))
    return np.exp(mean_diff), sigma


# ---- the walk
def walk(clu, bsn, genome_of_gene):
    """the dictionary walk of :1632-1659 as the header states it -> (events int64[n, 6], arena int32[], genomes: the sorted genome ids).  KeyError for a
    gene that is not in the map."""
    genomes = sorted(set(int(g) for g in genome_of_gene.values()))
    rank = {g: k for k, g in enumerate(genomes)}
    arena, events, lists = [], [], {}

    def single(gene):
        arena.append(rank[int(genome_of_gene[int(gene)])])
        return [len(arena) - 1, 1, 1]

    for rows, is_clu in ((clu, True), (bsn, False)):
        for r, q, value in rows:
            r, q = int(r), int(q)
            rr = lists[r] if r in lists else single(r)
            qq = lists.pop(q) if q in lists else single(q)
            events.append([rr[0], rr[1], qq[0], qq[1], int(value), 0 if is_clu else 1])
            if is_clu:
                rr, need = list(rr), rr[1] + qq[1]
                if need > rr[2] and rr[0] + rr[2] == len(arena):
                    arena.extend([0] * (rr[0] + need - len(arena)))
                    rr[2] = need
                elif need > rr[2]:
                    to = len(arena)
                    arena.extend([0] * (2 * need))
                    arena[to:to + rr[1]] = arena[rr[0]:rr[0] + rr[1]]
                    rr[0], rr[2] = to, 2 * need
                arena[rr[0] + rr[1]:rr[0] + need] = arena[qq[0]:qq[0] + qq[1]]
                rr[1] = need
                lists[r] = rr
    return np.array(events, dtype=np.int64).reshape(-1, 6), np.array(arena, dtype=np.int32), np.array(genomes, dtype=np.int32)


def items_by_key(events, arena):
    """the items of the header in sequence order -> dict (g1, g2) -> list of value codes, in insertion order (python dicts keep it)"""
    lists = {}
    for a_off, a_len, b_off, b_len, value, drop in np.asarray(events).reshape(-1, 6).tolist():
        for a in arena[a_off:a_off + a_len].tolist():
            for b in arena[b_off:b_off + b_len].tolist():
                if drop and a == b:
                    continue
                lists.setdefault((min(a, b), max(a, b)), []).append(value)
    return lists


def pair_statistics(events, arena, table):
    """what Context.global_diff returns, restated: (g1, g2, n, mean, var) in insertion order"""
    lists = items_by_key(events, arena)
    means = [two_means(table[np.array(codes)]) for codes in lists.values()]
    return (np.array([k[0] for k in lists], dtype=np.int32), np.array([k[1] for k in lists], dtype=np.int32),
            np.array([len(c) for c in lists.values()], dtype=np.uint64), np.array([m for m, _ in means], dtype=np.float64),
            np.array([v for _, v in means], dtype=np.float64))


# ---- the whole function
def select_rows(geneGroups, clu, bsn, geneInGenomes, nGene):
    """:1612-1629 on tables in memory (bsn with its rows of value <= 0 still in it)"""
    groupPresences = {}
    for grp, genes in geneGroups.items():
        gg = np.array([geneInGenomes[g] for g in genes])
        presence = np.unique(gg[gg >= 0], return_counts=True)
        groupPresences[grp] = [np.sum(presence[1] == 1), gg.size]
    groupScore = sorted([[-p[0], p[1] - p[0], int(hashlib.sha1(bytes(g)).hexdigest(), 16), g] for g, p in groupPresences.items() if p[0] > 1])
    selected = set()
    for g in groupScore[:nGene]:
        selected.update(int(x) for x in geneGroups[g[3]])
    clu, bsn = np.asarray(clu, dtype=np.int64).reshape(-1, 3), np.asarray(bsn, dtype=np.int64).reshape(-1, 3)
    bsn = bsn[bsn.T[2] > 0]
    return clu[[int(r) in selected for r in clu.T[0]]].reshape(-1, 3), bsn[[int(r) in selected for r in bsn.T[0]]].reshape(-1, 3)


def restated(geneGroups, clu, bsn, geneInGenomes, nGene):
    """get_global_difference -> list of ((g1, g2), (mean, sigma)) in the reference's row order; also the item count of every key"""
    sel_clu, sel_bsn = select_rows(geneGroups, clu, bsn, geneInGenomes, nGene)
    events, arena, genomes = walk(sel_clu, sel_bsn, {int(g): int(v) for g, v in geneInGenomes.items()})
    g1, g2, n, mean, var = pair_statistics(events, arena, log_table())
    return [((int(genomes[a]), int(genomes[b])), tail(m, v)) for a, b, m, v in zip(g1, g2, mean, var)], n.tolist()


# ---- the fixture
def load_cases(name='g22_globaldiff.json.gz'):
    """the cases as the generator made them: geneGroups with numpy int64 keys (what get_gene_group returns: sha1(bytes(g)) of the selection reads their
    eight bytes), the tables as int64 arrays, the expected rows as ((g1, g2), (mean, sigma)) with the floats back from their hex text"""
    with gzip.open(os.path.join(HERE, 'golden', name), 'rt') as f:
        raw = json.load(f)
    cases = []
    for c in raw['cases']:
        cases.append(dict(name=c['name'], nGene=c['nGene'], clu=np.array(c['clu'], dtype=np.int64).reshape(-1, 3), bsn=np.array(c['bsn'], dtype=np.int64).reshape(-1, 3),
                          geneInGenomes={int(g): int(v) for g, v in c['genes']},
                          geneGroups={np.int64(g): [np.int64(x) for x in members] for g, members in c['groups']},
                          shape=tuple(c['shape']),
                          rows=[((int(k[0]), int(k[1])), (float.fromhex(m), float.fromhex(s))) for k, m, s in c['rows']]))
    return cases


def write_tables(case, folder):
    """the case's two tables as the files get_global_difference reads -> (cluFile, bsnFile)"""
    prefix = os.path.join(str(folder), case['name'].replace(' ', '_'))
    np.save(prefix + '.npy', case['clu'])
    np.save(prefix + '.bsn.npy', case['bsn'])
    return prefix + '.clu', prefix + '.bsn.npy'


def same_rows(got, want):
    """an object array [k, 2] of ((g1, g2), (mean, sigma)) against the fixture's rows: keys, order, every float bit"""
    got = [((int(row[0][0]), int(row[0][1])), (float(row[1][0]), float(row[1][1]))) for row in got]
    if len(got) != len(want):
        return False
    return all(g[0] == w[0] and g[1][0].hex() == w[1][0].hex() and g[1][1].hex() == w[1][1].hex() for g, w in zip(got, want))
