"""What the K26 tests share: a plain-Python restatement of the front half of a round of filt_genes (PEPPAN.py:546-624, :641-656) as
include/peppan_hip.h defines it - lists, dicts and sets, no numpy in the arithmetic, nothing of the library -, the builders of seeded gene
tables, and the reader of the committed fixture (tests/golden/g29_batchprep.json.gz, made by tests/golden/make_golden_batchprep.py from the reference's
own filt_genes).

A table is a list of rows [exemplar, genome, score, identity, identity copy, locus, hits]; `cfl` maps a locus to its list of other_locus * 10 + kind."""
import gzip
import hashlib
import json
import math
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'g29_batchprep.json.gz')
NJ, SBH = 0, 1
BRANCHES = ('excluded', 'popped_at_0.6', 'kept_below_0.6', 'flip_1', 'flip_3', 'flip_4', 'used_positive', 'used_nonpositive', 'walk_skipped', 'walk_taken',
            'chain_kept', 'one_sided', 'foreign_locus', 'cut_low', 'cut_clust', 'cut_6g', 'final_at_threshold', 'one_row', 'sbh')


def quot(a, b):
    """one float64 division as numpy makes it: x / 0 is an infinity, 0 / 0 a NaN"""
    a, b = float(a), float(b)
    if b == 0.0:
        return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def screen(table, used, threshold):
    """stage A (:548-562) -> (the table with columns 3 and 4 rewritten, every row still there; present_iden; excluded)"""
    top = max(r[3] for r in table)
    out, present = [], 0
    for r in table:
        r = list(r)
        r[4] = int(quot(10000 * r[3], top))
        v = used.get(r[5])
        if v is None:
            present = max(present, r[4])
        else:
            r[3] = 0 if v > 0 else -r[3]
        out.append(r)
    return out, present, float(present) < threshold


def unsure_walk(order, tables, conflicts, seen=None):
    """stage B (:579-593) over the genes `order`; tables: gene -> table (rewritten: the rows with column 3 > 0 stay); conflicts: gene -> cfl.
    -> the popped genes, in order.  seen (optional dict): counts of the branches taken"""
    used2, popped = set(), []
    seen = {} if seen is None else seen
    for gene in order:
        table = tables[gene]
        pos = sum(1 for r in table if r[3] > 0)
        unsure = sum(1 for r in table if r[3] > 0 and r[5] in used2)
        if float(unsure) >= float(pos) * 0.6:
            popped.append(gene)
            if pos and unsure * 5 == pos * 3:
                seen['popped_at_0.6'] = seen.get('popped_at_0.6', 0) + 1
            continue
        if unsure:
            seen['kept_below_0.6'] = seen.get('kept_below_0.6', 0) + 1
        cfl = conflicts.get(gene, {})
        for r in table:
            if r[5] not in used2:
                used2.update(k // 10 for k in cfl.get(r[5], []))
        negative = [r for r in table if r[3] < 0]
        if negative:
            seen['flip_%d' % len(negative)] = seen.get('flip_%d' % len(negative), 0) + 1
        for r in negative[::3]:
            r[3] = -r[3]
        tables[gene] = [r for r in table if r[3] > 0]
    return popped


def _stats(table, order):
    first = {}
    for i in order:
        first.setdefault(table[i][1], i)
    return len(first), [first[table[i][1]] for i in order]


def _walk(table, cfl, order, own, seen):
    used2, kept, spared = set(), [], set()
    for i in order:
        locus = table[i][5]
        if locus in used2:
            seen['walk_skipped'] = seen.get('walk_skipped', 0) + 1
            spared.update(k // 10 for k in cfl.get(locus, []))
            continue
        kept.append(i)
        if locus in spared:                 # (named by a dropped row alone: the chain a -> b -> c)
            seen['chain_kept'] = seen.get('chain_kept', 0) + 1
        if not own:
            used2.update(k // 10 for k in cfl.get(locus, []))
        elif cfl.get(locus):                # (:653 adds a one-element list to the store's ARRAY: numpy sums them element by element)
            used2.update((k + locus * 10) // 10 for k in cfl[locus])
        else:
            used2.add(locus)
    return kept


def prune(table, cfl, mode, clust_identity, final_threshold, seen=None):
    """stage C -> (the source rows left, in final order; inparalog; final; whether two rows tied in column 2 at :603)"""
    seen = {} if seen is None else seen
    order, tie = list(range(len(table))), False
    G, best = _stats(table, order)
    if mode == NJ:
        if len(order) >= 2 * G:
            seen['walk_taken'] = seen.get('walk_taken', 0) + 1
            tie = len(set(table[i][2] for i in order)) < len(order)
            order = sorted(order, key=lambda i: -table[i][2])           # (sorted() is stable: equal keys keep their order)
            order = _walk(table, cfl, order, False, seen)
            order = sorted(order, key=lambda i: -table[i][3])
            G, best = _stats(table, order)
        n = len(order)
        if n > 3 * G and n > 1000:
            rs = [quot(table[i][4], table[b][4]) for i, b in zip(order, best)]
            down = sorted(rs, key=lambda x: (1, 0.0) if x != x else (0, x), reverse=True)
            cut = down[3 * G - 1]
            if cut >= clust_identity:
                if n > 6 * G:
                    cut, which = down[6 * G], 'cut_6g'
                else:
                    cut, which = clust_identity, 'cut_clust'
            else:
                which = 'cut_low'
            seen[which] = seen.get(which, 0) + 1
            order = [i for i, x in zip(order, rs) if x >= cut]
            G, _ = _stats(table, order)
        inparalog = len(order) > G
        low = min(table[i][3] for i in order) if order else 0
        final = len(order) <= 1 or (not inparalog and float(low) >= final_threshold)
        if len(order) == 1:
            seen['one_row'] = seen.get('one_row', 0) + 1
        elif not inparalog and float(low) == final_threshold:
            seen['final_at_threshold'] = seen.get('final_at_threshold', 0) + 1
        return order, inparalog, final, tie
    seen['sbh'] = seen.get('sbh', 0) + 1
    keep = []
    for i, b in zip(order, best):
        x, y = quot(table[i][2], table[b][2]), quot(table[i][4], table[b][4])
        rs = math.nan if (x != x or y != y) else min(x, y)
        if rs >= clust_identity:
            keep.append(i)
    order = _walk(table, cfl, keep, True, seen)
    G, _ = _stats(table, order)
    return order, len(order) > G, True, False


def front_half(genes, tab, conflict_lists, used, new_groups, mode, clust_identity, seen=None, conflicting=()):
    """:546-624 / :641-656 of one round.  genes: [(gene key x 1000, score)] as get_gene left them; tab: gene // 1000 -> table fresh from the store;
    conflict_lists: locus -> list (what load_conflict finds); used: locus -> value; new_groups: the keys of the genes that are groups already.
    conflicting: pairs (gene, partner) - exclude_gene (:736-743) takes an excluded gene's partners out of the round with it.
    -> dict(excluded, withdrawn, abandoned, after_a, popped, after_b, status, mats, inparalog, n_ties): after_a / after_b the tables at :579 / :595
    (gene -> table), status[gene] in 'final' / 'to_run', mats[gene] the matrix of :622 / :624 / :656; abandoned: the round ended at :563-564"""
    seen = {} if seen is None else seen
    out = dict(excluded=[], withdrawn=[], abandoned=False, after_a={}, popped=[], after_b={}, status={}, mats={}, inparalog={}, n_ties=0)
    threshold, final_threshold = (clust_identity - 0.02) * 10000, 10000 * clust_identity
    tables = {}
    for gene, _ in genes:
        if gene in new_groups:
            continue
        table, present, excluded = screen(tab[gene // 1000], used, threshold)
        for r, fresh in zip(table, tab[gene // 1000]):
            if r[5] in used:
                seen['used_positive' if used[r[5]] > 0 else 'used_nonpositive'] = 1
        if excluded:
            out['excluded'].append(gene)
            seen['excluded'] = seen.get('excluded', 0) + 1
        else:
            tables[gene] = [r for r in table if r[3] != 0]
    out['after_a'] = {g: [list(r) for r in t] for g, t in tables.items()}
    conflicts = {g: {r[5]: conflict_lists[r[5]] for r in t if conflict_lists.get(r[5])} for g, t in tables.items()}
    out['withdrawn'] = sorted(set(b for a, b in conflicting if a in out['excluded']) - set(out['excluded']))
    left = [g for g, _ in genes if (g in new_groups or g in tables) and g not in out['withdrawn']]
    if len(left) < len(genes) * 0.5:
        out['abandoned'] = True
        return out
    order = [g for g in sorted(left, key=lambda g: -dict(genes)[g]) if g not in new_groups]
    out['order'], out['conflicts'] = order, conflicts
    out['popped'] = unsure_walk(order, tables, conflicts, seen)
    out['after_b'] = {g: [list(r) for r in tables[g]] for g in order if g not in out['popped']}
    for g in left:
        if g in new_groups or g in out['popped']:
            continue
        table, cfl = tables[g], conflicts[g]
        own = set(r[5] for r in table)
        if any(k // 10 not in own for v in cfl.values() for k in v):
            seen['foreign_locus'] = 1
        if any(l * 10 + k % 10 not in cfl.get(k // 10, []) for l, v in cfl.items() for k in v if k // 10 in own):
            seen['one_sided'] = 1
        rows, inparalog, final, tie = prune(table, cfl, mode, clust_identity, final_threshold, seen)
        out['status'][g], out['mats'][g], out['inparalog'][g] = ('final' if final else 'to_run'), [table[i] for i in rows], inparalog
        out['n_ties'] += 1 if tie else 0
    return out


# ---- seeded tables for the library's tests
def random_gene(rng, n, n_genomes, locus0, exemplar=7, lists=0.3, list_len=3, ties2=False, ties3=False, foreign=0, tight=False):
    """a table of n rows over n_genomes genomes (every genome at least once while rows last) with its conflict lists: loci locus0 .. locus0 + n - 1 in a
    seeded order; columns 2 and 3 all different unless ties2 / ties3; tight: identities within a tenth of each other; foreign: list entries that name loci
    outside the table"""
    genomes = list(range(n_genomes))[:n] + [rng.randrange(n_genomes) for _ in range(max(0, n - n_genomes))]
    rng.shuffle(genomes)
    loci = list(range(locus0, locus0 + n))
    rng.shuffle(loci)
    c2 = rng.sample(range(10000, 10000 + 50 * n + 100), n)
    c3 = rng.sample(range(20000, 20000 + n + 50), n) if tight else rng.sample(range(7000, 7000 + 4 * n + 100), n)
    if ties2:
        c2 = [x - x % 7 for x in c2]
    if ties3:
        c3 = [x - x % 5 for x in c3]
    top = max(c3)
    table = [[exemplar, 100 + g, a, b, int(quot(10000 * b, top)), l, 1] for g, a, b, l in zip(genomes, c2, c3, loci)]
    cfl = {}
    for l in loci:
        if rng.random() < lists:
            others = [x for x in rng.sample(loci, min(n, list_len + 1)) if x != l][:list_len]
            vals = [x * 10 + rng.choice((1, 2)) for x in others] + [(locus0 + n + rng.randrange(50)) * 10 + 2 for _ in range(foreign)]
            if vals:
                cfl[l] = vals
    return table, cfl


def batch_of(cases):
    """[(table, cfl)] -> the tables of a library call: dict(gene_off, cols (seven lists), cfl_off, cfl)"""
    gene_off, cols, cfl_off, flat = [0], [[] for _ in range(7)], [0], []
    for table, cfl in cases:
        for r in table:
            for c in range(7):
                cols[c].append(r[c])
            flat += cfl.get(r[5], [])
            cfl_off.append(len(flat))
        gene_off.append(gene_off[-1] + len(table))
    return dict(gene_off=gene_off, cols=cols, cfl_off=cfl_off, cfl=flat)


def golden_inputs(G):
    """the fixture's inputs with their keys as integers -> (tab, lists, conflicting pairs of gene keys, both directions)"""
    pairs = [(a * 1000, b * 1000) for a, b, v in G['ortho_groups'] if v < 0]
    return int_keys(G['tab']), int_keys(G['lists']), pairs + [(b, a) for a, b in pairs]


def check_run(G, orthology, seen=None, each=None):
    """the restatement against what was recorded of the reference's run `orthology` at :546, :579, :595 and :658 of every round (AssertionError where
    they differ); each(round, restated): called per round that was not abandoned.  -> the rounds compared"""
    tab, lists, conflicting = golden_inputs(G)
    full = {r[5]: r for t in tab.values() for r in t}
    n = 0
    for rnd in G['runs'][orthology]['rounds']:
        start = rnd['start']
        got = front_half([(g, s) for g, s in start['genes']], tab, lists, dict((k, v) for k, v in start['used']), set(int(g) for g in start['new_groups']),
                         SBH if orthology == 'sbh' else NJ, G['clust_identity'], seen, conflicting)
        if got['abandoned']:
            assert 'after_a' not in rnd
            continue
        plain = lambda tables: {str(g): recorded(t) for g, t in tables.items()}      # noqa: E731
        assert plain(got['after_a']) == rnd['after_a']['tmpSet'], 'stage A'
        assert [g for g, _ in rnd['after_a']['genes']] == [g for g, _ in start['genes'] if g not in got['excluded'] and g not in got['withdrawn']]
        assert [g for g, _ in rnd['after_b']['genes']] == [g for g, _ in rnd['after_a']['genes'] if g not in got['popped']], 'stage B pops'
        for g, t in got['after_b'].items():
            assert recorded(t) == rnd['after_b']['tmpSet'][str(g)], ('stage B', g)
        for g, m in got['mats'].items():
            assert recorded(m) == rnd['after_c']['new_groups'][str(g)], ('stage C', g)
        assert all(full[r[5]][:3] == r[:3] for m in got['mats'].values() for r in m)
        if each is not None:
            each(rnd, got)
        n += 1
    return n


def compact(rows):
    """rows [[locus, column 3, column 4]] as the fixture records them: themselves up to 64 of them, their number and the SHA-1 of their JSON text beyond"""
    rows = [[int(x) for x in r] for r in rows]
    if len(rows) <= 64:
        return rows
    return dict(n=len(rows), sha1=hashlib.sha1(json.dumps(rows, separators=(',', ':')).encode()).hexdigest())


def recorded(table):
    """a table or matrix (rows of seven) in the fixture's form"""
    return compact([[r[5], r[3], r[4]] for r in table])


def rng_of(seed):
    return random.Random(seed)


def load_golden():
    with gzip.open(GOLDEN, 'rt') as f:
        return json.load(f)


def int_keys(d):
    return {int(k): v for k, v in d.items()}


def edge_cases():
    """name -> (table, cfl): the smallest shapes at which stage C can go wrong (tests/test_gpu_batchprep.py runs them in both modes on every path).  4096 is
    PEP_PREP_LDS_ROWS: the largest gene whose working arrays stay in LDS, and one row more"""
    rng, cases, locus0 = rng_of(26), {}, [0]

    def add(name, n, n_genomes, **kw):
        cases[name] = random_gene(rng, n, n_genomes, locus0[0], **kw)
        locus0[0] += n + 60

    for n in (1, 2, 63, 64, 65):
        add('n%d' % n, n, max(1, n // 3), lists=0.5)
    add('lds_max', 4096, 1000, lists=0.2, foreign=1)                 # n > 3 G and n > 1000: the cut, on the LDS path
    add('lds_max_plus_1', 4097, 300, lists=0.05, tight=True)         # n > 6 G, on the workspace path
    add('cut_plain', 1300, 400, lists=0.05, tight=True)
    add('one_genome', 70, 1, lists=0.3)
    add('g_equals_n', 66, 66, lists=0.5)
    add('empty_lists', 130, 40, lists=0.0)
    add('ties2', 48, 12, lists=0.8, list_len=2, ties2=True)
    add('ties3', 48, 12, lists=0.3, ties3=True)
    add('long_list', 200, 50, lists=0.1)
    table, cfl = cases['long_list']
    top = max(table, key=lambda r: r[2])
    cfl[top[5]] = [(locus0[0] + k) * 10 + 2 for k in range(4990)] + [r[5] * 10 for r in table[:11] if r is not top][:10]
    # two rows of one genome tie in column 2 and name each other: the first in table order stays
    cases['tie_decides'] = ([[7, 1, 50, 9000, 10000, locus0[0] + 6000, 1], [7, 1, 50, 8990, 9988, locus0[0] + 6001, 1], [7, 2, 40, 8980, 9977, locus0[0] + 6002, 1],
                             [7, 2, 30, 8970, 9966, locus0[0] + 6003, 1]], {locus0[0] + 6000: [(locus0[0] + 6001) * 10], locus0[0] + 6001: [(locus0[0] + 6000) * 10]})
    # ties in column 3 alone: the order the sort by column 2 left decides
    cases['tie3_order'] = ([[7, 1, 10, 9000, 9473, locus0[0] + 6010, 1], [7, 1, 20, 9000, 9473, locus0[0] + 6011, 1], [7, 2, 30, 9000, 9473, locus0[0] + 6012, 1],
                            [7, 2, 40, 9500, 10000, locus0[0] + 6013, 1]], {})
    return cases


def golden_stores(G, where):
    """the fixture's .tab and .conflicts stores and its exemplar FASTA written under `where` with this project's MapBsn -> params for filt_genes"""
    import numpy as np
    from peppan_amd.mapbsn import MapBsn
    tab, lists, _ = golden_inputs(G)
    with MapBsn(os.path.join(where, 'g.tab.npz'), 'w') as store:
        for ex, t in tab.items():
            store.save(ex, np.array(t, dtype=np.int64))
    with MapBsn(os.path.join(where, 'g.conflicts.npz'), 'w') as store:
        for m in sorted(set(r[5] // 30000 for t in tab.values() for r in t)):
            off, vals = [30001], []
            for idx in range(30000):
                vals += lists.get(m * 30000 + idx, [])
                off.append(30001 + len(vals))
            store.save(m, np.array(off + vals, dtype=np.int64))
    with open(os.path.join(where, 'clust.fas'), 'w') as f:
        for ex, n in G['clust_len'].items():
            f.write('>%s\n%s\n' % (ex, 'A' * n))
    return dict(clust=os.path.join(where, 'clust.fas'), clust_identity=G['clust_identity'], n_thread=2, map_bsn=os.path.join(where, 'g'))
