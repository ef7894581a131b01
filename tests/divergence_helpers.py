"""Shared by test_divergence_host.py / test_gpu_divergence.py (and tests/golden/make_golden_divergence.py, to classify its cases): the g20
fixture and an independent restatement of the divergence verdicts of filt_per_group, written from the contract - plain Python loops over
the pair counts of allele_diff_helpers.numpy_tri_edge, one pair at a time (not from the library, not vectorised as distances_from_diff is).

    gd        = (max(self_id, 2.0 / aln), 0.0) if genome[a] == genome[b] else global_differences.get(key, (0.5, 0.6))
    checkDiv  : mut / aln / (gd[0] * exp(gd[1] * sqrt(allowed_sigma))) > 1      rows a in {first, last} against every b != a
    distances : d = mut / aln / (gd[0] * exp(gd[1] * allowed_sigma)); beyond when d / gd[0] > 1 / gd[0]       all a < b
    leaders   : rows in order; j joins the FIRST leader g with mut(g, j) <= 0.01 * aln(g, j), else becomes a leader

For groups too large for plain Python loops (thousands of rows): matmul_counts (the pair counts as one-hot matrix products, independent of
numpy_tri_edge) and leaders_numpy (the leader rule alone, one numpy comparison per row); test_divergence_host.py pins both against restate.
"""
import base64
import gzip
import json
import os

import numpy as np

from allele_diff_helpers import decode_rows, numpy_tri_edge, square_from_tri

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_g20():
    with gzip.open(os.path.join(GOLDEN, 'g20_divergence.json.gz')) as f:
        cases = json.loads(f.read().decode())['cases']
    for c in cases:
        s = -(-c['ref_len'] // 3)
        c['packed'] = np.frombuffer(base64.b64decode(c['rows']), dtype=np.uint8).reshape(c['n'], s)
        c['genomes'] = np.array(c['genomes'], dtype=np.int64)
        c['gd'] = {(int(g1), int(g2)): (float(m), float(sg)) for g1, g2, m, sg in c['global_differences']}
    return cases


def pair_counts(packed, ref_len):
    """-> (tri int64[n(n-1)/2, 2], mut, aln as nested lists over [a][b], filled for a < b)"""
    seqs = decode_rows(packed, ref_len)
    tri, _ = numpy_tri_edge(seqs)
    sq = square_from_tri(len(seqs), tri)
    return tri, sq[:, :, 0].tolist(), sq[:, :, 1].tolist()


def restate(packed, ref_len, genomes, inparalog, gd, self_id, allowed_sigma, counts=None):
    """-> dict(verdict, divergent, edge_divergent (the first / last row of the whole group alone decide), beyond, groups, leader, tri)"""
    n = len(packed)
    out = dict(verdict=0, divergent=False, edge_divergent=False, beyond=False, groups=None, leader=None, tri=None)
    if n < 2:
        return out
    tri, mut_of, aln_of = counts if counts is not None else pair_counts(packed, ref_len)
    out['tri'] = tri
    genomes = [int(g) for g in genomes]
    cache = {}

    def bounds(a, b, aln):
        """(gd0, checkDiv's denominator, the distances' denominator) of rows a, b"""
        if genomes[a] == genomes[b]:
            gd0 = max(self_id, 2.0 / aln)
            return gd0, gd0 * float(np.exp(0. * np.sqrt(allowed_sigma))), gd0 * float(np.exp(0. * allowed_sigma))
        key = (min(genomes[a], genomes[b]), max(genomes[a], genomes[b]))
        if key not in cache:
            g = gd.get(key, (0.5, 0.6))
            cache[key] = (g[0], g[0] * float(np.exp(g[1] * np.sqrt(allowed_sigma))), g[0] * float(np.exp(g[1] * allowed_sigma)))
        return cache[key]

    def pair(a, b):
        lo, hi = (a, b) if a < b else (b, a)
        return float(mut_of[lo][hi]), float(aln_of[lo][hi])

    def check_div(rows):
        for a in (rows[0], rows[-1]):
            for b in rows:
                if a != b:
                    mut, aln = pair(a, b)
                    if mut / aln / bounds(a, b, aln)[1] > 1:
                        return True
        return False

    out['edge_divergent'] = check_div(list(range(n)))
    divergent = out['edge_divergent']
    if inparalog and not divergent:
        by_genome = {}
        for k, g in enumerate(genomes):
            by_genome.setdefault(g, []).append(k)
        divergent = any(check_div(rows) for rows in by_genome.values() if len(rows) > 1)
    out['divergent'] = divergent
    if not divergent:
        return out
    beyond = False
    for a in range(n):
        for b in range(a + 1, n):
            mut, aln = pair(a, b)
            gd0, _, den = bounds(a, b, aln)
            d = mut / aln / den
            if d / gd0 > 1 / gd0:
                beyond = True
                break
        if beyond:
            break
    out['beyond'] = beyond
    out['verdict'] = 2 if beyond else 1
    if beyond:
        groups, leader = [], [0] * n
        for j in range(n):
            for g in groups:
                mut, aln = pair(g[0], j)
                if mut <= 0.01 * aln:
                    g.append(j)
                    leader[j] = g[0]
                    break
            else:
                groups.append([j])
                leader[j] = j
        out['groups'], out['leader'] = groups, np.array(leader, dtype=np.uint32)
    return out


def restate_distances(n, mut_of, aln_of, genomes, gd, self_id, allowed_sigma):
    """distances float64[n, n, 2] (PEPPAN.py:371-380), one pair at a time"""
    genomes = [int(g) for g in genomes]
    distances = np.zeros((n, n, 2), dtype=np.float64)
    for a in range(n):
        for b in range(a + 1, n):
            mut, aln = float(mut_of[a][b]), float(aln_of[a][b])
            if genomes[a] == genomes[b]:
                g = (max(self_id, 2.0 / aln), 0.)
            else:
                g = gd.get((min(genomes[a], genomes[b]), max(genomes[a], genomes[b])), (0.5, 0.6))
            d = mut / aln / (g[0] * float(np.exp(g[1] * allowed_sigma)))
            distances[a, b] = distances[b, a] = (d / g[0], 1 / g[0])
    return distances


def restate_incompatible(distances, groups):
    """incompatible float64[n, n, 2] (PEPPAN.py:400-405) with a plain running sum per pair of leader groups, rows of the first group outside"""
    incompatible = np.zeros(distances.shape, dtype=np.float64)
    for i1, g1 in enumerate(groups):
        for g2 in groups[i1 + 1:]:
            s0 = s1 = 0.
            for a in g1:
                for b in g2:
                    s0 += float(distances[a, b, 0])
                    s1 += float(distances[a, b, 1])
            incompatible[g1[0], g2[0]] = incompatible[g2[0], g1[0]] = (s0, s1)
    return incompatible


def verdict_table(groups_packed, ref_lens):
    """list of packed [n, s] matrices -> (packed, row_off, row_len, index lists) of one row table"""
    rows = [r for p in groups_packed for r in p]
    row_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    row_len = np.concatenate([np.full(len(p), L, dtype=np.uint32) for p, L in zip(groups_packed, ref_lens)]) if rows else np.zeros(0, np.uint32)
    starts = np.concatenate([[0], np.cumsum([len(p) for p in groups_packed])])
    index = [np.arange(a, b, dtype=np.uint32) for a, b in zip(starts[:-1], starts[1:])]
    return (np.concatenate(rows) if rows else np.zeros(0, np.uint8)), row_off, row_len, index


def pack_codes(codes, rng=None):
    """int codes [n, L] of 0..4 -> packed uint8[n, ceil(L / 3)]; digits past L random when rng is given"""
    n, L = codes.shape
    s = -(-L // 3)
    full = rng.integers(0, 5, (n, 3 * s)) if rng is not None else np.zeros((n, 3 * s), dtype=np.int64)
    full[:, :L] = codes
    return (full[:, :s] * 25 + full[:, s:2 * s] * 5 + full[:, 2 * s:]).astype(np.uint8)


def clade(rng, anc, n, div, gap=0.):
    """n rows off one ancestor (codes 1..4): every column of every row replaced by another base with probability `div`, gapped with `gap`"""
    codes = np.repeat(anc[None, :], n, axis=0)
    mut = rng.random(codes.shape) < div
    codes[mut] = (codes[mut] - 1 + rng.integers(1, 4, int(mut.sum()))) % 4 + 1
    codes[rng.random(codes.shape) < gap] = 0
    return codes


def fuzz_groups(seed, count, n_max):
    """groups aimed in turn at the three verdicts (what comes out is the restatement's business): a calm clade of genomes that mostly know each
    other; a clade between checkDiv's bound and the distances' bound (allowed_sigma 5, where the two are far apart); and clades far apart or
    rows far from each other, with genomes that repeat.  n log-uniform in 2 .. n_max, ref_len 30 .. 3 000, gap rates 0 .. 0.3."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n = int(np.exp(rng.uniform(np.log(2), np.log(n_max + 1))))
        L = int(rng.integers(30, 3001))
        aim, self_id = k % 3, (0.002, 0.005)[(k // 3) % 2]
        sigma = 5 if aim == 1 else (1, 3, 5)[(k // 3) % 3]
        genomes = rng.permutation(n) + 1
        if aim == 0:
            codes = clade(rng, rng.integers(1, 5, L), n, rng.uniform(0, 0.004), gap=rng.uniform(0, 0.3))
            if n > 5 and rng.random() < 0.5:             # a genome twice among the inner rows: seen by an in-paralog sub-group only
                genomes[n // 2] = genomes[1]
        elif aim == 1:
            L = max(L, 400)
            lo, hi = 0.02 * np.exp(0.5 * np.sqrt(sigma)), 0.02 * np.exp(0.5 * sigma)
            codes = clade(rng, rng.integers(1, 5, L), n, np.sqrt(lo * hi) / 2 * rng.uniform(0.85, 1.15), gap=rng.uniform(0, 0.1))
        else:
            codes = clade(rng, rng.integers(1, 5, L), n, rng.choice([0.002, 0.01, 0.15]), gap=rng.uniform(0, 0.3))
            if n > 4 and rng.random() < 0.6:             # a second clade far from the first
                codes[n // 2:] = clade(rng, rng.integers(1, 5, L), n - n // 2, rng.choice([0.002, 0.006]))
            genomes = rng.integers(0, max(2, int(n * rng.choice([0.7, 3.0]))), n)
        ids = sorted(set(genomes.tolist()))
        keep = 1.0 if aim == 1 else 0.9
        gd = {(a, b): (0.02, 0.5) for i, a in enumerate(ids) for b in ids[i + 1:] if rng.random() < keep}
        out.append(dict(packed=pack_codes(codes, rng), ref_len=L, genomes=genomes, inparalog=bool(rng.integers(0, 2)), gd=gd, self_id=self_id, allowed_sigma=sigma))
    return out


def matmul_counts(seqs):
    """seqs uint8[n, L] of 0 / ASCII ACGT (decode_rows) -> (mut, aln) int32[n, n], symmetric: mut = mismatch + 1, aln = comparable + 2 of every pair of
    rows.  Matching columns = the sum over the four bases of onehot @ onehot.T, comparable columns = valid @ valid.T, mismatch = comparable -
    matching.  float32 products and sums of 0 / 1 are exact while a count stays below 2^24."""
    assert seqs.shape[1] < 1 << 24
    valid = (seqs > 0).astype(np.float32)
    comparable = valid @ valid.T
    matching = np.zeros_like(comparable)
    for base in b'ACGT':
        onehot = (seqs == base).astype(np.float32)
        matching += onehot @ onehot.T
    return (comparable - matching).astype(np.int32) + 1, comparable.astype(np.int32) + 2


def tri_from_square(mut, aln):
    """the packed upper triangle int32[n(n-1)/2, 2] in row-major pair order of two [n, n] arrays"""
    upper = np.triu(np.ones(mut.shape, dtype=bool), 1)
    return np.stack([mut[upper], aln[upper]], axis=1)


def leaders_numpy(mut, aln):
    """mut, aln: the integer [n, n] pair counts (read at [l, j] with l < j only) -> uint32[n], the row that leads row j.
    The contract: the rows are taken in order; row j joins the FIRST leader l, in the order in which the leaders were made, for which
    float(mut[l, j]) <= 0.01 * float(aln[l, j]) - one correctly rounded double product, one comparison -; when there is none, row j becomes the
    newest leader and leads itself.  Row 0 is therefore always a leader."""
    n = len(mut)
    out = np.zeros(n, dtype=np.uint32)
    leaders = np.zeros(n, dtype=np.int64)
    count = 0
    for j in range(n):
        l = leaders[:count]
        hit = np.flatnonzero(mut[l, j].astype(np.float64) <= 0.01 * aln[l, j].astype(np.float64))
        if len(hit):
            out[j] = l[hit[0]]
        else:
            leaders[count] = out[j] = j
            count += 1
    return out


def matching_leaders(mut, aln, lead, j):
    """the leaders (rows, in leader order) in front of row j that row j matches, from the same counts: what makes "the first one wins" a decision"""
    l = np.flatnonzero(lead[:j] == np.arange(j))
    return l[mut[l, j].astype(np.float64) <= 0.01 * aln[l, j].astype(np.float64)]


def founders_group(rng, D, L, variants=(), between=(), behind=()):
    """A group of D founders - independent uniformly random gap-free rows of L columns, about 3 L / 4 columns apart, so each of them becomes a leader,
    and founder p is leader number p - and of followers, for the leader rule at L = 200 (aln = 202, 0.01 * aln = 2.02: two rows match iff they
    differ in at most ONE column).
      variants  (src, var): the founder at leader position `var` is replaced by founder `src` with two columns changed - three columns from a match,
                so it stays a leader; behind everything else comes a follower made of founder `src` with one of the two changes: one column from
                both, it must join whichever of the two is the earlier leader
      between   k: a copy of founder k three rows behind it, between the founders (from there on the row index and the leader count differ)
      behind    k: a copy of founder k behind the last founder
    -> (codes int64[n, L], row_of int64[D]: the row of every founder, joins [(row, founder it must join)], triples [(row, earlier founder, later founder)])"""
    F = rng.integers(1, 5, (D, L))
    middles = []
    for src, var in variants:
        cols = rng.choice(L, 2, replace=False)
        F[var] = F[src]
        F[var, cols] = F[src, cols] % 4 + 1
        mid = F[src].copy()
        mid[cols[0]] = F[var, cols[0]]
        middles.append(mid)
    rows, row_of, joins, triples = [], np.zeros(D, dtype=np.int64), [], []
    for p in range(D):
        row_of[p] = len(rows)
        rows.append(F[p])
        if p - 3 in between:
            joins.append((len(rows), p - 3))
            rows.append(F[p - 3])
    for k in behind:
        joins.append((len(rows), k))
        rows.append(F[k])
    for (src, var), mid in zip(variants, middles):
        joins.append((len(rows), min(src, var)))
        triples.append((len(rows), min(src, var), max(src, var)))
        rows.append(mid)
    return np.array(rows), row_of, joins, triples
