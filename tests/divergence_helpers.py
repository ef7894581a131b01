"""Shared by test_divergence_host.py / test_gpu_divergence.py (and tests/golden/make_golden_divergence.py, to classify its cases): the g20
fixture and an independent restatement of the divergence verdicts of filt_per_group, written from the contract - plain Python loops over
the pair counts of allele_diff_helpers.numpy_tri_edge, one pair at a time (not from the library, not vectorised as distances_from_diff is).

    gd        = (max(self_id, 2.0 / aln), 0.0) if genome[a] == genome[b] else global_differences.get(key, (0.5, 0.6))
    checkDiv  : mut / aln / (gd[0] * exp(gd[1] * sqrt(allowed_sigma))) > 1      rows a in {first, last} against every b != a
    distances : d = mut / aln / (gd[0] * exp(gd[1] * allowed_sigma)); beyond when d / gd[0] > 1 / gd[0]       all a < b
    leaders   : rows in order; j joins the FIRST leader g with mut(g, j) <= 0.01 * aln(g, j), else becomes a leader
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
