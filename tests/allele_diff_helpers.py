"""Shared by test_allele_diff_host.py / test_gpu_allele_diff.py: the g19 fixture and an independent numpy formulation of
compare_seq / compare_seqX written from their definition (not from the reference's code, not from the library's bit planes)."""
import base64
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_g19():
    with gzip.open(os.path.join(GOLDEN, 'g19_allele_diff.json.gz')) as f:
        cases = json.loads(f.read().decode())['cases']
    for c in cases:
        s = -(-c['ref_len'] // 3)
        c['packed'] = np.frombuffer(base64.b64decode(c['rows']), dtype=np.uint8).reshape(c['n'], s)
        c['tri'] = np.array(c['tri'], dtype=np.int64).reshape(-1, 2)
        c['edge'] = np.array(c['edge'], dtype=np.int64).reshape(2, c['n'], 2)
        if c['sub']:
            c['sub']['tri'] = np.array(c['sub']['tri'], dtype=np.int64).reshape(-1, 2)
            c['sub']['edge'] = np.array(c['sub']['edge'], dtype=np.int64).reshape(2, len(c['sub']['index']), 2)
    return cases


def decode_rows(packed, ref_len):
    """packed uint8[n, s] -> uint8[n, ref_len] of 0 / ASCII ACGT: digit d of byte j is column d * s + j, columns >= ref_len are cut"""
    packed = np.asarray(packed, dtype=np.uint8)
    digits = np.concatenate([packed // 25, (packed // 5) % 5, packed % 5], axis=1)[:, :ref_len]
    return np.array([0, 65, 67, 71, 84], dtype=np.uint8)[digits]


def counts(a_rows, b_rows):
    """(mismatch + 1, comparable + 2) of every row of a_rows against every row of b_rows: int64[na, nb, 2], by broadcast compare"""
    both = (a_rows[:, None, :] > 0) & (b_rows[None, :, :] > 0)
    mism = both & (a_rows[:, None, :] != b_rows[None, :, :])
    return np.stack([mism.sum(2, dtype=np.int64) + 1, both.sum(2, dtype=np.int64) + 2], axis=2)


def numpy_tri_edge(seqs, block=64):
    """(tri int64[n(n-1)/2, 2] in row-major pair order, edge int64[2, n, 2]) of seqs uint8[n, L], evaluated in row blocks"""
    n = seqs.shape[0]
    tri = []
    for a0 in range(0, n, block):
        first = a0 // 512 * 512                         # (column blocks left of the diagonal hold no pair a < b)
        sq = np.concatenate([counts(seqs[a0:a0 + block], seqs[b0:b0 + 512]) for b0 in range(first, n, 512)], axis=1)
        for a in range(a0, min(a0 + block, n)):
            tri.append(sq[a - a0, a + 1 - first:])
    tri = np.concatenate(tri) if tri else np.zeros((0, 2), np.int64)
    edge = np.concatenate([counts(seqs[[0, n - 1]], seqs[b0:b0 + 512]) for b0 in range(0, n, 512)], axis=1)
    return tri, edge


def square_from_tri(n, tri, fill=0):
    sq = np.full((n, n, 2), fill, dtype=np.int64)
    iu = np.triu_indices(n, 1)
    sq[iu[0], iu[1]] = tri
    return sq


def random_group(rng, n, ref_len, gap=None, div=None):
    """packed rows uint8[n, ceil(ref_len / 3)] with garbage digits past ref_len"""
    s = -(-ref_len // 3)
    gap = rng.uniform(0, 0.5) if gap is None else gap
    div = rng.uniform(0, 0.3) if div is None else div
    anc = rng.integers(1, 5, ref_len)
    codes = np.repeat(anc[None, :], n, axis=0)
    mut = rng.random((n, ref_len)) < div
    codes[mut] = rng.integers(1, 5, int(mut.sum()))
    codes[rng.random((n, ref_len)) < gap] = 0
    full = rng.integers(0, 5, (n, 3 * s))
    full[:, :ref_len] = codes
    return (full[:, :s] * 25 + full[:, s:2 * s] * 5 + full[:, 2 * s:]).astype(np.uint8)


def plane_words(L):
    """64-bit words per bit plane of a row of L nt: ceil(3 * ceil(L / 3) / 64)"""
    return -(-3 * -(-L // 3) // 64)


def bit_of_column(L):
    """the bit of the planes that holds column c of a row of L columns: digit d of byte j is column d * s + j and bit 3 j + d"""
    s = -(-L // 3)
    c = np.arange(L)
    return 3 * (c % s) + c // s


def beyond_first_trip(L):
    """(the columns of a row of L nt, highest bit first, that a wavefront reaches in its second trip over the plane words or later - bit >= 4 096 -, that
    bit bound).  A row of exactly 64 words has no such column: there it is the last word, which lane 63 alone reads."""
    bit = bit_of_column(L)
    bound = 4096 if plane_words(L) > 64 else 64 * (plane_words(L) - 1)
    cols = np.flatnonzero(bit >= bound)
    return cols[np.argsort(-bit[cols])], bound
