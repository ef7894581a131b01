"""The cases of tests/seed_retry_cases.py on the CPU alone: every case meets the sizing conditions of the retries it must take (sufficient conditions, from
counts and the oracle's candidate count), stays clear of the others by seed_retry_cases.MARGIN, its control meets none, the count itself agrees with a
slow double loop, and the caps the conditions are built on still stand in the source text - so that no case of tests/test_gpu_seed_retry.py can pass
vacuously, and a changed cap fails here instead of leaving the cases tame."""
import os

import numpy as np
import pytest

import seed_retry_cases as S
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [(n, False) for n in S.NAMES] + [(n, True) for n in S.NAMES if n != 'quiet']


def _ilog2_ceil(x):
    b = 0
    while (1 << b) < x:
        b += 1
    return b


def test_caps_stand_in_the_source_text():
    for path, pins in S.SOURCE_PINS.items():
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        for pin in pins:
            assert pin in text, (path, pin)


def test_motif_letters_are_one_class_of_the_reduced_alphabet():
    p = O.default_params()
    red = [int(p.reduce[i]) for i in range(32)]
    assert sorted(chr(65 + c) for c in range(26) if red[c] == red[ord('K') - 65]) == sorted(S.MOTIF_LETTERS)
    assert [len(o) for o in S.shapes_of(p)] == [10, 10] and [o[-1] + 1 for o in S.shapes_of(p)] == [12, 15]
    # one pair of the family: 4 x 4 windows of the first shape, 1 x 1 of the second, all one key
    q, t = S.motif_family(1, 1), S.motif_family(1, 2)
    assert [c[2] for c in S.seed_counts(q, t, p)] == [16, 1]


@pytest.mark.parametrize('name,control', ALL, ids=lambda v: str(v))
def test_case_takes_what_it_says_and_nothing_else(name, control):
    c = S.case(name, control)
    p = S.native_params(c)
    takes = c['takes']
    if control:
        assert takes == S.NOTHING
    cnt = S.counts(name, control)
    q_lo, q_hi = S.packed_bounds(c['q'])
    t_lo, t_hi = S.packed_bounds(c['t'])
    # the starting sizes are the constants' whatever the packing adds
    assert 2 * t_hi <= S.HIT_CAP_MIN and _ilog2_ceil(64 * len(c['q'])) <= S.TABLE_BITS_MIN
    hit_cap, list_cap = S.HIT_CAP_MIN, 1 << (S.TABLE_BITS_MIN - 1)
    # slab: one key more than PART_CAP times among the query's seeds of one shape, where the partition build runs
    heaviest = max(S.max_key_count(c['q'], p, s) for s in range(p.n_shapes))
    if takes['slab']:
        assert _ilog2_ceil(2 * q_lo) >= S.PARTITION_MIN_BUCKET_BITS and heaviest > S.PART_CAP
    else:
        assert heaviest * S.MARGIN < S.PART_CAP or _ilog2_ceil(2 * q_hi) < S.PARTITION_MIN_BUCKET_BITS
    # hits: the shape with the most appended hits (a self-search drops at most one hit per query seed position)
    dropped = [cq if c['self_on'] else 0 for cq, ct, raw in cnt]
    most_lo, most_hi = max(raw - d for (cq, ct, raw), d in zip(cnt, dropped)), max(raw for cq, ct, raw in cnt)
    g = takes['hit_growths']
    if g:
        assert most_lo > hit_cap * 4 ** (g - 1) * S.MARGIN
    assert most_hi * S.MARGIN <= hit_cap * 4 ** g
    # set: the oracle's candidates
    cands = S.oracle_result(name, control)[2]['candidates']
    g = takes['set_growths']
    if g:
        assert cands > list_cap * 4 ** (g - 1)
    assert cands * S.MARGIN <= list_cap * 4 ** g
    assert len(S.oracle_result(name, control)[0]) > 0                   # (the hit table is not empty)
    assert S.oracle_result(name, control)[3] < 10.


def test_every_retry_is_taken_by_some_case_and_quiet_takes_none():
    takes = {n: S.case(n)['takes'] for n in S.NAMES}
    assert takes['quiet'] == S.NOTHING
    assert takes['hits_x1']['hit_growths'] == 1 and takes['hits_x2']['hit_growths'] == 2 and takes['set_x1']['set_growths'] == 1
    assert takes['slab']['slab'] and takes['slab_sensitive']['slab'] and takes['slab_hits'] == dict(slab=True, hit_growths=1, set_growths=0)
    assert S.native_params(S.case('slab_sensitive')).n_shapes == 4
    assert S.case('self_hits')['self_on'] and takes['self_hits']['hit_growths'] == 1
    assert S.case('nt_hits')['tool'] == 'nucleotide' and takes['nt_hits']['hit_growths'] == 1
    assert 8 <= len(S.case('quiet')['q']) <= 20


def test_gene_case_is_the_translation_of_its_genes():
    c = S.case('self_hits')
    assert len(c['q']) == len(c['genes']) and len(c['t']) >= 6 * len(c['genes'])
    for g, x in zip(c['genes'][:20], c['q'][:20]):
        assert O.query_frame(g.decode(), 11)[0] == 1 and len(x) == len(g) // 3 and x[0] == ord('M') - 65


def _slow_counts(q, t, p):
    out = []
    red = [int(p.reduce[i]) for i in range(32)]
    for offs in S.shapes_of(p):
        tab = []
        for seqs in (q, t):
            d = {}
            for x in seqs:
                for pos in range(len(x) - offs[-1]):
                    letters = [red[int(x[pos + o])] for o in offs]
                    if 0xFF not in letters:
                        k = sum(g * int(p.base) ** i for i, g in enumerate(letters))
                        d[k] = d.get(k, 0) + 1
            tab.append(d)
        out.append((sum(tab[0].values()), sum(tab[1].values()), sum(n * tab[1].get(k, 0) for k, n in tab[0].items())))
    return out


def test_seed_counts_equal_a_slow_double_loop():
    """6 x 6 proteins with an X, a sequence shorter than the longer shape's span and one of exactly the span; and a nucleotide set with an N"""
    p = O.default_params()
    rng = np.random.default_rng(3)
    q = S.motif_family(6, 21)
    t = S.motif_family(6, 22)
    q[1] = q[1].copy()
    q[1][len(q[1]) // 2] = ord('X') - 65
    q[2] = q[2][12:12 + 13]                      # shorter than 15, longer than 12: windows of the first shape only
    t[3] = t[3][10:10 + 15]                      # exactly the longer span: one window of it
    t[4] = t[4][:11]                             # shorter than both
    t[5] = q[0].copy()
    got = S.seed_counts(q, t, p)
    assert got == _slow_counts(q, t, p)
    assert all(c[2] > 0 for c in got) and got[0][0] > got[1][0]
    from peppan_amd import _native as N
    pn = N.nucleotide_params()
    nq = [rng.integers(0, 4, n).astype(np.uint8) for n in (16, 17, 40, 60)]
    nt = [nq[2].copy(), nq[3][5:50].copy(), rng.integers(0, 4, 30).astype(np.uint8)]
    nt[0][20] = 4
    got = S.seed_counts(nq, nt, pn)
    assert got == _slow_counts(nq, nt, pn) and got[0][0] == 0 + 1 + 24 + 44 and got[0][2] >= 29
