"""K10-K13 without a GPU: the restatements of tests/small_kernel_cases.py held against the C oracle on every hand-built case (and K12's on the
random tables of the parity test), and every case held to what its name says, so that a later edit of a builder cannot drop an edge unnoticed.
Every comparison is ==."""
import os
import sys

import numpy as np
import pytest
from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_kernel_cases as K  # noqa: E402

ALLELES = K.alleles_cases()
OVERLAPS = K.overlaps_cases()
COMPONENTS = K.components_cases()
DEDUP = K.dedup_cases()
by_name = lambda cases: {c['name']: c for c in cases}  # noqa: E731
ids = lambda cases: [c['name'] for c in cases]  # noqa: E731


def k12_args(c):
    return c['contigs'], c['rows'], c['cigar'], c['grp_off'], c['grp_qlen'], c['gtable']


# ---- K12
def test_locus_records_are_the_library_s():
    from peppan_amd import _native as N
    assert K.LOCUS_DTYPE == N.LOCUS_DTYPE == O.LOCUS_DTYPE


@pytest.mark.parametrize('case', ALLELES, ids=ids(ALLELES))
def test_alleles_restatement_equals_the_oracle_and_the_case_is_what_it_says(case):
    in_frame, orf, packed, seen = K.restate_alleles(*k12_args(case), detail=True)
    want = O.alleles(*k12_args(case))
    assert in_frame.dtype == want[0].dtype and packed.dtype == want[2].dtype
    for mine, theirs in zip((in_frame, orf, packed), want):
        assert mine.shape == theirs.shape and np.array_equal(mine, theirs)
    # what the builder worked out by hand
    e = case['expect']
    assert 'orf' not in e or orf.tolist() == e['orf']
    assert 'in_frame' not in e or in_frame.tolist() == e['in_frame']
    assert 'frames' not in e or [sc for _, sc, _ in seen] == e['frames']
    assert 'stops' not in e or [at for _, _, at in seen] == e['stops']
    # what pep_k12_alleles validates
    for g, ql in enumerate(case['grp_qlen'].tolist()):
        assert ql >= 3
        for r in range(int(case['grp_off'][g]), int(case['grp_off'][g + 1])):
            row, ms = case['rows'][r], seen[r][0]
            runs = case['cigar'][int(row['cigar_off']):int(row['cigar_off']) + int(row['cigar_runs'])]
            lo, hi = sorted((int(row['rs']), int(row['re'])))
            assert 1 <= lo and hi <= len(case['contigs'][row['contig']]) and row['q_start'] >= 1 and row['q_start'] - 1 + len(ms) <= ql
            assert sum(int(c) >> 2 for c in runs if int(c) & 3 != 1) == hi - lo + 1 and sum(int(c) >> 2 for c in runs if int(c) & 3 != 2) == len(ms)


def test_alleles_restatement_equals_the_oracle_on_the_random_tables_of_the_parity_test():
    rng = np.random.default_rng(1212)                       # test_k12_alleles_vs_oracle's generator, sizes and tables
    for n_groups, gtable in ((1, 11), (7, 4), (600, 11), (5000, 4)):
        contigs, rows, cigar, grp_off, grp_qlen = K.random_loci(rng, n_groups)
        mine = K.restate_alleles(contigs, rows, cigar, grp_off, grp_qlen, gtable)
        for a, b in zip(mine, O.alleles(contigs, rows, cigar, grp_off, grp_qlen, gtable)):
            assert a.shape == b.shape and np.array_equal(a, b)
        assert len(mine[0]) >= n_groups


def test_alleles_cases_hold_every_edge_the_kernel_has():
    cases = by_name(ALLELES)
    detail = {n: K.restate_alleles(*k12_args(c), detail=True) for n, c in cases.items()}
    rows = [(n, c, r) for n, c in cases.items() for r in range(len(c['rows']))]
    runs_of = lambda c, r: [(int(x) >> 2, int(x) & 3) for x in c['cigar'][int(c['rows'][r]['cigar_off']):][:int(c['rows'][r]['cigar_runs'])]]  # noqa: E731
    # contig edges; the last contig's last base on both strands
    assert any(min(c['rows'][r]['rs'], c['rows'][r]['re']) == 1 for n, c, r in rows)
    for strand in (1, -1):
        assert any(c['rows'][r]['contig'] == 2 and max(c['rows'][r]['rs'], c['rows'][r]['re']) == len(c['contigs'][2]) and
                   np.sign(int(c['rows'][r]['re']) - int(c['rows'][r]['rs'])) == strand for n, c, r in rows)
    assert any(c['rows'][r]['rs'] == c['rows'][r]['re'] for n, c, r in rows)
    # run lengths around the 64-lane stride, of all three kinds, on both strands
    for op, lens in ((0, (1, 63, 64, 65, 128, 129)), (1, (64, 65, 66)), (2, (64, 65, 66))):
        for ln in lens:
            for fwd in (True, False):
                assert any((ln, op) in runs_of(c, r) and (c['rows'][r]['rs'] < c['rows'][r]['re']) == fwd for n, c, r in rows), (op, ln, fwd)
    assert any(runs_of(c, r) == [(1, 0)] for n, c, r in rows)
    # the frame with the most M columns: each of the three, and not always frame 0
    best = {int(np.argmax(sc)) for n in cases for _, sc, _ in detail[n][3] if sorted(sc)[-1] > sorted(sc)[-2]}
    assert best == {0, 1, 2}
    # spans 0 .. 5: no codon, and one or two columns past the last codon
    spans = {len(ms) for n in cases for ms, _, _ in detail[n][3]}
    assert {0, 1, 2, 3, 4, 5} <= spans and {s % 3 for s in spans if s > 5} == {0, 1, 2}
    for n in cases:
        for (ms, _, _), o in zip(detail[n][3], detail[n][1].tolist()):
            assert len(ms) >= 3 or o == len(ms)
    # stops on both sides of the ballot window's edge, on both strands, under both tables; on codon 0, on the last codon, adjacent, at the row's end
    for cd in (0, 63, 64, 65):
        for tag in ('fwd', 'rev'):
            for gtable in (11, 4):
                assert any(cd in at for n, c in cases.items() if '/%s/' % tag in n and c['gtable'] == gtable for _, _, at in detail[n][3]), (cd, tag, gtable)
    assert any(at == [63, 64] for n in cases for _, _, at in detail[n][3])
    assert any(at and 3 * at[-1] + 3 == len(ms) for n in cases for ms, _, at in detail[n][3])
    # TGA is a stop under table 11 and none under table 4, in the same case otherwise
    for n, c in cases.items():
        if n.startswith('stop/') and '/TGA/' in n and n.endswith('gtable4'):
            twin = n[:-1] + '11'
            assert detail[n][3][0][2] == [] and detail[twin][3][0][2] != [] and detail[n][3][0][0] == detail[twin][3][0][0]
    # the non-stops hold the text of a stop and report none
    for n in cases:
        if n.startswith('nonstop/'):
            ms, _, at = detail[n][3][0]
            assert at == [] and detail[n][1].tolist()[0] == len(ms)
            if 'across-the-row-end' in n:                   # the stop's text ends in the next row of the table
                k, nxt = len(ms) % 3, detail[n][3][1][0]
                assert k and ms[-k:] + nxt[:3 - k] == n.split('/')[3] and detail[n][3][1][2] == [] and (len(ms) // 3) % 64
                continue
            text = n.split('/')[2]
            assert (text[0] + '-' + text[1:] if 'split-by-I' in n else text) in ms, n
    assert sum(1 for n in cases if n.startswith('nonstop/with-N/')) >= 6 and any('N' in detail[n][3][0][0] for n in cases if 'with-N' in n)
    # packing: gene lengths, a row ending on the gene's end, an empty group, 300 rows in one group, code 0 over a base, a hidden row
    qls = {int(q) for c in ALLELES for q in c['grp_qlen']}
    assert {3, 4, 5, 191, 192, 193, 195} <= qls
    assert any(int(c['rows'][r]['q_start']) - 1 + len(detail[n][3][r][0]) == int(c['grp_qlen'][c['rows'][r]['group']]) and c['rows'][r]['q_start'] > 1 for n, c, r in rows)
    assert any(len(c['rows']) == 0 and not detail[n][2].any() for n, c in cases.items())
    assert any(c['grp_off'][g] == c['grp_off'][g + 1] and len(c['rows']) for c in ALLELES for g in range(len(c['grp_qlen'])))
    assert any(int(np.diff(c['grp_off'].astype(np.int64)).max()) == 300 for c in ALLELES)
    for n in ('cover/later-insert-columns-overwrite-bases/fwd', 'cover/later-insert-columns-overwrite-bases/rev'):
        c = cases[n]
        alone = K.restate_alleles(c['contigs'], c['rows'][:1], c['cigar'], [0, 1], c['grp_qlen'], c['gtable'])[2]
        assert not np.array_equal(alone, detail[n][2])
    for n in ('cover/middle-row-hidden-by-last/fwd', 'cover/middle-row-hidden-by-last/rev'):
        c = cases[n]
        without = K.restate_alleles(c['contigs'], c['rows'][[0, 2]], c['cigar'], [0, 2], c['grp_qlen'], c['gtable'])[2]
        assert np.array_equal(without, detail[n][2])


# ---- K11
@pytest.mark.parametrize('case', OVERLAPS, ids=ids(OVERLAPS))
def test_overlaps_cases_are_sorted_and_give_the_pairs_they_are_built_for(case):
    n = len(case['contig'])
    key = list(zip(case['contig'].tolist(), case['start'].tolist(), case['end'].tolist()))
    assert key == sorted(key) and (case['start'] <= case['end']).all() and len(case['rid']) == n
    got = K.restate_overlaps(case['contig'].tolist(), case['start'].tolist(), case['end'].tolist(), case['rid'].tolist(), case['ovl_l'], case['ovl_p'])
    assert got.dtype == np.int64 and got.shape[1] == 3
    assert case['pairs'] is None or len(got) == case['pairs']


def test_overlaps_cases_hold_every_edge_the_call_has():
    cases = by_name(OVERLAPS)
    assert 0.6 * 5 == 3.0 == 0.1 * 30 and 0.28 * 25 > 7.0
    pairs = {n: K.restate_overlaps(c['contig'].tolist(), c['start'].tolist(), c['end'].tolist(), c['rid'].tolist(), c['ovl_l'], c['ovl_p']) for n, c in cases.items()}
    seen = set()
    for n, c in cases.items():
        if n.startswith('threshold/0.'):
            p, ln = (float(v) for v in n.split('/')[1].split('-')[0].split('x'))
            k = 0 if n.endswith('first-interval') else 1         # the interval whose length sets the threshold; the other test of the pair is far off
            ovl = int(min(c['end'][0], c['end'][1]) - c['start'][1] + 1)
            assert c['ovl_p'] == p and c['end'][k] - c['start'][k] + 1 == ln and ovl * 100 == round(p * 100) * ln
            assert min(c['ovl_l'], p * float(c['end'][1 - k] - c['start'][1 - k] + 1)) > ovl + 1
            assert len(pairs[n]) == int(ovl >= p * ln)
            seen.add((p, k, len(pairs[n])))
    assert seen == {(0.6, 0, 1), (0.6, 1, 1), (0.1, 0, 1), (0.1, 1, 1), (0.28, 0, 0), (0.28, 1, 0)}
    assert pairs['threshold/overlap-equals-ovl_l'][0, 2] == cases['threshold/overlap-equals-ovl_l']['ovl_l']
    assert pairs['geometry/start-equals-end-of-the-first'][:, 2].tolist() == [1]
    c = cases['contig-change/at-rows-256-and-2048']
    assert c['contig'][255] != c['contig'][256] and c['contig'][2047] != c['contig'][2048] and len(set(c['contig'].tolist())) == 3
    assert c['start'][256] <= c['end'][255] and c['start'][2048] <= c['end'][2047]            # only the contig keeps them apart
    first = pairs['long-first-interval/3000-successors']
    assert (first[:, 0] == cases['long-first-interval/3000-successors']['rid'][0]).sum() == 3000 > 2048
    n = len(cases['pairs/600-mutual-overlaps-exceed-the-first-buffer']['contig'])
    assert len(pairs['pairs/600-mutual-overlaps-exceed-the-first-buffer']) == 179700 > K.overlaps_cap(n) == 2400
    assert all(len(p) <= K.overlaps_cap(len(cases[k]['contig'])) for k, p in pairs.items() if not k.startswith('pairs/600'))
    assert len(pairs['pairs/none-at-all']) == 0
    assert cases['range/start-around-3e9']['start'].min() > 2 ** 31 and cases['range/start-around-3e9']['end'].max() > 2 ** 32
    assert pairs['range/rid-above-2-to-32'][:, :2].min() > 2 ** 32
    assert {c['ovl_p'] for c in OVERLAPS} >= {0., 0.1, 0.6, 1.5}


# ---- K10
@pytest.mark.parametrize('case', COMPONENTS, ids=ids(COMPONENTS))
def test_components_restatement_equals_the_oracle(case):
    want = O.components(case['n'], case['a'], case['b'])
    got = K.restate_components(case['n'], case['a'], case['b'])
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert (got <= np.arange(case['n'])).all() and (got[got] == got).all()


def test_components_cases_are_what_they_are_built_for():
    cases = by_name(COMPONENTS)
    lab = {n: K.restate_components(c['n'], c['a'], c['b']) for n, c in cases.items()}
    for n in cases:
        if n.startswith('path/') or n.startswith('star/'):
            assert not lab[n].any() and cases[n]['n'] == 20000 and len(cases[n]['a']) == 19999
    assert (np.diff(cases['path/edges-ascending']['a'].astype(np.int64)) == 1).all() and (np.diff(cases['path/edges-descending']['a'].astype(np.int64)) == -1).all()
    assert (cases['star/on-the-largest-id']['a'] == 19999).all() and (cases['star/on-node-0']['a'] == 0).all()
    c = cases['edges/every-edge-a-self-loop']
    assert np.array_equal(c['a'], c['b']) and np.array_equal(lab['edges/every-edge-a-self-loop'], np.arange(c['n']))
    c = cases['edges/one-edge-5000-times']
    assert len(c['a']) == 5000 and len(set(zip(c['a'].tolist(), c['b'].tolist()))) == 1 and (lab['edges/one-edge-5000-times'] != np.arange(c['n'])).sum() == 1
    c = cases['edges/both-orientations']
    assert set(zip(c['a'].tolist(), c['b'].tolist())) == set(zip(c['b'].tolist(), c['a'].tolist()))
    giant = lab['mixed/giant-component-and-isolated-nodes']
    assert np.bincount(giant).max() > 9000 and (giant[1::2] == np.arange(20000)[1::2]).all()
    bip = lab['mixed/complete-bipartite-40x40']
    assert len(cases['mixed/complete-bipartite-40x40']['a']) == 1600 and (np.bincount(bip) == 80).sum() == 1 and (bip[100:140] == 0).all()
    assert {(c['n'], len(c['a'])) for n, c in cases.items() if n.startswith('size/n-')} == {(n, m) for n in (255, 256, 257) for m in (255, 256, 257)}
    assert max(c['n'] for c in COMPONENTS) <= 20000
    # the table of hits: the three node maps are A, B, A, B is A but for its last entry, and that entry changes the labels
    h = K.hits_case()
    a, b, again = h['maps']
    assert np.array_equal(a, again) and len(a) == len(b) and (a != b).tolist() == [False] * (len(a) - 1) + [True]
    assert h['t'].max() == len(a) - 1 and (h['q'] + h['q_base']).max() < h['n'] and max(a.max(), b.max()) < h['n']
    la, lb = (K.restate_components(h['n'], h['q'] + h['q_base'], m[h['t']]) for m in (a, b))
    assert not np.array_equal(la, lb) and np.array_equal(la, O.components(h['n'], h['q'] + h['q_base'], a[h['t']]))


# ---- K13
@pytest.mark.parametrize('case', DEDUP, ids=ids(DEDUP))
def test_dedup_cases_give_what_they_are_built_for(case):
    assert case['digests'].shape == (len(case['lengths']), 20)
    rep = K.restate_dedup(case['lengths'], case['digests'])
    assert rep.dtype == np.uint32 and (rep <= np.arange(len(rep))).all()
    assert case['rep'] is None or rep.tolist() == case['rep']


def test_dedup_cases_hold_every_edge_the_table_has():
    cases = by_name(DEDUP)
    c = cases['collide/3000-keys-share-the-hashed-words']
    d, n = c['digests'], len(c['lengths'])
    assert len(set(c['lengths'].tolist())) == 1 and (d[:, :8] == d[0, :8]).all() and len({r.tobytes() for r in d[:3000, 8:]}) == 3000
    slot, mask = K.dedup_slot(0, d[0], n)
    assert mask == 8191 and slot == mask - 100 and slot + 3000 > mask + 1                     # the chain goes on at slot 0
    assert (d[2998] != d[2999]).tolist() == [False] * 19 + [True]
    two = cases['collide/two-keys-differ-in-the-last-byte']['digests']
    assert (two[0] != two[1]).tolist() == [False] * 19 + [True]
    c = cases['collide/duplicate-then-a-key-probing-past-it']
    assert (c['digests'][:, :8] == d[0, :8]).all() and K.restate_dedup(c['lengths'], c['digests']).tolist()[:6] == [0, 0, 2, 2, 4, 4]
    assert {len(c['lengths']) for n, c in cases.items() if n.startswith('distinct/')} == {8, 9, 2048, 2049, 4097}
    c = cases['runs/every-gene-a-new-length']
    assert (np.diff(c['lengths'].astype(np.int64)) != 0).all() and len({r.tobytes() for r in c['digests']}) == 1 and len(c['lengths']) > 2048
    c = cases['runs/alternating-lengths-5000']
    assert len(c['lengths']) == 5000 and (np.diff(c['lengths'].astype(np.int64)) != 0).all() and len({r.tobytes() for r in c['digests']}) == 1
    c = cases['runs/five-runs-of-1000-over-7-digests']
    rep = K.restate_dedup(c['lengths'], c['digests'])
    assert len(set(rep.tolist())) == 35 and (rep[2000:3000] >= 2000).all()                     # length 36 re-opened: nothing of the first run is seen
    c = cases['identical/3000-genes']
    assert len({r.tobytes() for r in c['digests']}) == 1 and len(set(c['lengths'].tolist())) == 1
