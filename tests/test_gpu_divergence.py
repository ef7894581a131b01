"""K16 on the GPU: Context.group_verdicts and orthofilter.group_verdicts against the facts recorded from the reference's own filt_per_group
(tests/golden/g20_divergence.json.gz) and an independent restatement in plain Python loops (tests/divergence_helpers.py).  Verdicts, leaders
and triangles are compared with ==: every float decision is a chain of single correctly rounded double operations, no tolerance anywhere.
Beside the fixture, the fuzz, the ties and the at-size case: a group of 4 200 leaders with rows that match two of them (the chunks of 256 of
verdict_leaders, its list beyond 4 096 leaders and "the first leader wins", against leaders_numpy over matmul_counts, which test_divergence_host.py
pins), and rows of 4 095 .. 12 300 nt, whose bit planes are longer than one trip of a wavefront."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from allele_diff_helpers import beyond_first_trip, bit_of_column, counts, decode_rows, numpy_tri_edge, plane_words, random_group, square_from_tri  # noqa: E402
from divergence_helpers import (clade, founders_group, fuzz_groups, leaders_numpy, load_g20, matching_leaders, matmul_counts, pack_codes, pair_counts,  # noqa: E402
                                restate, tri_from_square, verdict_table)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native as N
    with N.Context(0) as c:
        yield c


def table_of(gd, self_id, allowed_sigma):
    from peppan_amd import orthofilter as OF
    return OF.gd_table(gd, self_id, allowed_sigma)


def check_against(res, want, tag):
    verdict, tri, leader = res
    assert verdict == want['verdict'], tag
    if verdict == 2:
        assert tri.dtype == np.int32 and np.array_equal(tri, want['tri']), tag
        assert leader.dtype == np.uint32 and np.array_equal(leader, want['leader']), tag
    else:
        assert tri is None and leader is None, tag


def test_every_golden_case_exactly(ctx):
    from peppan_amd import orthofilter as OF
    for c in load_g20():
        gd = table_of(c['gd'], c['self_id'], c['allowed_sigma'])
        packed, row_off, row_len, index = verdict_table([c['packed']], [c['ref_len']])
        (verdict, tri, leader), = ctx.group_verdicts(packed, row_off, row_len, index, [c['genomes']], [c['inparalog']], gd, c['self_id'])
        want = restate(c['packed'], c['ref_len'], c['genomes'], c['inparalog'], c['gd'], c['self_id'], c['allowed_sigma'])
        # the three facts the reference's own function revealed
        assert (verdict > 0) == c['divergent'], c['name']
        check_against((verdict, tri, leader), want, c['name'])
        needs_tree = False
        if verdict == 2:
            n = c['n']
            diff = square_from_tri(n, tri).astype(np.float64)
            groups = [np.flatnonzero(leader == l).tolist() for l in np.unique(leader)]
            assert groups == want['groups'], c['name']
            _, needs_tree = OF.incompatible_of(OF.distances_from_diff(diff, c['genomes'], gd), groups)
            if c['tree_asked']:
                assert sorted(g[0] for g in groups) == c['leaders'], c['name']
        assert needs_tree == c['tree_asked'], c['name']


def run_by_params(ctx, cases, **kw):
    """one batch per (self_id, allowed_sigma) with the union of the cases' tables -> results in case order"""
    res = [None] * len(cases)
    for key in sorted({(c['self_id'], c['allowed_sigma']) for c in cases}):
        pick = [k for k, c in enumerate(cases) if (c['self_id'], c['allowed_sigma']) == key]
        # genome ids are made distinct per case so that one table serves the batch
        gd, genomes = {}, []
        for k in pick:
            base = k * 100000
            genomes.append(np.asarray(cases[k]['genomes']) + base)
            gd.update({(a + base, b + base): v for (a, b), v in cases[k]['gd'].items()})
        packed, row_off, row_len, index = verdict_table([cases[k]['packed'] for k in pick], [cases[k]['ref_len'] for k in pick])
        got = ctx.group_verdicts(packed, row_off, row_len, index, genomes, [cases[k]['inparalog'] for k in pick], table_of(gd, *key), key[0], **kw)
        for k, r in zip(pick, got):
            res[k] = r
    return res


def test_fuzz_300_groups_equal_the_restatement(ctx):
    cases = fuzz_groups(1600, 300, 400)
    want = [restate(c['packed'], c['ref_len'], c['genomes'], c['inparalog'], c['gd'], c['self_id'], c['allowed_sigma']) for c in cases]
    share = np.bincount([w['verdict'] for w in want], minlength=3) / len(want)
    print('fuzz verdict shares 0 / 1 / 2: %.2f %.2f %.2f' % tuple(share))
    assert share.min() >= 0.15, share
    assert any(w['verdict'] == 2 and len(w['groups']) > 1 for w in want)
    for k, (r, w) in enumerate(zip(run_by_params(ctx, cases), want)):
        check_against(r, w, k)


def ulp_neighbours_of_one():
    return np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0)


def rows_with_counts(L, mismatches, comparable):
    """two rows of L columns with exactly `comparable` columns both non-zero and `mismatches` of them different"""
    a = np.full(L, 1, dtype=np.int64)
    b = np.full(L, 1, dtype=np.int64)
    b[:mismatches] = 2
    b[comparable:] = 0
    return a, b


def test_constructed_ties_equal_numpy(ctx):
    cases = []
    # leaders: aln == 100 * mut exactly, mut in 1 .. 60 (mut = mismatches + 1, aln = comparable + 2), and one off on either side
    for mut in range(1, 61):
        for aln in (100 * mut - 1, 100 * mut, 100 * mut + 1):
            L = aln + 5
            a, b = rows_with_counts(L, mut - 1, aln - 2)
            far = np.full(L, 3, dtype=np.int64)          # a third row far from both: the group is divergent and beyond, so the leaders are computed
            cases.append(dict(packed=pack_codes(np.stack([a, b, far])), ref_len=L, genomes=np.array([1, 2, 3]), inparalog=False,
                              gd={(1, 3): (0.01, 0.1), (2, 3): (0.01, 0.1)}, self_id=0.002, allowed_sigma=3))
    # checkDiv / beyond: scan (mut, aln) and, a few ulp around mut / aln / exp(gd1 * sqrt(allowed_sigma)), the global_differences mean for quotients
    # that numpy rounds to the nearest double below 1, to 1 itself, or to the nearest double above 1
    below, one, above = ulp_neighbours_of_one()
    found = {below: [], one: [], above: []}
    for sigma in (1, 3):
        for gd1 in (0., 0.5):
            for aln in list(range(40, 140)) + list(range(900, 1100, 7)) + [2399, 2400]:
                for m in (1, 2, 3, aln // 50 + 1, aln // 20 + 2, aln // 7):
                    mean = np.float64(m) / np.float64(aln) / np.exp(gd1 * np.sqrt(sigma))
                    for step in (-3, -2, -1, 0, 1, 2, 3):
                        cand = mean
                        for _ in range(abs(step)):
                            cand = np.nextafter(cand, np.inf if step > 0 else 0.)
                        q = np.float64(m) / np.float64(aln) / (cand * np.exp(gd1 * np.sqrt(sigma)))
                        if q in found and len(found[q]) < 40 and 1 <= m < aln - 2:
                            found[q].append((m, aln, float(cand), gd1, sigma))
    # same-genome pairs give exact ties: mut / aln / max(self_id, 2 / aln) == 1 for mut == 2 (2 / aln wins) - and its neighbours
    for aln in (50, 300, 399, 400, 401, 1000):
        for m in (1, 2, 3):
            found[one].append((m, aln, None, 0., 3))
    assert min(len(v) for v in found.values()) >= 20, {k: len(v) for k, v in found.items()}
    print('ties found: below %d, at %d, above %d' % (len(found[below]), len(found[one]), len(found[above])))
    for q, hits in found.items():
        for m, aln, mean, gd1, sigma in hits:
            L = aln + 3
            a, b = rows_with_counts(L, m - 1, aln - 2)
            same = mean is None
            cases.append(dict(packed=pack_codes(np.stack([a, b])), ref_len=L, genomes=np.array([1, 1 if same else 2]), inparalog=False,
                              gd={} if same else {(1, 2): (mean, gd1)}, self_id=0.002, allowed_sigma=sigma))
    want = [restate(c['packed'], c['ref_len'], c['genomes'], c['inparalog'], c['gd'], c['self_id'], c['allowed_sigma']) for c in cases]
    assert {w['verdict'] for w in want} == {0, 1, 2} or {w['verdict'] for w in want} == {0, 2}
    assert any(len(w['groups']) == 2 for w in want[:180]) and any(len(w['groups']) == 3 for w in want[:180])
    for k, (r, w) in enumerate(zip(run_by_params(ctx, cases), want)):
        check_against(r, w, k)


def test_ragged_batch_equals_one_by_one_and_split_batch(ctx):
    cases = fuzz_groups(1601, 80, 300)
    for c in cases:
        c['self_id'], c['allowed_sigma'] = 0.002, 3
    cases[5]['packed'], cases[5]['genomes'] = cases[5]['packed'][:1], cases[5]['genomes'][:1]          # a one-row group
    cases[9]['packed'], cases[9]['genomes'] = cases[9]['packed'][:0], cases[9]['genomes'][:0]          # an empty group
    whole = run_by_params(ctx, cases)
    assert whole[5] == (0, None, None) and whole[9] == (0, None, None)
    for k, c in enumerate(cases):
        one, = run_by_params(ctx, [c])
        assert one[0] == whole[k][0] and (one[1] is None) == (whole[k][1] is None), k
        if one[1] is not None:
            assert np.array_equal(one[1], whole[k][1]) and np.array_equal(one[2], whole[k][2]), k
    need = [8 * (len(c['packed']) * (len(c['packed']) - 1) // 2) for c in cases]
    calls = []
    real = ctx._group_verdicts_call
    ctx._group_verdicts_call = lambda *a: calls.append(len(a[3])) or real(*a)
    try:
        split = run_by_params(ctx, cases, out_budget=max(max(need), sum(need) // 7))
    finally:
        del ctx._group_verdicts_call
    assert len(calls) >= 3 and sum(calls) == len(cases)
    for k in range(len(cases)):
        assert split[k][0] == whole[k][0], k
        if whole[k][1] is not None:
            assert np.array_equal(split[k][1], whole[k][1]) and np.array_equal(split[k][2], whole[k][2]), k


def test_shared_rows_and_subgroups_need_no_second_upload(ctx):
    rng = np.random.default_rng(354)
    L, n = 777, 90
    codes = np.concatenate([clade(rng, rng.integers(1, 5, L), 45, 0.002), clade(rng, rng.integers(1, 5, L), 45, 0.002)])
    p = pack_codes(codes, rng)
    genome = rng.integers(0, 25, n)
    gd_dict = {(a, b): (0.02, 0.5) for a in range(25) for b in range(a + 1, 25)}
    gd = table_of(gd_dict, 0.002, 3)
    packed, row_off, row_len, index = verdict_table([p], [L])
    subs = [np.flatnonzero(genome == g).astype(np.uint32) for g in np.unique(genome) if (genome == g).sum() > 1]
    groups = index + subs + [np.array([5, 5, 3, 80], dtype=np.uint32), index[0][::-1].copy()]
    got = ctx.group_verdicts(packed, row_off, row_len, groups, [genome[g] for g in groups], [1] * len(groups), gd, 0.002)
    assert {r[0] for r in got} >= {2}
    for g, r in zip(groups, got):
        check_against(r, restate(p[g], L, genome[g], True, gd_dict, 0.002, 3), g[:4])


def test_over_a_seq_store_through_orthofilter(ctx, tmp_path):
    from peppan_amd import orthofilter as OF
    from peppan_amd.mapbsn import MapBsn
    cases = [c for c in load_g20() if c['self_id'] == 0.002 and c['allowed_sigma'] == 3]
    assert len({c['kind'] for c in cases}) == 4
    path = str(tmp_path / 'genes.seq.npz')
    rows = [r for c in cases for r in c['packed']]
    order = np.random.default_rng(5).permutation(len(rows))            # locus ids scattered over the members
    where = np.argsort(order)
    with MapBsn(path, 'w') as store:
        for m in range(0, len(rows), 1000):
            member = np.empty(len(order[m:m + 1000]), dtype=object)
            for k, r in enumerate(order[m:m + 1000]):
                member[k] = rows[r]
            store.save(m // 1000, member)
    to_run, gd, at = [], {}, 0
    for k, c in enumerate(cases):
        mat = np.zeros((c['n'], 7), dtype=np.int64)
        mat[:, 1] = c['genomes'] + k * 100000
        mat[:, 5] = where[at:at + c['n']]
        at += c['n']
        gd.update({(a + k * 100000, b + k * 100000): v for (a, b), v in c['gd'].items()})
        to_run.append([mat, c['inparalog'], c['ref_len'], path, 'unused'])
    table = np.empty((len(gd), 2), dtype=object)
    for k, (key, val) in enumerate(sorted(gd.items())):
        table[k, 0], table[k, 1] = key, val
    params = dict(self_id=0.002, allowed_sigma=3)
    got = OF.group_verdicts(path, to_run, table, params)
    light = OF.group_verdicts(path, to_run, gd, params, detail=False)
    for c, v, w in zip(cases, got, light):
        assert (v.verdict > 0) == c['divergent'] and w.verdict == v.verdict and w.diff is None, c['name']
        want = restate(c['packed'], c['ref_len'], c['genomes'], c['inparalog'], c['gd'], 0.002, 3)
        assert v.verdict == want['verdict'], c['name']
        if v.verdict == 2:
            n = c['n']
            assert v.diff.dtype == np.float64 and np.array_equal(v.diff, square_from_tri(n, want['tri']).astype(np.float64)), c['name']
            assert v.groups == want['groups'] and v.needs_tree == c['tree_asked'], c['name']
            assert v.distances.shape == (n, n, 2) and v.incompatible.shape == (n, n, 2)
            assert bool(np.any(v.distances[:, :, 0] > v.distances[:, :, 1]))
        else:
            assert v.diff is None and v.groups is None and v.needs_tree is None and not c['tree_asked'], c['name']
    OF.close()


def test_bytes_to_host_do_not_depend_on_group_size(ctx):
    rng = np.random.default_rng(77)
    seen = []
    for n in (8, 300):
        groups, genomes = [], []
        for k in range(10):
            level = 0.002 if k % 2 else 0.06                   # verdict 0 and verdict 1 (between the two bounds at allowed_sigma 5)
            groups.append(pack_codes(clade(rng, rng.integers(1, 5, 1200), n, level), rng))
            genomes.append(np.arange(n))
        gd_dict = {(a, b): (0.02, 0.5) for a in range(n) for b in range(a + 1, n)}
        packed, row_off, row_len, index = verdict_table(groups, [1200] * 10)
        got = ctx.group_verdicts(packed, row_off, row_len, index, genomes, [0] * 10, table_of(gd_dict, 0.002, 5), 0.002)
        assert sorted({r[0] for r in got}) == [0, 1], [r[0] for r in got]
        seen.append(ctx.group_verdicts_times()[1])
    assert seen[0] == seen[1] == 10 + 4, seen


def test_at_size_2000_rows_of_1002_nt_each_verdict_once(ctx):
    rng = np.random.default_rng(2000)
    n, L = 2000, 1002
    groups = [pack_codes(clade(rng, rng.integers(1, 5, L), n, level, gap=0.05), rng) for level in (0.002, 0.06, 0.06)]
    groups[2][n // 2:] = pack_codes(clade(rng, rng.integers(1, 5, L), n - n // 2, 0.002), rng)          # a second clade: beyond, two sets of leaders
    genomes = [np.arange(n)] * 3
    # 2 000 genomes would need 2 000 000 keys: the table is left empty and its default row carries the one bound every pair has
    den_x, den = 0.02 * np.exp(0.5 * np.sqrt(5)), 0.02 * np.exp(0.5 * 5)
    gd = (np.zeros(0, np.uint64), np.zeros((0, 3)), np.array([0.02, den_x, den]))
    packed, row_off, row_len, index = verdict_table(groups, [L] * 3)
    t1 = time.time()
    got = ctx.group_verdicts(packed, row_off, row_len, index, genomes, [0, 0, 0], gd, 0.002)
    t2 = time.time()
    print('at size: Context.group_verdicts of 3 x 2 000 rows %.3f s' % (t2 - t1))
    assert [r[0] for r in got] == [0, 1, 2]
    for k, (p, (verdict, tri, leader)) in enumerate(zip(groups, got)):
        seqs = decode_rows(p, L)
        ex = counts(seqs[[0, n - 1]], seqs).astype(np.float64)
        q = ex[:, :, 0] / ex[:, :, 1] / den_x
        q[0, 0] = q[1, n - 1] = 0
        divergent = bool((q > 1).any())
        if k == 0:
            assert not divergent and verdict == 0
            continue
        # all pairs: numpy for the group whose triangle comes back, K15 (pinned against numpy at this size by its own test) for the other
        want_tri = numpy_tri_edge(seqs)[0] if k == 2 else ctx.allele_diff(p.reshape(-1), row_off[:n + 1], row_len[:n], [index[0]], 1, out_budget=1 << 31)[0][0]
        t = want_tri.astype(np.float64)
        d = t[:, 0] / t[:, 1] / den
        beyond = bool((d / 0.02 > 1 / 0.02).any())
        assert verdict == (0 if not divergent else 2 if beyond else 1)
        if verdict == 2:
            assert np.array_equal(tri, want_tri)
            sq = square_from_tri(n, want_tri)
            mut_of, aln_of = sq[:, :, 0].tolist(), sq[:, :, 1].tolist()
            leaders, want = [], np.zeros(n, dtype=np.uint32)
            for j in range(n):
                for l in leaders:
                    if float(mut_of[l][j]) <= 0.01 * float(aln_of[l][j]):
                        want[j] = l
                        break
                else:
                    leaders.append(j)
                    want[j] = j
            assert len(leaders) > 1 and np.array_equal(leader, want)


def test_leaders_past_256_and_past_the_lds_list(ctx):
    """verdict_leaders keeps 4 096 leaders in LDS and the rest in a global list, tests them 256 at a time and must return the FIRST match in leader
    order.  ref_len 200 without gaps: two rows match iff they differ in at most one column (founders_group).  What the group was built for is
    asserted from the reference (leaders_numpy over matmul_counts), never from the device."""
    rng = np.random.default_rng(4200)
    L, D = 200, 4200
    # (src, var) by leader position: LDS against the global list; both in the global list, in two wavefronts of chunk 16; two wavefronts of chunk 0; one
    # wavefront; and one whose two-column variant is the EARLIER row (chunks 1 and 3)
    variants = [(10, 4150), (4120, 4180), (70, 200), (5, 40), (1000, 300)]
    behind = [0, 63, 64, 255, 256, 257, 4095, 4096, 4097, D - 1]
    built = [founders_group(rng, D, L, variants, between=(100, 4100), behind=behind)]
    built += [founders_group(rng, d, L, behind=(d - 1, 0)) for d in (255, 256, 257)]           # the chunk boundary alone, and a ragged batch around the big group
    groups = [pack_codes(b[0], rng) for b in built]
    den_x, den = 0.02 * np.exp(0.5 * np.sqrt(5)), 0.02 * np.exp(0.5 * 5)
    gd = (np.zeros(0, np.uint64), np.zeros((0, 3)), np.array([0.02, den_x, den]))              # (as at size: one bound for every pair, from the default row)
    packed, row_off, row_len, index = verdict_table(groups, [L] * len(groups))
    order = [1, 0, 2, 3]                                                                        # the big group in the middle of the batch
    t0 = time.time()
    got = ctx.group_verdicts(packed, row_off, row_len, [index[k] for k in order], [np.arange(len(groups[k])) for k in order], [0] * 4, gd, 0.002)
    got = [got[order.index(k)] for k in range(4)]
    t1 = time.time()
    for k, ((codes, row_of, joins, triples), p, (verdict, tri, leader)) in enumerate(zip(built, groups, got)):
        n = len(codes)
        mut, aln = matmul_counts(decode_rows(p, L))
        lead = leaders_numpy(mut, aln)
        # the reference shows what the group was built for
        assert np.array_equal(np.flatnonzero(lead == np.arange(n)), row_of), k                 # founder p is leader number p
        assert len(row_of) == (D, 255, 256, 257)[k] and n == len(row_of) + len(joins)
        assert all(lead[row] == row_of[f] for row, f in joins), k
        if k == 0:
            assert len(row_of) > 4096 and n == D + 2 + len(behind) + len(variants)
            assert [int(lead[row]) for row, _ in joins[2:2 + len(behind)]] == [int(row_of[f]) for f in behind]
            assert [(row - int(row_of[f])) for row, f in joins[:2]] == [4, 4] and row_of[4100] == 4101 and row_of[D - 1] == D + 1
            assert [(first, second) for _, first, second in triples] == [(10, 4150), (4120, 4180), (70, 200), (5, 40), (300, 1000)]
            for row, first, second in triples:
                assert matching_leaders(mut, aln, lead, row).tolist() == [row_of[first], row_of[second]]
        # the verdict, with numpy: checkDiv of the first and last row, then every pair against the distances' bound
        q = mut[[0, n - 1]].astype(np.float64) / aln[[0, n - 1]].astype(np.float64) / den_x
        q[0, 0] = q[1, n - 1] = 0
        want_tri = tri_from_square(mut, aln)
        t = want_tri.astype(np.float64)
        assert bool((q > 1).any()) and bool((t[:, 0] / t[:, 1] / den / 0.02 > 1 / 0.02).any())
        assert verdict == 2, k
        assert tri.dtype == np.int32 and np.array_equal(tri, want_tri), k
        assert leader.dtype == np.uint32 and np.array_equal(leader, lead), k
    t2 = time.time()
    print('leaders: Context.group_verdicts of 4 217 + 257 + 258 + 259 rows %.3f s, matmul counts and numpy leaders %.2f s' % (t1 - t0, t2 - t1))


def test_rows_of_more_than_64_plane_words(ctx):
    """verdict_edge and allele_planes walk a row's plane words 64 at a time; every other test stays below 48 words.  Per length a calm group, a group
    whose first and last row differ from the others ONLY where a later trip reads, and a two-clade group."""
    rng = np.random.default_rng(4096)
    lens = (4095, 4096, 8190, 8191, 12300)
    assert [plane_words(L) for L in lens] == [64, 65, 128, 129, 193]
    n = 6
    gd_dict = {(a, b): (0.02, 0.5) for a in range(n) for b in range(a + 1, n)}
    den_x, den = 0.02 * np.exp(0.5 * np.sqrt(5)), 0.02 * np.exp(0.5 * 5)
    gd = (np.zeros(0, np.uint64), np.zeros((0, 3)), np.array([0.02, den_x, den]))

    def ref(codes):
        return restate(pack_codes(codes), codes.shape[1], np.arange(n), False, gd_dict, 0.002, 5)

    groups, ref_lens, want = [], [], []
    for L in lens:
        calm = clade(rng, rng.integers(1, 5, L), n, 0.002, gap=0.05)
        # group two: all rows alike and gapped but for `shared` columns below the bound; beyond it the first and the last row carry another base than the
        # inner rows in h columns.  h is the smallest number at which the reference calls the group divergent.
        high, bound = beyond_first_trip(L)
        low = np.flatnonzero(bit_of_column(L) < bound)
        assert len(high) >= 1 and len(high) + len(low) == L
        shared = rng.choice(low, 20 * min(len(high), 15), replace=False)
        late = None
        for h in range(1, min(len(high), 60) + 1):
            codes = np.zeros((n, L), dtype=np.int64)
            codes[:, shared] = 1
            codes[:, high[:h]] = 2
            codes[0, high[:h]] = codes[n - 1, high[:h]] = 3
            if ref(codes)['verdict'] > 0:
                late = codes
                break
        assert late is not None and ref(late[:, low])['verdict'] == 0, L           # what a walk of one trip sees of it is calm
        two = np.concatenate([clade(rng, rng.integers(1, 5, L), n // 2, 0.002), clade(rng, rng.integers(1, 5, L), n - n // 2, 0.002)])
        for codes in (calm, late, two):
            groups.append(pack_codes(codes, rng))
            ref_lens.append(L)
            want.append(restate(groups[-1], L, np.arange(n), False, gd_dict, 0.002, 5))
        assert [w['verdict'] for w in want[-3:]] in ([0, 1, 2], [0, 2, 2]), L
    packed, row_off, row_len, index = verdict_table(groups, ref_lens)
    got = ctx.group_verdicts(packed, row_off, row_len, index, [np.arange(n)] * len(groups), [0] * len(groups), gd, 0.002)
    for k, (r, w) in enumerate(zip(got, want)):
        check_against(r, w, (ref_lens[k], k % 3))


def test_error_conventions_and_context_stays_usable(ctx):
    from peppan_amd import _native as N
    rng = np.random.default_rng(7)
    p = random_group(rng, 6, 100)
    packed, row_off, row_len, index = verdict_table([p], [100])
    genomes, gd = [np.arange(6)], table_of({(0, 5): (0.01, 0.5)}, 0.002, 3)
    good = ctx.group_verdicts(packed, row_off, row_len, index, genomes, [0], gd, 0.002)

    def still_good():
        again = ctx.group_verdicts(packed, row_off, row_len, index, genomes, [0], gd, 0.002)
        assert again[0][0] == good[0][0] and (good[0][1] is None or np.array_equal(again[0][1], good[0][1]))

    def fails(code, text, *a, **kw):
        with pytest.raises(N.PepError, match=r'pep_group_verdicts failed \(%d\): pep_group_verdicts: %s' % (code, text)):
            ctx.group_verdicts(*a, **kw)
        still_good()

    bad_len = row_len.copy()
    bad_len[2] = 103
    fails(-2, 'row 2 does not hold', packed, row_off, bad_len, index, genomes, [0], gd, 0.002)
    mixed = verdict_table([p, random_group(rng, 3, 40)], [100, 40])
    fails(-2, 'group 0 mixes rows of different row_len', mixed[0], mixed[1], mixed[2], [np.array([0, 1, 7])], [np.arange(3)], [0], gd, 0.002)
    fails(-2, 'row index 6 of group 0 out of range', packed, row_off, row_len, [np.array([0, 6])], [np.arange(2)], [0], gd, 0.002)
    spoiled = packed.copy()
    spoiled[int(row_off[4]) + 7] = 125
    fails(-2, 'row 4 holds a byte above 124', spoiled, row_off, row_len, index, genomes, [0], gd, 0.002)
    fails(-2, 'grp_inparalog of group 0', packed, row_off, row_len, index, genomes, [2], gd, 0.002)
    fails(-2, 'self_id must be finite and > 0', packed, row_off, row_len, index, genomes, [0], gd, 0.0)
    fails(-2, 'gd_key must be strictly increasing', packed, row_off, row_len, index, genomes, [0], (np.array([7, 7], np.uint64), np.ones((2, 3)), np.ones(3)), 0.002)
    fails(-2, 'gd_key 0 has g1 > g2', packed, row_off, row_len, index, genomes, [0], (np.array([(5 << 32) | 1], np.uint64), np.ones((1, 3)), np.ones(3)), 0.002)
    fails(-2, 'gd_val row 0 must be finite', packed, row_off, row_len, index, genomes, [0], (np.array([7], np.uint64), np.array([[1., 0., 1.]]), np.ones(3)), 0.002)
    fails(-2, 'gd_default must be finite', packed, row_off, row_len, index, genomes, [0], (np.array([7], np.uint64), np.ones((1, 3)), np.array([1., np.inf, 1.])), 0.002)
    # one group beyond the device budget of a call: 24 000 index entries onto one 1-nt row ask for 2.3 GB of triangle
    tiny = verdict_table([np.array([[25]], dtype=np.uint8)], [1])
    big = np.zeros(24000, dtype=np.uint32)
    with pytest.raises(N.PepError, match=r'pep_group_verdicts failed \(-3\): pep_group_verdicts: 2303904000 bytes of triangles asked for, the device budget .*reached at group 0'):
        ctx._group_verdicts_call(tiny[0], tiny[1], tiny[2], [big], [big], np.zeros(1, np.uint8), gd, 0.002, True, np.array([24000]), True)
    still_good()
    with pytest.raises(N.PepError, match='group 0 .24000 rows. needs 2303904000 bytes'):
        ctx.group_verdicts(tiny[0], tiny[1], tiny[2], [big], [big], [0], gd, 0.002, out_budget=1 << 40)
    with pytest.raises(N.PepError, match='budget'):
        ctx.group_verdicts(packed, row_off, row_len, index, genomes, [0], gd, 0.002, out_budget=64)
    still_good()
    # a result whose device data a newer call has replaced says so
    import ctypes as C
    args, keep = N._verdict_tables(packed, row_off, row_len, index, genomes, np.zeros(1, np.uint8), gd)
    verdict, first, second = np.zeros(1, np.uint8), C.c_void_p(), C.c_void_p()
    assert ctx._lib.pep_group_verdicts(ctx._h, *args, C.c_double(0.002), N._ptr(verdict), C.byref(first)) == 0
    assert ctx._lib.pep_group_verdicts(ctx._h, *args, C.c_double(0.002), N._ptr(verdict), C.byref(second)) == 0
    if verdict[0] == 2:
        assert ctx._lib.pep_verdict_detail_copy(first, C.c_uint32(0), None, None) == -4
    assert ctx._lib.pep_verdict_detail_copy(second, C.c_uint32(0), None, None) == 0
    assert ctx._lib.pep_verdict_detail_copy(second, C.c_uint32(1), None, None) == -2
    ctx._lib.pep_verdict_result_free(first)
    ctx._lib.pep_verdict_result_free(second)
    still_good()
    # legal: empty batch, empty group, one-row group
    assert ctx.group_verdicts(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), [], [], [], gd, 0.002) == []
    res = ctx.group_verdicts(packed, row_off, row_len, [np.zeros(0, np.uint32), np.array([3])], [np.zeros(0, np.uint32), np.array([1])], [1, 1], gd, 0.002)
    assert res == [(0, None, None), (0, None, None)]
