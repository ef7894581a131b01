"""K15 on the GPU: Context.allele_diff, the compare_seq / compare_seqX drop-ins and group_differences against the reference's own values
(tests/golden/g19_allele_diff.json.gz) and an independent numpy formulation (tests/allele_diff_helpers.py).  Bit for bit everywhere.
Beside the fixture, the fuzz and the at-size case: rows of 4 095 .. 12 300 nt (more than 64 words per bit plane, the second and later trips of
allele_planes' word loop) and every group size around the 64-row tile at every width around the four words staged per step."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from allele_diff_helpers import (beyond_first_trip, bit_of_column, load_g19, decode_rows, numpy_tri_edge, plane_words, square_from_tri,  # noqa: E402
                                 random_group)
from divergence_helpers import pack_codes, restate  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7777


@pytest.fixture(scope='module')
def ctx():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native as N
    with N.Context(0) as c:
        yield c


def table(groups_packed, ref_lens):
    """list of packed [n, s] matrices -> (packed, row_off, row_len, index lists) of one row table"""
    rows = [r for p in groups_packed for r in p]
    row_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    row_len = np.concatenate([np.full(len(p), L, dtype=np.uint32) for p, L in zip(groups_packed, ref_lens)]) if rows else np.zeros(0, np.uint32)
    starts = np.concatenate([[0], np.cumsum([len(p) for p in groups_packed])])
    index = [np.arange(a, b, dtype=np.uint32) for a, b in zip(starts[:-1], starts[1:])]
    return (np.concatenate(rows) if rows else np.zeros(0, np.uint8)), row_off, row_len, index


def same(got, want):
    return got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)


def check_dropins(OF, seqs, tri, edge):
    n = seqs.shape[0]
    diff = np.full((n, n, 2), SENTINEL, dtype=np.int64)
    out = OF.compare_seq(seqs, diff)
    assert out is diff and np.array_equal(diff, square_from_tri(n, tri, SENTINEL))
    diffX = np.full((n, n, 2), SENTINEL, dtype=np.int64)
    want = diffX.copy()
    want[0], want[n - 1] = edge[0], edge[1]
    out = OF.compare_seqX(seqs, diffX)
    assert out is diffX and np.array_equal(diffX, want)


def test_every_golden_case_bit_for_bit(ctx):
    from peppan_amd import orthofilter as OF
    cases = load_g19()
    packed, row_off, row_len, index = table([c['packed'] for c in cases], [c['ref_len'] for c in cases])
    res = ctx.allele_diff(packed, row_off, row_len, index, 3)
    assert len(res) == len(cases)
    for c, (tri, edge) in zip(cases, res):
        assert same(tri, c['tri']), c['name']
        assert same(edge, c['edge']), c['name']
    # each mode on its own leaves the other out
    only_tri = ctx.allele_diff(packed, row_off, row_len, index, 1)
    only_edge = ctx.allele_diff(packed, row_off, row_len, index, 2)
    for c, (t1, e1), (t2, e2) in zip(cases, only_tri, only_edge):
        assert e1 is None and t2 is None and same(t1, c['tri']) and same(e2, c['edge']), c['name']
    for c in cases:
        check_dropins(OF, decode_rows(c['packed'], c['ref_len']), c['tri'], c['edge'])


def test_fuzz_200_random_groups(ctx):
    rng = np.random.default_rng(1915)
    groups, lens = [], []
    for _ in range(200):
        n, L = int(rng.integers(1, 301)), int(rng.integers(1, 2501))
        groups.append(random_group(rng, n, L))
        lens.append(L)
    packed, row_off, row_len, index = table(groups, lens)
    res = ctx.allele_diff(packed, row_off, row_len, index, 3)
    for k, (p, L, (tri, edge)) in enumerate(zip(groups, lens, res)):
        want_tri, want_edge = numpy_tri_edge(decode_rows(p, L))
        assert same(tri, want_tri), (k, p.shape, L)
        assert same(edge, want_edge), (k, p.shape, L)


def test_ragged_batch_equals_one_by_one_and_split_batch(ctx):
    rng = np.random.default_rng(300)
    groups, lens = [], []
    for k in range(300):
        n = int(rng.integers(0, 4)) if k % 10 == 0 else int(np.exp(rng.uniform(np.log(2), np.log(400))))
        L = int(rng.integers(1, 1200))
        groups.append(random_group(rng, n, L))
        lens.append(L)
    modes = rng.integers(1, 4, 300).astype(np.uint8)
    packed, row_off, row_len, index = table(groups, lens)
    whole = ctx.allele_diff(packed, row_off, row_len, index, modes)
    for k in range(300):
        p1, ro1, rl1, ix1 = table([groups[k]], [lens[k]])
        (tri, edge), = ctx.allele_diff(p1, ro1, rl1, ix1, int(modes[k]))
        for got, one in ((whole[k][0], tri), (whole[k][1], edge)):
            assert (got is None and one is None) or same(got, one), k
    need = sum(0 if t is None else t.nbytes for t, _ in whole) + sum(0 if e is None else e.nbytes for _, e in whole)
    biggest = max((0 if t is None else t.nbytes) + (0 if e is None else e.nbytes) for t, e in whole)
    budget = max(biggest, need // 7)
    calls = []
    real = ctx._allele_diff_call
    ctx._allele_diff_call = lambda *a: calls.append(len(a[3])) or real(*a)
    try:
        split = ctx.allele_diff(packed, row_off, row_len, index, modes, out_budget=budget)
    finally:
        del ctx._allele_diff_call
    assert len(calls) >= 3 and sum(calls) == 300
    for k in range(300):
        for got, one in zip(split[k], whole[k]):
            assert (got is None and one is None) or same(got, one), k


def test_subgroups_by_index_equal_dropin_on_the_rows(ctx):
    from peppan_amd import orthofilter as OF
    rng = np.random.default_rng(354)
    for c in [c for c in load_g19() if c['sub']]:
        packed, row_off, row_len, _ = table([c['packed']], [c['ref_len']])
        idx = np.array(c['sub']['index'], dtype=np.uint32)
        (tri, edge), = ctx.allele_diff(packed, row_off, row_len, [idx], 3)
        assert same(tri, c['sub']['tri']) and same(edge, c['sub']['edge']), c['name']
    # the :354-360 pattern: the rows of one genome, taken from the same uploaded table, next to the whole group
    L, n = 777, 90
    p = random_group(rng, n, L)
    genome = rng.integers(0, 25, n)
    dup = [np.flatnonzero(genome == g).astype(np.uint32) for g in np.unique(genome) if (genome == g).sum() > 1]
    packed, row_off, row_len, index = table([p], [L])
    res = ctx.allele_diff(packed, row_off, row_len, index + dup + [np.array([5, 5, 3], dtype=np.uint32)], 2)
    seqs = decode_rows(p, L)
    for idx, (tri, edge) in zip(index + dup + [np.array([5, 5, 3])], res):
        diffX = OF.compare_seqX(seqs[idx], np.zeros((len(idx), len(idx), 2), dtype=np.int64))
        assert tri is None and np.array_equal(edge[0], diffX[0]) and np.array_equal(edge[1], diffX[-1])
        assert np.array_equal(edge, numpy_tri_edge(seqs[idx])[1])


def test_group_differences_over_a_seq_store(ctx, tmp_path):
    from peppan_amd import orthofilter as OF
    from peppan_amd.mapbsn import MapBsn, decodeSeq
    rng = np.random.default_rng(626)
    # three members of 1000 loci each (the last one shorter); locus id = member * 1000 + row
    lens = {}
    path = str(tmp_path / 'genes.seq.npz')
    with MapBsn(path, 'w') as store:
        for m, count in ((0, 1000), (1, 1000), (2, 37)):
            member = np.empty(count, dtype=object)
            for r in range(count):
                lens[m * 1000 + r] = int(rng.choice([300, 301, 302, 903]))
            for L in set(lens[m * 1000 + r] for r in range(count)):
                which = [r for r in range(count) if lens[m * 1000 + r] == L]
                rows = random_group(rng, len(which), L)
                for r, row in zip(which, rows):
                    member[r] = row
            store.save(m, member)
    mats, ref_lens = [], []
    by_len = {}
    for i, L in lens.items():
        by_len.setdefault(L, []).append(i)
    for L, ids in sorted(by_len.items()):
        ids = np.array(ids)
        for size in (1, 2, 40, 130):
            last = ids[ids >= 2000][:min(2, size - 1)]                   # (crosses the members' 1000-id boundaries)
            pick = rng.permutation(np.concatenate([last, rng.choice(ids[ids < 2000], size=size - len(last), replace=False)]))
            mat = np.zeros((size, 6), dtype=np.int64)
            mat[:, 5] = pick
            mats.append(mat)
            ref_lens.append(L)
    assert {int(i) // 1000 for mat in mats for i in mat[:, 5]} == {0, 1, 2}
    assert any(len({int(i) // 1000 for i in mat[:, 5]}) == 3 for mat in mats)
    for source in (path, None):
        store = MapBsn(path) if source is None else None
        try:
            got = OF.group_differences(source or store, mats, ref_lens)
        finally:
            if store is not None:
                store.close()
        assert len(got) == len(mats)
        with MapBsn(path) as conn:
            for mat, L, (diffX, diff) in zip(mats, ref_lens, got):
                rows = np.array([conn.get(int(i) // 1000)[int(i) % 1000] for i in mat[:, 5].tolist()])
                seqs = np.array([0, 65, 67, 71, 84], dtype=np.uint8)[decodeSeq(rows)][:, :L]
                n = len(mat)
                assert diffX.dtype == np.int64 and diff.dtype == np.int64 and diffX.shape == (n, n, 2) and diff.shape == (n, n, 2)
                assert np.array_equal(diff, OF.compare_seq(seqs, np.zeros((n, n, 2), dtype=np.int64)))
                assert np.array_equal(diffX, OF.compare_seqX(seqs, np.zeros((n, n, 2), dtype=np.int64)))
                tri, edge = numpy_tri_edge(seqs)
                assert np.array_equal(diff, square_from_tri(n, tri))
                assert np.array_equal(diffX[0], edge[0]) and np.array_equal(diffX[-1], edge[1]) and (n <= 2 or not diffX[1:-1].any())
    only = OF.group_differences(path, mats[:3], ref_lens[:3], full=False)
    assert all(d is None and np.array_equal(x, g[0]) for (x, d), g in zip(only, got))


def test_at_size_2000_rows_of_1002_nt(ctx):
    from peppan_amd import orthofilter as OF
    rng = np.random.default_rng(2000)
    n, L = 2000, 1002
    p = random_group(rng, n, L, gap=0.05, div=0.04)
    seqs = decode_rows(p, L)
    t0 = time.time()
    want_tri, want_edge = numpy_tri_edge(seqs)
    t1 = time.time()
    packed, row_off, row_len, index = table([p], [L])
    (tri, edge), = ctx.allele_diff(packed, row_off, row_len, index, 3)
    t2 = time.time()
    print('at size: numpy formulation %.2f s, Context.allele_diff %.3f s' % (t1 - t0, t2 - t1))
    assert same(tri, want_tri) and same(edge, want_edge)
    assert int(tri[:, 1].max()) <= L + 2
    diff = OF.compare_seq(seqs, np.zeros((n, n, 2), dtype=np.int64))
    assert np.array_equal(diff, square_from_tri(n, want_tri))
    diffX = OF.compare_seqX(seqs, np.zeros((n, n, 2), dtype=np.int64))
    assert np.array_equal(diffX[0], want_edge[0]) and np.array_equal(diffX[-1], want_edge[1]) and not diffX[1:-1].any()


def test_rows_of_more_than_64_plane_words(ctx):
    """allele_planes gives lane l the words l, l + 64, ...: every other test stays below 48 words, one trip.  Random groups of 5 and 70 rows per length,
    and per length two groups of one row copied, changed and gapped only beyond the first trip (bit >= 4 096) or only within it."""
    rng = np.random.default_rng(4096)
    lens = (4095, 4096, 8190, 8191, 12300)
    assert [plane_words(L) for L in lens] == [64, 65, 128, 129, 193]
    groups, ref_lens, kinds = [], [], []
    for L in lens:
        high, bound = beyond_first_trip(L)
        low = np.flatnonzero(bit_of_column(L) < bound)
        low = low[np.argsort(-bit_of_column(L)[low])]
        assert len(high) >= 1 and len(high) + len(low) == L and (bound == 4096 or plane_words(L) == 64)
        made = [random_group(rng, 5, L), random_group(rng, 70, L)]
        for cols in (high, low):
            # the highest bits of the part, its lowest one and some between
            touch = np.unique(np.concatenate([cols[:12], cols[-1:], rng.choice(cols, min(len(cols), 20), replace=False)]))
            codes = np.repeat(rng.integers(1, 5, L)[None, :], 7, axis=0)
            how = rng.integers(0, 3, (6, len(touch)))                            # per row (the first one stays) and column: as it is, another base, a gap
            how[0, :], how[1, :] = 1, 2                                          # ... every column with another base in one row and a gap in another
            part = codes[1:, touch]
            part[how == 1] = part[how == 1] % 4 + 1
            part[how == 2] = 0
            codes[1:, touch] = part
            made.append(pack_codes(codes, rng))
        groups += made
        ref_lens += [L] * 4
        kinds += ['5 rows', '70 rows', 'beyond the first trip', 'within the first trip']
    packed, row_off, row_len, index = table(groups, ref_lens)
    t0 = time.time()
    res = ctx.allele_diff(packed, row_off, row_len, index, 3)
    t1 = time.time()
    for p, L, kind, (tri, edge) in zip(groups, ref_lens, kinds, res):
        seqs = decode_rows(p, L)
        want_tri, want_edge = numpy_tri_edge(seqs)
        if 'trip' in kind:
            # from the reference: there is something to lose (k mismatches, gaps), and nothing of it in the other part of the row
            high, bound = beyond_first_trip(L)
            keep = bit_of_column(L) < bound if 'beyond' in kind else bit_of_column(L) >= bound
            assert want_tri[:, 0].max() > 1 and want_tri[:, 1].min() < L + 2, (L, kind)
            rest = numpy_tri_edge(seqs[:, keep])[0]
            assert np.all(rest[:, 0] == 1) and np.all(rest[:, 1] == keep.sum() + 2), (L, kind)
        assert same(tri, want_tri), (L, kind)
        assert same(edge, want_edge), (L, kind)
    print('long rows: Context.allele_diff of %d groups %.3f s, numpy formulation %.2f s' % (len(groups), t1 - t0, time.time() - t1))


def test_tile_and_staging_boundaries(ctx):
    """every group size around the 64-row tile (one tile, a tile and a row, two, three and a row) at every plane width around the K15_KW = 4 words staged
    per step, in all three modes; and the same groups through K16, whose verdict_pairs masks a < b && b < n over the same tiles"""
    rng = np.random.default_rng(6465)
    sizes, lens = (2, 63, 64, 65, 127, 128, 129, 193), (1, 21, 22, 64, 190, 193, 256, 257, 320, 575, 577)
    assert {plane_words(L) for L in lens} >= {1, 2, 3, 4, 5, 9} and {plane_words(L) % 4 for L in lens} == {0, 1, 2, 3}
    assert {L % 3 for L in lens} == {0, 1, 2} and {3 * -(-L // 3) % 64 == 0 for L in lens} == {True, False}
    groups, ref_lens = [], []
    for k, (n, L) in enumerate((n, L) for n in sizes for L in lens):
        groups.append(random_group(rng, n, L, gap=(0.15, 0.02)[k % 2], div=0.002 if L in (22, 257) else 0.6))       # (two widths that others repeat stay calm)
        ref_lens.append(L)
    want = [numpy_tri_edge(decode_rows(p, L)) for p, L in zip(groups, ref_lens)]
    packed, row_off, row_len, index = table(groups, ref_lens)
    modes = rng.integers(1, 4, len(groups)).astype(np.uint8)
    for mode in (1, 2, 3, modes):
        res = ctx.allele_diff(packed, row_off, row_len, index, mode)
        for k, ((tri, edge), (want_tri, want_edge)) in enumerate(zip(res, want)):
            m = int(mode if np.isscalar(mode) else mode[k])
            assert (same(tri, want_tri) if m & 1 else tri is None) and (same(edge, want_edge) if m & 2 else edge is None), (m, len(groups[k]), ref_lens[k])
    # K16 over the same rows: genome ids 0 .. n - 1 in every group, one table for all
    from peppan_amd import orthofilter as OF
    gd_dict = {(a, b): (0.02, 0.5) for a in range(max(sizes)) for b in range(a + 1, max(sizes))}
    got = ctx.group_verdicts(packed, row_off, row_len, index, [np.arange(len(p)) for p in groups], [0] * len(groups), OF.gd_table(gd_dict, 0.002, 5), 0.002)
    seen = set()
    for p, L, (want_tri, _), (verdict, tri, leader) in zip(groups, ref_lens, want, got):
        n = len(p)
        sq = square_from_tri(n, want_tri)
        w = restate(p, L, np.arange(n), False, gd_dict, 0.002, 5, counts=(want_tri, sq[:, :, 0].tolist(), sq[:, :, 1].tolist()))
        assert verdict == w['verdict'], (n, L)
        if verdict == 2:
            assert tri.dtype == np.int32 and np.array_equal(tri, w['tri']) and leader.dtype == np.uint32 and np.array_equal(leader, w['leader']), (n, L)
            seen.add((n, plane_words(L) % 4))
        else:
            assert tri is None and leader is None
    assert seen == {(n, r) for n in sizes for r in range(4)}, sorted(seen)          # a returned triangle at every size and every staging tail


def test_error_conventions_and_context_stays_usable(ctx):
    from peppan_amd import _native as N
    rng = np.random.default_rng(7)
    p = random_group(rng, 6, 100)
    packed, row_off, row_len, index = table([p], [100])
    good = ctx.allele_diff(packed, row_off, row_len, index, 3)

    def still_good():
        again = ctx.allele_diff(packed, row_off, row_len, index, 3)
        assert same(again[0][0], good[0][0]) and same(again[0][1], good[0][1])

    # a row that does not hold ceil(row_len / 3) bytes
    bad_len = row_len.copy()
    bad_len[2] = 103
    with pytest.raises(N.PepError, match=r'pep_allele_diff failed \(-2\): pep_allele_diff: row 2 does not hold'):
        ctx.allele_diff(packed, row_off, bad_len, index, 3)
    still_good()
    # a group that mixes row_len
    p2 = random_group(rng, 3, 40)
    mixed = table([p, p2], [100, 40])
    with pytest.raises(N.PepError, match=r'\(-2\): pep_allele_diff: group 0 mixes rows of different row_len'):
        ctx.allele_diff(mixed[0], mixed[1], mixed[2], [np.array([0, 1, 7], dtype=np.uint32)], 1)
    still_good()
    # a row index >= n_rows
    with pytest.raises(N.PepError, match=r'\(-2\): pep_allele_diff: row index 6 of group 0 out of range'):
        ctx.allele_diff(packed, row_off, row_len, [np.array([0, 6], dtype=np.uint32)], 3)
    still_good()
    # a byte above 124
    spoiled = packed.copy()
    spoiled[int(row_off[4]) + 7] = 125
    with pytest.raises(N.PepError, match=r'\(-2\): pep_allele_diff: row 4 holds a byte above 124'):
        ctx.allele_diff(spoiled, row_off, row_len, index, 3)
    still_good()
    # ... also where no kernel runs (one-row triangle, no mode bit), and with the library's text whether or not the wrapper splits the batch
    for grp, mode in (([np.array([4], dtype=np.uint32)], 1), (index, 0)):
        with pytest.raises(N.PepError, match=r'\(-2\): pep_allele_diff: row 4 holds a byte above 124'):
            ctx.allele_diff(spoiled, row_off, row_len, grp, mode)
    with pytest.raises(N.PepError, match=r'\(-2\): pep_allele_diff: row index 6 of group 1 out of range'):
        ctx.allele_diff(packed, row_off, row_len, [index[0], np.array([0, 6], dtype=np.uint32), index[0]], 3, out_budget=200)
    still_good()
    # outputs that overlap, or run past out_cap (the raw entry: the wrapper lays its own buffer out correctly)
    import ctypes as C
    two = table([p, p], [100, 100])
    grp_off = np.array([0, 6, 12], dtype=np.uint64)
    grp_rows = np.arange(12, dtype=np.uint32)
    mode = np.array([1, 1], dtype=np.uint8)
    out = np.zeros(64, dtype=np.int32)

    def raw(out_off, cap):
        oo = np.array(out_off, dtype=np.uint64)
        return ctx._lib.pep_allele_diff(ctx._h, N._ptr(two[0]), N._ptr(two[1]), N._ptr(two[2]), C.c_uint64(12), C.c_uint32(2), N._ptr(grp_off), N._ptr(grp_rows),
                                        N._ptr(mode), N._ptr(out), N._ptr(oo), C.c_uint64(cap))
    assert raw([0, 30], 60) == 0
    assert np.array_equal(out[:30].reshape(-1, 2), good[0][0]) and np.array_equal(out[30:60], out[:30])
    assert raw([0, 29], 64) == -2
    assert 'overlaps' in ctx._lib.pep_last_error(ctx._h).decode()
    assert raw([30, 0], 59) == -2
    assert 'runs past out_cap' in ctx._lib.pep_last_error(ctx._h).decode()
    assert raw([34, 2], 64) == 0                                     # any order, any gaps
    assert np.array_equal(out[34:64], out[2:32]) and np.array_equal(out[2:32].reshape(-1, 2), good[0][0])
    still_good()
    # one group beyond the device budget of a call: 24 000 index entries onto one 1-nt row ask for 2.3 GB of pairs
    # (the raw entry again: the wrapper never asks for more than the library's budget, and the check comes before `out` is looked at)
    tiny = table([np.array([[25]], dtype=np.uint8)], [1])
    big_off, big_rows, one = np.array([0, 24000], dtype=np.uint64), np.zeros(24000, dtype=np.uint32), np.array([1], dtype=np.uint8)
    rc = ctx._lib.pep_allele_diff(ctx._h, N._ptr(tiny[0]), N._ptr(tiny[1]), N._ptr(tiny[2]), C.c_uint64(1), C.c_uint32(1), N._ptr(big_off), N._ptr(big_rows),
                                  N._ptr(one), N._ptr(out), N._ptr(np.zeros(1, dtype=np.uint64)), C.c_uint64(len(out)))
    assert rc == -3
    with pytest.raises(N.PepError, match=r'pep_allele_diff failed \(-3\): pep_allele_diff: 2303904000 bytes of output asked for, the device budget'):
        ctx._check(rc, 'pep_allele_diff')
    still_good()
    # ... and the wrapper: a single group beyond its budget (whatever the caller sets, never more than the library's) is refused before anything is uploaded
    with pytest.raises(N.PepError, match='group 0 .24000 rows. needs 2303904000 bytes'):
        ctx.allele_diff(tiny[0], tiny[1], tiny[2], [big_rows], 1, out_budget=1 << 40)
    with pytest.raises(N.PepError, match='budget'):
        ctx.allele_diff(packed, row_off, row_len, index, 3, out_budget=64)
    still_good()
    # legal: empty batch, empty group, one-row group, a group without a mode bit
    assert ctx.allele_diff(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), [], 3) == []
    res = ctx.allele_diff(packed, row_off, row_len, [np.zeros(0, np.uint32), np.array([3], dtype=np.uint32), index[0]], [3, 3, 0])
    assert res[0][0].shape == (0, 2) and res[0][1].shape == (2, 0, 2)
    assert res[1][0].shape == (0, 2) and res[1][1].shape == (2, 1, 2) and res[1][1][0].tolist() == res[1][1][1].tolist()
    assert res[1][1][0, 0, 0] == 1
    assert res[2] == (None, None)


def test_dropins_make_a_new_context_after_close(ctx):
    from peppan_amd import orthofilter as OF
    seqs = np.array([[65, 67, 0, 84], [65, 71, 84, 84], [0, 0, 0, 0]], dtype=np.uint8)
    want = np.zeros((3, 3, 2), dtype=np.int64)
    want[0, 1], want[0, 2], want[1, 2] = (2, 5), (1, 2), (1, 2)
    assert np.array_equal(OF.compare_seq(seqs, np.zeros((3, 3, 2), dtype=np.int64)), want)
    assert any(k[0] == os.getpid() for k in OF._CONTEXTS)
    OF.close()
    assert not any(k[0] == os.getpid() for k in OF._CONTEXTS)
    assert np.array_equal(OF.compare_seq(seqs, np.zeros((3, 3, 2), dtype=np.int64)), want)
    OF.close()
