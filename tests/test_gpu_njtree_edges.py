"""K21 on the GPU (csrc/njtree.hip) at the branches tests/test_gpu_njtree.py does not reach, against the same references: the numpy restatement of
include/peppan_hip.h's rules (node ids as integers, branch lengths as bit patterns) and numpy's Kimura counts (tests/njtree_helpers.py).

  ties            several pairs attain the smallest Q, in rows of different wavefronts and of different workgroups, in both LDS classes, the in-place
                  class and the launch chain: nj_take and the order in which a lane visits its rows decide the tree
  1030 leaves     the chain has 256 workgroups at most, so from 1026 leaves a wavefront of nj_scan_rows takes a second row
  chain state     r, the partial results, the live lists and node are sized by the largest chain tree of a call and reused tree after tree
  overflow        finite distances whose row sums overflow: no Q below +infinity (the first two live slots are joined), NaN among the Q
  the C layout    pep_nj_trees with offsets that start behind 0 and leave gaps; pep_kimura_pairs with outputs in any order, with gaps, and its refusals
  kimura_pairs    groups of 64, 65, 128 and 129 rows (a tile of pairs is 64 x 64 rows), and the whole 5 x 5 table of codes

tests/test_njtree_host.py proves from the restatement's trace, without a GPU, that every tie and overflow matrix used here reaches its branch.  The
restatements are made once per process (H.edge_case) and shared with that module."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import njtree_helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu

TIE_CASES = [(kind, n) for kind, sizes in (('tied', H.TIED_SIZES), ('clades', H.TIED_SIZES), ('constant', H.CONSTANT_SIZES), ('cgav12', H.CGAV12_SIZES))
             for n in sizes]


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


@pytest.fixture(scope='module')
def ctx(N):
    with N.Context(0) as c:
        yield c


def held_to_the_cases(got, cases, nan_bits_free=False):
    """got: what Context.nj_trees returned for the matrices of `cases` ((kind, n) of H.edge_case).  nan_bits_free: a length that is NaN in the
    restatement has to be NaN, with whatever sign and payload"""
    assert len(got) == len(cases)
    for (node, length), (kind, n) in zip(got, cases):
        _, want_node, want_length, _ = H.edge_case(kind, n)
        assert node.dtype == np.uint32 and np.array_equal(node, want_node), (kind, n)
        assert length.dtype == np.float64 and len(length) == len(want_length), (kind, n)
        nan = np.isnan(want_length) if nan_bits_free else np.zeros(len(want_length), bool)
        assert np.array_equal(np.isnan(length) & nan, nan), (kind, n)
        assert np.array_equal(length.view(np.uint64)[~nan], want_length.view(np.uint64)[~nan]), (kind, n)


def matrices(cases):
    return [H.edge_case(kind, n)[0] for kind, n in cases]


def test_ties_in_every_class_in_one_call(ctx):
    held_to_the_cases(ctx.nj_trees(matrices(TIE_CASES)), TIE_CASES)


@pytest.mark.parametrize('kind,n', TIE_CASES)
def test_ties_one_tree_per_call(ctx, kind, n):
    held_to_the_cases(ctx.nj_trees(matrices([(kind, n)])), [(kind, n)])


def test_the_chain_beyond_256_workgroups(ctx):
    cases = [('planted', 1030), ('tied', 1030), ('clades', 1030)]
    got = ctx.nj_trees(matrices(cases))
    assert got[0][0][:2].tolist() == [1026, 1028]               # list row 1026: the second trip of its wavefront
    held_to_the_cases(got, cases)


def test_several_chain_trees_in_one_call(ctx):
    """the chain state is sized by the second tree and used by all four; then with an LDS tree and an in-place tree between them"""
    cases = [('clades', 257), ('clades', 1030), ('cgav12', 301), ('clades', 258)]
    held_to_the_cases(ctx.nj_trees(matrices(cases)), cases)
    cases = [('clades', 257), ('clades', 20), ('clades', 1030), ('cgav12', 100), ('cgav12', 301), ('clades', 258)]
    held_to_the_cases(ctx.nj_trees(matrices(cases)), cases)


def test_overflowing_row_sums(ctx):
    """Distances of 1e308: every row sum is +infinity and every Q NaN, so every round joins the first two live slots; one row of 1.5e308: the Q of that
    row are NaN, all others -infinity and tied.  Node ids are equal; the lengths are NaN where the restatement's are, and equal bit for bit elsewhere.
    The sign and the payload of a NaN are no part of the header's contract: x86 makes the default NaN of an invalid operation negative, the GPU
    positive, and both pass an operand's payload on."""
    cases = [('all_nan', n) for n in H.ALL_NAN_SIZES] + [('huge_row', n) for n in H.HUGE_ROW_SIZES]
    assert H.edge_case('all_nan', 6)[1].tolist() == [0, 1, 6, 2, 7, 3, 8, 4, 5]
    assert all(np.isnan(H.edge_case(kind, n)[2]).any() for kind, n in cases)
    held_to_the_cases(ctx.nj_trees(matrices(cases)), cases, nan_bits_free=True)
    for case in cases:
        held_to_the_cases(ctx.nj_trees(matrices([case])), [case], nan_bits_free=True)
    ordinary = [('cgav12', 100), ('clades', 33), ('tied', 257)]
    held_to_the_cases(ctx.nj_trees(matrices(ordinary)), ordinary)


def test_nj_trees_c_layout_with_a_start_behind_zero_and_gaps(ctx, N):
    sizes = (90, 2, 300, 33, 3, 20)
    mats = [H.euclidean(n, 600 + n) for n in sizes]
    n_leaves = np.array(sizes, np.uint32)
    dist_off, out_off = [5], [7]
    for n in sizes:
        dist_off.append(dist_off[-1] + n * n + 3)                 # 3 spare doubles behind every matrix
        out_off.append(out_off[-1] + (2 if n == 2 else 2 * n - 3) + 2)      # 2 spare entries behind every tree
    dist = np.full(dist_off[-1], np.nan)                          # outside the matrices: never read, the finiteness check included
    for m, at in zip(mats, dist_off):
        dist[at:at + m.size] = m.reshape(-1)
    before = dist.tobytes()
    node, length = np.full(out_off[-1], 0xDEADBEEF, np.uint32), np.full(out_off[-1], -7.0)
    d_off, o_off = np.array(dist_off, np.uint64), np.array(out_off, np.uint64)
    rc = ctx._lib.pep_nj_trees(ctx._h, N._ptr(dist), N._ptr(d_off), N._ptr(n_leaves), len(sizes), N._ptr(node), N._ptr(length), N._ptr(o_off))
    assert rc == 0, ctx._lib.pep_last_error(ctx._h).decode()
    assert dist.tobytes() == before
    between = np.ones(out_off[-1], bool)
    between[:7] = False
    for m, at in zip(mats, out_off):
        want_node, want_length = H.nj_restated(m)
        assert np.array_equal(node[at:at + len(want_node)], want_node), len(m)
        assert np.array_equal(length[at:at + len(want_node)].view(np.uint64), want_length.view(np.uint64)), len(m)
        between[at:at + len(want_node)] = False
    assert between.sum() == 2 * len(sizes) and not node[between].any() and not length[between].view(np.uint64).any()
    assert (node[:7] == 0xDEADBEEF).all() and (length[:7] == -7.0).all()


def kimura_groups(rows_per_group, columns, seed):
    """one group of random rows over 0..4 per entry of rows_per_group -> (the library's tables as a dict, codes per group)"""
    rng = np.random.default_rng(seed)
    codes = [rng.integers(0, 5, (n, columns)).astype(np.uint8) for n in rows_per_group]
    return kimura_tables(codes), codes


def kimura_tables(codes):
    rows = [r for c in codes for r in H.pack_codes(c)]
    starts = np.concatenate([[0], np.cumsum([len(c) for c in codes])])
    return dict(packed=np.concatenate(rows), row_off=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64),
                row_len=np.concatenate([np.full(len(c), c.shape[1], np.uint32) for c in codes]),
                groups=[np.arange(a, b, dtype=np.uint32) for a, b in zip(starts[:-1], starts[1:])])


def test_kimura_pairs_c_layout_any_order_gaps_and_refusals(ctx, N):
    T, codes = kimura_groups((3, 4, 5, 6), 50, 81)
    want = [H.kimura_counts(c).reshape(-1) for c in codes]
    need = [len(w) for w in want]
    assert need == [9, 18, 30, 45]
    grp_off = np.array([0, 3, 7, 12, 18], np.uint64)
    grp_rows = np.arange(18, dtype=np.uint32)
    SENTINEL = -12345

    def raw(out_off, cap):
        out = np.full(cap + 4, SENTINEL, np.int32)
        oo = np.array(out_off, np.uint64)
        rc = ctx._lib.pep_kimura_pairs(ctx._h, N._ptr(T['packed']), N._ptr(T['row_off']), N._ptr(T['row_len']), 18, 4, N._ptr(grp_off), N._ptr(grp_rows),
                                       N._ptr(out), N._ptr(oo), cap)
        return rc, out

    def laid_out(out_off, cap):
        rc, out = raw(out_off, cap)
        assert rc == 0, ctx._lib.pep_last_error(ctx._h).decode()
        untouched = np.ones(len(out), bool)
        for g, at in enumerate(out_off):
            assert np.array_equal(out[at:at + need[g]], want[g]), (out_off, g)
            untouched[at:at + need[g]] = False
        assert untouched.sum() == len(out) - sum(need) and (out[untouched] == SENTINEL).all(), out_off

    laid_out([0, 9, 27, 57], 102)                                    # as the wrapper lays them out: one copy
    laid_out([120, 95, 60, 10], 135)                                 # descending, a gap before, between and behind: four copies
    laid_out([30, 84, 0, 39], 102)                                   # a permutation without gaps: four copies
    laid_out([0, 9, 40, 70], 115)                                    # two groups in one copy, then gaps
    rc, out = raw([0, 8, 30, 60], 200)
    assert rc == -2 and 'pep_kimura_pairs: output of group 1 overlaps another group\'s' in ctx._lib.pep_last_error(ctx._h).decode()
    assert (out == SENTINEL).all()
    rc, out = raw([0, 9, 27, 57], 101)
    assert rc == -2 and 'pep_kimura_pairs: output of group 3 runs past out_cap' in ctx._lib.pep_last_error(ctx._h).decode()
    assert (out == SENTINEL).all()
    laid_out([120, 95, 60, 10], 135)
    got = ctx.kimura_pairs(T['packed'], T['row_off'], T['row_len'], T['groups'])
    assert all(np.array_equal(g.reshape(-1), w) for g, w in zip(got, want))


def test_kimura_pairs_at_the_tile_edges(ctx):
    """64 rows: one tile of pairs; 65: a second tile row of one row; 128 and 129: the same one tile further, three tile rows"""
    T, codes = kimura_groups((64, 65, 128, 129), 65, 82)
    got = ctx.kimura_pairs(T['packed'], T['row_off'], T['row_len'], T['groups'])
    for g, c in zip(got, codes):
        want = H.kimura_counts(c)
        assert g.dtype == np.int32 and g.shape == want.shape == (len(c) * (len(c) - 1) // 2, 3) and np.array_equal(g, want), len(c)


def test_kimura_pairs_over_the_whole_code_table(ctx):
    """five constant rows, row k all code k: comparable is the length when both codes are no gap; transitions are A <-> G (1, 3) and C <-> T (2, 4) and
    nothing else; the other four pairs of different bases are transversions"""
    lengths = (1, 2, 3, 64, 65, 128, 129, 193)
    codes = [np.repeat(np.arange(5, dtype=np.uint8)[:, None], L, axis=1) for L in lengths]
    T = kimura_tables(codes)
    got = ctx.kimura_pairs(T['packed'], T['row_off'], T['row_len'], T['groups'])
    pairs = [(a, b) for a in range(5) for b in range(a + 1, 5)]
    for g, c, L in zip(got, codes, lengths):
        want = [(L if a else 0, L if (a, b) in ((1, 3), (2, 4)) else 0, L if a and (a, b) not in ((1, 3), (2, 4)) else 0) for a, b in pairs]
        assert g.tolist() == [list(w) for w in want], L
        assert np.array_equal(g, H.kimura_counts(c)), L
