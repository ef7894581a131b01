"""K21 on the GPU (csrc/njtree.hip: neighbour-joining trees, the two rapidnj calls of the reference, PEPPAN.py:19, 409-417 and PEPPAN_parser.py:168) against
the numpy restatement of include/peppan_hip.h's rules (tests/njtree_helpers.py): node ids as integers, branch lengths as bit patterns; Kimura's
pair counts against numpy counts.

The sizes are those at which the code takes another path: a matrix of up to 32 and up to 80 leaves lives in LDS (two kernels), up to
PEP_NJ_BLOCK_LEAVES in device memory with one workgroup per tree, beyond that a chain of launches; a wavefront covers 64 columns of a row; a tile of
pairs is 64 x 64 rows, a plane word 64 digits, and the last byte of a packed row is padded with digits beyond the row's length."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import njtree_helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu


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


def held_to_the_restatement(got, matrices, tag=''):
    assert len(got) == len(matrices)
    for k, ((node, length), m) in enumerate(zip(got, matrices)):
        want_node, want_length = H.nj_restated(m)
        assert node.dtype == np.uint32 and np.array_equal(node, want_node), (tag, k, len(m))
        assert length.dtype == np.float64 and np.array_equal(length.view(np.uint64), want_length.view(np.uint64)), (tag, k, len(m))


def test_small_trees_and_the_wavefront_edge(ctx):
    mats = [H.euclidean(n, 300 + n) for n in (2, 3, 4, 5, 63, 64, 65)]
    held_to_the_restatement(ctx.nj_trees(mats), mats)
    node, length = ctx.nj_trees([np.array([[0., 0.3], [9., 0.]])])[0]          # only the entries with row < column are read
    assert node.tolist() == [0, 1] and length.tolist() == [0.3, 0.3]


def test_the_two_lds_classes_and_their_edges(ctx):
    mats = [H.euclidean(n, 400 + n) for n in (32, 33, 80, 81)]
    held_to_the_restatement(ctx.nj_trees(mats), mats)


def test_around_the_one_workgroup_limit(ctx, N):
    B = N.NJ_BLOCK_LEAVES
    mats = [H.euclidean(n, 500 + n) for n in (B - 1, B, B + 1)]
    held_to_the_restatement(ctx.nj_trees(mats), mats)


def test_a_launch_chain_of_300_leaves_beside_small_trees(ctx):
    mats = [H.euclidean(7, 1), H.cgav_like(301, 2), H.euclidean(90, 3)]
    held_to_the_restatement(ctx.nj_trees(mats), mats)


def test_200_mixed_trees_in_one_call(ctx):
    mats = H.mixed_batch(200)
    assert not mats[10].any() and {len(m) for m in mats} >= {2, 3, 4, 5, 63, 64, 65, 70}
    want = [H.nj_restated(m) for m in mats]
    assert min(float(length.min()) for _, length in want) < -0.01          # a negative branch length is among them
    got = ctx.nj_trees(mats)
    for k, ((node, length), (want_node, want_length)) in enumerate(zip(got, want)):
        assert np.array_equal(node, want_node) and np.array_equal(length.view(np.uint64), want_length.view(np.uint64)), (k, len(mats[k]))
    assert ctx.nj_trees([]) == []


def test_refusals_leave_the_context_usable(ctx, N):
    with pytest.raises(N.PepError, match='tree 1 has 1 leaves'):
        ctx.nj_trees([np.zeros((2, 2)), np.zeros((1, 1))])
    bad = H.euclidean(5, 9)
    bad[1, 3] = np.inf
    with pytest.raises(N.PepError, match=r'distance \[1, 3\] of tree 0 is not finite'):
        ctx.nj_trees([bad])
    bad[1, 3], bad[3, 1] = 1., np.nan                                    # below the diagonal: not read
    held_to_the_restatement(ctx.nj_trees([bad]), [bad])
    with pytest.raises(ValueError):
        ctx.nj_trees([np.zeros((2, 3))])


def kimura_case(lengths, seed):
    """per length a group of random rows over 0..4 -> (packed, row_off, row_len, groups, codes per group)"""
    rng = np.random.default_rng(seed)
    codes = [rng.integers(0, 5, (int(rng.integers(3, 9)), L)).astype(np.uint8) for L in lengths]
    packed = [H.pack_codes(c) for c in codes]
    rows = [r for p in packed for r in p]
    row_off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    row_len = np.concatenate([np.full(len(c), c.shape[1], np.uint32) for c in codes])
    starts = np.concatenate([[0], np.cumsum([len(c) for c in codes])])
    groups = [np.arange(a, b, dtype=np.uint32) for a, b in zip(starts[:-1], starts[1:])]
    return np.concatenate(rows), row_off, row_len, groups, codes


def test_kimura_pairs_at_the_edges_of_a_word_and_a_byte(ctx):
    packed, row_off, row_len, groups, codes = kimura_case((1, 63, 64, 65, 193), 77)
    # one row serves two groups (rows of the 64-column group, once reversed and overlapping); one group has a single row; one has none
    groups += [groups[2][::-1].copy(), groups[2][1:3].copy(), groups[4][:1].copy(), np.zeros(0, np.uint32)]
    codes += [codes[2][::-1], codes[2][1:3], codes[4][:1], codes[4][:0]]
    got = ctx.kimura_pairs(packed, row_off, row_len, groups)
    assert len(got) == len(groups)
    for k, (g, c) in enumerate(zip(got, codes)):
        want = H.kimura_counts(c)
        assert g.dtype == np.int32 and g.shape == want.shape and np.array_equal(g, want), k
    assert got[-1].shape == (0, 3) and got[-2].shape == (0, 3)
    assert ctx.kimura_pairs(packed, row_off, row_len, []) == []
    assert ctx.kimura_pairs(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), []) == []


def test_kimura_pairs_over_more_than_one_tile(ctx, N):
    rng = np.random.default_rng(78)
    codes = rng.integers(0, 5, (70, 100)).astype(np.uint8)
    packed = H.pack_codes(codes)
    row_off = np.arange(71, dtype=np.uint64) * np.uint64(packed.shape[1])
    got, = ctx.kimura_pairs(packed.reshape(-1), row_off, np.full(70, 100, np.uint32), [np.arange(70, dtype=np.uint32)])
    assert np.array_equal(got, H.kimura_counts(codes))
    with pytest.raises(N.PepError, match='row index 70'):
        ctx.kimura_pairs(packed.reshape(-1), row_off, np.full(70, 100, np.uint32), [np.array([0, 70], np.uint32)])
    packed[3, 5] = 125
    with pytest.raises(N.PepError, match='row 3 holds a byte above 124'):
        ctx.kimura_pairs(packed.reshape(-1), row_off, np.full(70, 100, np.uint32), [np.arange(70, dtype=np.uint32)])


def paralog_group(rng, L, clades, per_clade, apart):
    """`clades` tight clades (0.2 % inside, so one leader each) `apart` from a common ancestor, every clade over the same genomes: paralogs"""
    anc = rng.integers(1, 5, L)
    rows, genomes = [], []
    for _ in range(clades):
        centre = anc.copy()
        hit = rng.random(L) < apart
        centre[hit] = (centre[hit] - 1 + rng.integers(1, 4, int(hit.sum()))) % 4 + 1
        for g in range(per_clade):
            row = centre.copy()
            hit = rng.random(L) < 0.002
            row[hit] = (row[hit] - 1 + rng.integers(1, 4, int(hit.sum()))) % 4 + 1
            row[rng.random(L) < 0.01] = 0
            rows.append(row)
            genomes.append(g + 1)
    return np.array(rows, dtype=np.uint8), genomes


def records_of(monkeypatch, ctx, N, name, which):
    """the list that receives call_times(which) after every library call `name` of ctx from now on"""
    seen, call = [], ctx._call

    def spy(called, *args):
        call(called, *args)
        if called == name:
            seen.append(ctx.call_times(which))
    monkeypatch.setattr(ctx, '_call', spy)
    return seen


def test_totals_of_the_split_wrappers_are_the_sums_of_their_calls(ctx, N, monkeypatch):
    """nj_trees with the budget of one library call below its two matrices, kimura_pairs with an out_budget of one group's counts: two library calls each,
    and call_times(.., total=True) is the sum of the two records read after each call, bit for bit.  The chain slot of the trees is > 0 only for the call
    that holds the tree of 257 leaves."""
    ctx.set_timing(2)
    try:
        mats = [H.euclidean(5, 1), H.euclidean(N.NJ_BLOCK_LEAVES + 1, 2)]
        monkeypatch.setattr(N, 'NJ_MAX_BYTES', 8 * 25)
        seen = records_of(monkeypatch, ctx, N, 'pep_nj_trees', N.CALL_NJ_TREES)
        held_to_the_restatement(ctx.nj_trees(mats), mats)
        assert len(seen) == 2
        (first, _, _), (second, _, _) = seen
        print('nj_trees: ms %r, %r' % (first.tolist(), second.tolist()))
        assert first[0] > 0 and not first[1:].any() and second[1] > 0 and not second[2:].any()
        total, to_device, to_host = ctx.call_times(N.CALL_NJ_TREES, total=True)
        assert total.tobytes() == (first + second).tobytes() and (to_device, to_host) == (0, 0)
        monkeypatch.undo()
        packed, row_off, row_len, groups, codes = kimura_case((40, 90), 6)
        need = [12 * (len(c) * (len(c) - 1) // 2) for c in codes]
        seen = records_of(monkeypatch, ctx, N, 'pep_kimura_pairs', N.CALL_KIMURA_PAIRS)
        got = ctx.kimura_pairs(packed, row_off, row_len, groups, out_budget=max(need))
        assert len(seen) == 2 and all(np.array_equal(g, H.kimura_counts(c)) for g, c in zip(got, codes))
        (first, _, _), (second, _, _) = seen
        print('kimura_pairs: ms %r, %r' % (first.tolist(), second.tolist()))
        assert (first[:2] > 0).all() and (second[:2] > 0).all() and not first[2:].any() and not second[2:].any()
        assert ctx.call_times(N.CALL_KIMURA_PAIRS, total=True)[0].tobytes() == (first + second).tobytes()
    finally:
        monkeypatch.undo()
        ctx.set_timing(0)


def test_gene_trees_over_a_seq_store(N, tmp_path):
    from peppan_amd import njtree as NJ, orthofilter as OF
    from peppan_amd.mapbsn import MapBsn
    rng = np.random.default_rng(79)
    shapes = [(600, 5, 3, 0.08), (301, 3, 4, 0.15), (900, 2, 2, 0.10), (450, 9, 2, 0.05)]
    all_codes = [paralog_group(rng, *s) for s in shapes]
    calm = np.repeat(rng.integers(1, 5, 300)[None, :], 4, axis=0).astype(np.uint8)            # four identical rows: not divergent, no tree
    all_codes.append((calm, [1, 2, 3, 4]))
    rows = [r for codes, _ in all_codes for r in H.pack_codes(codes)]
    # ... and, as loci 1000 and 1001, a group whose two leaders share no column: Kimura's distance is undefined, the group gets no tree
    blind = np.zeros((2, 60), np.uint8)
    blind[0, :30], blind[1, 30:] = 1, 2
    path = str(tmp_path / 'genes.seq.npz')
    with MapBsn(path, 'w') as store:
        for key, packed_rows in ((0, rows), (1, list(H.pack_codes(blind)))):
            member = np.empty(len(packed_rows), dtype=object)
            for k, r in enumerate(packed_rows):
                member[k] = r
            store.save(key, member)
    to_run, at = [], 0
    for codes, genomes in all_codes:
        mat = np.zeros((len(codes), 7), dtype=np.int64)
        mat[:, 1], mat[:, 5] = genomes, np.arange(at, at + len(codes))
        at += len(codes)
        to_run.append([mat, True, codes.shape[1], path, 'unused'])
    gd = {(a, b): (0.01, 0.3) for a in range(1, 6) for b in range(a + 1, 6)}
    verdicts = OF.group_verdicts(path, to_run, gd, dict(self_id=0.002, allowed_sigma=3))
    assert [v.verdict for v in verdicts] == [2, 2, 2, 2, 0] and all(v.needs_tree for v in verdicts[:4])
    mat = np.zeros((2, 7), dtype=np.int64)
    mat[:, 1], mat[:, 5] = [1, 1], [1000, 1001]
    to_run.append([mat, True, 60, path, 'unused'])
    forced = OF.GroupVerdict(2)
    forced.groups, forced.needs_tree = [[0], [1]], True
    texts, n_undefined = OF.group_trees(path, to_run, verdicts + [forced])
    assert n_undefined == 1 and texts[4] is None and texts[5] is None
    for (codes, _), v, text in zip(all_codes[:4], verdicts, texts):
        leaders = [g[0] for g in v.groups]
        assert len(leaders) >= 2
        tags = codes[leaders]
        counts = H.kimura_counts(tags)
        d, undefined = NJ.kimura_distances(counts[:, 0], counts[:, 1], counts[:, 2])
        assert not undefined.any()
        want = NJ.newick(NJ.NjTree(*H.nj_restated(d), len(d)), ['X%d' % a for a in leaders])
        assert text == want
        assert sorted(NJ.parse_newick(text)[0]) == sorted('X%d' % a for a in leaders)
    OF.close()


def test_writecgav_writes_all_three_files(N, tmp_path, monkeypatch):
    from peppan_amd import njtree as NJ, panparser as PP
    rng = np.random.default_rng(80)
    genomes = ['g%02d' % k for k in range(12)]
    founders = rng.integers(1, 5, (3, 80))
    ortho = {}
    for k, g in enumerate(genomes):
        alleles = founders[k % 3].copy()
        change = rng.random(80) < 0.2
        alleles[change] = rng.integers(1, 9, int(change.sum()))
        ortho[g] = {'gene%03d' % j: {'%s_%d' % (g, j): int(a)} for j, a in enumerate(alleles)}
    monkeypatch.setattr(PP.shutil, 'which', lambda name: None)
    prefix = str(tmp_path / 'run')
    PP.writeCGAV(prefix, ortho, 95)
    for ext in ('profile', 'dist', 'nwk'):
        assert os.path.getsize('%s_CGAV.%s' % (prefix, ext)) > 0
    names, _, profiles = PP.cgav_profiles(ortho, 95)
    distances = PP.getDistance(np.array(profiles))
    want = NJ.newick(NJ.NjTree(*H.nj_restated(distances), 12), names) + '\n'
    text = open(prefix + '_CGAV.nwk').read()
    assert text == want and sorted(NJ.parse_newick(text)[0]) == genomes
    PP.close()


def test_live_resources_return_to_their_start(N):
    before = N.live_resources()
    with N.Context(0) as c:
        c.set_timing(2)
        mats = [H.euclidean(20, 1), H.euclidean(60, 2), H.euclidean(100, 3), H.euclidean(N.NJ_BLOCK_LEAVES + 2, 4)]
        held_to_the_restatement(c.nj_trees(mats), mats)
        ms = c.call_times(N.CALL_NJ_TREES, total=True)[0]
        assert ms[0] > 0 and ms[1] > 0
        packed, row_off, row_len, groups, codes = kimura_case((90,), 5)
        assert np.array_equal(c.kimura_pairs(packed, row_off, row_len, groups)[0], H.kimura_counts(codes[0]))
        ms = c.call_times(N.CALL_KIMURA_PAIRS, total=True)[0]
        assert ms[0] > 0 and ms[1] > 0
        during = N.live_resources()
        assert during[0] > before[0]
    assert N.live_resources() == before
