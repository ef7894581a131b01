"""K25 on the GPU (csrc/treecut.hip: the tree cutting of filt_per_group, PEPPAN.py:424-482) against the numpy restatement of
include/peppan_hip.h (tests/treecut_helpers.py): the partition, the counts and the doubles of the cut log compared with ==, on the
one-workgroup path and on the launch chain alike; and filt_per_groups from a .seq store against the matrices the reference's own lines returned
(tests/golden/g28_treecut.json.gz).

The shapes are the smallest at which the code can go wrong: 2, 3 and 4 leaves; 64 and 65 (a word of a bit set); 256 and 257 (the limit of the
one-workgroup path: 257 leaves run the chain whatever the selector says, and `block` refuses them); and the named cases of treecut_helpers.edge_cases,
each of which tests/test_treecut_host.py holds to the branch of the definition it is meant to reach."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import treecut_helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = sorted(H.edge_cases())


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


def run(ctx, cases, names, path):
    c = [cases[k] for k in names]
    return ctx.tree_cuts([H.sets_of(x['sides']) for x in c], [x['lengths'] for x in c], [x['W0'] for x in c], [x['W1'] for x in c], [x['strong'] for x in c],
                         [x['cap'] for x in c], path)


@pytest.fixture(scope='module')
def batches(ctx, N):
    """every edge case in ONE call per path (the batch that mixes them all): path -> name -> result.  Trees beyond the one-workgroup limit are left out of
    the `block` batch, which refuses them."""
    cases, _ = H.restated_edge_cases()
    out = {}
    for path in (N.CUT_AUTO, N.CUT_BLOCK, N.CUT_CHAIN):
        names = [k for k in NAMES if path != N.CUT_BLOCK or cases[k]['sides'].shape[1] <= N.NJ_BLOCK_LEAVES]
        out[path] = dict(zip(names, run(ctx, cases, names, path)))
    return out


@pytest.mark.parametrize('name', NAMES)
def test_both_paths_equal_the_restatement(batches, N, name):
    cases, done = H.restated_edge_cases()
    want = done[name][0]
    n = cases[name]['sides'].shape[1]
    for path in (N.CUT_AUTO, N.CUT_BLOCK, N.CUT_CHAIN):
        if path == N.CUT_BLOCK and n > N.NJ_BLOCK_LEAVES:
            continue
        got = batches[path][name]
        assert got[0].dtype == np.int32 and got[5].dtype == np.float64
        assert H.same_result(got, want) is None, (name, path, H.same_result(got, want))


def test_a_tree_alone_gives_what_it_gives_in_the_batch(ctx, batches, N):
    cases, _ = H.restated_edge_cases()
    for name in ('queue', 'n65_float', 'ties'):
        for path in (N.CUT_BLOCK, N.CUT_CHAIN):
            alone = run(ctx, cases, [name], path)[0]
            for a, b in zip(alone, batches[path][name]):
                assert np.array_equal(a, b) and np.asarray(a).tobytes() == np.asarray(b).tobytes(), (name, path)


def records_of(monkeypatch, ctx, N, name, which):
    """the list that receives call_times(which) after every library call `name` of ctx from now on"""
    seen, call = [], ctx._call

    def spy(called, *args):
        call(called, *args)
        if called == name:
            seen.append(ctx.call_times(which))
    monkeypatch.setattr(ctx, '_call', spy)
    return seen


def test_call_times_of_tree_cut_and_their_total_over_a_split_batch(ctx, N, monkeypatch):
    """pep_call_times(PEP_CALL_TREE_CUT): with every phase timed, slot 0 (the preparation and the one-workgroup kernel) is > 0 for every call and slot 1 (the
    launch chains) only for a call with a tree above PEP_NJ_BLOCK_LEAVES leaves - 257 here -, the other six and the byte counts 0; untimed, every slot is 0.
    With the budget of one library call below the two matrices, tree_cuts makes two calls, and its total is the sum of their two records, bit for bit."""
    cases, done = H.restated_edge_cases()
    names = ['n2', 'n257']
    assert cases['n257']['sides'].shape[1] == N.NJ_BLOCK_LEAVES + 1
    ctx.set_timing(2)
    try:
        got = run(ctx, cases, names, N.CUT_AUTO)
        ms, to_device, to_host = ctx.call_times(N.CALL_TREE_CUT)
        print('one call: ms %r' % ms.tolist())
        assert ms.shape == (8,) and ms[0] > 0 and ms[1] > 0 and not ms[2:].any() and (to_device, to_host) == (0, 0)
        assert ctx.call_times(N.CALL_TREE_CUT, total=True)[0].tobytes() == ms.tobytes()
        monkeypatch.setattr(N, 'NJ_MAX_BYTES', 64)             # n2's matrix is 32 bytes; n257's goes alone
        seen = records_of(monkeypatch, ctx, N, 'pep_tree_cut', N.CALL_TREE_CUT)
        split = run(ctx, cases, names, N.CUT_AUTO)
        assert len(seen) == 2 and all(np.array_equal(x, y) for a, b in zip(split, got) for x, y in zip(a, b))
        (first, _, _), (second, _, _) = seen
        print('two calls: ms %r, %r' % (first.tolist(), second.tolist()))
        assert first[0] > 0 and not first[1:].any() and second[0] > 0 and second[1] > 0 and not second[2:].any()
        total, to_device, to_host = ctx.call_times(N.CALL_TREE_CUT, total=True)
        assert total.tobytes() == (first + second).tobytes() and (to_device, to_host) == (0, 0)
    finally:
        ctx.set_timing(0)
    run(ctx, cases, names, N.CUT_AUTO)
    assert not ctx.call_times(N.CALL_TREE_CUT)[0].any() and not ctx.call_times(N.CALL_TREE_CUT, total=True)[0].any()


def test_empty_batches_and_the_block_limit(ctx, N):
    assert ctx.tree_cuts([], [], [], [], []) == []
    cases, _ = H.restated_edge_cases()
    with pytest.raises(N.PepError, match=r'tree 0 has 257 leaves, the one-workgroup path takes 256'):
        run(ctx, cases, ['n257'], N.CUT_BLOCK)


def test_matrices_are_checked_before_any_launch(ctx, N):
    cases, _ = H.restated_edge_cases()
    c = dict(cases['n4'])
    for field, a, b, value, text in (('W0', 1, 2, np.nan, r'W0 \[1, 2\] of tree 0 is not finite and >= 0'),
                                     ('W1', 0, 3, np.inf, r'W1 \[0, 3\] of tree 0 is not finite and >= 0'),
                                     ('W0', 0, 1, -1.0, r'W0 \[0, 1\] of tree 0 is not finite and >= 0')):
        bad = dict(c)
        bad[field] = c[field].copy()
        bad[field][a, b] = bad[field][b, a] = value
        with pytest.raises(N.PepError, match=text):
            run(ctx, {'bad': bad}, ['bad'], N.CUT_AUTO)
    bad = dict(c)
    bad['W1'] = c['W1'].copy()
    bad['W1'][2, 1] += 0.5
    with pytest.raises(N.PepError, match=r'W1 \[1, 2\] of tree 0 is not its mirror entry: the matrix is not symmetric'):
        run(ctx, {'bad': bad}, ['bad'], N.CUT_AUTO)
    bad = dict(c)
    bad['lengths'] = c['lengths'].copy()
    bad['lengths'][3] = np.inf
    with pytest.raises(N.PepError, match=r'the length of branch 3 of tree 0 is not finite'):
        run(ctx, {'bad': bad}, ['bad'], N.CUT_AUTO)


def test_cut_trees_takes_texts_and_leaders_that_are_not_contiguous(N):
    from peppan_amd import treecut
    # rows 2, 5, 11 and 12 lead; the others are members.  Leaders 2 and 5 agree, 11 and 12 agree, the two pairs do not
    inc = np.zeros((14, 14, 2))
    lead = [2, 5, 11, 12]
    for a in lead:
        for b in lead:
            if a != b:
                inc[a, b] = (3.0, 32.0) if (a < 10) == (b < 10) else (70.0 + a + b, 32.0)
    text = '((X12:0.1,X11:0.2):0.05,X5:0.1,X2:0.3);'
    sides = np.array([[0, 0, 0, 1], [0, 0, 1, 0], [0, 0, 1, 1], [0, 1, 0, 0], [1, 0, 0, 0]], bool)
    want = H.cut_restated(sides, [0.1, 0.2, 0.05, 0.1, 0.3], inc[np.ix_(lead, lead)][:, :, 0], inc[np.ix_(lead, lead)][:, :, 1], [True, False, False, False])
    assert want['n_cuts'] == 1 and want['part'].tolist() == [0, 0, -1, -1]
    for path in (N.CUT_BLOCK, N.CUT_CHAIN):
        for tree in (text, text.replace('X', '')):
            # leaders given out of order: strong goes with them
            got, = treecut.cut_trees([tree], [inc], [[12, 2, 11, 5]], [[False, True, False, False]], path=path)
            assert got.leaves.tolist() == lead
            assert H.same_result(tuple(got[1:]), want) is None, H.same_result(tuple(got[1:]), want)
    assert treecut.cut_trees([], [], [], []) == []
    with pytest.raises(ValueError, match='the tree names leaves'):
        treecut.cut_trees([text], [inc], [[2, 5, 11]], [[True] * 3])


def test_a_compatible_tree_hands_back_the_matrix_itself(N):
    from peppan_amd import orthofilter, treecut
    mat = np.arange(5 * 7).reshape(5, 7)
    inc = np.zeros((5, 5, 2))
    inc[:, :, 1] = 32.0
    got, = treecut.cut_trees(['(X0:0.1,X1:0.1,X3:0.2);'], [inc], [[0, 1, 3]], [[True] * 3])
    assert (got.n_parts, got.n_cuts, got.part.tolist()) == (1, 0, [0, 0, 0])
    mats = orthofilter.mats_of_cut(mat, [[0, 2], [1], [3, 4]], got.leaves, got.part, got.n_parts)
    assert len(mats) == 1 and mats[0] is mat


# ---- the reference's own lines: filt_per_groups from a .seq store

@pytest.fixture(scope='module')
def golden():
    return H.load_golden()


def test_filt_per_groups_returns_what_the_reference_returned(golden, tmp_path_factory, N):
    from peppan_amd import orthofilter
    store, to_run, gds, params = H.golden_store(golden, str(tmp_path_factory.mktemp('treecut')))
    n_cut = 0
    for key, idx in H.golden_by_params(golden).items():
        got, n_ties = orthofilter.filt_per_groups(store, [to_run[k] for k in idx], gds[key], params[key])
        assert n_ties == 0
        for k, mats in zip(idx, got):
            case = golden['cases'][k]
            assert [m[:, 6].tolist() for m in mats] == case['returned'], case['name']
            assert all(np.array_equal(m, to_run[k][0][m[:, 6]]) for m in mats), case['name']
            if case['returned'] == [list(range(case['n']))]:
                assert len(mats) == 1 and mats[0] is to_run[k][0], case['name']
            n_cut += len(case['returned']) > 1 or case['returned'][0] != list(range(case['n']))
    assert n_cut >= 10
    orthofilter.close()


def test_the_device_makes_the_texts_the_fixture_recorded(golden, tmp_path_factory, N):
    # the generator made its tree texts with the numpy restatement of K21, which the device equals bit for bit: the same text, so the same tree is cut
    from peppan_amd import orthofilter
    store, to_run, gds, params = H.golden_store(golden, str(tmp_path_factory.mktemp('treecut_texts')))
    for key, idx in H.golden_by_params(golden).items():
        groups = [to_run[k] for k in idx]
        verdicts = orthofilter.group_verdicts(store, groups, gds[key], params[key])
        texts, _ = orthofilter.group_trees(store, groups, verdicts)
        assert texts == [golden['cases'][k]['text'] for k in idx]
    orthofilter.close()


def test_ml_is_refused_by_name(golden, tmp_path_factory, N):
    from peppan_amd import orthofilter
    store, to_run, gds, params = H.golden_store(golden, str(tmp_path_factory.mktemp('treecut_ml')))
    key, idx = next((key, idx) for key, idx in H.golden_by_params(golden).items() if any(golden['cases'][k]['text'] for k in idx))
    with pytest.raises(NotImplementedError, match='FastTree'):
        orthofilter.filt_per_groups(store, [to_run[k] for k in idx], gds[key], dict(params[key], orthology='ml'))
    orthofilter.close()
