"""K25 (the tree cutting of filt_per_group, PEPPAN.py:424-482) without a GPU: the numpy restatement of tests/treecut_helpers.py against what the reference's
own lines returned for the committed fixture (tests/golden/g28_treecut.json.gz, made by tests/golden/make_golden_treecut.py over a stand-in for ete3), the
edge cases of the GPU tests held to the branches of the definition they are meant to reach, every refusal of the device-free pep_tree_cut_check, the
expansion of a partition into matrices, and the K25 section of the header against _native's constants.

The tolerance is zero: partitions, counts, codes and messages are compared with ==."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import treecut_helpers as H  # noqa: E402
import test_abi as ABI  # noqa: E402
from divergence_helpers import pair_counts, restate  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEP_ERR_ARG, PEP_ERR_LIMIT = -2, -3


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


def test_restatement_returns_what_the_reference_returned(N):
    from peppan_amd import njtree, orthofilter, treecut
    golden = H.load_golden()
    assert len(golden['cases']) >= 18 and {c['kind'] for c in golden['cases']} == {'dyadic', 'float', 'calm'}
    n_cut = n_dropped = 0
    for k, c in enumerate(golden['cases']):
        mat, packed = H.golden_mat(c, k), np.array(H.golden_rows(c))
        if c['text'] is None:
            assert c['returned'] == [list(range(c['n']))]
            continue
        gd = {(a + k * 100000, b + k * 100000): (m, s) for a, b, m, s in c['global_differences']}
        mine = restate(packed, c['ref_len'], mat[:, 1], c['inparalog'], gd, c['self_id'], c['allowed_sigma'])
        _, mut, aln = pair_counts(packed, c['ref_len'])
        diff = np.zeros((c['n'], c['n'], 2))
        diff[:, :, 0], diff[:, :, 1] = np.array(mut, dtype=float), np.array(aln, dtype=float)
        distances = orthofilter.distances_from_diff(diff, mat[:, 1], orthofilter.gd_table(gd, c['self_id'], c['allowed_sigma']))
        incompatible, needs_tree = orthofilter.incompatible_of(distances, mine['groups'])
        assert needs_tree, c['name']
        leaves = np.array([g[0] for g in mine['groups']])
        sets, lengths = treecut.branch_sets(*njtree.parse_newick(c['text']), leaves)
        inc = incompatible[np.ix_(leaves, leaves)]
        if c['kind'] == 'dyadic':                               # every entry a multiple of 2^-10, every sum exact in any order
            assert np.array_equal(inc * 1024, np.round(inc * 1024)) and inc.sum() < 2.0 ** 40
        report = {}
        cut = H.cut_restated(H.sides_of(sets, len(leaves)), lengths, inc[:, :, 0], inc[:, :, 1], mat[leaves, 4] >= (c['clust_identity'] - 0.02) * 10000, report=report)
        got = orthofilter.mats_of_cut(mat, mine['groups'], leaves, cut['part'], cut['n_parts'])
        assert [m[:, 6].tolist() for m in got] == c['returned'], c['name']
        assert cut['n_ties'] == 0, c['name']
        if c['kind'] == 'float':
            assert report['ic0_margin'] > 1e-9 and report['gap'] > 1e-9, (c['name'], report)
        n_cut += cut['n_cuts'] > 0
        n_dropped += (cut['part'] < 0).any()
    assert n_cut >= 12 and n_dropped >= 3


def test_edge_cases_reach_the_branches_they_are_meant_to():
    cases, done = H.restated_edge_cases()
    r = {k: v[0] for k, v in done.items()}
    rep = {k: v[1] for k, v in done.items()}
    assert all(r[k]['n_cuts'] >= 1 for k in ('n2', 'n3', 'n4', 'n64', 'n65', 'n256', 'n257', 'n64_float', 'n65_float', 'n256_float', 'n257_float'))
    assert (r['compatible']['n_cuts'], rep['compatible']['scored']) == (0, 0)
    assert (r['no_candidate']['n_cuts'], rep['no_candidate']['scored']) == (0, 1) and (cases['no_candidate']['W0'] > cases['no_candidate']['W1']).any()
    # the branch of the cut is given (also) as the side that holds leaf 0: the part with leaf 0 keeps the place whichever side a branch names
    assert r['swap']['part'].tolist() == [0, 0, 0, 1, 1, 1] and (cases['swap']['sides'] == np.array([1, 1, 1, 0, 0, 0], bool)).all(1).any()
    assert r['dropped']['part'].tolist() == [0] * 5 + [-1] * 3 and r['dropped']['n_parts'] == 1
    assert r['dropped_first']['part'].tolist() == [0] * 3 + [1] * 5                  # leaf 0 is weak, and its part stays all the same: only a detached part is dropped
    assert r['queue']['n_cuts'] == 3 and r['queue']['log_where'][:, 0].tolist() == [0, 0, 1] and r['queue']['n_parts'] == 4      # the appended part is cut again, in queue order
    assert r['queue_cap1']['n_cuts'] == 2 and r['queue_cap1']['log_where'][:, 0].tolist() == [0, 1]
    assert r['queue_cap2']['n_cuts'] == 3 and r['queue_cap0']['n_cuts'] == 0
    assert rep['queue']['merged'] >= 1 and rep['merged']['merged'] >= 1              # two branches induce the winner's restricted bipartition
    assert (r['key_zero']['log_val'][:, 3] == 0).all() and (r['key_zero']['log_val'][:, 0] > 1).all() and r['key_zero']['n_cuts'] == 2
    assert r['ties']['n_ties'] > 0 and r['ties_one_length']['n_ties'] > 0 and r['ties']['part'].tolist() != r['ties_one_length']['part'].tolist()
    assert all(v['n_ties'] == 0 for k, v in r.items() if not k.startswith('ties'))
    # dyadic cases: the three sums are exact, so the plain numpy sums give the same doubles
    c, res = cases['n65'], r['n65']
    T = np.ones(65, bool)
    e = res['log_where'][0, 1]
    F = ~c['sides'][e] if c['sides'][e, 0] else c['sides'][e]
    assert res['log_val'][0, 0] == c['W0'][np.ix_(F, T & ~F)].sum() and res['log_val'][0, 1] == c['W1'][np.ix_(F, T & ~F)].sum()


def check(N, n, leaf_off, mat_off, branch_off, set_off, sets, path=0):
    try:
        N.tree_cut_check(n, leaf_off, mat_off, branch_off, set_off, sets, path)
    except N.PepError as err:
        m = re.match(r'pep_tree_cut_check failed \((-?\d+)\): (.*)$', str(err), flags=re.S)
        return int(m.group(1)), m.group(2)
    return 0, ''


def test_every_refusal_of_the_check(N):
    # a tree of 4 leaves ((0,1),(2,3)) with its five branches, and one of 2 leaves
    four = [0b0001, 0b0010, 0b0011, 0b0100, 0b1000]
    ok = ([4, 2], [0, 4, 6], [0, 16, 20], [0, 5, 7], [0, 5, 7], four + [0b01, 0b10])
    assert check(N, *ok) == (0, '')
    assert check(N, [], [0], [0], [0], [0], []) == (0, '')                                  # an empty batch is legal
    def bad(**kw):
        args = dict(zip(('n', 'leaf_off', 'mat_off', 'branch_off', 'set_off', 'sets'), ok))
        path = kw.pop('path', 0)
        args.update(kw)
        return check(N, *args.values(), path)
    for kw, code, text in ((dict(sets=None), PEP_ERR_ARG, 'null table'),
                           (dict(leaf_off=None), PEP_ERR_ARG, 'null table'),
                           (dict(n=[4, 1]), PEP_ERR_ARG, 'tree 1 has 1 leaves, a tree needs 2'),
                           (dict(n=[4, 8193]), PEP_ERR_LIMIT, 'tree 1 has 8193 leaves, more than 8192'),
                           (dict(leaf_off=[0, 3, 6]), PEP_ERR_ARG, 'the leaves of tree 0 (4 from 0) overlap the next tree\'s or run past the array (leaf_off[1] = 3)'),
                           (dict(mat_off=[0, 16, 19]), PEP_ERR_ARG, 'the matrix entries of tree 1 (4 from 16) overlap the next tree\'s or run past the array (mat_off[2] = 19)'),
                           (dict(set_off=[0, 4, 7]), PEP_ERR_ARG, 'the bit-set words of tree 0 (5 from 0) overlap the next tree\'s or run past the array (set_off[1] = 4)'),
                           (dict(branch_off=[0, 5, 4]), PEP_ERR_ARG, 'the branches of tree 1 (1 from 5) overlap the next tree\'s or run past the array (branch_off[2] = 4)'),
                           (dict(branch_off=[0, 5, 5]), PEP_ERR_ARG, 'tree 1 has 0 branches, a tree of 2 leaves has 1 .. 4'),
                           (dict(sets=[0b10001] + four[1:] + [1, 2]), PEP_ERR_ARG, 'branch 0 of tree 0 is no bipartition of the leaves: it names a leaf beyond 3'),
                           (dict(sets=[0] + four[1:] + [1, 2]), PEP_ERR_ARG, 'branch 0 of tree 0 is no bipartition of the leaves: one side is empty'),
                           (dict(sets=four + [0b11, 0b10]), PEP_ERR_ARG, 'branch 0 of tree 1 is no bipartition of the leaves: one side is empty'),
                           (dict(sets=[0b0001, 0b0010, 0b0011, 0b0100, 0b0110] + [1, 2]), PEP_ERR_ARG, 'the branches of tree 0 are not pairwise compatible: branch 4 crosses another one'),
                           (dict(path=3), PEP_ERR_ARG, 'path 3 is none of PEP_CUT_AUTO, PEP_CUT_BLOCK, PEP_CUT_CHAIN')):
        assert bad(**kw) == (code, 'pep_tree_cut: ' + text), kw
    # the one-workgroup path refuses what is beyond it; the same tree is legal on the other paths
    n = N.NJ_BLOCK_LEAVES + 1
    words = (n + 63) // 64
    stars = np.zeros((n, words), np.uint64)
    stars[np.arange(n), np.arange(n) // 64] = np.uint64(1) << (np.arange(n) % 64).astype(np.uint64)
    big = ([n], [0, n], [0, n * n], [0, n], [0, n * words], stars.reshape(-1))
    assert check(N, *big) == (0, '') and check(N, *big, path=N.CUT_CHAIN) == (0, '')
    assert check(N, *big, path=N.CUT_BLOCK) == (PEP_ERR_LIMIT, 'pep_tree_cut: tree 0 has 257 leaves, the one-workgroup path takes 256')
    assert check(N, [2], [0, 2], [0, 4 + (N.NJ_MAX_BYTES >> 3)], [0, 2], [0, 2], [1, 2])[0] == PEP_ERR_LIMIT
    # compatible branches given as their complements, twice over, and in any order are legal
    assert check(N, [4], [0, 4], [0, 16], [0, 7], [0, 7], [0b1100, 0b0011, 0b1110, 0b0010, 0b1011, 0b0111, 0b1100]) == (0, '')
    with pytest.raises(ValueError):
        N.tree_cut_check([4], [0, 4, 5], [0, 16], [0, 5], [0, 5], four)


def test_null_context_is_an_argument_error(N):
    restype, *argtypes = N.SIGNATURES['pep_tree_cut']
    assert restype is C.c_int and argtypes[0] is C.c_void_p
    assert N.load_library().pep_tree_cut(*[None if t is C.c_void_p else t(0) for t in argtypes]) == PEP_ERR_ARG


def test_treecut_section_of_the_header(N):
    """the K25 section of include/peppan_hip.h declares its two functions in this order, cites what it replaces, and its paths and counts are _native's (the
    prototypes: tests/test_abi.py)"""
    hdr = open(os.path.join(ROOT, 'include', 'peppan_hip.h')).read()
    names = [name for _, name, _ in ABI._header_prototypes()]
    own = ['pep_tree_cut', 'pep_tree_cut_check']
    assert names[names.index(own[0]):][:len(own)] == own == [name for name in N.SIGNATURES if name in own]
    defines = dict(re.findall(r'^#define (PEP_\w+) \(?(-?\w+)\)?$', hdr, flags=re.M))
    for name, want in (('AUTO', N.CUT_AUTO), ('BLOCK', N.CUT_BLOCK), ('CHAIN', N.CUT_CHAIN), ('ROUND', N.CUT_ROUND), ('DEFAULT_CAP', N.CUT_DEFAULT_CAP)):
        assert int(defines['PEP_CUT_' + name]) == want, name
    assert int(re.search(r'#define PEP_ABI_VERSION (\d+)', hdr).group(1)) == N.ABI_VERSION
    assert 'PEPPAN.py:424-482' in hdr


def test_mats_of_cut_expands_leaders_in_queue_order():
    from peppan_amd import orthofilter
    mat = np.arange(9 * 7).reshape(9, 7)
    groups = [[0, 4], [1], [2, 3, 8], [5, 7], [6]]
    leaves = [0, 1, 2, 5, 6]
    whole = orthofilter.mats_of_cut(mat, groups, leaves, [0, 0, 0, 0, 0], 1)
    assert len(whole) == 1 and whole[0] is mat
    got = orthofilter.mats_of_cut(mat, groups, leaves, [0, 2, 1, -1, 0], 3)          # leader 5 and its member 7 are dropped
    assert [m[:, 0].tolist() for m in got] == [[0, 28, 42], [14, 21, 56], [7]]
    # every leader in one component but some dropped: fewer leaves than tags, so the rows are gathered, not the table handed back
    got = orthofilter.mats_of_cut(mat, groups, leaves, [0, 0, 0, -1, 0], 1)
    assert len(got) == 1 and got[0] is not mat and got[0][:, 0].tolist() == [0, 7, 14, 21, 28, 42, 56]


def test_cut_groups_keeps_groups_without_a_tree_whole():
    from peppan_amd import orthofilter
    mats = [np.zeros((3, 7), np.int64), np.ones((2, 7), np.int64)]
    to_run = [(m, False, 30) for m in mats]
    verdicts = [orthofilter.GroupVerdict(0), orthofilter.GroupVerdict(1)]
    out, found = orthofilter.cut_groups(to_run, verdicts, [None, None], dict(clust_identity=0.9), detail=True)     # no tree anywhere: no device is touched
    assert [len(o) for o in out] == [1, 1] and out[0][0] is mats[0] and out[1][0] is mats[1] and found == [None, None]
    with pytest.raises(ValueError):
        orthofilter.cut_groups(to_run, verdicts, [None], dict(clust_identity=0.9))
