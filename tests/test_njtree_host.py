"""K21 (neighbour-joining trees, the two rapidnj calls of the reference: PEPPAN.py:19, 409-417 and PEPPAN_parser.py:168) without a GPU: the numpy
restatement of the rules of include/peppan_hip.h (tests/njtree_helpers.py) and njtree.kimura_distances against what rapidnj printed for the committed
fixtures (tests/golden/njtree_pd.json.gz, njtree_fa.json.gz, made by tests/golden/make_golden_njtree.py), the text writer and reader, the device-free table
check of pep_nj_trees, the K21 section of the header against _native's constants, and writeCGAV without rapidnj.

Tolerances.  rapidnj prints five significant digits, so a printed branch length is within half a unit of its fifth digit of what rapidnj computed; it
computes in float32, the restatement in float64.  profiles/njtree_vs_reference.txt (python tests/njtree_helpers.py) records the worst excess over the digit
bound on the committed fixtures, 1.524e-06 for a branch length and 1.631e-07 for a Kimura distance over its printed quantum of 5e-7; four times that
is allowed, because float32 error grows with n and with the order of summation and ten cases only sample it."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import njtree_helpers as H  # noqa: E402
import test_abi as ABI  # noqa: E402
from peppan_amd import njtree as NJ  # noqa: E402  (pure Python: the library is loaded on first use)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRANCH_ALLOWANCE = 4 * 1.524e-06
KIMURA_ALLOWANCE = 4 * 1.631e-07
SIZES = [2, 3, 4, 5, 8, 17, 33, 64, 65, 100]
PEP_ERR_ARG, PEP_ERR_LIMIT = -2, -3


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


@pytest.fixture(scope='module')
def pd_cases():
    cases = H.load_cases('njtree_pd.json.gz')
    assert [c['n'] for c in cases if c['kind'] == 'euclidean'] == SIZES and any(c['kind'] == 'cgav' for c in cases)
    return cases


def test_restatement_has_rapidnj_s_trees_and_distances_on_every_fixture(pd_cases):
    """every case of both fixtures, none left out: the same splits (asserted by njtree_helpers.against_text), every branch length within its printed digit
    + the allowance, every Kimura distance of the restatement's counts within the printed quantum + the allowance"""
    fa = H.load_cases('njtree_fa.json.gz')
    assert [c['n'] for c in fa] == SIZES and all(round(x, 6) == x for c in pd_cases for x in c['upper'])
    for c in fa:
        gaps = (H.codes_of(c) == 0).any(0).mean()
        assert 0.01 <= gaps <= 0.12 or c['n'] < 8, gaps        # (3 - 8 % of 300 columns are drawn; with a few rows not each of them gets a gap)
    report = H.fixture_report(NJ.kimura_distances, NJ.parse_newick)
    assert len(report) == len(pd_cases) + len(fa)
    for name, n, diff, excess, dist_excess in report:
        print('%s n = %d: worst branch difference %.3e, excess over the digit bound %.3e, Kimura excess %r' % (name, n, diff, excess, dist_excess))
        assert excess <= BRANCH_ALLOWANCE, (name, n, excess)
        assert dist_excess is None or dist_excess <= KIMURA_ALLOWANCE, (name, n, dist_excess)


def test_kimura_undefined_pairs_are_marked():
    # rows 0 / 1 share no column; rows 0 / 2 are saturated with transversions (1 - 2 Q <= 0); rows 0 / 3 differ in one transition of four columns
    codes = np.array([[1, 1, 1, 1, 0, 0], [0, 0, 0, 0, 2, 2], [2, 2, 1, 1, 0, 0], [3, 1, 1, 1, 0, 0]])
    counts = H.kimura_counts(codes)
    assert counts[0].tolist() == [0, 0, 0] and counts[1].tolist() == [4, 0, 2] and counts[2].tolist() == [4, 1, 0]
    d, undefined = NJ.kimura_distances(counts[:, 0], counts[:, 1], counts[:, 2])
    assert undefined[0, 1] and undefined[1, 0] and undefined[0, 2] and not undefined[0, 3] and not undefined.diagonal().any()
    assert np.isnan(d[0, 1]) and np.isnan(d[0, 2]) and d[0, 3] == -0.5 * np.log((1 - 2 * 0.25) * np.sqrt(1.0))
    square_counts = NJ.square_of(counts[:, 0])
    assert np.array_equal(NJ.kimura_distances(square_counts, NJ.square_of(counts[:, 1]), NJ.square_of(counts[:, 2]))[1], undefined)


def test_newick_round_trip():
    for n, seed in ((2, 1), (3, 2), (4, 3), (9, 4), (40, 5)):
        m = H.euclidean(n, seed)
        node, length = H.nj_restated(m)
        names = ['t%d' % (7 * k) for k in range(n)]
        text = NJ.newick(NJ.NjTree(node, length, n), names, digits=17)
        assert text.endswith(');') and "'" not in text and text.count('(') == max(n - 2, 1)
        leaves, branches = NJ.parse_newick(text)
        want = [(frozenset(names[k] for k in side), d) for side, d in H.branches_of_record(node, length, n)]
        assert sorted(leaves) == sorted(names)
        assert sorted((sorted(s), d) for s, d in branches) == sorted((sorted(s), d) for s, d in want)          # 17 digits: the lengths come back exactly
        if n > 3:                                             # the trifurcation is outermost, in the arrays' order: its three branches partition the leaves
            outer = [s for s, _ in want[-3:]]
            assert [s for s, _ in branches if s in outer] == outer and sum(len(s) for s in outer) == n and branches[-1][0] == outer[-1]
    with pytest.raises(ValueError):
        NJ.parse_newick('(a:1,b:2)')
    with pytest.raises(ValueError):
        NJ.parse_newick('(a:1,b);')
    with pytest.raises(ValueError):
        NJ.newick(NJ.NjTree(node, length, n), names[:-1])


def test_texts_of_two_and_three_leaves_are_rapidnj_s_characters():
    """what rapidnj printed for these inputs (read off its output, quotes stripped): short decimals, so float32 and float64 print the same digits"""
    for upper, names, want in (([0.3], ['A', 'B'], '(A:0.3,B:0.3);'),
                               ([0.3, 0.5, 0.6], ['A', 'B', 'C'], '(B:0.2,A:0.1,C:0.4);'),
                               ([0.9, 0.5, 0.6], ['A', 'B', 'C'], '(B:0.5,A:0.4,C:0.1);'),
                               ([0.25, 0.75, 1], ['A', 'B', 'C'], '(B:0.25,A:0,C:0.75);')):
        n = len(names)
        node, length = H.nj_restated(H.square(upper, n))
        assert NJ.newick(NJ.NjTree(node, length, n), names) == want


def test_fixture_texts_of_two_and_three_leaves(pd_cases):
    """... and the committed fixtures of 2 and 3 leaves, whose inputs have six decimals: the same leaf order, every length within its printed digit"""
    for c in pd_cases[:2]:
        node, length = H.nj_restated(H.square(c['upper'], c['n']))
        mine = NJ.newick(NJ.NjTree(node, length, c['n']), c['names'])
        theirs = c['newick'].replace("'", '').strip()
        assert re.sub(r':[^,)]+', '', mine) == re.sub(r':[^,)]+', '', theirs)


def check(N, n_leaves, dist_off, out_off):
    msg = C.create_string_buffer(512)
    n = np.array(n_leaves, np.uint32)
    d, o = np.array(dist_off, np.uint64), np.array(out_off, np.uint64)
    rc = N.load_library().pep_nj_trees_check(N._ptr(n), len(n), N._ptr(d), N._ptr(o), msg, len(msg))
    return rc, msg.value.decode()


def test_every_refusal_of_the_table_check(N):
    assert check(N, [2, 3, 5], [0, 4, 13, 38], [0, 2, 5, 12]) == (0, '')
    assert check(N, [2, 3, 5], [7, 11, 30, 55], [1, 4, 9, 16]) == (0, '')           # gaps and a start behind 0 are legal
    assert N.load_library().pep_nj_trees_check(None, 0, None, None, None, 0) == 0    # an empty batch needs no table
    rc, msg = check(N, [2, 1], [0, 4, 5], [0, 2, 3])
    assert rc == PEP_ERR_ARG and 'tree 1 has 1 leaves' in msg
    rc, msg = check(N, [0], [0, 0], [0, 0])
    assert rc == PEP_ERR_ARG and 'tree 0 has 0 leaves' in msg
    rc, msg = check(N, [3, 3], [0, 8, 17], [0, 3, 6])
    assert rc == PEP_ERR_ARG and 'matrix of tree 0' in msg and 'overlaps' in msg
    rc, msg = check(N, [3, 3], [0, 9, 17], [0, 3, 6])
    assert rc == PEP_ERR_ARG and 'matrix of tree 1' in msg and 'runs past' in msg
    rc, msg = check(N, [3, 3], [9, 0, 9], [0, 3, 6])
    assert rc == PEP_ERR_ARG and 'matrix of tree 0' in msg
    rc, msg = check(N, [3, 4], [0, 9, 25], [0, 2, 7])
    assert rc == PEP_ERR_ARG and 'output of tree 0' in msg
    rc, msg = check(N, [3, 4], [0, 9, 25], [0, 3, 7])
    assert rc == PEP_ERR_ARG and 'output of tree 1' in msg and '5 entries' in msg
    rc, msg = check(N, [2], [0, 4], [0, 1])
    assert rc == PEP_ERR_ARG and '2 entries' in msg
    big = N.NJ_MAX_LEAVES + 1
    rc, msg = check(N, [big], [0, big * big], [0, 2 * big - 3])
    assert rc == PEP_ERR_LIMIT and '%d leaves' % big in msg
    n, count = 4096, N.NJ_MAX_BYTES // 8 // 4096 ** 2 + 1
    rc, msg = check(N, [n] * count, [k * n * n for k in range(count + 1)], [k * (2 * n - 3) for k in range(count + 1)])
    assert rc == PEP_ERR_LIMIT and '%d distances' % (count * n * n) in msg and str(N.NJ_MAX_BYTES) in msg
    with pytest.raises(N.PepError, match='tree 0 has 1 leaves'):
        N.nj_trees_check([1], [0, 1], [0, 0])
    with pytest.raises(ValueError):
        N.nj_trees_check([2], [0], [0, 2])
    with pytest.raises(C.ArgumentError):
        N.load_library().pep_nj_trees_check(None, 1.5, None, None, None, 0)


def test_null_handles_are_argument_errors(N):
    lib = N.load_library()
    for name in ('pep_kimura_pairs', 'pep_nj_trees'):
        restype, *argtypes = N.SIGNATURES[name]
        assert restype is C.c_int and argtypes[0] is C.c_void_p
        assert getattr(lib, name)(*[None if t is C.c_void_p else t(0) for t in argtypes]) == PEP_ERR_ARG, name
        assert getattr(lib, name)(*[None if t is C.c_void_p else t(3) for t in argtypes]) == PEP_ERR_ARG, name


def test_njtree_section_of_the_header(N):
    """the K21 section of include/peppan_hip.h declares its three functions in this order, cites what it replaces, and its limits are _native's (the prototypes:
    tests/test_abi.py)"""
    hdr = open(os.path.join(ROOT, 'include', 'peppan_hip.h')).read()
    names = [name for _, name, _ in ABI._header_prototypes()]
    own = ['pep_kimura_pairs', 'pep_nj_trees', 'pep_nj_trees_check']
    assert names[names.index(own[0]):][:len(own)] == own == [name for name in N.SIGNATURES if name in own]
    for define, value in (('PEP_NJ_BLOCK_LEAVES', N.NJ_BLOCK_LEAVES), ('PEP_NJ_MAX_LEAVES', N.NJ_MAX_LEAVES)):
        assert int(re.search(r'#define %s (\d+)\b' % define, hdr).group(1)) == value
    assert re.search(r'#define PEP_NJ_MAX_BYTES \(1ull << (\d+)\)', hdr).group(1) == str(N.NJ_MAX_BYTES.bit_length() - 1)
    assert int(re.search(r'#define PEP_ABI_VERSION (\d+)', hdr).group(1)) == N.ABI_VERSION
    for ref in ('PEPPAN.py:19, 409-417', 'PEPPAN_parser.py:168'):
        assert ref in hdr


def test_writecgav_without_rapidnj_writes_the_tree(monkeypatch, tmp_path):
    from peppan_amd import panparser as PP
    rng = np.random.default_rng(11)
    genomes = ['genome_%02d' % k for k in range(9)]
    ortho = {g: {'gene%d' % j: {'%s_%d' % (g, j): int(rng.integers(1, 4))} for j in range(30)} for g in genomes}
    distances = H.cgav_like(len(genomes), 12)
    log = []
    monkeypatch.setattr(PP.shutil, 'which', lambda name: None)
    monkeypatch.setattr(PP, 'getDistance', lambda profiles, device=None: distances)
    monkeypatch.setattr(PP.njtree, 'nj_trees', lambda mats, device=None: [NJ.NjTree(*H.nj_restated(m), len(m)) for m in mats])
    monkeypatch.setattr(PP, 'logger', log.append)
    prefix = str(tmp_path / 'out')
    PP.writeCGAV(prefix, ortho, 95)
    text = open(prefix + '_CGAV.nwk').read()
    assert text.endswith(';\n') and "'" not in text
    leaves, branches = NJ.parse_newick(text)
    assert sorted(leaves) == genomes and len(branches) == 2 * len(genomes) - 3
    assert H.bipartitions(branches, genomes) == H.bipartitions(H.named_branches(distances, genomes), genomes)
    assert log[-1] == 'Core gene allelic variation tree is saved in %s_CGAV.nwk' % prefix and not any('skipped' in line for line in log)
    assert os.path.exists(prefix + '_CGAV.profile') and os.path.exists(prefix + '_CGAV.dist')


# ---- the tie and overflow matrices of tests/test_gpu_njtree_edges.py reach the branches they are for: proved from the restatement's trace alone

def tie_rounds(trace):
    """(rounds in which two usable pairs or more attain the smallest Q; of those, rounds in which they lie in rows of two wavefronts - a wavefront of
    nj_scan_rows has the list rows of one i % 4 -; rounds in which they lie in rows of two workgroups of nj_chain_argmin)"""
    tied = sum(1 for r in trace if r[3] >= 2)
    waves = sum(1 for r in trace if len({i % 4 for i in r[4]}) >= 2)
    groups = sum(1 for r in trace if len({(i // 4) % H.chain_parts(r[0]) for i in r[4]}) >= 2)
    return tied, waves, groups


TIE_CASES = [(kind, n) for kind, sizes in (('tied', H.TIED_SIZES), ('clades', H.TIED_SIZES), ('constant', H.CONSTANT_SIZES), ('cgav12', H.CGAV12_SIZES))
             for n in sizes]


@pytest.mark.parametrize('kind,n', TIE_CASES)
def test_tie_matrices_tie_across_wavefronts_and_workgroups(kind, n):
    """Every tie matrix: finite lengths, a tied round, above 64 leaves a round whose tied minima lie in rows of two wavefronts, at chain sizes one whose
    tied minima lie in rows of two workgroups.  The ultrametric and the constant matrices tie in a quarter of their rounds at least (measured: all but
    five).  Independent draws of 0..2 (H.tied) and the 12-gene profiles do not, whatever the seed or the number of levels above one - the updates halve
    the integers and the ties are gone after a few joins: 2 - 7 tied rounds of 29 - 298 for H.tied, 14 of 97 and 54 of 298 for the profiles - so of
    them only what they do have is asserted, and the quarter is carried by H.tied_clades at the same sizes."""
    matrix, node, length, trace = H.edge_case(kind, n)
    assert len(trace) == n - 3 and np.isfinite(length).all() and len(node) == 2 * n - 3
    assert all(r[3] >= 1 and not r[5] and not r[6] and r[1] in r[4] for r in trace)
    tied, waves, groups = tie_rounds(trace)
    print('%s %d: %d rounds, %d tied, %d over two wavefronts, %d over two workgroups' % (kind, n, len(trace), tied, waves, groups))
    assert tied >= 1
    if kind in ('clades', 'constant'):
        assert 4 * tied >= len(trace)
    if n > 64:
        assert waves >= 1
    if n > 256:
        assert groups >= 1


def test_trace_changes_nothing():
    for kind, n in (('tied', 33), ('clades', 66), ('all_nan', 6), ('huge_row', 6)):
        matrix, node, length, trace = H.edge_case(kind, n)
        again_node, again_length = H.nj_restated(matrix)
        assert np.array_equal(node, again_node) and np.array_equal(length.view(np.uint64), again_length.view(np.uint64))
        assert [r[0] for r in trace] == list(range(n, 3, -1)) and all(0 <= r[1] < r[2] < r[0] for r in trace)
    assert (H.tied(9, 4) == H.tied(9, 4).T).all() and set(np.unique(H.tied(40, 4))) == {0., 1., 2.} and not H.tied(9, 4).diagonal().any()
    assert (H.tied_clades(9, 4) == H.tied_clades(9, 4).T).all() and set(np.unique(H.tied_clades(40, 4))) == {0., 1., 2.}
    assert np.array_equal(H.constant(3, 0.25), [[0, .25, .25], [.25, 0, .25], [.25, .25, 0]])
    d, e = H.planted(9, 4, 2, 5), H.euclidean(9, 4)
    assert d[2, 5] == d[5, 2] == 1e-9 and (d != e).sum() == 2


def test_the_1030_leaf_matrices_reach_the_second_trip_of_the_chain():
    """256 workgroups of four wavefronts have list rows 0 .. 1023 on their first trip; row 1026 is the second trip of workgroup 0's wavefront 2"""
    n = 1030
    assert H.chain_parts(n) == 256 and H.chain_parts(1025) == 256 and H.chain_parts(1024) == 256 and H.chain_parts(1021) == 255
    matrix, node, length, trace = H.edge_case('planted', n)
    assert trace[0][:4] == (n, 1026, 1028, 1) and node[:2].tolist() == [1026, 1028] and np.isfinite(length).all()
    assert 1026 >= 4 * H.chain_parts(n)
    for kind in ('tied', 'clades'):
        matrix, node, length, trace = H.edge_case(kind, n)
        tied, waves, groups = tie_rounds(trace)
        both_trips = sum(1 for r in trace if r[3] >= 2 and max(r[4]) >= 4 * H.chain_parts(r[0]) > min(r[4]))
        print('%s %d: %d rounds, %d tied, %d over two wavefronts, %d over two workgroups, %d over both trips' % (kind, n, len(trace), tied, waves, groups, both_trips))
        assert np.isfinite(length).all() and tied >= 1 and waves >= 1 and groups >= 1
        if kind == 'clades':                                  # ... and tied minima in rows of a wavefront's first and second trip
            assert 4 * tied >= len(trace) and both_trips >= 1


def test_overflow_matrices_take_the_fallback_and_meet_nan():
    for n in H.ALL_NAN_SIZES:
        matrix, node, length, trace = H.edge_case('all_nan', n)
        assert len(trace) == n - 3 and all(r[6] and r[5] and r[1:5] == (0, 1, 0, set()) for r in trace)
    assert H.edge_case('all_nan', 6)[1].tolist() == [0, 1, 6, 2, 7, 3, 8, 4, 5]
    for n in H.HUGE_ROW_SIZES:
        matrix, node, length, trace = H.edge_case('huge_row', n)
        assert np.isfinite(matrix).all() and matrix[0, 1] == 1.5e308
        met = [r for r in trace if r[5] and not r[6]]              # a NaN among the Q, and a usable winner: finite or -infinity by the definition of usable
        assert len(met) >= 1 and all(r[3] >= 1 and r[1] in r[4] for r in met)
        assert trace[0][1:3] == (1, 2) and np.isnan(length).any() and not np.isnan(length).all()
