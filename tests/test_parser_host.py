"""K20 (the counting loops of PEPPAN_parser: writeCurve, PEPPAN_parser.py:63-115, and getDistance, :172-179) without a GPU: the g25 fixture recorded from
the reference's own functions against the independent restatement in plain loops (tests/parser_helpers.py), its section of
include/peppan_hip.h against _native's limits, the table checks of the two entry points, which need no device, and the host half of
peppan_amd.panparser - GFF reading, genome orders from a seed, bit packing, recoding, and the three text writers fed with the recorded counts."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from peppan_amd import panparser as PP  # noqa: E402  (pure Python: the library is loaded on first use)
from parser_helpers import groups_of_case, load_g25, presence_of_groups, restate_curves, restate_pairs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


@pytest.fixture(scope='module')
def g25():
    return load_g25()


def test_restatement_equals_every_recorded_case(g25):
    assert len(g25['cases']) >= 5 and len(g25['pairs']) >= 4
    for c in g25['cases']:
        assert restate_curves(presence_of_groups(groups_of_case(c)), c['orders']) == c['curves'], c['name']
        shared, presence = restate_pairs(c['cgav']['profiles'])
        assert [[v.hex() for v in row] for row in PP.distances_of(np.array(shared).reshape(len(shared), -1), np.array(presence).reshape(len(shared), -1)).tolist()] == \
            c['cgav']['dist_hex'], c['name']
    for p in g25['pairs']:
        assert restate_pairs(p['profiles']) == (p['shared'], p['presence']), p['name']
        assert [[v.hex() for v in row] for row in PP.distances_of(np.array(p['shared']), np.array(p['presence'])).tolist()] == p['dist_hex'], p['name']
    assert {c['n_iter'] for c in g25['cases']} >= {37, 50, 129, 130, 1000}
    assert any(not c['cgav']['profiles'][0] for c in g25['cases']) and any(len(c['cgav']['profiles'][0]) > 10 for c in g25['cases'])


def test_orders_are_reproduced_from_the_seed(g25):
    for c in g25['cases']:
        np.random.seed(c['seed'])
        orders = PP.shuffled_orders(len(c['groups']), c['n_iter'])
        assert orders.dtype == np.uint32 and orders.tolist() == c['orders'], c['name']


def test_getortho_reads_the_gff_as_the_reference_does(g25, tmp_path):
    cases = [c for c in g25['cases'] if 'gff' in c]
    assert {c['no_pseudogene'] for c in cases} == {True, False}
    for k, c in enumerate(cases):
        path = tmp_path / ('in%d.gff' % k)
        path.write_text(c['gff'])
        got = PP.getOrtho(str(path), c['no_pseudogene'])
        want = groups_of_case(c)
        assert got == want and list(got) == list(want), c['name']
        assert [list(v) for v in got.values()] == [list(v) for v in want.values()]          # the groups in the order they were met: genes are numbered by it
        assert PP.presence_matrix(got).astype(int).tolist() == presence_of_groups(want)
    import gzip
    with gzip.open(str(tmp_path / 'in.gff.gz'), 'wt') as f:
        f.write(cases[0]['gff'])
    assert PP.getOrtho(str(tmp_path / 'in.gff.gz'), cases[0]['no_pseudogene']) == groups_of_case(cases[0])


def _split_fit_lines(text):
    lines = text.splitlines(True)
    return [ln for k, ln in enumerate(lines) if k not in (4, 5, 6)], lines[4:7]


def test_curve_text_from_the_recorded_curves_is_the_recorded_file(g25):
    import scipy
    same_scipy = scipy.__version__ == g25['scipy']
    import warnings
    for c in g25['cases']:
        groups = groups_of_case(c)
        presence = PP.presence_matrix(groups)
        mean_size = np.mean(presence.sum(1))
        assert float(mean_size).hex() == c['mean_size']
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                                  # (scipy: the covariance of a fit through a handful of points)
            text = PP.curve_text(np.array(c['curves']), len(groups), mean_size, presence.shape[1], c['pseudogene'])
        rest, fits = _split_fit_lines(text)
        want_rest, want_fits = _split_fit_lines(c['curve_text'])
        assert rest == want_rest, c['name']
        assert len(fits) == 3 and [ln.split('\t')[0] for ln in fits] == [ln.split('\t')[0] for ln in want_fits]
        if same_scipy:
            assert fits == want_fits, c['name']
    if not same_scipy:
        pytest.skip('scipy %s is installed, the fixture was recorded with %s: the three curve_fit lines (Heaps\' law, power law, core genome) of each file were '
                    'compared by their labels only; every other line was compared exactly' % (scipy.__version__, g25['scipy']))


def test_cgav_texts_from_the_recorded_counts_are_the_recorded_files(g25):
    for c in g25['cases']:
        genomes, genes, profiles = PP.cgav_profiles(groups_of_case(c), c['cgav']['pCore'])
        assert profiles == c['cgav']['profiles'], c['name']
        assert PP.profile_text(genomes, genes, profiles) == c['cgav']['profile_text'], c['name']
        shared, presence = restate_pairs(profiles)
        n = len(profiles)
        dist = PP.distances_of(np.array(shared).reshape(n, n), np.array(presence).reshape(n, n))
        assert PP.dist_text(genomes, dist) == c['cgav']['dist_text'], c['name']


def test_pack_presence_sets_one_bit_per_gene_and_no_padding(N):
    rng = np.random.default_rng(2520)
    for n_genes in (1, 63, 64, 65, 127, 128, 129, 300):
        P = rng.random((5, n_genes)) < 0.5
        P[0], P[1] = True, False
        bits = N.pack_presence(P)
        assert bits.dtype == np.uint64 and bits.shape == (5, (n_genes + 63) // 64)
        for g in range(5):
            for e in range(bits.shape[1] * 64):
                assert (int(bits[g, e // 64]) >> (e % 64)) & 1 == (int(P[g, e]) if e < n_genes else 0)
    assert N.pack_presence(np.zeros((3, 0), bool)).shape == (3, 0)
    with pytest.raises(ValueError):
        N.pack_presence(np.zeros(5, bool))


def test_profiles_outside_int32_are_recoded_injectively(g25):
    big = np.array(next(p for p in g25['pairs'] if p['name'] == 'beyond_int32')['profiles'])
    assert big.dtype == np.int64 and big.max() >= 2 ** 40 and big.min() < -2 ** 31
    code = PP._as_int32(big)
    assert code.dtype == np.int32 and np.array_equal(code > 0, big > 0)
    for a in np.unique(big):
        assert len(np.unique(code[big == a])) == 1
    assert len(np.unique(code)) == len(np.unique(big))
    assert restate_pairs(code.tolist()) == restate_pairs(big.tolist())
    small = np.array([[3, 0, -7], [2 ** 31 - 1, -2 ** 31, 1]])
    assert PP._as_int32(small).tolist() == small.tolist() and PP._as_int32(small).dtype == np.int32     # what fits is passed unchanged
    assert PP._as_int32(np.array([[True, False]])).tolist() == [[1, 0]]
    # no pair, no gene: counted on the host, no device is asked for
    for empty in (np.zeros((0, 5), int), np.zeros((4, 0), int), np.array([])):
        shared, presence = PP.pair_counts(empty)
        assert shared.shape == presence.shape == (len(empty), len(empty)) and not shared.any()
    assert PP.getDistance(np.zeros((3, 0))).tolist() == [[0., -np.log(0.5), -np.log(0.5)], [-np.log(0.5), 0., -np.log(0.5)], [-np.log(0.5), -np.log(0.5), 0.]]


def test_parser_section_of_the_header(N):
    """the K20 section of include/peppan_hip.h cites what it replaces, and its limits are _native's (the prototypes: tests/test_abi.py)"""
    hdr = open(os.path.join(ROOT, 'include', 'peppan_hip.h')).read()
    assert 'PEPPAN_parser.py:74-80' in hdr and 'PEPPAN_parser.py:172-179' in hdr
    assert int(re.search(r'#define PEP_PARSER_MAX_GENES \(1ull << (\d+)\)', hdr).group(1)) == N.PARSER_MAX_GENES.bit_length() - 1 == 31
    assert int(re.search(r'#define PEP_PARSER_MAX_CURVE_POINTS \(1ull << (\d+)\)', hdr).group(1)) == N.PARSER_MAX_CURVE_POINTS.bit_length() - 1 == 28
    assert int(re.search(r'#define PEP_PARSER_MAX_PROFILES (\d+)\b', hdr).group(1)) == N.PARSER_MAX_PROFILES == 16384


def _refused(call, N, code, text):
    with pytest.raises(N.PepError) as e:
        call()
    assert '(%d)' % code in str(e.value) and text in str(e.value), str(e.value)


def test_curve_check_refuses_each_bad_input_with_its_code(N):
    ARG, LIMIT = -2, -3
    P = np.ones((4, 70), bool)
    bits = N.pack_presence(P)
    good = np.array([[0, 1, 2, 3], [3, 1, 0, 2], [2, 3, 1, 0]])
    N.rarefaction_curves_check(bits, 70, good)
    N.rarefaction_curves_check(N.pack_presence(np.ones((1, 1), bool)), 1, [[0]])                       # the smallest legal call
    N.rarefaction_curves_check(N.pack_presence(np.ones((4, 128), bool)), 128, good)                    # no padding at all
    _refused(lambda: N.rarefaction_curves_check(bits, 70, [[0, 1, 2, 3], [3, 1, 1, 2]]), N, ARG, 'entry 2 of order 1 names genome 1 again')
    _refused(lambda: N.rarefaction_curves_check(bits, 70, [[0, 1, 2, 4]]), N, ARG, 'entry 3 of order 0 names genome 4 of 4')
    _refused(lambda: N.rarefaction_curves_check(bits, 70, [[0, 1, 2, 2 ** 32 - 1]]), N, ARG, 'names genome 4294967295 of 4')
    for bit in (6, 63):                                                                                # genes 70 and 127 of the row do not exist
        spoiled = bits.copy()
        spoiled[2, 1] |= np.uint64(1 << bit)
        _refused(lambda: N.rarefaction_curves_check(spoiled, 70, good), N, ARG, 'genome 2 has a padding bit set')
    _refused(lambda: N.rarefaction_curves_check(np.zeros((4, 0), np.uint64), 0, good), N, ARG, 'must be positive')
    _refused(lambda: N.rarefaction_curves_check(np.zeros((0, 2), np.uint64), 70, np.zeros((3, 0), np.uint32)), N, ARG, 'must be positive')
    _refused(lambda: N.rarefaction_curves_check(bits, 70, np.zeros((0, 4), np.uint32)), N, ARG, 'must be positive')
    # the limits: read from the sizes before any table is looked at, so small tables do
    lib = N.load_library()
    msg = C.create_string_buffer(256)
    one = np.zeros(1, np.uint64)
    assert lib.pep_rarefaction_curves_check(N._ptr(one), 1, 2 ** 31, N._ptr(one), 1, msg, len(msg)) == LIMIT and b'2^31 genes' in msg.value
    assert lib.pep_rarefaction_curves_check(N._ptr(one), 2 ** 14, 1, N._ptr(one), 2 ** 14, msg, len(msg)) == LIMIT and b'n_genomes * n_iter' in msg.value
    assert lib.pep_rarefaction_curves_check(None, 1, 1, N._ptr(one), 1, msg, len(msg)) == ARG and b'null table' in msg.value
    # shapes and values that never reach the library, where they would be cut
    for call in (lambda: N.rarefaction_curves_check(bits, 64, good), lambda: N.rarefaction_curves_check(bits, 129, good),
                 lambda: N.rarefaction_curves_check(bits, 70, [[0, 1, 2]]), lambda: N.rarefaction_curves_check(bits, 70, [[0, 1, 2, -1]]),
                 lambda: N.rarefaction_curves_check(bits, 70, [[0, 1, 2, 2 ** 32]]), lambda: N.rarefaction_curves_check(bits, 70, [[0., 1., 2., 3.]]),
                 lambda: N.rarefaction_curves_check(bits.astype(np.int64), 70, good), lambda: N.rarefaction_curves_check(bits[0], 70, good)):
        with pytest.raises(ValueError):
            call()


def test_pair_check_refuses_each_bad_size_with_its_code(N):
    ARG, LIMIT = -2, -3
    N.profile_pairs_check(1, 1)
    N.profile_pairs_check(16384, 2 ** 31 - 1)
    _refused(lambda: N.profile_pairs_check(0, 5), N, ARG, 'must be positive')
    _refused(lambda: N.profile_pairs_check(5, 0), N, ARG, 'must be positive')
    _refused(lambda: N.profile_pairs_check(16385, 5), N, LIMIT, 'more than 16384 profiles')
    _refused(lambda: N.profile_pairs_check(5, 2 ** 31), N, LIMIT, '2^31 genes or more')
    with pytest.raises(ValueError):
        N.profile_pairs_check(-1, 5)
    with pytest.raises(ValueError):
        N.profile_pairs_check(2 ** 32, 5)
