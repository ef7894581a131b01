"""K15 (pairwise allele differences, PEPPAN.py:296-316) without a GPU: the ABI, the g19 fixture against an independent numpy formulation,
the host packing of the drop-ins and the argument checks that need no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from allele_diff_helpers import load_g19, decode_rows, numpy_tri_edge  # noqa: E402


def test_library_exports_allele_diff_and_the_abi_version():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native as N
    lib = N.load_library()
    assert hasattr(lib, 'pep_allele_diff')
    assert 'pep_allele_diff' in N.EXPORTS
    assert lib.pep_version() == N.ABI_VERSION          # (17 when K15 arrived; 18 gained pep_live_resources; 19 one header and pep_call_times; 20 took in K21 - K26)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'peppan_hip.h')).read()
    assert '#define PEP_ABI_VERSION %d' % N.ABI_VERSION in hdr and 'PEPPAN.py:296-316, 332-333' in hdr


def test_fixture_covers_the_cases_the_feature_is_pinned_by():
    cases = load_g19()
    assert {c['n'] for c in cases} == {1, 2, 3, 17, 64, 65, 130}
    assert {c['ref_len'] for c in cases} == {1, 2, 3, 63, 64, 65, 191, 192, 193, 1000, 1002}
    assert any(c['sub'] for c in cases)
    garbage = all_gap = identical = 0
    for c in cases:
        s = c['packed'].shape[1]
        digits = np.concatenate([c['packed'] // 25, (c['packed'] // 5) % 5, c['packed'] % 5], axis=1)
        garbage += int(digits[:, c['ref_len']:].any()) if 3 * s > c['ref_len'] else 0
        seqs = decode_rows(c['packed'], c['ref_len'])
        if c['n'] >= 3:
            all_gap += int(not seqs[1].any())
            identical += int(np.array_equal(seqs[0], seqs[-1]))
    assert garbage > 10 and all_gap > 10 and identical > 10


def test_fixture_equals_independent_numpy_formulation():
    for c in load_g19():
        seqs = decode_rows(c['packed'], c['ref_len'])
        tri, edge = numpy_tri_edge(seqs)
        assert np.array_equal(tri, c['tri']), c['name']
        assert np.array_equal(edge, c['edge']), c['name']
        if c['sub']:
            tri, edge = numpy_tri_edge(seqs[c['sub']['index']])
            assert np.array_equal(tri, c['sub']['tri']) and np.array_equal(edge, c['sub']['edge']), c['name']
        # the definition itself, cell by cell, for the small ones
        if c['n'] <= 3 and c['ref_len'] <= 65:
            for a in range(c['n']):
                both = (seqs[a] > 0) & (seqs[-1] > 0)
                assert c['edge'][1, a].tolist() == [int((both & (seqs[a] != seqs[-1])).sum()) + 1, int(both.sum()) + 2]


def test_host_packing_round_trips_through_decodeseq():
    from peppan_amd import orthofilter as OF
    from peppan_amd.mapbsn import decodeSeq, encodeSeq
    rng = np.random.default_rng(11)
    for n, L in ((1, 1), (2, 2), (3, 3), (5, 10), (7, 64), (4, 301), (3, 1002)):
        seqs = np.array([0, 65, 67, 71, 84], dtype=np.uint8)[rng.integers(0, 5, (n, L))]
        packed = OF.pack_rows(seqs)
        assert packed.dtype == np.uint8 and packed.shape == (n, -(-L // 3))
        back = np.array([0, 65, 67, 71, 84], dtype=np.uint8)[decodeSeq(packed)]
        assert np.array_equal(back[:, :L], seqs) and not back[:, L:].any()
        codes = np.zeros(256, np.uint8)
        codes[[65, 67, 71, 84]] = (1, 2, 3, 4)
        for r in range(n if L >= 3 else 0):              # (encodeSeq serves genes of one codon and more: K12 accepts no shorter one)
            assert np.array_equal(packed[r], encodeSeq(codes[seqs[r]]))
        assert np.array_equal(decode_rows(packed, L), seqs)


def test_dropins_reject_bad_arguments_without_a_device():
    from peppan_amd import orthofilter as OF
    good = np.array([[65, 0, 84], [67, 71, 0]], dtype=np.uint8)
    diff = np.zeros((2, 2, 2), dtype=np.int64)
    for fn in (OF.compare_seq, OF.compare_seqX):
        bad = good.copy()
        bad[1, 2] = 45                                  # '-': the reference's caller zeroes it (PEPPAN.py:333) before the kernels see it
        with pytest.raises(ValueError, match='45'):
            fn(bad, diff)
        with pytest.raises(ValueError, match='78'):
            fn(np.array([[78]], dtype=np.uint8), np.zeros((1, 1, 2), dtype=np.int64))
        with pytest.raises(TypeError):
            fn(good.astype(np.int64), diff)
        with pytest.raises(ValueError):
            fn(good[0], diff)
        with pytest.raises(TypeError):
            fn(good, diff.astype(np.float64))
        with pytest.raises(TypeError):
            fn(good, diff.astype(np.int32))
        with pytest.raises(ValueError):
            fn(good, np.zeros((3, 3, 2), dtype=np.int64))
        with pytest.raises(ValueError):
            fn(good, np.zeros((2, 2), dtype=np.int64))
    assert not diff.any()
