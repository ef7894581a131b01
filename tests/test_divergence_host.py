"""K16 (divergence verdicts of gene groups, PEPPAN.py:335-392) without a GPU: the ABI, the host half of the float layer (gd_table,
distances_from_diff, incompatible_of) against expressions evaluated one key / one pair at a time, the g20 fixture against the independent
restatement, the table checks of pep_group_verdicts, which need no device, and the fast reference of the large-group GPU tests (matmul_counts,
leaders_numpy) against the restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from allele_diff_helpers import decode_rows, random_group, square_from_tri  # noqa: E402
from divergence_helpers import (founders_group, fuzz_groups, leaders_numpy, load_g20, matching_leaders, matmul_counts, pack_codes, pair_counts, restate,  # noqa: E402
                                restate_distances, restate_incompatible, tri_from_square, verdict_table)


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


def test_library_exports_group_verdicts_and_the_abi_version(N):
    lib = N.load_library()
    names = ('pep_group_verdicts', 'pep_group_verdicts_check', 'pep_verdict_detail_size', 'pep_verdict_detail_copy', 'pep_verdict_result_free', 'pep_call_times')
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'peppan_hip.h')).read()
    for name in names:
        assert hasattr(lib, name) and name in N.EXPORTS and name + '(' in hdr, name
    assert lib.pep_version() == N.ABI_VERSION          # (K16 itself left it at 17; 18 gained pep_live_resources; 19 one header and pep_call_times; 20 took in K21 - K26)
    assert '#define PEP_ABI_VERSION %d' % N.ABI_VERSION in hdr and 'PEPPAN.py:335-344, 352-366, 371-392' in hdr


def test_gd_table_equals_the_three_expressions_one_key_at_a_time():
    from peppan_amd import orthofilter as OF
    rng = np.random.default_rng(20)
    gd = {}
    for _ in range(400):
        a, b = sorted(int(x) for x in rng.integers(0, 3000, 2))
        gd[(a, b)] = (float(np.exp(rng.normal(-4, 1))), float(rng.uniform(0, 1.5)))
    gd[(7, 7)] = (0.25, 0.)                             # (a same-genome key is never looked up, but it is a legal entry)
    gd[(0, 4000000000)] = (0.5, 0.6)
    obj = np.empty((len(gd), 2), dtype=object)
    for k, (key, val) in enumerate(gd.items()):
        obj[k, 0], obj[k, 1] = key, np.array(val) if k % 2 else val
    for self_id in (0.002, 0.005):
        for sigma in (1, 3, 5, 2.5):
            for source in (gd, obj):
                t = OF.gd_table(source, self_id, sigma)
                assert t.keys.dtype == np.uint64 and t.vals.dtype == np.float64 and t.vals.shape == (len(gd), 3) and t.default.shape == (3,)
                assert np.all(t.keys[1:] > t.keys[:-1]) and t.self_id == self_id
                for key, row in zip(t.keys.tolist(), t.vals):
                    g = gd[(key >> 32, key & 0xFFFFFFFF)]
                    assert row[0] == g[0]
                    assert row[1] == g[0] * np.exp(g[1] * np.sqrt(sigma))
                    assert row[2] == g[0] * np.exp(g[1] * sigma)
                assert t.default.tolist() == [0.5, 0.5 * np.exp(0.6 * np.sqrt(sigma)), 0.5 * np.exp(0.6 * sigma)]
    empty = OF.gd_table({}, 0.002, 3)
    assert len(empty.keys) == 0 and empty.vals.shape == (0, 3)
    assert len(OF.gd_table({(5, 2): (0.1, 0.1), (2, 5): (0.2, 0.2)}, 0.002, 3).keys) == 1          # g1 > g2 can never be looked up
    for bad in (0., -1., float('nan')):
        with pytest.raises(ValueError):
            OF.gd_table(gd, bad, 3)
    with pytest.raises(ValueError):
        OF.gd_table({(1, 2): (0., 0.5)}, 0.002, 3)
    with pytest.raises(ValueError):
        OF.gd_table({(1, 1 << 32): (0.1, 0.5)}, 0.002, 3)


def test_fixture_covers_what_the_feature_is_pinned_by():
    cases = load_g20()
    assert len(cases) >= 60
    kinds = [c['kind'] for c in cases]
    assert min(kinds.count(k) for k in ('calm', 'band', 'compatible', 'tree')) >= 8
    assert {c['self_id'] for c in cases} == {0.002, 0.005} and {c['allowed_sigma'] for c in cases} == {1, 3, 5}
    assert {2, 3, 64, 65, 130} <= {c['n'] for c in cases}
    sub_only = dup_ignored = missing = 0
    for c in cases:
        want = restate(c['packed'], c['ref_len'], c['genomes'], c['inparalog'], c['gd'], c['self_id'], c['allowed_sigma'])
        assert want['divergent'] == c['divergent'] and (want['verdict'] > 0) == c['divergent'], c['name']
        assert c['kind'] == ('calm' if not c['divergent'] else 'band' if want['verdict'] == 1 else 'tree' if c['tree_asked'] else 'compatible'), c['name']
        if c['tree_asked']:
            assert want['verdict'] == 2 and [g[0] for g in want['groups']] == c['leaders'], c['name']
        sub_only += int(c['divergent'] and not want['edge_divergent'])
        dup_ignored += int(len(set(c['genomes'].tolist())) < c['n'] and not c['inparalog'])
        ids = sorted(set(c['genomes'].tolist()))
        missing += int(any((a, b) not in c['gd'] for i, a in enumerate(ids) for b in ids[i + 1:]))
    assert sub_only >= 5 and dup_ignored >= 5 and missing >= 5


def test_distances_and_incompatible_equal_the_restatement_on_fixture_cases():
    from peppan_amd import orthofilter as OF
    done = 0
    for c in load_g20():
        if not c['divergent'] or c['n'] > 65:
            continue
        n = c['n']
        tri, mut_of, aln_of = pair_counts(c['packed'], c['ref_len'])
        want = restate(c['packed'], c['ref_len'], c['genomes'], c['inparalog'], c['gd'], c['self_id'], c['allowed_sigma'], counts=(tri, mut_of, aln_of))
        diff = square_from_tri(n, tri).astype(np.float64)
        for source in (c['gd'], OF.gd_table(c['gd'], c['self_id'], c['allowed_sigma'])):
            gd = source if isinstance(source, OF.GdTable) else OF.gd_table(source, c['self_id'], c['allowed_sigma'])
            distances = OF.distances_from_diff(diff, c['genomes'], gd)
            assert np.array_equal(distances, restate_distances(n, mut_of, aln_of, c['genomes'], c['gd'], c['self_id'], c['allowed_sigma'])), c['name']
        assert bool(np.any(distances[:, :, 0] > distances[:, :, 1])) == (want['verdict'] == 2), c['name']
        if want['verdict'] == 2:
            incompatible, needs_tree = OF.incompatible_of(distances, want['groups'])
            # the sum over a pair of leader groups is numpy's (as in the reference); a plain running sum may differ from it in the last bits
            assert np.allclose(incompatible, restate_incompatible(distances, want['groups']), rtol=1e-12, atol=0), c['name']
            assert needs_tree == c['tree_asked'], c['name']           # ... the decision is the reference's own, recorded in the fixture
            done += 1
    assert done >= 10


def test_table_checks_need_no_device(N):
    from peppan_amd import orthofilter as OF
    rng = np.random.default_rng(7)
    p = random_group(rng, 6, 100)
    packed, row_off, row_len, index = verdict_table([p], [100])
    genomes, gd = [np.arange(6)], OF.gd_table({(0, 5): (0.01, 0.5), (1, 2): (0.02, 0.1)}, 0.002, 3)
    assert N.group_verdicts_check(packed, row_off, row_len, index, genomes, [0], gd, 0.002) is None

    def fails(code, text, *a):
        with pytest.raises(N.PepError, match=r'pep_group_verdicts_check failed \(%d\): pep_group_verdicts: %s' % (code, text)):
            N.group_verdicts_check(*a)

    ones = np.ones((2, 3))
    fails(-2, 'gd_key must be strictly increasing .entry 1.', packed, row_off, row_len, index, genomes, [0], (np.array([9, 8], np.uint64), ones, ones[0]), 0.002)
    fails(-2, 'gd_key must be strictly increasing', packed, row_off, row_len, index, genomes, [0], (np.array([8, 8], np.uint64), ones, ones[0]), 0.002)
    fails(-2, 'gd_key 1 has g1 > g2', packed, row_off, row_len, index, genomes, [0], (np.array([8, (3 << 32) | 2], np.uint64), ones, ones[0]), 0.002)
    for bad in (0., -0.5, np.inf, np.nan):
        for col in range(3):
            vals = ones.copy()
            vals[1, col] = bad
            fails(-2, 'gd_val row 1 must be finite and > 0', packed, row_off, row_len, index, genomes, [0], (np.array([8, 9], np.uint64), vals, ones[0]), 0.002)
            fails(-2, 'gd_default must be finite and > 0', packed, row_off, row_len, index, genomes, [0], (np.array([8, 9], np.uint64), ones, vals[1]), 0.002)
        fails(-2, 'self_id must be finite and > 0', packed, row_off, row_len, index, genomes, [0], gd, bad)
    # K15's table errors
    bad_len = row_len.copy()
    bad_len[2] = 103
    fails(-2, 'row 2 does not hold', packed, row_off, bad_len, index, genomes, [0], gd, 0.002)
    mixed = verdict_table([p, random_group(rng, 3, 40)], [100, 40])
    fails(-2, 'group 0 mixes rows of different row_len', mixed[0], mixed[1], mixed[2], [np.array([0, 1, 7])], [np.arange(3)], [0], gd, 0.002)
    fails(-2, 'row index 6 of group 0 out of range', packed, row_off, row_len, [np.array([0, 6])], [np.arange(2)], [0], gd, 0.002)
    fails(-2, 'grp_inparalog of group 0 is neither 0 nor 1', packed, row_off, row_len, index, genomes, [3], gd, 0.002)
    tiny = verdict_table([np.array([[25]], dtype=np.uint8)], [1])
    big = np.zeros(24000, dtype=np.uint32)
    fails(-3, '2303904024 bytes of triangles asked for, the device budget of one call is 2147483648 .reached at group 1', tiny[0], tiny[1], tiny[2],
          [big[:3], big], [big[:3], big], [0, 0], gd, 0.002)
    with pytest.raises(ValueError):
        N.group_verdicts_check(packed, row_off, row_len, index, [np.arange(5)], [0], gd, 0.002)
    assert N.group_verdicts_check(packed, row_off, row_len, index, genomes, [1], gd, 0.005) is None


def test_leaders_numpy_over_matmul_counts_equals_the_restatement():
    """the reference of the large-group GPU tests is only as good as this: on every fuzz group that reaches verdict 2 and on the constructed
    founder / variant / follower groups at small size, triangle and leaders are the restatement's"""
    rng = np.random.default_rng(16)
    cases = fuzz_groups(1602, 240, 120)
    # the construction of test_leaders_past_256_and_past_the_lds_list, 30 founders instead of 4 200 (every pair known to the table, as its default row says there)
    for variants, between, behind in (([(10, 25)], (), (0, 29)), ([(3, 9), (20, 14)], (5, 22), (0, 7, 29)), ((), (0,), (26,))):
        codes, row_of, joins, triples = founders_group(rng, 30, 200, variants, between, behind)
        n = len(codes)
        cases.append(dict(packed=pack_codes(codes, rng), ref_len=200, genomes=np.arange(n), inparalog=False, self_id=0.002, allowed_sigma=5,
                          gd={(a, b): (0.02, 0.5) for a in range(n) for b in range(a + 1, n)}, built=(row_of, joins, triples)))
    done = several = 0
    for c in cases:
        want = restate(c['packed'], c['ref_len'], c['genomes'], c['inparalog'], c['gd'], c['self_id'], c['allowed_sigma'])
        assert want['verdict'] == 2 or 'built' not in c
        if want['verdict'] != 2:
            continue
        mut, aln = matmul_counts(decode_rows(c['packed'], c['ref_len']))
        assert mut.dtype == np.int32 and np.array_equal(mut, mut.T) and np.array_equal(aln, aln.T)
        assert np.array_equal(tri_from_square(mut, aln), want['tri'])
        lead = leaders_numpy(mut, aln)
        assert lead.dtype == np.uint32 and np.array_equal(lead, want['leader'])
        done += 1
        several += int(len(want['groups']) > 2)
        if 'built' in c:
            row_of, joins, triples = c['built']
            assert np.array_equal(np.flatnonzero(lead == np.arange(len(lead))), row_of)          # founder p is leader number p
            assert all(lead[row] == row_of[k] for row, k in joins) and len(joins) >= 2
            for row, first, second in triples:
                assert matching_leaders(mut, aln, lead, row).tolist() == [row_of[first], row_of[second]]
    assert done >= 50 + 3 and several >= 10, (done, several)
