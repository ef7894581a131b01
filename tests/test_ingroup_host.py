"""K17 (in-group rows and gene scores of `initializing`, PEPPAN.py:1041-1056, 1058-1076) without a GPU: the ABI, the g21 fixture recorded from
the reference's own determineGroup / initializing2 against the independent restatement in plain loops (tests/ingroup_helpers.py), and the table
checks of pep_gene_ingroups, which need no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from peppan_amd import ingroups as IG  # noqa: E402  (pure Python: the library is loaded on first use)
from ingroup_helpers import EDGE_GD, EDGE_PARAMS, SIZES, edge_variants, load_g21, restate, restate_gene, sort_keys, threshold  # noqa: E402


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


def test_library_exports_gene_ingroups_and_abi_is_unchanged(N):
    lib = N.load_library()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'peppan_hip.h')).read()
    for name in ('pep_gene_ingroups', 'pep_gene_ingroups_check', 'pep_call_times'):
        assert hasattr(lib, name) and name in N.EXPORTS and name + '(' in hdr, name
    assert lib.pep_version() == N.ABI_VERSION
    assert 'PEPPAN.py:1041-1056, 1058-1076' in hdr


def test_restatement_equals_every_determine_group_case_of_the_fixture():
    data = load_g21()
    cases = data['determine']
    assert len(cases) >= 95
    tally = dict(left_out=0, brought_in=0, up=0, down=0, same_genome=0, default=0)
    at_threshold = 0
    for c in cases:
        mine = restate(c['genome'], c['iden'], c['gd'], c['min_iden'], c['nSigma'], c['self_id'])
        assert mine['keep'] == [bool(v) for v in c['ingroup']], c['name']
        for key in tally:
            tally[key] += int(mine[key])
        if c['min_iden'] == 0.9 and {8799, 8800, 8801} <= set(c['iden']):
            at_threshold += 1
            # (0.9 - 0.02) * 10000 is 8800.0 exactly: 8800 is a seed, 8799 is not
            seeds = {v: mine['raw'][j] for j, v in enumerate(c['iden']) if v in (8800, 8801)}
            assert threshold(0.9) == 8800.0 and all(seeds.values())
    assert tally['left_out'] * 4 >= len(cases) and tally['brought_in'] * 4 >= len(cases), tally
    assert min(tally[k] for k in ('up', 'down', 'same_genome', 'default')) >= 10 and at_threshold >= 3, (tally, at_threshold)
    assert {(c['min_iden'], c['nSigma'], c['self_id']) for c in cases} >= {(0.9, 3., 0.005), (0.95, 2., 0.002), (0.8, 1., 0.01)}


def test_restatement_equals_every_initializing2_case_of_the_fixture():
    init = load_g21()['initializing']
    assert len(init['tables']) >= 40 and len(init['runs']) == 2
    ties = cut = 0
    for run in init['runs']:
        for gene, rec in run['genes'].items():
            table = init['tables'][gene]
            if rec['tie']:
                ties += 1
                assert len(set(sort_keys(table))) == len(table) - 1
                continue
            rows, score = restate_gene(table, init['gd'], run['clust_identity'], run['allowed_sigma'], run['self_id'])
            assert rows == rec['kept'] and score == rec['score'], gene
            cut += int(len(rows) < len(table))
    assert 2 <= ties <= 10 and cut >= 16
    one_row = [g for g, t in init['tables'].items() if len(t) == 1]
    assert one_row and all(run['genes'][g]['kept'] == init['tables'][g] and run['genes'][g]['score'] == init['tables'][g][0][2] for g in one_row for run in init['runs'])


def test_edge_variants_are_what_they_are_built_for():
    rng = np.random.default_rng(17)
    for n in SIZES:
        for name, genome, iden in edge_variants(n, rng):
            r = restate(genome, iden, EDGE_GD, **EDGE_PARAMS)
            if name == 'all-seeds':
                assert all(r['keep']) and not r['brought_in']
            elif name == 'no-seeds':
                assert not any(r['keep'])
            elif name == 'row0-to-last':
                assert r['raw'][n - 1] and iden[n - 1] < 8800 and sum(1 for v in iden[:n - 1] if v == 9000) == 1 and iden[0] == 9000
            elif name == 'seed-behind':
                assert sum(r['raw']) == n - 1 and not r['keep'][int(np.flatnonzero(genome == 2)[0])]
            elif name == 'panel-before':
                i = int(np.flatnonzero(iden == 9000)[0])
                assert r['raw'][n - 1] and (n <= 256 or (i // 256 == (n - 1) // 256 - 1 and i % 256 == 255))
            elif name == 'first-out-later-in':
                assert r['up'] and r['raw'][n - 1] and not r['keep'][n - 1] and not r['keep'][0]
            elif name == 'first-in-later-out':
                assert r['down'] and not r['raw'][n - 1] and r['keep'][n - 1]
            else:
                raise AssertionError(name)


def test_table_checks_need_no_device(N):
    gd = (np.array([(1 << 32) | 2, (1 << 32) | 5], np.uint64), np.ones((2, 3)), np.ones(3))
    genome, iden, score = np.array([1, 2, 1, 5]), np.array([10000, 9000, 8000, 7000]), np.array([5, -6, 7, 8])
    ok = lambda *a: N.gene_ingroups_check(*a) is None  # noqa: E731
    assert ok(genome, iden, score, [0, 4], gd, 0.005, 8800.)
    # the legal corners: an empty batch, an empty gene, a gene of one row, an empty table of pairs
    none = np.zeros(0, np.int64)
    assert ok(none, none, none, [0], gd, 0.005, 8800.)
    assert ok(none, none, none, [0, 0, 0], gd, 0.005, 8800.)
    assert ok(genome, iden, score, [0, 0, 1, 1, 4, 4], gd, 0.005, 8800.)
    assert ok(genome, iden, score, [0, 4], (np.zeros(0, np.uint64), np.zeros((0, 3)), np.ones(3)), 0.005, -3.5)

    def fails(code, text, *a):
        with pytest.raises(N.PepError, match=r'pep_gene_ingroups_check failed \(%d\): pep_gene_ingroups: %s' % (code, text)):
            N.gene_ingroups_check(*a)

    fails(-2, 'gene_off must start at 0', genome, iden, score, [1, 4], gd, 0.005, 8800.)
    fails(-2, 'gene_off must be non-decreasing .gene 1.', genome, iden, score, [0, 3, 2, 4], gd, 0.005, 8800.)
    fails(-2, 'gene_off must end at n_rows', genome, iden, score, [0, 3], gd, 0.005, 8800.)
    fails(-2, 'gene_off of gene 0 runs past n_rows', genome, iden, score, [0, 5], gd, 0.005, 8800.)
    fails(-2, 'iden of row 2 is negative', genome, np.array([1, 2, -1, 4]), score, [0, 4], gd, 0.005, 8800.)
    ones = np.ones((2, 3))
    fails(-2, 'gd_key must be strictly increasing .entry 1.', genome, iden, score, [0, 4], (np.array([9, 8], np.uint64), ones, ones[0]), 0.005, 8800.)
    fails(-2, 'gd_key 1 has g1 > g2', genome, iden, score, [0, 4], (np.array([8, (3 << 32) | 2], np.uint64), ones, ones[0]), 0.005, 8800.)
    for bad in (0., -0.5, np.inf, np.nan):
        vals = ones.copy()
        vals[1, 2] = bad
        fails(-2, 'gd_val row 1 must be finite and > 0', genome, iden, score, [0, 4], (np.array([8, 9], np.uint64), vals, ones[0]), 0.005, 8800.)
        fails(-2, 'gd_default must be finite and > 0', genome, iden, score, [0, 4], (np.array([8, 9], np.uint64), ones, vals[1]), 0.005, 8800.)
    for bad in (np.inf, -np.inf, np.nan):
        fails(-2, 'self_id must be finite', genome, iden, score, [0, 4], gd, bad, 8800.)
        fails(-2, 'thr must be finite', genome, iden, score, [0, 4], gd, 0.005, bad)
    with pytest.raises(ValueError):
        N.gene_ingroups_check(genome, iden[:3], score, [0, 4], gd, 0.005, 8800.)


def test_python_layer_refuses_what_cannot_travel():
    params = dict(clust_identity=0.9, allowed_sigma=3., self_id=0.005)
    with pytest.raises(ValueError, match='empty table'):
        IG.gene_ingroups([np.zeros((0, 7), np.int64)], {}, params)
    wide = np.zeros((2, 7), np.int64)
    wide[:, 2] = (9, 1)
    wide[:, 3] = (1, -5)                                # row 0 leads (keys 1001 and 106.1), column 4 of row 1 becomes 10000 * -5 / 1
    with pytest.raises(ValueError, match=r'column 4 .identity. must lie in \[0, 2\^31\)'):
        IG.gene_ingroups([wide], {}, params)
    with pytest.raises(ValueError, match='number the rows'):
        IG.determine_group(np.array([[1, 9000, 1], [2, 9000, 0]]), {}, 0.9, 3., 0.005)
    with pytest.raises(ValueError, match='allowed_sigma'):
        IG.determine_group(np.array([[1, 9000, 0]]), IG.gd_table({}, 0.005, 2.), 0.9, 3., 0.005)
    assert IG.determine_group(np.zeros((0, 3), np.int64), {}, 0.9, 3., 0.005).shape == (0,)
    # a table of one row passes through untouched, without a device
    one = np.array([[7, 3, -12, 9000, 9000, 7000, 0]])
    (m, s), = IG.gene_ingroups([one], {}, params)
    assert m is one and s == -12
