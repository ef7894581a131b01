"""K17 on the GPU: Context.gene_ingroups and peppan_amd.ingroups against the results recorded from the reference's own determineGroup /
initializing2 (tests/golden/g21_ingroup.json.gz) and the independent restatement in plain Python loops (tests/ingroup_helpers.py).  Every
comparison is ==: the float chain is three single correctly rounded double operations, no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from peppan_amd import ingroups as IG  # noqa: E402  (pure Python: the library is loaded on first use)
from ingroup_helpers import (EDGE_GD, EDGE_PARAMS, SIZES, edge_variants, flat, gd_object_array, load_g21, random_genes, restate, restate_gene,  # noqa: E402
                             threshold)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native as N
    with N.Context(0) as c:
        yield c


@pytest.fixture(scope='module')
def g21():
    return load_g21()


def table_of(gd, self_id, sigma):
    from peppan_amd import orthofilter as OF
    return OF.gd_table(gd, self_id, sigma)


def check_batch(ctx, genes, gd, min_iden, sigma, self_id, tag=''):
    """one batch through Context.gene_ingroups against the restatement, gene by gene -> the restatement's results"""
    genome, iden, score, gene_off = flat(genes)
    keep, total = ctx.gene_ingroups(genome, iden, score, gene_off, table_of(gd, self_id, sigma), self_id, threshold(min_iden))
    assert keep.dtype == bool and keep.shape == (len(genome),) and total.dtype == np.int64 and total.shape == (len(genes),)
    want = []
    for g, (lo, hi) in enumerate(zip(gene_off[:-1].tolist(), gene_off[1:].tolist())):
        r = restate(genes[g][0], genes[g][1], gd, min_iden, sigma, self_id, score=genes[g][2])
        assert keep[lo:hi].tolist() == r['keep'], (tag, g)
        assert int(total[g]) == r['score'], (tag, g)
        want.append(r)
    return want


def test_every_determine_group_case_exactly(g21):
    for k, c in enumerate(g21['determine']):
        n = len(c['genome'])
        gIden = np.stack([c['genome'], c['iden'], np.arange(n)], axis=1).astype(np.int64)
        source = (c['gd'], gd_object_array(c['gd']), table_of(c['gd'], c['self_id'], c['nSigma']))[k % 3]
        got = IG.determine_group(gIden, source, c['min_iden'], c['nSigma'], c['self_id'])
        assert got.dtype == bool and got.tolist() == [bool(v) for v in c['ingroup']], c['name']
    IG.close()


def rows_as_set(rows):
    return sorted(tuple(int(v) for v in r) for r in rows)


def check_run(run, tables, results):
    for gene, (matches, score) in results.items():
        rec = run['genes'][gene]
        assert matches.dtype == np.int64 and isinstance(score, (int, np.integer)) and int(score) == rec['score'], gene
        if rec['tie']:
            assert rows_as_set(matches) == rows_as_set(rec['kept']), gene
        else:
            assert matches.tolist() == rec['kept'], gene


def test_initializing2_cases_through_gene_ingroups(g21):
    init = g21['initializing']
    genes = sorted(init['tables'])
    tables = [np.array(init['tables'][g], dtype=np.int64) for g in genes]
    before = [t.copy() for t in tables]
    for k, run in enumerate(init['runs']):
        params = dict(clust_identity=run['clust_identity'], allowed_sigma=run['allowed_sigma'], self_id=run['self_id'])
        source = init['gd'] if k else gd_object_array(init['gd'])
        got = IG.gene_ingroups(tables, source, params)
        check_run(run, init['tables'], dict(zip(genes, got)))
        for g, (rows, score) in zip(genes, got):
            if not run['genes'][g]['tie']:
                want_rows, want_score = restate_gene(init['tables'][g], init['gd'], run['clust_identity'], run['allowed_sigma'], run['self_id'])
                assert rows.tolist() == want_rows and int(score) == want_score, g
    assert all(np.array_equal(a, b) for a, b in zip(tables, before))               # the caller's tables stay as they were
    IG.close()


def test_initializing_over_a_tab_store_and_the_store_read_back(g21, tmp_path):
    from peppan_amd.mapbsn import MapBsn
    init = g21['initializing']
    global_file = str(tmp_path / 'global.npy')
    np.save(global_file, gd_object_array(init['gd']), allow_pickle=True)
    for k, run in enumerate(init['runs']):
        prefix = str(tmp_path / ('run%d' % k))
        with MapBsn(prefix + '.tab.npz', 'w') as store:
            for gene, t in init['tables'].items():
                store.save(int(gene), np.array(t, dtype=np.int64))
        params = dict(clust_identity=run['clust_identity'], allowed_sigma=run['allowed_sigma'], self_id=run['self_id'])
        scores = IG.initializing(prefix, global_file, params, batch_rows=500)
        assert sorted(scores) == sorted(int(g) for g in init['tables'])
        assert not os.path.exists(prefix + '.tmp.npz')
        with MapBsn(prefix + '.tab.npz') as store:
            assert sorted(store.keys()) == sorted(init['tables'])
            check_run(run, init['tables'], {g: (store.get(g), scores[int(g)]) for g in init['tables']})
    IG.close()


def test_panel_and_chunk_edges_in_one_batch(ctx):
    rng = np.random.default_rng(256)
    genes, names = [], []
    for n in SIZES:
        for name, genome, iden in edge_variants(n, rng):
            genes.append((genome, iden, rng.integers(-9000, 9000, n)))
            names.append((n, name))
    assert {n for n, _ in names} == set(SIZES) and len({name for _, name in names}) == 7
    want = check_batch(ctx, genes, EDGE_GD, EDGE_PARAMS['min_iden'], EDGE_PARAMS['nSigma'], EDGE_PARAMS['self_id'], 'edges')
    # what the variants are built for, from the restatement (test_ingroup_host.py holds the details)
    for (n, name), r in zip(names, want):
        if name == 'no-seeds':
            assert not any(r['keep']) and r['score'] == 0
        if name in ('row0-to-last', 'panel-before'):
            assert r['raw'][n - 1] and r['brought_in']
        if name == 'seed-behind':
            assert not all(r['raw'])
        if name == 'first-out-later-in':
            assert r['up']
        if name == 'first-in-later-out':
            assert r['down']


def test_random_ragged_batch_equals_the_restatement(ctx):
    genes, gd = random_genes(1700, 120, 700)
    lens = [len(g[0]) for g in genes]
    assert min(lens) == 1 and max(lens) > 512
    for min_iden, sigma, self_id in ((0.9, 3., 0.005), (0.95, 2., 0.002)):
        want = check_batch(ctx, genes, gd, min_iden, sigma, self_id, 'fuzz')
        share = [sum(int(r[k]) for r in want) / len(want) for k in ('left_out', 'brought_in', 'same_genome', 'default')]
        print('fuzz shares left_out / brought_in / same_genome / default: %.2f %.2f %.2f %.2f' % tuple(share))
        assert min(share) >= 0.1, share


def test_ties_of_the_float_chain_equal_numpy(ctx):
    """gd1 = 0 makes den == gd0.  With x = 1. - iden_j / iden_i, gd0 = x gives sc == 1.0 exactly (out), gd0 = nextafter(x, 1) a quotient below 1 (in);
    the same with self_id for two rows of one genome."""
    rng = np.random.default_rng(1)
    pairs = [(int(i), int(j)) for i, j in zip(rng.integers(8800, 10001, 150), rng.integers(3000, 8800, 150))]
    genes, gd, expect = [], {}, []
    for k, (iden_i, iden_j) in enumerate(pairs):
        x = np.float64(1.) - np.float64(iden_j) / np.float64(iden_i)
        for step, bound in enumerate((x, np.nextafter(x, 1.))):
            a, b = 10 + 4 * k + 2 * step, 11 + 4 * k + 2 * step
            gd[(a, b)] = (float(bound), 0.)
            genes.append((np.array([a, b]), np.array([iden_i, iden_j]), np.array([3, 4])))
            sc = x / (bound * np.exp(np.float64(3.) * 0.))
            assert (sc == 1.0) if step == 0 else (sc < 1.0)
            expect.append(step == 1)
    want = check_batch(ctx, genes, gd, 0.9, 3., 0.005, 'ties')
    assert [r['keep'][1] for r in want] == expect and all(r['keep'][0] for r in want)
    # Two rows of one genome: the bound is self_id, one call per value.  A row that meets a seed of its own genome is never the first row of that
    # genome, and keep reads the first row's flag alone: the same-genome bound decides raw[j] and can never show in keep or in the score.  So the
    # results are the restatement's on either side of the tie, and the first row's flag is what both rows get.
    empty = (np.zeros(0, np.uint64), np.zeros((0, 3)), np.array([0.5, 1., 3.]))
    for iden_i, iden_j in pairs[:6]:
        x = np.float64(1.) - np.float64(iden_j) / np.float64(iden_i)
        for self_id in (float(x), float(np.nextafter(x, 1.))):
            for genome, iden in (([7, 7], [iden_i, iden_j]), ([7, 7, 7], [iden_j, iden_i, iden_j])):
                keep, score = ctx.gene_ingroups(genome, iden, [5, -6, 8][:len(iden)], [0, len(iden)], empty, self_id, threshold(0.9))
                r = restate(genome, iden, {}, 0.9, 3., self_id, score=[5, -6, 8][:len(iden)])
                assert r['same_genome'] and keep.tolist() == r['keep'] == [len(iden) == 2] * len(iden) and int(score[0]) == r["score"], (iden, self_id)


def test_bytes_to_host_for_any_mix_of_gene_sizes(ctx):
    genes, gd = random_genes(1701, 60, 600)
    genome, iden, score, gene_off = flat(genes)
    table = table_of(gd, 0.005, 3.)
    ctx.set_timing(2)
    try:
        ctx.gene_ingroups(genome, iden, score, gene_off, table, 0.005, 8800.)
        ms, moved = ctx.gene_ingroups_times()
        assert moved == len(genome) + 8 * len(genes) and ms.shape == (2,) and (ms > 0).all()
    finally:
        ctx.set_timing(0)
    # empty genes in front, between and behind; one gene alone; an empty batch
    off = np.concatenate([[0, 0], gene_off[:5], [gene_off[4]], gene_off[5:], [gene_off[-1]] * 3]).astype(np.uint64)
    keep, total = ctx.gene_ingroups(genome, iden, score, off, table, 0.005, 8800.)
    ms, moved = ctx.gene_ingroups_times()
    assert moved == len(genome) + 8 * (len(off) - 1) and (ms == 0).all()
    ref_keep, ref_total = ctx.gene_ingroups(genome, iden, score, gene_off, table, 0.005, 8800.)
    assert np.array_equal(keep, ref_keep) and np.array_equal(total[total != 0], ref_total[ref_total != 0]) and total[0] == 0 and total[-1] == 0
    keep, total = ctx.gene_ingroups(genome[:1], iden[:1], score[:1], [0, 1], table, 0.005, 8800.)
    assert ctx.gene_ingroups_times()[1] == 1 + 8 and keep.shape == (1,)
    keep, total = ctx.gene_ingroups([], [], [], [0], table, 0.005, 8800.)
    assert ctx.gene_ingroups_times()[1] == 0 and keep.shape == (0,) and total.shape == (0,)
    keep, total = ctx.gene_ingroups([], [], [], [0, 0, 0], table, 0.005, 8800.)
    assert ctx.gene_ingroups_times()[1] == 16 and keep.shape == (0,) and total.tolist() == [0, 0]


def test_split_by_batch_rows_equals_one_batch():
    from peppan_amd import orthofilter as OF
    genes, gd = random_genes(1702, 70, 400)
    rng = np.random.default_rng(3)
    tables = []
    for genome, iden, score in genes:
        t = np.zeros((len(genome), 6), dtype=np.int64)
        t[:, 1], t[:, 2], t[:, 3], t[:, 5] = genome, score * 7 + 1, iden, rng.permutation(len(genome))
        t[:, 4] = t[:, 3]
        tables.append(t)
    params = dict(clust_identity=0.9, allowed_sigma=3., self_id=0.005)
    whole = IG.gene_ingroups(tables, gd, params)
    c = OF._context(None)
    calls, real = [], c.gene_ingroups
    c.gene_ingroups = lambda *a: calls.append(len(a[0])) or real(*a)
    try:
        split = IG.gene_ingroups(tables, gd, params, batch_rows=1000)
    finally:
        del c.gene_ingroups
    many = sum(len(t) for t in tables if len(t) > 1)
    assert len(calls) >= 4 and sum(calls) == many and all(n <= 1000 or n in [len(t) for t in tables] for n in calls)
    assert any(len(m) < len(t) for (m, _), t in zip(whole, tables))
    for (m1, s1), (m2, s2) in zip(whole, split):
        assert np.array_equal(m1, m2) and s1 == s2
    IG.close()


def test_errors_write_nothing_and_the_context_stays_usable(ctx):
    from peppan_amd import _native as N
    import ctypes as C
    genes, gd = random_genes(1703, 10, 300)
    genome, iden, score, gene_off = flat(genes)
    table = table_of(gd, 0.005, 3.)
    good = ctx.gene_ingroups(genome, iden, score, gene_off, table, 0.005, 8800.)
    bad_iden = iden.copy()
    bad_iden[3] = -1
    args, n_rows, n_genes, alive = N._ingroup_tables(genome, bad_iden, score, gene_off, table)
    keep, total = np.full(n_rows, 7, np.uint8), np.full(n_genes, -7, np.int64)
    rc = ctx._lib.pep_gene_ingroups(ctx._h, *args, C.c_double(0.005), C.c_double(8800.), N._ptr(keep), N._ptr(total))
    assert rc == -2 and 'iden of row 3 is negative' in ctx._lib.pep_last_error(ctx._h).decode()
    assert (keep == 7).all() and (total == -7).all()
    for a, text in (((genome, iden, score, gene_off[:-1], table, 0.005, 8800.), 'gene_off must end at n_rows'),
                    ((genome, iden, score, gene_off, (np.array([5, 5], np.uint64), np.ones((2, 3)), np.ones(3)), 0.005, 8800.), 'gd_key must be strictly increasing'),
                    ((genome, iden, score, gene_off, table, 0.005, float('nan')), 'thr must be finite')):
        with pytest.raises(N.PepError, match=r'pep_gene_ingroups failed \(-2\): pep_gene_ingroups: ' + text):
            ctx.gene_ingroups(*a)
        again = ctx.gene_ingroups(genome, iden, score, gene_off, table, 0.005, 8800.)
        assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])


def test_live_resources_return_to_their_start():
    from peppan_amd import _native as N
    genes, gd = random_genes(1704, 20, 300)
    genome, iden, score, gene_off = flat(genes)
    start = N.live_resources()
    with N.Context(0) as c:
        c.set_timing(2)
        c.gene_ingroups(genome, iden, score, gene_off, table_of(gd, 0.005, 3.), 0.005, 8800.)
        assert N.live_resources()[0] > start[0]
    assert N.live_resources() == start
