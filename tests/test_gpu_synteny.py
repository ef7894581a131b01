"""K18 on the GPU: Context.synteny_pairs and peppan_amd.synteny against the results recorded from the reference's own ite_synteny_resolver /
synteny_resolver (tests/golden/g22_synteny.json.gz) and the independent restatement in plain Python loops (tests/synteny_helpers.py).  Every
comparison is ==: the stage is integer arithmetic, no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from peppan_amd import synteny as SY  # noqa: E402  (pure Python: the library is loaded on first use)
from synteny_helpers import (LIST_SIZES, SIZES, case_inputs, expected_names, flat, load_g22, locus_group, prediction_columns, record_of, restate_pairs,  # noqa: E402
                             same_record)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native as N
    with N.Context(0) as c:
        yield c


@pytest.fixture(scope='module')
def g22():
    return load_g22()


def check_batch(ctx, groups, n_neighbor, tag=''):
    """one batch through Context.synteny_pairs against the restatement, group by group -> the restatement's details"""
    member_off, genome, nb_off, nb = flat(groups)
    has, dc, conf_off, conf, walk_off, walk = ctx.synteny_pairs(member_off, genome, nb_off, nb, n_neighbor)
    G = len(groups)
    assert has.dtype == bool and has.shape == (G,) and dc.dtype == np.int32 and dc.shape == (G,)
    assert conf_off.shape == (G + 1,) and walk_off.shape == (G + 1,) and conf_off[0] == 0 and walk_off[0] == 0
    assert conf.dtype == np.uint32 and conf.shape == (int(conf_off[-1]), 2) and walk.dtype == np.uint32 and walk.shape == (int(walk_off[-1]), 2)
    want = []
    for g, (gen, lists) in enumerate(groups):
        r = restate_pairs(gen, lists, n_neighbor)
        assert bool(has[g]) == r['has'] and int(dc[g]) == r['dc'], (tag, g, int(dc[g]), r['dc'])
        assert [tuple(p) for p in conf[conf_off[g]:conf_off[g + 1]].tolist()] == r['conf'], (tag, g, 'conflict pairs')
        assert [tuple(p) for p in walk[walk_off[g]:walk_off[g + 1]].tolist()] == r['walk'], (tag, g, 'walked pairs')
        want.append(r)
    return want


def test_group_sizes_around_the_chunk_of_64_members(ctx):
    """0 .. 300 members in one batch: rows of less than one, exactly one and several chunks of 64 lanes, groups that start anywhere"""
    rng = np.random.default_rng(1801)
    groups = [locus_group(rng, n, max(2, n // 5), 4, sizes=(6, 6, 7), noise=0.1, pool=5, drop=0.04) if n else ([], []) for n in SIZES]
    want = check_batch(ctx, groups, 2, 'sizes')
    assert sum(r['has'] for r in want) >= 6 and sum(len(r['walk']) for r in want) > 10000 and sum(len(r['conf']) for r in want) > 1000


def test_many_tiny_groups_around_one_large_group(ctx):
    rng = np.random.default_rng(1802)
    tiny = lambda: locus_group(rng, int(rng.integers(0, 6)), 2, 2, sizes=(6, 5), noise=0.1)
    groups = [tiny() for _ in range(70)] + [locus_group(rng, 190, 9, 4, sizes=(6, 7), noise=0.1, pool=5)] + [tiny() for _ in range(70)]
    assert sum(len(g[0]) for g in groups[:70]) % 64 != 0                          # the large group starts in the middle of a block of rows
    want = check_batch(ctx, groups, 2, 'tiny-large')
    assert want[70]['has'] and sum(r['has'] for r in want) > 20 and sum(not r['has'] for r in want) > 20


def test_list_lengths_across_the_fixed_slots(ctx):
    """lists of 0, 1, 6, 7, 8, 9 and 40 ids: rows of at most 8 ids sit in registers, longer rows take the merge; both meet every length"""
    rng = np.random.default_rng(1803)
    groups = []
    for sizes in ((0,), (1,), (6,), (7,), (8,), (9,), (40,), LIST_SIZES, (8, 9), (0, 40), (6, 40)):
        groups.append(locus_group(rng, 14, 4, 2, sizes=sizes, noise=0.15, pool=4, drop=0.))
    assert {len(a) for g in groups for a in g[1]} >= {0, 1, 6, 7, 8, 9, 40}
    for nn in (1, 2, 3):
        check_batch(ctx, groups, nn, 'lists nN=%d' % nn)


def test_constructed_inputs(ctx):
    rng = np.random.default_rng(1804)
    full = lambda base, size=6: list(range(base, base + size))
    groups = {
        'all one genome': ([7] * 20, locus_group(rng, 20, 1, 3, sizes=(6,), noise=0.1)[1]),
        'no conflict: genomes all apart': (list(range(15)), locus_group(rng, 15, 1, 3, sizes=(6,), noise=0.1)[1]),
        'no conflict: one neighbourhood': ([1, 1, 2, 2, 3], [full(100)] * 5),
        'strongly negative d': ([1, 2, 1, 2], [full(0, 40), full(0, 40), full(0, 39), full(500, 40)]),
        'a single pair': ([3, 3], [full(0), full(10)]),
    }
    # dc at each of 1 .. 5 (nNeighbor 2): two copies in one genome that share nothing, the second list of 6, 5, 4, 3, 2 ids, + a third member
    for short, dc in ((6, 5), (5, 4), (4, 3), (3, 2), (2, 1)):
        groups['dc %d' % dc] = ([1, 1, 2], [full(0), full(100, short), full(0)])
    names = list(groups)
    want = check_batch(ctx, [groups[k] for k in names], 2, 'constructed')
    got = dict(zip(names, want))
    for dc in (1, 2, 3, 4, 5):
        assert got['dc %d' % dc]['has'] and got['dc %d' % dc]['dc'] == dc
    assert not got['no conflict: genomes all apart']['has'] and not got['no conflict: one neighbourhood']['has']
    assert got['strongly negative d']['d_min'] <= -100 and got['strongly negative d']['has']
    assert got['all one genome']['has'] and got['a single pair']['conf'] == [(0, 1)] and got['a single pair']['walk'] == []
    for nn in (1, 3):
        check_batch(ctx, [groups[k] for k in names], nn, 'constructed nN=%d' % nn)


def test_empty_batches(ctx):
    for member_off in ([0], [0, 0, 0], [0, 1, 1, 2]):
        n = member_off[-1]
        has, dc, conf_off, conf, walk_off, walk = ctx.synteny_pairs(member_off, [5] * n, [0] * (n + 1), [], 2)
        assert not has.any() and not dc.any() and len(has) == len(member_off) - 1 and conf.shape == (0, 2) and walk.shape == (0, 2)
        assert conf_off.tolist() == [0] * len(member_off) and walk_off.tolist() == [0] * len(member_off)
    assert SY.resolve_groups([], 2) == []


def test_a_refused_call_leaves_the_context_usable(ctx):
    from peppan_amd import _native as N
    groups = [([1, 1, 2], [[1, 2, 3, 4, 5, 6], [11, 12, 13, 14, 15, 16], [1, 2, 3, 4, 5, 6]])] * 2
    member_off, genome, nb_off, nb = flat(groups)
    with pytest.raises(N.PepError) as e:
        ctx.synteny_pairs([0, 16385], np.zeros(16385, np.uint32), np.zeros(16386, np.uint64), [], 2)
    assert '(-3)' in str(e.value) and 'group 0 (16385 members)' in str(e.value)
    with pytest.raises(N.PepError) as e:
        ctx.synteny_pairs(member_off, genome, nb_off, nb, 0)
    assert '(-2)' in str(e.value)
    check_batch(ctx, groups, 2, 'after a refusal')


def test_times_and_bytes(ctx):
    rng = np.random.default_rng(1805)
    groups = [locus_group(rng, 120, 6, 3, sizes=(6,), noise=0.1)]
    member_off, genome, nb_off, nb = flat(groups)
    ctx.set_timing(2)
    try:
        _, _, conf_off, _, walk_off, _ = ctx.synteny_pairs(member_off, genome, nb_off, nb, 2)
        ms, moved = ctx.synteny_times()
    finally:
        ctx.set_timing(0)
    assert ms.shape == (3,) and (ms > 0).all() and int(conf_off[-1]) > 0 and moved == 12 * 1 + 16 + 8 * int(conf_off[-1] + walk_off[-1])
    ctx.synteny_pairs(member_off, genome, nb_off, nb, 2)
    assert not ctx.synteny_times()[0].any()


def test_every_recorded_group_through_ite_synteny_resolver(g22):
    for c in g22['groups']:
        tag, ids, genomes, neighbors, nn = case_inputs(c)
        got = SY.ite_synteny_resolver((tag, ids, genomes, neighbors, nn))
        assert same_record(record_of(got), c['returned']), c['name']
        if got[1] is not None:                                                     # the lists in the reference's order, keyed by the surviving tag
            assert {int(k): [int(x) for x in v] for k, v in got[1].items()} == {k: v for k, v in c['returned']['parts']}, c['name']
    SY.close()


@pytest.mark.parametrize('pair_cap', [SY.PAIR_CAP, 40])
def test_every_recorded_group_through_resolve_groups(g22, pair_cap):
    """all groups of one nNeighbor in one batch, and with a pair cap that forces many library calls (a group above the cap gets a call of its own)"""
    for nn in (1, 2, 3):
        cases = [c for c in g22['groups'] if c['nNeighbor'] == nn]
        got = SY.resolve_groups([case_inputs(c)[:4] for c in cases], nn, pair_cap=pair_cap)
        assert len(got) == len(cases)
        for c, r in zip(cases, got):
            assert same_record(record_of(r), c['returned']), (c['name'], pair_cap)
    n = np.array([len(c['ids']) for c in g22['groups']])
    assert len(SY._plan((n * (n - 1) // 2).tolist(), [1] * len(n), 40)) > 100
    SY.close()


def test_split_names_on_the_recorded_runs(g22):
    for run in g22['runs']:
        rows, name, gid, genome, contig, start = prediction_columns(run['prediction'])
        got, order = SY.split_names(name, gid, genome, contig, start, run['nNeighbor'])
        assert got.tolist() == expected_names(run['prediction'], run['synteny_prediction'])
        assert sorted(order.tolist()) == list(range(len(rows)))
        keys = [(contig[i], start[i]) for i in order.tolist()]
        assert keys == sorted(keys)
    SY.close()


def test_synteny_resolver_byte_for_byte(g22, tmp_path):
    pytest.importorskip('pandas')
    for k, run in enumerate(g22['runs']):
        src = tmp_path / ('run%d.Prediction' % k)
        src.write_text(run['prediction'])
        out = SY.synteny_resolver(str(tmp_path / ('run%d' % k)), str(src), run['nNeighbor'])
        assert out == str(tmp_path / ('run%d.synteny.Prediction' % k))
        with open(out, 'rb') as f:
            assert f.read() == run['synteny_prediction'].encode()
    SY.close()


def test_nothing_is_left_on_the_device_after_close():
    from peppan_amd import _native as N
    SY.close()
    before = N.live_resources()
    rng = np.random.default_rng(1806)
    with N.Context(0) as c:
        check_batch(c, [locus_group(rng, 80, 5, 3, sizes=(6, 9), noise=0.1)], 2, 'close')
        assert N.live_resources()[0] > before[0]
    assert N.live_resources() == before
    genome, lists = locus_group(rng, 30, 4, 3, sizes=(6,), noise=0.1)
    SY.ite_synteny_resolver((9, np.arange(30), np.array(genome), [set(a) for a in lists], 2))
    assert N.live_resources()[0] > before[0]
    SY.close()
    assert N.live_resources() == before
