"""K22 on the GPU (csrc/globaldiff.hip: the genome-pair identity statistics of get_global_difference, PEPPAN.py:1611-1666): the drop-in against what the
reference's own function returned for every case of tests/golden/g22_globaldiff.json.gz, and Context.global_diff on synthetic events against the
restatement of include/peppan_hip.h's rules (tests/globaldiff_helpers.py).

The tolerance is zero: keys, their order, counts as integers, every float as its bit pattern.  Every float operation on the device is an IEEE add,
subtract, multiply or divide, which have one correct result.

Shapes.  numpy's sum changes its path at 8 (no accumulators below), at 128 (one leaf up to there), and at 8192 (one buffer up to there), so the synthetic
keys have n = 1, 7, 8, 9, 127, 128, 129, 8192, 8193 and 16385 values; they are built from events of a few items each with differing values, a few
thousand events in all.  chunk_items = 64 cuts those into hundreds of chunks: an event of 8 x 16 items is split, and every long key is fed from many."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import globaldiff_helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 8, 9, 127, 128, 129, 8192, 8193, 16385]


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


def same(got, want):
    """(g1, g2, n, mean, var) twice: integers equal, floats bit for bit"""
    assert [len(a) for a in got] == [len(a) for a in want]
    for k in range(3):
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), k
    for k in (3, 4):
        assert np.array_equal(np.asarray(got[k]).view(np.uint64), np.asarray(want[k]).view(np.uint64)), k


def sized_keys():
    """genome 0 against genomes 1 .. 10: key (0, g) gets SIZES[g - 1] values.  The arena: one entry of genome 0, then per genome a run of 16 entries; an
    event is (the 0 entry) x (a prefix of 1 .. 16 entries of the run), values differ from event to event.  One more event of 8 x 16 items - 8 entries
    of genome 11 against 16 of genome 12 - is larger than a chunk of 64."""
    rng = np.random.default_rng(22)
    arena = [0] + [g for g in range(1, len(SIZES) + 1) for _ in range(16)] + [11] * 8 + [12] * 16
    left = {g: n for g, n in zip(range(1, len(SIZES) + 1), SIZES)}
    events = []
    while left:
        g = int(rng.choice(sorted(left)))
        take = min(left[g], int(rng.integers(1, 4 if SIZES[g - 1] < 16 else 17)))           # (the short keys from several events too)
        flip = bool(rng.integers(0, 2))                     # (the genome-0 list on either side: both orientations land in one key)
        a, b = (0, 1), (1 + 16 * (g - 1), take)
        events.append(list(b + a if flip else a + b) + [int(rng.integers(0, 10050)), int(rng.integers(0, 2))])
        left[g] -= take
        if not left[g]:
            del left[g]
        if len(events) == 40:
            events.append([1 + 16 * len(SIZES), 8, 1 + 16 * len(SIZES) + 8, 16, 4321, 1])
    return np.array(events, dtype=np.int64), np.array(arena, dtype=np.int32)


@pytest.fixture(scope='module')
def sized(ctx):
    events, arena = sized_keys()
    table = H.log_table()
    want = H.pair_statistics(events, arena, table)
    assert sorted(want[2].tolist()) == sorted(SIZES + [128]) and len(events) > 3000
    return events, arena, table, want


def test_every_golden_case_bit_for_bit(N, tmp_path):
    from peppan_amd import globaldiff as GD
    for c in H.load_cases():
        clu_file, bsn_file = H.write_tables(c, tmp_path)
        got = GD.get_global_difference(c['geneGroups'], clu_file, bsn_file, c['geneInGenomes'], c['nGene'])
        assert got.dtype == object and got.shape == c['shape'], c['name']
        assert H.same_rows(got, c['rows']), c['name']


def test_sized_keys_are_the_restatement(ctx, sized):
    events, arena, table, want = sized
    got = ctx.global_diff(events, arena, 13, table)
    for g2, n, m, v in zip(got[1], got[2], got[3], got[4]):
        print('key (0, %d): n = %d, m = %r, v = %r' % (g2, n, m, v))
    same(got, want)


def test_chunks_of_64_items_change_nothing(ctx, sized):
    events, arena, table, want = sized
    assert int((events[:, 1] * events[:, 3]).max()) > 64 and int((events[:, 1] * events[:, 3]).sum()) > 100 * 64
    same(ctx.global_diff(events, arena, 13, table, chunk_items=64), want)
    same(ctx.global_diff(events, arena, 13, table, chunk_items=1000), want)


def test_two_keys_first_met_in_one_event(ctx):
    """event 0 meets (2, 3) before (1, 3), event 1 meets (0, 3) before (0, 0): the order of the items, not of the keys"""
    arena = np.array([2, 1, 3, 0, 0], dtype=np.int32)
    events = [[0, 2, 2, 1, 100, 0], [3, 2, 2, 3, 200, 0]]
    got = ctx.global_diff(events, arena, 4, H.log_table())
    same(got, H.pair_statistics(events, arena, H.log_table()))
    assert list(zip(got[0].tolist(), got[1].tolist())) == [(2, 3), (1, 3), (0, 3), (0, 0)] and got[2].tolist() == [1, 1, 2, 4]


def test_drop_same_event_of_one_genome_gives_no_key(ctx):
    arena = np.array([5, 5, 5, 2], dtype=np.int32)
    table = H.log_table()
    got = ctx.global_diff([[0, 3, 0, 2, 9000, 1]], arena, 6, table)
    assert all(len(a) == 0 for a in got)
    events = [[0, 3, 0, 2, 9000, 1], [0, 3, 0, 3, 9000, 0], [0, 3, 0, 4, 8000, 1]]
    got = ctx.global_diff(events, arena, 6, table)
    same(got, H.pair_statistics(events, arena, table))
    assert list(zip(got[0].tolist(), got[1].tolist(), got[2].tolist())) == [(5, 5, 9), (2, 5, 3)]


def test_swapped_orientation_lands_in_one_key(ctx):
    arena = np.array([1, 4], dtype=np.int32)
    table = H.log_table()
    events = [[0, 1, 1, 1, 10, 1], [1, 1, 0, 1, 20, 1], [1, 1, 0, 1, 30, 0]]
    got = ctx.global_diff(events, arena, 5, table)
    same(got, H.pair_statistics(events, arena, table))
    assert got[0].tolist() == [1] and got[1].tolist() == [4] and got[2].tolist() == [3]


def test_one_genome_and_an_empty_call(ctx):
    table = H.log_table()
    events = [[0, 2, 0, 2, 77, 0], [0, 1, 1, 1, 78, 0]]
    got = ctx.global_diff(events, np.zeros(2, dtype=np.int32), 1, table)
    same(got, H.pair_statistics(events, np.zeros(2, dtype=np.int32), table))
    assert got[2].tolist() == [5]
    for events, arena, n_genomes in (([], [], 0), ([], [0, 1], 2), (np.zeros((0, 6), dtype=np.int64), np.zeros(0, dtype=np.int32), 16384)):
        assert all(len(a) == 0 for a in ctx.global_diff(events, arena, n_genomes, table))


def test_a_smaller_second_call_returns_the_smaller_result(N, sized):
    """the grow-only buffers keep the first call's sizes and contents; the second call's result is its own"""
    events, arena, table, want = sized
    with N.Context(0) as fresh:
        same(fresh.global_diff(events, arena, 13, table), want)
        small = events[:25]
        same(fresh.global_diff(small, arena, 13, table), H.pair_statistics(small, arena, table))
        tiny_arena = np.array([0, 1], dtype=np.int32)
        same(fresh.global_diff([[0, 1, 1, 1, 5, 1]], tiny_arena, 2, table), H.pair_statistics([[0, 1, 1, 1, 5, 1]], tiny_arena, table))
        same(fresh.global_diff(events, arena, 13, table, chunk_items=64), want)


def test_call_times_of_global_diff(N, ctx):
    """pep_call_times(PEP_CALL_GLOBAL_DIFF): with every phase timed the three slots the header states - counting, chunks, sums - are > 0, the other five and
    the byte counts 0; untimed, every slot is 0.  The wrapper makes one library call: its total is that call's record."""
    arena, events, table = np.array([2, 1, 3, 0, 0], dtype=np.int32), [[0, 2, 2, 1, 100, 0], [3, 2, 2, 3, 200, 0]], H.log_table()
    ctx.set_timing(2)
    try:
        ctx.global_diff(events, arena, 4, table)
        for total in (False, True):
            ms, to_device, to_host = ctx.call_times(N.CALL_GLOBAL_DIFF, total=total)
            print('total=%r: ms %r' % (total, ms.tolist()))
            assert ms.shape == (8,) and (ms[:3] > 0).all() and not ms[3:].any() and (to_device, to_host) == (0, 0)
    finally:
        ctx.set_timing(0)
    ctx.global_diff(events, arena, 4, table)
    assert not ctx.call_times(N.CALL_GLOBAL_DIFF)[0].any() and not ctx.call_times(N.CALL_GLOBAL_DIFF, total=True)[0].any()


def test_device_refusals_name_what_was_asked_for(N, ctx):
    table = H.log_table()
    with pytest.raises(N.PepError, match='16385 genomes'):
        ctx.global_diff([], [], 16385, table)
    with pytest.raises(N.PepError, match='event 0 has the value 10050'):
        ctx.global_diff([[0, 1, 0, 1, 10050, 0]], [0], 1, table)
    with pytest.raises(ValueError):
        ctx.global_diff([[0, 1, 0, 1, 5, 0]], [0], 1, table[:-1])
    assert ctx.global_diff([[0, 1, 0, 1, 5, 0]], [0], 1, table)[2].tolist() == [1]         # the context goes on after a refusal
