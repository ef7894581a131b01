"""K18 (neighbourhood paralog splitting, PEPPAN.py:1097-1151, 1153-1191) without a GPU: the g22 fixture recorded from the reference's own
ite_synteny_resolver / synteny_resolver against the independent restatement in plain loops (tests/synteny_helpers.py), its section of
include/peppan_hip.h against _native's limits, the table checks of pep_synteny_pairs, which need no device, and the host walk."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from peppan_amd import synteny as SY  # noqa: E402,F401  (pure Python: the library is loaded on first use)
from synteny_helpers import case_inputs, flat, load_g22, parse_prediction, restate, same_record  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


@pytest.fixture(scope='module')
def g22():
    return load_g22()


@pytest.fixture(scope='module')
def restated(g22):
    """the restatement of every recorded group, computed once: [(record, details)]"""
    return [restate(c['tag'], c['ids'], c['genomes'], c['neighbors'], c['nNeighbor']) for c in g22['groups']]


def test_restatement_equals_every_recorded_group(g22, restated):
    cases = g22['groups']
    assert len(cases) >= 150
    tally = dict(none=0, refused=0, partition=0)
    skipped, dcs, big, sizes = 0, {}, [], set()
    for c, (mine, detail) in zip(cases, restated):
        assert same_record(mine, c['returned']), c['name']
        assert c['ids'] == sorted(set(c['ids']))
        tally[c['returned']['verdict']] += 1
        skipped += int(detail['skipped'] > 0)
        if detail['has'] and c['nNeighbor'] == 2:
            dcs[detail['dc']] = dcs.get(detail['dc'], 0) + 1
        big.append(len(c['ids']))
        sizes |= {len(a) for a in c['neighbors']}
    assert min(tally.values()) >= 15 and skipped >= 15, (tally, skipped)
    assert all(dcs.get(d, 0) >= 5 for d in (1, 2, 3, 4, 5)), dcs
    assert {c['nNeighbor'] for c in cases} == {1, 2, 3}
    assert {0, 6, 7, 9} <= sizes and max(sizes) >= 20
    assert sum(n >= 65 for n in big) >= 5 and max(big) >= 257


def test_recorded_runs_hold_what_they_are_pinned_by(g22):
    """a name ending in /2 gets '/0.1' appended (the '.k' branch of :1183-1184 is dead), an id spans two rows, an id is carried by no row, and
    the group of one genome keeps its name"""
    assert len(g22['runs']) == 3
    for run in g22['runs']:
        before, after = parse_prediction(run['prediction']), parse_prediction(run['synteny_prediction'])
        assert len(before) == len(after) and sorted(tuple(r[1:]) for r in before) == sorted(tuple(r[1:]) for r in after)
        names = {r[0] for r in after}
        assert 'Q/2/0.1' in names and 'Q/2.1' not in names and 'P/0.1' in names
        assert 'S' in names and not any(n.startswith('S/') for n in names)
        ids = [int(r[2]) for r in before]
        assert len(ids) > len(set(ids)) and set(range(1, max(ids) + 1)) - set(ids)
        assert after == sorted(after, key=lambda r: (r[0], int(r[2]), float(r[7])))


def test_synteny_section_of_the_header(N):
    """the K18 section of include/peppan_hip.h cites what it replaces, and its limits are _native's (the prototypes: tests/test_abi.py)"""
    hdr = open(os.path.join(ROOT, 'include', 'peppan_hip.h')).read()
    assert 'PEPPAN.py:1101-1117' in hdr and 'PEPPAN.py:1118-1151' in hdr
    assert int(re.search(r'#define PEP_SYNTENY_MAX_PAIRS \(1ull << (\d+)\)', hdr).group(1)) == N.SYNTENY_MAX_PAIRS.bit_length() - 1
    assert int(re.search(r'#define PEP_SYNTENY_MAX_COUNTERS \(1ull << (\d+)\)', hdr).group(1)) == N.SYNTENY_MAX_COUNTERS.bit_length() - 1
    assert N.SYNTENY_MAX_PAIRS == 1 << 27 and N.SYNTENY_MAX_COUNTERS == 1 << 26


GOOD = dict(member_off=[0, 3, 5], genome=[1, 1, 2, 4, 4], nb_off=[0, 2, 2, 5, 6, 6], nb=[3, 9, 1, 2, 7, 5], n_neighbor=2)


def _check(N, code=None, text=None, **change):
    args = dict(GOOD, **change)
    if code is None:
        return N.synteny_pairs_check(args['member_off'], args['genome'], args['nb_off'], args['nb'], args['n_neighbor'])
    with pytest.raises(N.PepError) as e:
        N.synteny_pairs_check(args['member_off'], args['genome'], args['nb_off'], args['nb'], args['n_neighbor'])
    assert '(%d)' % code in str(e.value) and text in str(e.value), str(e.value)


def test_check_refuses_each_bad_input_with_its_code(N):
    ARG, LIMIT = -2, -3
    _check(N)
    _check(N, n_neighbor=1)
    _check(N, n_neighbor=1 << 20)
    _check(N, member_off=[0], genome=[], nb_off=[0], nb=[])                        # an empty batch is legal
    _check(N, member_off=[0, 0, 5, 5])                                             # ... and so are empty groups
    for bad in (0, -1, (1 << 20) + 1, (1 << 31) - 1):
        _check(N, ARG, 'n_neighbor', n_neighbor=bad)
    for bad in (1 << 31, (1 << 32) + 2, -(1 << 31) - 1, 2.5):                       # never reaches the library, where ctypes would cut it to 32 bits
        with pytest.raises(ValueError):
            _check(N, n_neighbor=bad)
    _check(N, ARG, 'not strictly ascending', nb=[9, 3, 1, 2, 7, 5])
    _check(N, ARG, 'not strictly ascending', nb=[3, 9, 1, 2, 2, 5])
    _check(N, ARG, 'member_off must start at 0', member_off=[1, 3, 5])
    _check(N, ARG, 'member_off must be non-decreasing (group 1)', member_off=[0, 4, 3, 5])
    _check(N, ARG, 'member_off must end at n_members', member_off=[0, 3, 4])
    _check(N, ARG, 'runs past n_members', member_off=[0, 3, 6])
    _check(N, ARG, 'nb_off must start at 0', nb_off=[1, 2, 2, 5, 6, 6])
    _check(N, ARG, 'nb_off must be non-decreasing (member 1)', nb_off=[0, 2, 1, 5, 6, 6])
    _check(N, ARG, 'nb_off must end at n_nb', nb_off=[0, 2, 2, 5, 5, 5])
    _check(N, ARG, 'runs past n_nb', nb_off=[0, 2, 2, 5, 6, 7])
    # the cap on the pairs of a call: 16 385 members are 2^27 + 8 192 pairs; the message names the group at which the sum passes it
    n = 16385
    _check(N, LIMIT, 'group 0 (16385 members)', member_off=[0, n], genome=np.zeros(n, np.uint32), nb_off=np.zeros(n + 1, np.uint64), nb=[])
    _check(N, member_off=[0, n - 1], genome=np.zeros(n - 1, np.uint32), nb_off=np.zeros(n, np.uint64), nb=[])
    _check(N, member_off=[0, n - 1, n + 127], genome=np.zeros(n + 127, np.uint32), nb_off=np.zeros(n + 128, np.uint64), nb=[])       # 2^27 - 8 192 + 8 128 pairs
    _check(N, LIMIT, 'group 1 (129 members) takes the call past %d pairs' % N.SYNTENY_MAX_PAIRS, member_off=[0, n - 1, n + 128], genome=np.zeros(n + 128, np.uint32),
           nb_off=np.zeros(n + 129, np.uint64), nb=[])


def pair_lists(details):
    """the restatement's two lists of a batch of groups as the library's tables"""
    conf_off, walk_off, conf, walk = [0], [0], [], []
    for d in details:
        conf += d['conf']
        walk += d['walk']
        conf_off.append(len(conf))
        walk_off.append(len(walk))
    return conf_off, np.array(conf, dtype=np.uint32).reshape(-1, 2), walk_off, np.array(walk, dtype=np.uint32).reshape(-1, 2)


def test_walk_reproduces_every_recorded_outcome_member_order_included(N, g22, restated):
    cases = g22['groups']
    member_off = np.concatenate([[0], np.cumsum([len(c['ids']) for c in cases])])
    conf_off, conf, walk_off, walk = pair_lists([d for _, d in restated])
    verdict, comps = N.synteny_walk(member_off, conf_off, conf, walk_off, walk)
    assert verdict.dtype == np.uint8 and len(verdict) == len(comps) == len(cases)
    for c, v, cc in zip(cases, verdict.tolist(), comps):
        want = c['returned']
        assert ('none', 'refused', 'partition')[v] == want['verdict'], c['name']
        if v == 2:
            ids = c['ids']
            got = [[ids[root], [ids[m] for m in members.tolist()]] for root, members in cc]
            assert got == sorted(want['parts']), c['name']                       # by ascending root, every list in the reference's order
        else:
            assert cc is None
    # one group at a time gives the same
    for g in (0, 40, len(cases) - 1):
        d = restated[g][1]
        v1, c1 = N.synteny_walk([0, len(cases[g]['ids'])], [0, len(d['conf'])], np.array(d['conf'], np.uint32).reshape(-1, 2), [0, len(d['walk'])],
                                np.array(d['walk'], np.uint32).reshape(-1, 2))
        assert v1.tolist() == [verdict[g]] and (c1[0] is None) == (comps[g] is None)
        if c1[0] is not None:
            assert [(r, m.tolist()) for r, m in c1[0]] == [(r, m.tolist()) for r, m in comps[g]]


def test_walk_refuses_pairs_outside_their_group_and_takes_an_empty_batch(N):
    v, c = N.synteny_walk([0], [0], np.zeros((0, 2)), [0], np.zeros((0, 2)))
    assert len(v) == 0 and c == []
    for conf, walk in (([[0, 3]], []), ([[1, 1]], []), ([[0, 1]], [[2, 1]]), ([[0, 1]], [[0, 5]])):
        with pytest.raises(N.PepError) as e:
            N.synteny_walk([0, 3], [0, len(conf)], np.array(conf).reshape(-1, 2), [0, len(walk)], np.array(walk).reshape(-1, 2))
        assert '(-2)' in str(e.value) and 'is not m < k < n' in str(e.value)
    with pytest.raises(N.PepError):
        N.synteny_walk([0, 3, 2], [0, 0, 0], np.zeros((0, 2)), [0, 0, 0], np.zeros((0, 2)))


def test_walk_of_a_chain_of_a_million_merges(N):
    """A million members chained by walk pairs around one conflict pair, every merge absorbing the whole chain so far into a new root.  The lists
    come out in the reference's order.  A walk that retags or copies the absorbed component per merge, as the reference does, takes n^2 / 2 =
    5 x 10^11 steps here - minutes, where the union-find over linked lists takes milliseconds; no time is asserted."""
    n = 1000000
    walk = np.stack([np.arange(1, n - 1), np.arange(2, n)], axis=1)[::-1]          # merges (n-2, n-1), (n-3, n-2) ...: every root is absorbed by the next
    v, c = N.synteny_walk([0, n], [0, 1], [[0, 1]], [0, len(walk)], walk)
    assert v.tolist() == [2] and [r for r, _ in c[0]] == [0, 1]
    assert c[0][0][1].tolist() == [0] and np.array_equal(c[0][1][1], np.arange(1, n))


def test_flat_and_planner_are_consistent(N):
    member_off, genome, nb_off, nb = flat([([1, 1], [[1, 2], []]), ([3], [[7]])])
    assert member_off.tolist() == [0, 2, 3] and nb_off.tolist() == [0, 2, 2, 3] and nb.tolist() == [1, 2, 7] and genome.tolist() == [1, 1, 3]
    assert SY._plan([3, 1, 6, 0, 2], [1] * 5, 4) == [(0, 2), (2, 3), (3, 5)]
