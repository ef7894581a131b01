"""K22 (genome-pair identity statistics, the reference's get_global_difference: PEPPAN.py:1611-1666) without a GPU: the restatement of
tests/globaldiff_helpers.py against what the reference's own function returned for the committed fixture (tests/golden/g22_globaldiff.json.gz, made by
tests/golden/make_golden_globaldiff.py), the host walk of the library (pep_global_diff_walk) against the restated walk, the logarithm table, the
device-free checks of pep_global_diff, and the K22 section of the header against _native's constants.

The tolerance is zero: keys, order and every float bit.  The oracle is the reference's function; every float operation of the restated sums is an IEEE
add, subtract, multiply or divide."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import globaldiff_helpers as H  # noqa: E402
import test_abi as ABI  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEP_ERR_ARG, PEP_ERR_LIMIT = -2, -3


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


@pytest.fixture(scope='module')
def cases():
    cases = H.load_cases()
    assert [c['name'] for c in cases] == ['families 11', 'families 12', 'star', 'chain', 'bsn after pop', 'exact counts', 'ties', 'nothing', 'big']
    return cases


def test_restatement_is_the_reference_on_every_fixture_case(cases):
    """keys, order, every float bit; and the fixture still holds what it is pinned by: a key of every size class around numpy's 8, 128 and 8192"""
    counts = []
    for c in cases:
        rows, n = H.restated(c['geneGroups'], c['clu'], c['bsn'], c['geneInGenomes'], c['nGene'])
        assert H.same_rows(rows, c['rows']), c['name']
        assert c['shape'] == ((len(rows), 2) if rows else (0, 0)), c['name']
        counts += n
    for lo, hi in ((1, 1), (2, 7), (8, 8), (9, 127), (128, 128), (129, 8192), (8193, 1 << 40), (16385, 1 << 40)):
        assert any(lo <= n <= hi for n in counts), (lo, hi)


def test_the_buffer_rule_is_what_the_fixture_tells_apart(cases):
    """the recorded mean of some key of `big` beyond one buffer is neither a running sum's nor one pairwise sum's over the whole list"""
    c = cases[-1]
    sel_clu, sel_bsn = H.select_rows(c['geneGroups'], c['clu'], c['bsn'], c['geneInGenomes'], c['nGene'])
    events, arena, genomes = H.walk(sel_clu, sel_bsn, c['geneInGenomes'])
    lists = H.items_by_key(events, arena)
    assert max(len(codes) for codes in lists.values()) > 2 * H.BUFFER
    told_apart = 0
    for key, codes in lists.items():
        if len(codes) <= H.BUFFER:
            continue
        x = H.log_table()[np.array(codes)]
        want = dict(c['rows'])[(int(genomes[key[0]]), int(genomes[key[1]]))][0]
        plain = np.float64(0.)
        for v in x:
            plain = plain + v
        assert H.tail(*H.two_means(x))[0] == want
        told_apart += H.tail(plain / len(x), 0.)[0] != want and H.tail(H.pairwise(x) / len(x), 0.)[0] != want
    assert told_apart >= 1


def test_numpy_sum_restated_is_np_mean():
    rng = np.random.default_rng(5)
    table = H.log_table()
    for n in (1, 7, 8, 9, 127, 128, 129, 1000, 8192, 8193, 20000, 40000):
        x = table[rng.integers(0, 10001, n)]
        m, v = H.two_means(x)
        assert m == np.mean(x) and v == np.mean((x - m) ** 2), n


def test_log_table_is_the_reference_s_logarithm():
    from peppan_amd import globaldiff as GD
    table = GD.log_table()
    assert table.dtype == np.float64 and len(table) == 10050 and np.array_equal(table, H.log_table()) and np.isfinite(table).all()
    rng = np.random.default_rng(9)
    for n in (1, 2, 3, 8, 9, 100, 4097):
        data = rng.integers(0, 10050, n).tolist()
        assert np.array_equal(table[np.array(data)], np.log(1.005 - np.array(data) / 10000.))
    assert np.array_equal(table, np.log(1.005 - np.array(list(range(10050))) / 10000.))


def walks_agree(N, clu, bsn, genes):
    ids = sorted(genes)
    events, arena, genomes = N.global_diff_walk(clu, bsn, ids, [genes[g] for g in ids])
    want = H.walk(clu, bsn, genes)
    assert np.array_equal(events, want[0]) and np.array_equal(arena, want[1]) and np.array_equal(genomes, want[2])
    return events, arena, genomes


def test_walk_is_the_restated_walk_on_every_fixture_case(N, cases):
    for c in cases:
        sel_clu, sel_bsn = H.select_rows(c['geneGroups'], c['clu'], c['bsn'], c['geneInGenomes'], c['nGene'])
        events, arena, genomes = walks_agree(N, sel_clu, sel_bsn, c['geneInGenomes'])
        assert len(events) == len(sel_clu) + len(sel_bsn), c['name']
        N.global_diff_check(events, arena, len(genomes))


def test_walk_quirks_one_at_a_time(N):
    genes = {1: 5, 2: -1, 3: 7, 4: 5, 5: 9}
    # get(r, [r]) looks up the key itself: 2 sits in 1's list, a row of r = 2 still starts from [2]
    ev, arena, genomes = walks_agree(N, [[1, 2, 9000], [2, 3, 8000]], [], genes)
    assert genomes.tolist() == [-1, 5, 7, 9] and ev[1, 1] == 1 and arena[ev[1, 0]] == 0
    # pop(q, [q]): 1's list goes to 3, then 1 returns as r and starts from [1]
    ev, arena, _ = walks_agree(N, [[1, 2, 9000], [3, 1, 8000], [1, 4, 7000]], [], genes)
    assert ev[:, [1, 3]].tolist() == [[1, 1], [1, 2], [1, 1]]
    # r == q in the clu phase meets its own list and doubles it
    ev, arena, _ = walks_agree(N, [[1, 2, 9000], [1, 1, 10000], [1, 3, 8000]], [], genes)
    assert ev[1].tolist()[:4] == [ev[1, 0], 2, ev[1, 0], 2] and ev[2, 1] == 4
    # r == q without a list: two lists [r]
    ev, arena, _ = walks_agree(N, [[1, 1, 10000], [1, 2, 9000]], [], genes)
    assert ev[0, 0] != ev[0, 2] and ev[1, 1] == 2
    # the bsn phase pops q's list and writes nothing back, r's list is not stored
    ev, arena, _ = walks_agree(N, [[1, 2, 9000], [3, 4, 8000]], [[1, 3, 7000], [1, 3, 6000], [1, 1, 5000], [1, 5, 4000]], genes)
    assert ev[2:, [1, 3, 5]].tolist() == [[2, 2, 1], [2, 1, 1], [2, 2, 1], [1, 1, 1]]
    # nothing at all
    ev, arena, genomes = walks_agree(N, [], [], {})
    assert ev.shape == (0, 6) and len(arena) == 0 and len(genomes) == 0


def test_walk_is_the_restated_walk_on_random_rows(N):
    """few reps, many rows: lists that grow in place at the arena's end, lists that move, lists with room left, self rows, pops and returns in any order"""
    rng = np.random.default_rng(31)
    for n_genes, n_clu, n_bsn in ((4, 30, 10), (12, 80, 30), (40, 200, 60), (40, 200, 0)):
        genes = {int(g): int(rng.integers(-1, 6)) for g in range(100, 100 + n_genes)}
        ids = sorted(genes)
        clu = [[int(rng.choice(ids[:4])), int(rng.choice(ids)), int(rng.integers(0, 10050))] for _ in range(n_clu)]
        clu = [[r, q if r != q or k % 8 == 0 else ids[-1], v] for k, (r, q, v) in enumerate(clu)]          # (every self row doubles a list: keep them few)
        bsn = [[int(rng.choice(ids)), int(rng.choice(ids)), int(rng.integers(0, 10050))] for _ in range(n_bsn)]
        events, arena, _ = walks_agree(N, clu, bsn, genes)
        assert len(arena) < 1 << 22 and int(events[:, 1].max()) > 4


def test_walk_refusals(N):
    genes = {1: 0, 2: 1}
    with pytest.raises(N.PepError, match=r'\(-2\).*gene 77 of clu row 1 is not in the gene -> genome map'):
        N.global_diff_walk([[1, 2, 9000], [1, 77, 9000]], [], [1, 2], [0, 1])
    with pytest.raises(N.PepError, match=r'\(-2\).*gene 78 of bsn row 0'):
        N.global_diff_walk([[1, 2, 9000]], [[78, 1, 500]], [1, 2], [0, 1])
    with pytest.raises(N.PepError, match=r'\(-2\).*clu row 0 has the value 10050'):
        N.global_diff_walk([[1, 2, 10050]], [], [1, 2], [0, 1])
    with pytest.raises(N.PepError, match=r'\(-2\).*bsn row 1 has the value -1'):
        N.global_diff_walk([], [[1, 2, 10049], [1, 2, -1]], [1, 2], [0, 1])
    with pytest.raises(N.PepError, match='not strictly ascending'):
        N.global_diff_walk([], [], [2, 1], [0, 1])
    with pytest.raises(ValueError):
        N.global_diff_walk([], [], [1, 2], [0])
    assert len(N.global_diff_walk([[1, 2, 10049]], [], [1, 2], [0, 1])[0]) == 1 and H.walk([[1, 2, 10049]], [], genes)[0][0, 4] == 10049


def check(N, events, arena, n_genomes, chunk_items=0):
    msg = C.create_string_buffer(512)
    ev, ar = np.array(events, dtype=np.int64).reshape(-1, 6), np.array(arena, dtype=np.int32)
    rc = N.load_library().pep_global_diff_check(N._ptr_or_null(ev), len(ev), N._ptr_or_null(ar), len(ar), n_genomes, chunk_items, msg, len(msg))
    return rc, msg.value.decode()


def test_every_refusal_of_the_device_free_check(N):
    assert check(N, [[0, 2, 1, 2, 9000, 0]], [0, 1, 2], 3) == (0, '')
    assert check(N, [], [], 0) == (0, '') and check(N, [], [], 16384) == (0, '')
    rc, msg = check(N, [], [], 16385)
    assert rc == PEP_ERR_LIMIT and '16385 genomes' in msg
    # two events of 2^16 x 2^16 items over one list of 2^16 entries: 2^33 items, nothing large is allocated
    arena = np.zeros(1 << 16, dtype=np.int32)
    rc, msg = check(N, [[0, 1 << 16, 0, 1 << 16, 1, 0]] * 2, arena, 1)
    assert rc == PEP_ERR_LIMIT and '%d items' % (1 << 33) in msg and str(N.GDIFF_MAX_ITEMS) in msg
    assert check(N, [[0, 1 << 16, 0, 1 << 16, 1, 0]], arena, 1)[0] == 0                 # 2^32 items are within the limit
    rc, msg = check(N, [[0, 1 << 16, 0, 1 << 16, 1, 0], [0, 1, 0, 1, 1, 1]], arena, 1)
    assert rc == PEP_ERR_LIMIT and '%d items' % ((1 << 32) + 1) in msg
    # the workspace: 2^32 items over the largest key table
    rc, msg = check(N, [[0, 1 << 16, 0, 1 << 16, 1, 0]], arena, 16384)
    assert rc == PEP_ERR_LIMIT and 'bytes of workspace' in msg and str(N.GDIFF_MAX_BYTES) in msg and '%d items' % (1 << 32) in msg
    rc, msg = check(N, [[0, 1, 0, 1, 10050, 0]], [0], 1)
    assert rc == PEP_ERR_ARG and 'event 0 has the value 10050' in msg
    rc, msg = check(N, [[0, 1, 0, 1, 5, 0], [0, 1, 0, 1, -1, 0]], [0], 1)
    assert rc == PEP_ERR_ARG and 'event 1 has the value -1' in msg
    rc, msg = check(N, [[0, 1, 1, 1, 5, 0]], [0], 1)
    assert rc == PEP_ERR_ARG and 'event 0 names entries 1 .. 1 + 1 of an arena of 1' in msg
    rc, msg = check(N, [[0, 0, 0, 1, 5, 0]], [0], 1)
    assert rc == PEP_ERR_ARG and 'a list of 0 entries' in msg
    rc, msg = check(N, [[0, 1, 0, 1, 5, 2]], [0], 1)
    assert rc == PEP_ERR_ARG and 'drop_same = 2' in msg
    rc, msg = check(N, [[0, 1, 0, 1, 5, 0]], [0, 3], 3)
    assert rc == PEP_ERR_ARG and 'arena entry 1 is 3' in msg
    rc, msg = check(N, [[0, 1, 0, 1, 5, 0]], [0], 1, (1 << 26) + 1)
    assert rc == PEP_ERR_ARG and 'chunk_items' in msg
    with pytest.raises(N.PepError, match='16385 genomes'):
        N.global_diff_check([], [], 16385)
    with pytest.raises(ValueError):
        N.global_diff_check([[0, 1, 0, 1, 5]], [0], 1)


def test_null_handles_are_argument_errors(N):
    lib = N.load_library()
    for name in ('pep_global_diff', 'pep_global_diff_copy'):
        restype, *argtypes = N.SIGNATURES[name]
        assert restype is C.c_int and argtypes[0] is C.c_void_p
        assert getattr(lib, name)(*[None if t is C.c_void_p else t(0) for t in argtypes]) == PEP_ERR_ARG, name
    assert lib.pep_global_diff_walk(None, 0, None, 0, None, None, 0, None, None, 0) == PEP_ERR_ARG
    assert lib.pep_global_diff_walk_size(None, None, None, None) == PEP_ERR_ARG
    lib.pep_global_diff_walk_free(None)


def test_globaldiff_section_of_the_header(N):
    """the K22 section of include/peppan_hip.h declares its seven functions in this order, cites what it replaces, and its limits are _native's (the prototypes:
    tests/test_abi.py)"""
    hdr = open(os.path.join(ROOT, 'include', 'peppan_hip.h')).read()
    names = [name for _, name, _ in ABI._header_prototypes()]
    own = ['pep_global_diff_walk', 'pep_global_diff_walk_size', 'pep_global_diff_walk_copy', 'pep_global_diff_walk_free', 'pep_global_diff', 'pep_global_diff_copy',
           'pep_global_diff_check']
    assert names[names.index(own[0]):][:len(own)] == own == [name for name in N.SIGNATURES if name in own]
    for define, value in (('PEP_GDIFF_MAX_GENOMES', N.GDIFF_MAX_GENOMES), ('PEP_GDIFF_TABLE', N.GDIFF_TABLE)):
        assert int(re.search(r'#define %s (\d+)\b' % define, hdr).group(1)) == value
    for define, value in (('PEP_GDIFF_MAX_ITEMS', N.GDIFF_MAX_ITEMS), ('PEP_GDIFF_CHUNK_ITEMS', N.GDIFF_CHUNK_ITEMS), ('PEP_GDIFF_MAX_BYTES', N.GDIFF_MAX_BYTES)):
        assert re.search(r'#define %s \(1u(?:ll)? << (\d+)\)' % define, hdr).group(1) == str(value.bit_length() - 1)
    assert int(re.search(r'#define PEP_ABI_VERSION (\d+)', hdr).group(1)) == N.ABI_VERSION
    assert 'PEPPAN.py:1611-1666' in hdr


def test_the_returned_array_feeds_gd_table(cases):
    """the [k, 2] object array get_global_difference returns goes into orthofilter.gd_table unchanged (here: built from the fixture's rows as the public
    function builds it), and gives what the dict of the same rows gives"""
    from peppan_amd import orthofilter as OF
    c = cases[2]                                            # (star: 781 keys, no genome -1, which gd_table does not take)
    arr = np.empty((len(c['rows']), 2), dtype=object)
    for k, (key, val) in enumerate(c['rows']):
        arr[k, 0], arr[k, 1] = key, (np.float64(val[0]), np.float64(val[1]))
    a, b = OF.gd_table(arr, 0.005, 3.), OF.gd_table(dict(c['rows']), 0.005, 3.)
    assert len(a.keys) == len(c['rows']) and np.array_equal(a.keys, b.keys) and np.array_equal(a.vals, b.vals)
