"""K20 on the GPU: Context.rarefaction_curves, Context.profile_pairs and peppan_amd.panparser against what was recorded from the reference's own writeCurve,
writeCGAV and getDistance (tests/golden/g25_parser.json.gz) and against the independent restatement in plain Python loops (tests/parser_helpers.py).  Every
comparison is ==: both kernels count, and the floats are made on the host from exact counts by the reference's expressions.

The sizes are the smallest at which csrc/parser.hip takes another path: a word is 64 genes, a slice of the walk 65 536 genes (1 024 words, four per lane of a
256-lane workgroup), a chunk of its per-step array 2 048 genomes; a tile of pairs is 64 x 64 profiles, staged 16 genes at a time."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from peppan_amd import panparser as PP  # noqa: E402  (pure Python: the library is loaded on first use)
from parser_helpers import (groups_of_case, load_g25, presence_of_groups, random_orders, random_presence, random_profiles, restate_curves,  # noqa: E402
                            restate_pairs)

pytestmark = pytest.mark.gpu

SLICE_GENES = 65536
CHUNK_STEPS = 2048


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


@pytest.fixture(scope='module')
def g25():
    return load_g25()


@pytest.fixture(scope='module')
def ctx(N):
    with N.Context(0) as c:
        yield c


def curves_of(N, ctx, P, orders):
    got = ctx.rarefaction_curves(N.pack_presence(P), P.shape[1], orders)
    assert got.dtype == np.int64 and got.shape == (P.shape[0], len(orders), 2)
    return got.tolist()


def test_every_recorded_curve(N, ctx, g25):
    for c in g25['cases']:
        P = np.array(presence_of_groups(groups_of_case(c)))
        assert curves_of(N, ctx, P, c['orders']) == c['curves'], c['name']


@pytest.mark.parametrize('n_genes', [1, 63, 64, 65, 127, 128, 129, 2 * SLICE_GENES + 77])
def test_curves_at_every_word_edge(N, ctx, n_genes):
    """5 genomes: one with every gene, one with the last gene alone, which every genome has; three orders"""
    rng = np.random.default_rng(2530 + n_genes % 1000)
    P = random_presence(rng, 5, n_genes)
    P[1] = 1
    P[3] = 0
    P[3, -1] = 1
    P[:, -1] = 1
    orders = [[3, 1, 0, 2, 4], [0, 2, 4, 1, 3], [1, 3, 0, 2, 4]]
    want = restate_curves(P, orders)
    assert curves_of(N, ctx, P, orders) == want
    assert want[0][0] == [1, 1] and want[1][0] == [n_genes, 1] and want[0][2] == [n_genes, n_genes] and want[4][1] == [n_genes, 1]
    # the padding of the last word never counts, whatever the words in front of it hold
    full = np.ones((2, n_genes), np.uint8)
    assert curves_of(N, ctx, full, [[0, 1]]) == [[[n_genes, n_genes]], [[n_genes, n_genes]]]


@pytest.mark.parametrize('n_genomes,n_genes,n_iter', [(1, 70, 1), (2, 70, 7), (65, 70, 3), (257, 130, 7), (CHUNK_STEPS + 1, 70, 2), (CHUNK_STEPS + 1, SLICE_GENES + 5, 1)])
def test_curves_at_every_genome_count(N, ctx, n_genomes, n_genes, n_iter):
    rng = np.random.default_rng(2540 + n_genomes)
    if n_genes > SLICE_GENES:                                                 # sparse, so that the plain-loop restatement stays quick: a hundred genes per genome
        P = (rng.random((n_genomes, n_genes)) < 0.002).astype(np.uint8)
        P[:, SLICE_GENES + 1] = 1
    else:
        P = random_presence(rng, n_genomes, n_genes, core=0.1, shell=0.2)
        P[:, 3] = 1                                                           # in every genome: core never drops below 1
        P[:, 5] = 0
        P[n_genomes // 2, 5] = 1                                              # in exactly one genome
    orders = random_orders(rng, n_genomes, n_iter)
    want = restate_curves(P, orders)
    assert curves_of(N, ctx, P, orders) == want
    assert all(row[-1] >= 1 for row in want[-1])


def test_walk_whose_and_empties_and_or_fills_at_once(N, ctx):
    """two complementary genomes first: from the second step on every delta of the walk is zero - the path that skips the reduction - for 300 steps, in an order
    beside one that keeps changing to its end"""
    rng = np.random.default_rng(2550)
    P = random_presence(rng, 300, 200, core=0., shell=0.6)
    P[0] = np.arange(200) % 2
    P[1] = 1 - P[0]
    late = np.arange(300)[::-1].copy()
    orders = np.array([np.arange(300), late], dtype=np.uint32)
    want = restate_curves(P.tolist(), orders)
    assert want[1][0] == [200, 0] and want[299][0] == [200, 0] and want[1][1] != [200, 0]
    assert curves_of(N, ctx, P, orders) == want


def test_buffers_regrow_between_calls_of_one_context(N, g25):
    before = N.live_resources()
    rng = np.random.default_rng(2560)
    small = random_presence(rng, 3, 10)
    large = random_presence(rng, 70, 700)
    with N.Context(0) as c:
        for P, n_iter in ((small, 2), (large, 9), (small, 1), (large, 9)):
            orders = random_orders(rng, len(P), n_iter)
            assert curves_of(N, c, P, orders) == restate_curves(P.tolist(), orders)
        for prof in (random_profiles(rng, 3, 5), random_profiles(rng, 70, 40), random_profiles(rng, 2, 3)):
            shared, presence = c.profile_pairs(prof)
            assert (shared.tolist(), presence.tolist()) == restate_pairs(prof.tolist())
        c.set_timing(2)
        orders = random_orders(rng, 70, 9)
        c.rarefaction_curves(N.pack_presence(large), 700, orders)
        ms_curves, ms_pairs, up, down = c.parser_times()
        assert ms_curves > 0 and up == 70 * 11 * 8 + 9 * 70 * 4 and down == 70 * 9 * 8
        c.profile_pairs(random_profiles(rng, 70, 40))
        ms_curves_2, ms_pairs, up, down = c.parser_times()
        assert ms_pairs > 0 and ms_curves_2 == ms_curves and up == 70 * 40 * 4 and down == 2 * 70 * 70 * 4
        c.set_timing(0)
        c.profile_pairs(random_profiles(rng, 70, 40))
        assert c.parser_times()[1] == 0.
        assert N.live_resources()[0] > before[0]
    assert N.live_resources() == before


def test_refused_calls_leave_the_context_usable(N, ctx):
    P = np.ones((3, 70), np.uint8)
    bits = N.pack_presence(P)
    with pytest.raises(N.PepError) as e:
        ctx.rarefaction_curves(bits, 70, [[0, 1, 1]])
    assert '(-2)' in str(e.value) and 'names genome 1 again' in str(e.value)
    spoiled = bits.copy()
    spoiled[1, 1] |= np.uint64(1 << 40)
    with pytest.raises(N.PepError) as e:
        ctx.rarefaction_curves(spoiled, 70, [[0, 1, 2]])
    assert '(-2)' in str(e.value) and 'padding bit' in str(e.value)
    with pytest.raises(N.PepError) as e:
        ctx.profile_pairs(np.zeros((3, 0), np.int32))
    assert '(-2)' in str(e.value)
    with pytest.raises(ValueError):
        ctx.profile_pairs(np.array([[2 ** 31]]))
    assert curves_of(N, ctx, P, [[0, 1, 2]]) == [[[70, 70]]] * 3
    assert [m.tolist() for m in ctx.profile_pairs([[1, 2, 0], [1, 3, 0]])] == [[[0, 1], [1, 0]], [[0, 2], [2, 0]]]


def _same_file(text, want, same_scipy):
    if same_scipy:
        return text == want
    keep = lambda t: [ln for k, ln in enumerate(t.splitlines(True)) if k not in (4, 5, 6)]    # noqa: E731  (the three curve_fit lines)
    return keep(text) == keep(want)


def test_writecurve_writes_the_recorded_file(g25, tmp_path):
    import scipy
    c = next(c for c in g25['cases'] if c['name'] == 'gff_cds')
    groups = groups_of_case(c)
    np.random.seed(c['seed'])
    assert PP.rarefaction_curves(groups, c['n_iter']).tolist() == c['curves']
    assert PP.rarefaction_curves(groups, orders=c['orders']).tolist() == c['curves']
    prefix = str(tmp_path / 'out')
    np.random.seed(c['seed'])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        summary = PP.writeCurve(prefix, groups, c['pseudogene'], c['n_iter'])
    assert summary.shape == (len(groups), 2, 5) and not summary.any()
    assert _same_file(open(prefix + '_content.curve').read(), c['curve_text'], scipy.__version__ == g25['scipy'])
    tiny = next(c for c in g25['cases'] if c['n_iter'] == 1000)              # the default n_iter
    np.random.seed(tiny['seed'])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        PP.writeCurve(prefix + '2', groups_of_case(tiny))
    assert _same_file(open(prefix + '2_content.curve').read(), tiny['curve_text'], scipy.__version__ == g25['scipy'])
    PP.close()


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 130])
def test_pairs_at_every_tile_edge(N, ctx, n):
    rng = np.random.default_rng(2570 + n)
    for n_genes in (1, 15, 16, 17, 63, 64, 65):
        prof = random_profiles(rng, n, n_genes)
        if n > 2:
            prof[0] = 0                                                       # no allele at all
            prof[1] = -np.abs(prof[2]) - 1                                    # negatives, equal to nothing
            prof[n - 1] = prof[n - 2]                                         # identical rows
        shared, presence = ctx.profile_pairs(prof)
        assert shared.dtype == presence.dtype == np.int32 and shared.shape == presence.shape == (n, n)
        assert (shared.tolist(), presence.tolist()) == restate_pairs(prof.tolist()), n_genes
        if n > 2:
            assert not shared[0].any() and not presence[1].any() and shared[n - 1, n - 2] == presence[n - 1, n - 2]


def test_getdistance_is_the_drop_in(g25):
    for p in g25['pairs']:
        got = PP.getDistance(np.array(p['profiles']))
        assert got.dtype == np.float64 and [[v.hex() for v in row] for row in got.tolist()] == p['dist_hex'], p['name']
    first = PP.getDistance(np.array(g25['pairs'][0]['profiles']))
    assert first[3, 0] == first[5, 6] == -np.log(0.5) and not np.diag(first).any()
    PP.close()


def test_writecgav_writes_the_recorded_files(g25, tmp_path):
    for c in g25['cases']:
        if not c['cgav']['profiles'][0]:
            continue                                                          # (no gene reaches pCore: counted on the host, test_parser_host.py)
        prefix = str(tmp_path / c['name'])
        PP.writeCGAV(prefix, groups_of_case(c), c['cgav']['pCore'])
        assert open(prefix + '_CGAV.profile').read() == c['cgav']['profile_text'], c['name']
        assert open(prefix + '_CGAV.dist').read() == c['cgav']['dist_text'], c['name']
    PP.close()
