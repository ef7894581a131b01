"""K26 (the front half of a round of filt_genes, PEPPAN.py:546-624 and :641-656) without a GPU: the plain-Python restatement of
tests/batchprep_helpers.py against what the reference's own filt_genes left at :546, :579, :595 and :658 of every round of the committed fixture
(tests/golden/g29_batchprep.json.gz, made by tests/golden/make_golden_batchprep.py), pep_batch_unsure_walk (host C++) against the restatement on the
fixture's rounds and on seeded random rounds, every refusal of the three device-free ..._check functions, and the K26 section of the header against
_native's constants.

The tolerance is zero: tables, flags, codes and messages are compared with ==."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batchprep_helpers as H  # noqa: E402
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
def golden():
    return H.load_golden()


def test_restatement_equals_the_reference_at_every_recorded_point(golden):
    seen = {}
    for orthology in ('nj', 'sbh'):
        assert H.check_run(golden, orthology, seen) == len(golden['runs'][orthology]['rounds']) == 3
        assert len(golden['runs'][orthology]['mat_out']) == 13
    assert not [b for b in H.BRANCHES if not seen.get(b)], seen


def library_walk(N, order, tables, conflicts, n_loci):
    """pep_batch_unsure_walk over the genes `order` -> (popped genes, gene -> the rows with column 3 > 0 as the walk left them)"""
    B = H.batch_of([(tables[g], conflicts.get(g, {})) for g in order])
    col3, popped = N.batch_unsure_walk(B['gene_off'], B['cols'][3], B['cols'][5], B['cfl_off'], B['cfl'], n_loci)
    left = {}
    for k, g in enumerate(order):
        rows = [list(r) for r in tables[g]]
        for r, x in zip(rows, col3[B['gene_off'][k]:B['gene_off'][k + 1]].tolist()):
            r[3] = x
        left[g] = [r for r in rows if r[3] > 0]
    return [g for g, p in zip(order, popped.tolist()) if p], left


def test_unsure_walk_equals_the_restatement_on_the_fixture(N, golden):
    n_loci = max(int(l) for l in golden['lists']) + 2000
    rounds = []

    def each(rnd, got):
        tables = {g: [list(r) for r in t] for g, t in got['after_a'].items()}
        popped, left = library_walk(N, got['order'], tables, got['conflicts'], n_loci)
        assert popped == got['popped']
        assert {g: t for g, t in left.items() if g not in popped} == got['after_b']
        rounds.append(len(popped))

    for orthology in ('nj', 'sbh'):
        H.check_run(golden, orthology, each=each)
    assert len(rounds) == 6 and sum(rounds) == 2                   # P is popped in round 1 of both runs


def test_unsure_walk_equals_the_restatement_on_random_rounds(N):
    n_pop = n_flip = 0
    for seed in range(20):
        rng = H.rng_of(1000 + seed)
        tables, conflicts, order, locus0 = {}, {}, [], 0
        for g in range(rng.randrange(1, 9)):
            n = rng.randrange(1, 40)
            table, _ = H.random_gene(rng, n, rng.randrange(1, n + 1), locus0, exemplar=g)
            for r in table:                                            # what stage A leaves: some rows negated
                if rng.random() < 0.25:
                    r[3] = -r[3]
            tables[g], order = table, order + [g]
            locus0 += n
        for g in order:                                                # lists that name loci of the whole round
            conflicts[g] = {r[5]: [rng.randrange(locus0) * 10 + rng.choice((0, 1, 2)) for _ in range(rng.randrange(1, 6))] for r in tables[g] if rng.random() < 0.4}
        mine = {g: [list(r) for r in t] for g, t in tables.items()}
        popped, left = library_walk(N, order, tables, conflicts, locus0)
        assert popped == H.unsure_walk(order, mine, conflicts)
        assert {g: t for g, t in left.items() if g not in popped} == {g: t for g, t in mine.items() if g not in popped}
        n_pop += len(popped)
        n_flip += sum(1 for g in order if g not in popped and any(r[3] < 0 for r in tables[g]))
    assert n_pop >= 5 and n_flip >= 20


def refusal(N, fn, *args, **kw):
    try:
        fn(*args, **kw)
    except N.PepError as err:
        m = re.match(r'pep_\w+ failed \((-?\d+)\): (.*)$', str(err), flags=re.S)
        return int(m.group(1)), m.group(2)
    return 0, ''


def test_every_refusal_of_the_checks(N):
    # two genes of 3 and 2 rows; the lists of rows 0 and 3
    ok = dict(gene_off=[0, 3, 5], genome=[1, 2, 2, 1, 3], col2=[50, 40, 30, 20, 10], col3=[9000, 8000, -7000, 9500, 9400], col4=[10000, 8888, 7777, 10000, 9894],
              locus=[5, 6, 7, 8, 5], cfl_off=[0, 2, 2, 2, 3, 3], cfl=[61, 82, 50], n_loci=9)

    def screen(**kw):
        a = dict(ok, **kw)
        return refusal(N, N.batch_screen_check, a['gene_off'], a['col3'], a['locus'], a['n_loci'])

    def walk(**kw):
        a = dict(ok, **kw)
        return refusal(N, N.batch_unsure_walk, a['gene_off'], a['col3'], a['locus'], a['cfl_off'], a['cfl'], a['n_loci'], check_only=True)

    def prune(mode=0, path=0, **kw):
        a = dict(ok, **kw)
        return refusal(N, N.batch_prune_check, mode, a['gene_off'], a['genome'], a['col2'], a['col3'], a['col4'], a['locus'], a['cfl_off'], a['cfl'], a['n_loci'], path)

    assert screen() == walk() == prune() == prune(1, 2) == (0, '')
    empty = dict(gene_off=[0], genome=[], col2=[], col3=[], col4=[], locus=[], cfl_off=[0], cfl=[])
    assert screen(**empty) == walk(**empty) == prune(**empty) == (0, '')                  # a batch of zero genes is legal
    for name, fn in (('pep_batch_screen', screen), ('pep_batch_unsure_walk', walk), ('pep_batch_prune', prune)):
        for kw, code, text in ((dict(gene_off=[1, 3, 5]), PEP_ERR_ARG, 'gene_off[0] is 1, not 0'),
                               (dict(locus=[5, 6, 7, 8, 9]), PEP_ERR_ARG, 'row 1 of gene 1 names locus 9, outside [0, 9)'),
                               (dict(locus=[5, 6, 7, 8, -1]), PEP_ERR_ARG, 'row 1 of gene 1 names locus -1, outside [0, 9)'),
                               (dict(locus=[5, 6, 5, 8, 5]), PEP_ERR_ARG, 'locus 5 comes twice in the table of gene 0'),
                               (dict(col3=[9000, 8000, -(1 << 31), 9500, 9400]), PEP_ERR_ARG, 'column 3 of row 2 of gene 0 is -2147483648, 2^31 or more in magnitude'),
                               (dict(n_loci=(1 << 40) + 1), PEP_ERR_ARG, 'n_loci 1099511627777 is more than 1099511627776')):
            assert fn(**kw) == (code, name + ': ' + text), (name, kw)
        # offsets that fall (the binding sizes the arrays by the last offset: the library is handed six rows directly)
        six = dict(gene_off=[0, 6, 5], genome=[1] * 6, col2=[1] * 6, col3=[1] * 6, col4=[1] * 6, locus=list(range(6)), cfl_off=[0] * 7, cfl=[])
        msg = C.create_string_buffer(512)
        assert getattr(N.load_library(), name + '_check')(*raw_args(name, six), msg, len(msg)) == PEP_ERR_ARG
        assert msg.value.decode() == name + ": the rows of gene 1 (from 6) overlap the next gene's (gene_off[2] = 5)"
        big = N.PREP_MAX_ROWS + 1
        kw = dict(gene_off=[0, big], genome=[0] * big, col2=[1] * big, col3=[1] * big, col4=[1] * big, locus=list(range(big)), cfl_off=[0] * (big + 1), cfl=[], n_loci=big)
        assert fn(**kw) == (PEP_ERR_LIMIT, name + ': gene 0 has 65537 rows, more than 65536')
    # stage A alone
    assert screen(col3=[9000, 8000, -7000, 0, -5]) == (PEP_ERR_ARG, 'pep_batch_screen: gene 1 has no row with column 3 above 0 (its maximum is 0)')
    assert screen(gene_off=[0, 5, 5], locus=[1, 2, 3, 4, 5]) == (PEP_ERR_ARG, 'pep_batch_screen: gene 1 has no row with column 3 above 0 (no row at all)')
    # the conflict lists, stages B and C
    for name, fn in (('pep_batch_unsure_walk', walk), ('pep_batch_prune', prune)):
        assert fn(cfl=[61, -2, 50]) == (PEP_ERR_ARG, name + ': conflict value -2 of row 0 of gene 0 names no locus of [0, 9)')
        assert fn(cfl_off=[0, 2, 1, 2, 3, 3]) == (PEP_ERR_ARG, name + ": the conflict list of row 1 of gene 0 (from 2) overlaps the next row's (cfl_off[2] = 1)")
    assert walk(cfl=[61, 90, 50]) == (PEP_ERR_ARG, 'pep_batch_unsure_walk: conflict value 90 of row 0 of gene 0 names no locus of [0, 9)')
    assert prune(cfl=[61, 90, 50]) == (0, '')                                         # (stage C ignores what names no row of the gene)
    # stage C alone
    assert prune(gene_off=[0, 5, 5], locus=[1, 2, 3, 4, 5]) == (PEP_ERR_ARG, 'pep_batch_prune: gene 1 has no rows')
    assert prune(mode=2) == (PEP_ERR_ARG, 'pep_batch_prune: mode 2 is neither PEP_PREP_NJ nor PEP_PREP_SBH')
    assert prune(path=3) == (PEP_ERR_ARG, 'pep_batch_prune: path 3 is none of PEP_PREP_AUTO, PEP_PREP_LDS, PEP_PREP_WS')
    assert prune(genome=[1, 2, 2, 1, 1 << 32]) == (PEP_ERR_ARG, 'pep_batch_prune: the genome id of row 1 of gene 1 is 4294967296, 2^32 or more in magnitude')
    assert prune(genome=[1, -2, 2, 1, 3]) == (PEP_ERR_ARG, 'pep_batch_prune: the genome id of row 1 of gene 0 is -2, below 0')
    assert prune(col4=[10000, 8888, 7777, 1 << 31, 9894]) == (PEP_ERR_ARG, 'pep_batch_prune: column 4 of row 0 of gene 1 is 2147483648, 2^31 or more in magnitude')
    n = N.PREP_LDS_ROWS + 1
    kw = dict(gene_off=[0, n], genome=[0] * n, col2=[1] * n, col3=[1] * n, col4=[1] * n, locus=list(range(n)), cfl_off=[0] * (n + 1), cfl=[], n_loci=n)
    assert prune(**kw) == prune(path=N.PREP_WS, **kw) == (0, '')
    assert prune(path=N.PREP_LDS, **kw) == (PEP_ERR_LIMIT, 'pep_batch_prune: gene 0 has 4097 rows, the LDS path takes 4096')
    # more conflict values than the budget: the offsets alone say so (no such array is made)
    lib, over = N.load_library(), (N.PREP_MAX_CFL_BYTES >> 3) + 1
    one = [np.array(x, dtype=t) for x, t in (([0, 1], np.uint64), ([3], np.int64), ([0], np.int64), ([0, over], np.uint64))]
    msg = C.create_string_buffer(512)
    rc = lib.pep_batch_unsure_walk_check(1, one[0].ctypes.data, one[1].ctypes.data, one[2].ctypes.data, one[3].ctypes.data, None, 1, msg, len(msg))
    assert rc == PEP_ERR_LIMIT and msg.value.decode() == ('pep_batch_unsure_walk: %d conflict values (8 bytes each) asked for up to row 0 of gene 0, the budget of one call is '
                                                        '2147483648 bytes (split the batch)' % over)
    # null tables
    assert lib.pep_batch_screen_check(1, None, None, None, 1, msg, len(msg)) == PEP_ERR_ARG and msg.value == b'pep_batch_screen: null table'
    assert lib.pep_batch_unsure_walk_check(1, one[0].ctypes.data, one[1].ctypes.data, one[2].ctypes.data, None, None, 1, msg, len(msg)) == PEP_ERR_ARG
    assert msg.value == b'pep_batch_unsure_walk: null table'
    with pytest.raises(ValueError):
        N.batch_screen_check([0, 3], [1, 2], [0, 1], 5)


def raw_args(name, a):
    """the arguments of a ..._check function from a dict of tables, handed to the library as they are (the binding would refuse offsets that fall)"""
    arr = {k: np.array(v, dtype=np.uint64 if k.endswith('_off') else np.int64) for k, v in a.items() if k != 'n_loci'}
    arr['cfl'] = arr['cfl'] if len(arr['cfl']) else np.zeros(1, np.int64)
    raw_args.keep = arr
    p = {k: v.ctypes.data for k, v in arr.items()}
    n = len(a['gene_off']) - 1
    if name == 'pep_batch_screen':
        return (n, p['gene_off'], p['col3'], p['locus'], 9)
    if name == 'pep_batch_unsure_walk':
        return (n, p['gene_off'], p['col3'], p['locus'], p['cfl_off'], p['cfl'], 9)
    return (0, n, p['gene_off'], p['genome'], p['col2'], p['col3'], p['col4'], p['locus'], p['cfl_off'], p['cfl'], 9, 0)


def test_null_context_is_an_argument_error(N):
    for name in ('pep_batch_screen', 'pep_batch_prune'):
        restype, *argtypes = N.SIGNATURES[name]
        assert restype is C.c_int and argtypes[0] is C.c_void_p
        assert getattr(N.load_library(), name)(*[None if t is C.c_void_p else t(0) for t in argtypes]) == PEP_ERR_ARG


def test_batchprep_section_of_the_header(N):
    """the K26 section of include/peppan_hip.h declares its six functions in this order, cites what it replaces, and its modes, paths and limits are _native's (the
    prototypes: tests/test_abi.py)"""
    hdr = open(os.path.join(ROOT, 'include', 'peppan_hip.h')).read()
    names = [name for _, name, _ in ABI._header_prototypes()]
    own = ['pep_batch_screen', 'pep_batch_screen_check', 'pep_batch_unsure_walk', 'pep_batch_unsure_walk_check', 'pep_batch_prune', 'pep_batch_prune_check']
    assert names[names.index(own[0]):][:len(own)] == own == [name for name in N.SIGNATURES if name in own]
    assert int(re.search(r'#define PEP_ABI_VERSION (\d+)', hdr).group(1)) == N.ABI_VERSION
    assert 'PEPPAN.py:546-624' in hdr
    defines = dict(re.findall(r'^#define (PEP_\w+) \(?(-?\w+)(?: << (\d+))?\)?$', hdr, flags=re.M) and
                   [(a, (b, c)) for a, b, c in re.findall(r'^#define (PEP_\w+) \(?(-?\w+)(?: << (\d+))?\)?$', hdr, flags=re.M)])
    value = lambda k: int(defines[k][0].rstrip('ul')) << int(defines[k][1] or 0)      # noqa: E731
    assert (value('PEP_PREP_NJ'), value('PEP_PREP_SBH')) == (N.PREP_NJ, N.PREP_SBH)
    assert (value('PEP_PREP_AUTO'), value('PEP_PREP_LDS'), value('PEP_PREP_WS')) == (N.PREP_AUTO, N.PREP_LDS, N.PREP_WS)
    assert value('PEP_PREP_LDS_ROWS') == N.PREP_LDS_ROWS and value('PEP_PREP_MAX_ROWS') == N.PREP_MAX_ROWS >= 65536
    assert value('PEP_PREP_MAX_CFL_BYTES') == N.PREP_MAX_CFL_BYTES and value('PEP_PREP_MAX_LOCI') == N.PREP_MAX_LOCI
