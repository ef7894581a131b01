"""K24 (the allele pass of write_output, PEPPAN.py:1391-1472) without a GPU: the restatement of tests/outalleles_helpers.py against what the reference's own
write_output did for the committed fixture (tests/golden/g27_outalleles.json.gz, made by tests/golden/make_golden_outalleles.py), the tables
peppan_amd.outalleles makes of a prediction table, every refusal of the device-free pep_out_alleles_check, and the K24 section of the header against
_native's constants.

The tolerance is zero: tables, dictionaries, their order, codes and messages are compared with ==."""
import copy
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outalleles_helpers as H  # noqa: E402
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
def fx():
    fx = H.load()
    assert [c['name'] for c in fx['small']] == [name for name, _, _ in H.SMALL_CASES] and fx['two_batch']['n_rows'] == H.TWO_BATCH_ROWS
    return fx


def test_restatement_is_the_reference_on_every_small_case(fx):
    for case in fx['small']:
        genomes, encodes, clust_ref = H.dictionaries_of(case)
        table = copy.deepcopy(case['before'])
        alleles, rows = H.restate(table, genomes, encodes, clust_ref, case['pseudogene'], case['gtable'])
        assert table == case['after'], case['name']
        assert [[g, list(a.items())] for g, a in alleles.items()] == [[g, [tuple(x) for x in a]] for g, a in case['alleles']], case['name']
        sent = {x['pid']: x for x in case['sent']}
        assert sorted(sent) == [i for i, r in enumerate(rows) if r and r['sent']]
        for i, x in sent.items():
            assert (rows[i]['s2'], rows[i]['e2'], rows[i]['lp']) == (x['s2'], x['e2'], x['lp']), (case['name'], i)


def test_small_cases_are_rebuilt_by_the_helpers(fx):
    # the builders are deterministic: what the fixture recorded belongs to the cases as they are built today
    for case in fx['small']:
        inputs = H.small_case(case['name']).inputs()
        assert {str(k): list(v) for k, v in inputs['genomes'].items()} == case['genomes'] and inputs['encodes'] == case['encodes']


def test_restatement_is_the_reference_across_a_batch_boundary(fx):
    tb = fx['two_batch']
    case = H.two_batch_case(tb['seed'])
    inputs = case.inputs()
    table = H.table_of(case)
    assert len(table) == tb['n_rows'] >= H.BATCH + 6
    stale = copy.deepcopy(table)
    alleles, rows = H.restate(table, inputs['genomes'], inputs['encodes'], inputs['clust_ref'], tb['pseudogene'], tb['gtable'])
    assert [[r[9], r[10], r[13], r[15]] for r in table] == tb['cols']
    assert [[g, [[len(s), i] for s, i in a.items()]] for g, a in alleles.items()] == tb['alleles'] and H.allele_digest(alleles) == tb['allele_sha1']
    assert sum(1 for r in rows if r and r['sent']) == tb['sent']
    # the write-back shows: in one batch of the whole table at least one '-' head row gets another window
    one = H.restate(stale, inputs['genomes'], inputs['encodes'], inputs['clust_ref'], tb['pseudogene'], tb['gtable'], batch=len(stale))[1]
    moved = [i for i in range(H.BATCH, H.BATCH + 5) if rows[i] and one[i]['s2'] != rows[i]['s2']]
    assert len(moved) == tb['heads_moved'] >= 1 and all(table[i][11] == '-' for i in moved)


def test_tables_of_a_prediction_table(N, fx):
    from peppan_amd import outalleles as OA
    case = fx['small'][0]
    genomes, encodes, clust_ref = H.dictionaries_of(case)
    before = case['before']
    T = OA.tables(H.as_object_table(before), genomes, encodes, clust_ref, case['pseudogene'])
    names = []
    for r in before:
        if r[15] != 'misc_feature' and r[0] not in names:
            names.append(r[0])
    assert T.gene_names == names and T.seeded == [g in encodes and encodes[g] in clust_ref for g in names]
    rows = T.rows
    assert rows.shape == (len(before), N.OUTA_COLS)
    for i, r in enumerate(before):
        assert T.gene_names[rows[i, N.OUTA_GENE]] == r[0]
        assert rows[i, N.OUTA_S:N.OUTA_CLEN + 1].tolist() == [r[9], r[10], r[1], r[7], r[8], r[12], r[13]]
        assert rows[i, N.OUTA_VARY] == int(r[12] * (1 - case['pseudogene']) + 0.01)
        assert rows[i, N.OUTA_FLAGS] == (N.OUTA_SECONDARY if r[4] else 0) + (N.OUTA_MINUS if r[11] != '+' else 0)
        lo, hi = T.contig_off[rows[i, N.OUTA_CONTIG]], T.contig_off[rows[i, N.OUTA_CONTIG] + 1]
        assert T.nt[int(lo):int(hi)].decode() == genomes[encodes[r[5]]][1]
        base = r[0].rsplit('/', 2)[0]
        if base in encodes and encodes[base] in clust_ref:
            x = case['pseudogene'] * len(clust_ref[encodes[base]])
            assert all((n < x) == (n < rows[i, N.OUTA_SVMIN]) for n in range(0, 2 * len(clust_ref[encodes[base]])))
        else:
            assert rows[i, N.OUTA_SVMIN] == 0
    for g, name in enumerate(T.gene_names):
        c = T.seed_contig[g]
        assert (c >= 0) == T.seeded[g]
        if c >= 0:
            assert T.nt[int(T.contig_off[c]):int(T.contig_off[c + 1])].decode() == clust_ref[encodes[name]]
    assert N.out_alleles_check(T.contig_off, T.seed_contig, rows) is None
    assert OA.rc('acgTNRx-') == H.reverse_complement('acgTNRx-') == 'NNNNACGT'
    with pytest.raises(ValueError):
        OA._ascii('ACGß', 'contig')


def check(N, contig_off, seed_contig, rows, look9=None, key_bits=0):
    msg = C.create_string_buffer(512)
    off, seeds = np.array(contig_off, dtype=np.uint64), np.array(seed_contig, dtype=np.int32)
    table = np.array(rows, dtype=np.int32).reshape(-1, N.OUTA_COLS)
    look = None if look9 is None else np.array(look9, dtype=np.int32)
    rc = N.load_library().pep_out_alleles_check(N._ptr(off), len(off) - 1, len(seeds), N._ptr_or_null(seeds), len(table), N._ptr_or_null(table.reshape(-1)),
                                                None if look is None else N._ptr(look), key_bits, msg, len(msg))
    return rc, msg.value.decode()


def row(N, s, e, contig=0, gene=0, flags=0, part=1, q_lo=1, q_hi=None, ref_len=None, clen=1000, vary=None, svmin=0):
    ref_len = e - s + 1 if ref_len is None else ref_len
    return [gene, contig, flags, s, e, part, q_lo, ref_len if q_hi is None else q_hi, ref_len, clen, ref_len // 5 if vary is None else vary, svmin]


def test_every_refusal_of_the_device_free_check(N):
    M, NONAME, MINUS = N.OUTA_MISC, N.OUTA_NONAME, N.OUTA_MINUS
    ok = row(N, 101, 190)
    assert check(N, [0, 1000], [-1], [ok]) == (0, '') and check(N, [0], [], []) == (0, '') and check(N, [0, 1000, 1090], [1], [ok, row(N, 301, 390, flags=MINUS)]) == (0, '')
    # a skipped row is not looked at beyond its contig index
    assert check(N, [0, 1000], [-1], [row(N, -5, -9, gene=77, flags=M), row(N, 0, 0, gene=-3, flags=NONAME)]) == (0, '')
    for bad, text in ((row(N, 0, 90), 'row 1 starts before its contig (s 0, e 90)'),
                      (row(N, 101, 99), 'row 1 ends before it starts (s 101, e 99)'),
                      (row(N, 950, 1001), 'row 1 leaves its contig of 1000 bytes (s 950, e 1001)'),
                      (row(N, 101, 190, q_lo=0), 'row 1 has column 7 = 0, below 1'),
                      # '-' with column 13 below e: lp = e2 - e < 0
                      (row(N, 101, 190, flags=MINUS, clen=150), "the window of row 1 starts inside its region: the reference's slice would wrap (s 101, e 190)"),
                      # no neighbour and column 8 far beyond column 12: 600 + col12 - col8 < 0 moves the far end across the near one, on either strand
                      (row(N, 101, 190, q_hi=1500), 'the window of row 1 ends before it starts (s 101, e 190)'),
                      (row(N, 101, 190, q_hi=1500, flags=MINUS), 'the window of row 1 ends before it starts (s 101, e 190)'),
                      # column 13 beyond the actual contig
                      (row(N, 901, 990, clen=1300), 'the window of row 1 leaves its contig of 1000 bytes (s 901, e 990)')):
        rc, msg = check(N, [0, 1000], [-1], [row(N, 1, 0, flags=M), bad])
        assert rc == PEP_ERR_ARG and msg == 'pep_out_alleles: ' + text, (rc, msg)
    # '+' with column 13 below e: rp < 0, a shorter allele, legal
    assert check(N, [0, 1000], [-1], [row(N, 101, 190, clen=150)]) == (0, '')
    # '+' with a nested neighbour: e2 < s2 - 1 is no window
    rc, msg = check(N, [0, 5000], [-1], [row(N, 2000, 2999, clen=5000), row(N, 2001, 1999, clen=5000, flags=M), row(N, 1200, 1300, clen=5000, ref_len=101, part=2)])
    assert rc == PEP_ERR_ARG and msg == 'pep_out_alleles: the window of row 0 ends before it starts (s 2000, e 2999)'
    # the head of a batch looks at look9, every other row at the rows themselves
    table = [row(N, 10 + 100 * i, 99 + 100 * i, clen=2000000, flags=MINUS) for i in range(N.OUTA_BATCH + 2)]
    off = [0, 2000000]
    assert check(N, off, [-1], table)[0] == 0
    look = [r[N.OUTA_S] for r in table]
    look[N.OUTA_BATCH - 5] += 2000000                                   # seen by row OUTA_BATCH alone: its s2 lands beyond its e
    rc, msg = check(N, off, [-1], table, look9=look)
    assert rc == PEP_ERR_ARG and 'the window of row %d ends before it starts' % N.OUTA_BATCH in msg
    look[N.OUTA_BATCH - 5] -= 2000000
    look[N.OUTA_BATCH - 4] += 2000000                                   # the farthest of row OUTA_BATCH + 1, but of its own batch's reach only through row OUTA_BATCH - 4: updated
    rc, msg = check(N, off, [-1], table, look9=look)
    assert rc == PEP_ERR_ARG and 'the window of row %d ends before it starts' % (N.OUTA_BATCH + 1) in msg
    look[N.OUTA_BATCH - 4] -= 2000000
    look[N.OUTA_BATCH - 6] += 2000000                                   # out of every head's reach
    look[N.OUTA_BATCH + 1] += 2000000                                   # of the heads' own batch: not read
    assert check(N, off, [-1], table, look9=look) == (0, '')
    # the tables themselves
    for args, code, text in ((([1, 1000], [-1], [ok]), PEP_ERR_ARG, 'contig_off must start at 0'),
                             (([0, 1000, 900], [-1], [ok]), PEP_ERR_ARG, 'contig_off must be non-decreasing (contig 1)'),
                             (([0, 1 << 31], [-1], [ok]), PEP_ERR_LIMIT, 'contig 0 holds 2^31 bytes or more'),
                             (([0, 1000], [1], [ok]), PEP_ERR_ARG, 'the seed of gene 0 names contig 1 of 1'),
                             (([0, 1000], [-2], [ok]), PEP_ERR_ARG, 'the seed of gene 0 names contig -2 of 1'),
                             (([0, 1000], [-1], [row(N, 101, 190, gene=1)]), PEP_ERR_ARG, 'row 0 names gene 1 of 1'),
                             (([0, 1000], [-1], [row(N, 101, 190, contig=1)]), PEP_ERR_ARG, 'row 0 names contig 1 of 1'),
                             (([0, 1000], [-1], [row(N, 101, 190, contig=-1, flags=M)]), PEP_ERR_ARG, 'row 0 names contig -1 of 1'),
                             (([0, 1000], [-1], [row(N, 101, 190, flags=16)]), PEP_ERR_ARG, 'row 0 has flag bits beyond the four (16)'),
                             (([0, 1000], [-1], [row(N, 101, 190, svmin=-1)]), PEP_ERR_ARG, 'row 0 has a negative structural-variation length')):
        rc, msg = check(N, *args)
        assert (rc, msg) == (code, 'pep_out_alleles: ' + text), args
    rc, msg = check(N, [0, 1000], [-1], [ok], key_bits=32)
    assert rc == PEP_ERR_ARG and 'key_bits 32 is beyond 31' in msg
    lib = N.load_library()
    msg = C.create_string_buffer(64)
    assert lib.pep_out_alleles_check(None, 0, 0, None, 0, None, None, 0, msg, len(msg)) == PEP_ERR_ARG and msg.value == b'pep_out_alleles: null table'
    # ... and through the binding: PepError with code and text, ValueError for what does not fit the columns
    with pytest.raises(N.PepError, match=r'pep_out_alleles_check failed \(-2\): pep_out_alleles: row 0 starts before its contig'):
        N.out_alleles_check([0, 1000], [-1], [row(N, 0, 90)])
    with pytest.raises(ValueError):
        N.out_alleles_check([0, 1000], [-1], [row(N, 1, 1 << 31)])
    with pytest.raises(ValueError):
        N.out_alleles_check([0, 1000], [-1], [ok[:-1]])
    with pytest.raises(ValueError):
        N.out_alleles_check([0, 1000], [-1], [ok], look9=[1, 2])


def test_null_context_is_an_argument_error(N):
    restype, *argtypes = N.SIGNATURES['pep_out_alleles']
    assert restype is C.c_int and argtypes[0] is C.c_void_p
    assert N.load_library().pep_out_alleles(*[None if t is C.c_void_p else t(0) for t in argtypes]) == PEP_ERR_ARG


def test_outalleles_section_of_the_header(N):
    """the K24 section of include/peppan_hip.h declares its two functions in this order, cites what it replaces, and its columns, bits, classes, limits and error
    code are _native's (the prototypes: tests/test_abi.py)"""
    hdr = open(os.path.join(ROOT, 'include', 'peppan_hip.h')).read()
    names = [name for _, name, _ in ABI._header_prototypes()]
    own = ['pep_out_alleles_check', 'pep_out_alleles']
    assert names[names.index(own[0]):][:len(own)] == own == [name for name in N.SIGNATURES if name in own]
    defines = dict(re.findall(r'^#define (PEP_\w+) \(?(-?\w+(?: << \d+)?)\)?$', hdr, flags=re.M))
    value = lambda text: (1 << int(text.split('<<')[1])) if '<<' in text else int(text)
    for name, want in (('COLS', N.OUTA_COLS), ('PLAN_COLS', N.OUTA_PLAN_COLS), ('BATCH', N.OUTA_BATCH), ('MAX_CONTIG', N.OUTA_MAX_CONTIG), ('MAX_ITEMS', N.OUTA_MAX_ITEMS),
                       ('GENE', N.OUTA_GENE), ('CONTIG', N.OUTA_CONTIG), ('FLAGS', N.OUTA_FLAGS), ('S', N.OUTA_S), ('E', N.OUTA_E), ('PART', N.OUTA_PART), ('QS', N.OUTA_QS),
                       ('QE', N.OUTA_QE), ('REFLEN', N.OUTA_REFLEN), ('CLEN', N.OUTA_CLEN), ('VARY', N.OUTA_VARY), ('SVMIN', N.OUTA_SVMIN), ('MISC', N.OUTA_MISC),
                       ('NONAME', N.OUTA_NONAME), ('SECONDARY', N.OUTA_SECONDARY), ('MINUS', N.OUTA_MINUS), ('SKIPPED', N.OUTA_SKIPPED), ('FRAGMENT', N.OUTA_FRAGMENT),
                       ('INTACT', N.OUTA_INTACT), ('STRUCTVAR', N.OUTA_STRUCTVAR)):
        assert value(defines['PEP_OUTA_' + name]) == want, name
    assert value(defines['PEP_ERR_ALLELE_CLASS']) == N.ERR_ALLELE_CLASS and N.ERR_ALLELE_CLASS not in (0, -1, -2, -3, -4, -5) and N.OUTA_BATCH == H.BATCH
    assert int(re.search(r'#define PEP_ABI_VERSION (\d+)', hdr).group(1)) == N.ABI_VERSION
    assert 'PEPPAN.py:1391-1472' in hdr
