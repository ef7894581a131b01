"""K24 on the GPU (csrc/outalleles.hip: the allele pass of write_output, PEPPAN.py:1391-1472): allele_pass against what the reference's own write_output did
for every case of tests/golden/g27_outalleles.json.gz - every column of the table and the returned dictionary with the order of both levels - and
allele_ids on synthetic tables against the restatement of tests/outalleles_helpers.py.

The tolerance is zero: everything is integers, bytes and strings, compared with ==.

Shapes.  The kernels run one thread per row or per allele in blocks of 256; the digest changes its padding at 55 / 56, 63 / 64 and 119 / 120 bytes (in the
fixture, on both strands); the comparison reads sixteen bytes of text per step, forward or from the span's far end, in every pairing of strands of a row and its
class's first row, with tails of 0 .. 15 bytes.  The synthetic tables take 1, 255, 256, 257 and 700 rows - below, at and beyond one block, and more than two - with skipped rows of
both kinds, rows out of order (the only way to a '-' row whose neighbour lies beyond it, i.e. rp < 0 on that strand), seeds that are met again and
seeds that are not, and allele lengths 0 .. 130 on both strands.  The batch boundary is the fixture's two-batch case, regenerated from its seed."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outalleles_helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


@pytest.fixture(scope='module')
def OA(N):
    from peppan_amd import outalleles
    yield outalleles
    outalleles.close()


@pytest.fixture(scope='module')
def fx():
    return H.load()


@pytest.mark.parametrize('name', [name for name, _, _ in H.SMALL_CASES])
def test_allele_pass_is_the_reference(OA, fx, name):
    case = next(c for c in fx['small'] if c['name'] == name)
    genomes, encodes, clust_ref = H.dictionaries_of(case)
    table = H.as_object_table(copy.deepcopy(case['before']))
    alleles = OA.allele_pass(table, genomes, encodes, clust_ref, case['pseudogene'], case['gtable'])
    got = [[int(v) if isinstance(v, (int, np.integer)) else [int(x) for x in v] if isinstance(v, list) else v for v in r] for r in table.tolist()]
    for i, (a, b) in enumerate(zip(got, case['after'])):
        assert a == b, (name, i)
    assert len(got) == len(case['after'])
    assert [[g, list(a.items())] for g, a in alleles.items()] == [[g, [tuple(x) for x in a]] for g, a in case['alleles']]


def test_allele_pass_across_a_batch_boundary(OA, fx):
    tb = fx['two_batch']
    case = H.two_batch_case(tb['seed'])
    inputs = case.inputs()
    table = H.as_object_table(H.table_of(case))
    assert len(table) == tb['n_rows']
    alleles = OA.allele_pass(table, inputs['genomes'], inputs['encodes'], inputs['clust_ref'], tb['pseudogene'], tb['gtable'])
    got = [[int(r[9]), int(r[10]), r[13], r[15]] for r in table]
    for i, (a, b) in enumerate(zip(got, tb['cols'])):
        assert a == b, i
    assert [[g, [[len(s), i] for s, i in a.items()]] for g, a in alleles.items()] == tb['alleles'] and H.allele_digest(alleles) == tb['allele_sha1']


def synthetic(rng, n_rows):
    """a table that no reference run would make - rows out of order, empty names, misc_feature rows anywhere - with its dictionaries"""
    encodes, clust_ref, genomes = {}, {}, {}
    n_contigs = 1 + n_rows // 120
    for c in range(n_contigs):
        encodes['sc%d' % c] = 1000 + c
        genomes[1000 + c] = ('genome', H.random_dna(rng, 30000, 'ACGTACGTACGTNRacgt'))
    stems = [H.random_dna(rng, 130) for _ in range(4)]
    for g in range(12):
        encodes['sg%d' % g] = g
        if g % 3:
            clust_ref[g] = stems[g % 4][:int(rng.integers(20, 131))]
    table = []
    for c in range(n_contigs):
        text = list(genomes[1000 + c][1])
        at = int(rng.integers(1, 8))
        rows = []
        while len(rows) < (n_rows + n_contigs - 1) // n_contigs and at + 140 < 30000:
            g = int(rng.integers(0, 12))
            length = len(clust_ref[g]) if g in clust_ref and rng.random() < .3 else int(rng.integers(1, 131))       # (the seed's length: its allele may be met again)
            strand = '+' if rng.random() < .5 else '-'
            if rng.random() < .5:                                       # one of few alleles, so that classes have members on both strands and in many rows
                allele = stems[g % 4][:length] if rng.random() < .6 else stems[g % 4][:length - 1] + 'A'
                text[at - 1:at - 1 + length] = list(allele if strand == '+' else H.reverse_complement(allele))
            ref_len = max(1, length + int(rng.integers(-20, 30)))
            name = 'sg%d' % g if rng.random() < .8 else 'sg%d/%d' % (g, int(rng.integers(1, 3)))
            kind = 'misc_feature' if rng.random() < .12 else 'CDS'
            if rng.random() < .05:
                name = ''
            rows.append([name, 2 if rng.random() < .1 else 1, len(table) + len(rows) + 1, 'x', 'sg0:1' if rng.random() < .2 else '', 'sc%d' % c, 99., 4 if rng.random() < .2 else 1,
                         ref_len if rng.random() < .7 else max(1, ref_len - 3), at, at + length - 1, strand, ref_len, 30000, [0], kind, ''])
            at += length + int(rng.integers(0, 90))
        for k in range(2, len(rows) - 1, 7):                            # rows out of order
            rows[k], rows[k + 1] = rows[k + 1], rows[k]
        genomes[1000 + c] = ('genome', ''.join(text))
        table += rows
    table = table[:n_rows]
    if n_rows == 1:
        table[0][0], table[0][15] = 'sg1', 'CDS'
    if n_rows >= 255:               # on a contig of their own, a '-' row whose only neighbour starts more than 300 beyond its start: rp < 0, a shorter allele
        encodes['sc_last'], genomes[999] = 999, ('genome', H.random_dna(rng, 3000))
        table[-2] = ['sg1', 1, 0, 'x', '', 'sc_last', 99., 1, 100, 1350, 1449, '+', 100, 3000, [0], 'CDS', '']
        table[-1] = ['sg1', 1, 0, 'x', '', 'sc_last', 99., 1, 100, 1000, 1099, '-', 100, 3000, [0], 'CDS', '']
    return table, genomes, encodes, clust_ref


@pytest.mark.parametrize('n_rows', [1, 255, 256, 257, 700])
def test_allele_ids_against_the_restatement(N, OA, n_rows):
    rng = np.random.default_rng(2400 + n_rows)
    table, genomes, encodes, clust_ref = synthetic(rng, n_rows)
    assert len(table) == n_rows
    T = OA.tables(H.as_object_table(table), genomes, encodes, clust_ref, 0.8)
    plan, first, rank, tflag = OA.allele_ids(T.nt, T.contig_off, T.seed_contig, T.rows)
    work = copy.deepcopy(table)
    _, seen = H.restate(work, genomes, encodes, clust_ref, 0.8, 11, structure=lambda item: (item[0], 'CDS', item[3], item[4]))
    want = H.expected_ids(table, seen, clust_ref, encodes)
    got = [tuple(plan[i, [0, 1, 2, 3, 5]].tolist()) + (int(first[i]), int(rank[i]), int(tflag[i])) for i in range(n_rows)]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, (i, table[i])
    # the allele itself, cut where the plan says
    for i, info in enumerate(seen):
        if info is not None:
            text = genomes[encodes[table[i][5]]][1][int(plan[i, 4]):int(plan[i, 4]) + int(plan[i, 5])]
            assert (text if table[i][11] == '+' else H.reverse_complement(text)) == info['allele'], i
    if n_rows >= 255:
        kinds = set(w[0] for w in want)
        assert kinds == {0, 1, 2, 3} and any(w[5] == -1 for w in want) and any(w[7] for w in want) and any(not w[7] and w[5] >= 0 for w in want)
        assert want[-1][0] in (2, 3) and want[-1][4] < 100 and table[-1][11] == '-'           # the shorter allele of rp < 0 on '-'
        members = {}
        for i, w in enumerate(want):
            if w[0]:
                members.setdefault((table[i][0], w[5]), set()).add(table[i][11])
        assert any(len(v) == 2 for v in members.values())               # a class with members on both strands: the byte-wise comparison ran
    # the plan alone is the same plan
    alone = OA.allele_ids(None, T.contig_off, T.seed_contig, T.rows, plan_only=True)
    assert alone[1] is None and np.array_equal(alone[0], plan)


def test_no_row_one_row_and_nothing_but_skipped_rows(N, OA):
    empty = np.zeros((0, N.OUTA_COLS), np.int32)
    plan, first, rank, tflag = OA.allele_ids(b'ACGT', [0, 4], [0], empty)
    assert plan.shape == (0, N.OUTA_PLAN_COLS) and len(first) == len(rank) == len(tflag) == 0
    assert OA.allele_pass(np.empty((0, 17), dtype=object), {}, {}, {}, 0.8, 11) == {}
    nt = b'CCATGAAATAACC' + b'ATGAAATAA'
    one = [[0, 0, 0, 3, 11, 1, 1, 9, 9, 13, 1, 0]]
    plan, first, rank, tflag = OA.allele_ids(nt, [0, 13, 22], [1], one)
    assert plan.tolist() == [[2, 3, 11, 0, 2, 9]] and (first.tolist(), rank.tolist(), tflag.tolist()) == ([-1], [1], [0])
    plan, first, rank, tflag = OA.allele_ids(nt, [0, 13, 22], [-1], one)
    assert (first.tolist(), rank.tolist(), tflag.tolist()) == ([0], [1], [0])
    skipped = [[0, 0, N.OUTA_MISC, 3, 11, 1, 1, 9, 9, 13, 1, 0], [5, 0, N.OUTA_NONAME, -4, 99, 1, 0, 9, 9, 13, 1, 0]] * 150
    plan, first, rank, tflag = OA.allele_ids(nt, [0, 13, 22], [1], skipped)
    assert not plan.any() and set(first.tolist()) == {-2} and not rank.any() and not tflag.any()
    table = H.as_object_table([['old:a', -1, 7, 'c', 'old:a', 'c', 1., 1, 9, 3, 11, '+', 9, 13, -1, 'misc_feature', 'Too_short'],
                               ['', 1, 8, 'c', '', 'c', 1., 1, 9, 3, 11, '+', 9, 13, [0], 'CDS', '']])
    assert OA.allele_pass(table, {1: ('g', 'CCATGAAATAACC')}, {'c': 1}, {}, 0.8, 11) == {'': {}}
    assert table[:, 13].tolist() == ['old:a:t0:1-9:3-11', ':t0:1-9:3-11'] and table[:, 15].tolist() == ['misc_feature', 'CDS']


def test_a_class_that_holds_different_bytes_is_reported(N, OA):
    rng = np.random.default_rng(2424)
    alleles = [H.random_dna(rng, 40 + k % 9) for k in range(64)]
    nt = ''.join(alleles).encode()
    off = np.concatenate([[0], np.cumsum([len(a) for a in alleles])])
    rows = [[k % 2, 0, 0, int(off[k]) + 1, int(off[k + 1]), 1, 1, len(a), len(a), len(nt), len(a) // 5, 0] for k, a in enumerate(alleles)]
    plan, first, rank, tflag = OA.allele_ids(nt, [0, len(nt)], [-1, -1], rows)
    assert first.tolist() == list(range(64)) and rank.tolist() == [1 + k // 2 for k in range(64)]
    # one bit of the digest as the class key: 32 distinct alleles of a gene in at most two classes - the comparison must refuse to merge them
    with pytest.raises(N.PepError, match=r'pep_out_alleles failed \(-24\): pep_out_alleles: row \d+ and row \d+ share a digest class and hold different bytes'):
        OA.allele_ids(nt, [0, len(nt)], [-1, -1], rows, key_bits=1)
    # equal alleles in one class pass under the same key
    same = [[0, 0, 0, 1, 40, 1, 1, 40, 40, len(nt), 8, 0]] * 3
    plan, first, rank, tflag = OA.allele_ids(nt, [0, len(nt)], [-1], same, key_bits=1)
    assert first.tolist() == [0, 0, 0] and rank.tolist() == [1, 1, 1]
    # ... and the context goes on working
    plan, first, rank, tflag = OA.allele_ids(nt, [0, len(nt)], [-1, -1], rows)
    assert first.tolist() == list(range(64))


def test_call_times_of_out_alleles(N, OA):
    """pep_call_times(PEP_CALL_OUT_ALLELES): with every phase timed the six slots the header states - plan, digest, classes, comparison, sort, ranks - are > 0
    and the last two 0 (one row and its seed: two items, so every stage launches); the plan alone fills slot 0 alone; untimed, every slot is 0.  No bytes
    are counted.  The wrapper makes one library call: its total is that call's record."""
    ctx = OA._context(None)
    nt, one = b'CCATGAAATAACC' + b'ATGAAATAA', [[0, 0, 0, 3, 11, 1, 1, 9, 9, 13, 1, 0]]
    ctx.set_timing(2)
    try:
        for plan_only, used in ((False, 6), (True, 1)):
            ctx.out_alleles(nt, [0, 13, 22], [1], one, plan_only=plan_only)
            for total in (False, True):
                ms, to_device, to_host = ctx.call_times(N.CALL_OUT_ALLELES, total=total)
                print('plan_only=%r total=%r: ms %r' % (plan_only, total, ms.tolist()))
                assert ms.shape == (8,) and (ms[:used] > 0).all() and not ms[used:].any() and (to_device, to_host) == (0, 0)
    finally:
        ctx.set_timing(0)
    ctx.out_alleles(nt, [0, 13, 22], [1], one)
    assert not ctx.call_times(N.CALL_OUT_ALLELES)[0].any() and not ctx.call_times(N.CALL_OUT_ALLELES, total=True)[0].any()


def test_nothing_is_left_on_the_device_after_close(N, OA):
    OA.close()
    before = N.live_resources()
    with N.Context(0) as ctx:
        got = ctx.out_alleles(b'CCATGAAATAACC', [0, 13], [-1], [[0, 0, 0, 3, 11, 1, 1, 9, 9, 13, 1, 0]])
        assert got[1].tolist() == [0] and N.live_resources()[0] > before[0]
    assert N.live_resources() == before
