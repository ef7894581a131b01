"""K19 on the GPU: Context.gene_structure and peppan_amd.genestruct against the tuples recorded from the reference's own determineGeneStructure
(tests/golden/g23_genestruct.json.gz) and the independent restatement in plain Python loops (tests/genestruct_helpers.py).  Every comparison is
==: the stage is integer arithmetic, the one float is formatted on the host by the reference's expression."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from peppan_amd import genestruct as GS  # noqa: E402  (pure Python: the library is loaded on first use)
from genestruct_helpers import (FRAME_LISTS, contig_form, item_of_case, load_g23, make_item, planted_orf, random_window, rc, restate, reversible,  # noqa: E402
                                shifted_back)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


@pytest.fixture(scope='module')
def g23():
    return load_g23()


def test_every_recorded_case_through_both_window_forms(N, g23):
    cases = g23['cases']
    items = [item_of_case(c) for c in cases]
    want = [tuple(c['returned']) for c in cases]
    assert GS.gene_structures(items) == want
    # the contig form: every window inside a longer sequence, '-' windows stored reverse-complemented and read backward; seq is not passed
    moved, contigs = contig_form(items, np.random.default_rng(1901))
    assert all(m[2] is None for m in moved) and sum(m[1][11] == '-' for m in moved) > 100
    got = GS.gene_structures(moved, genomes=contigs)
    assert [shifted_back(r, it, m) for r, it, m in zip(got, items, moved)] == want
    # ... and with the contig named through a mapping and through a function
    code = {name: k for k, name in enumerate(sorted(contigs))}
    coded = {code[name]: seq.encode() for name, seq in contigs.items()}
    assert GS.gene_structures(moved[:50], genomes=coded, contig_key=code) == got[:50]
    assert GS.gene_structures(moved[:50], genomes=coded, contig_key=code.get) == got[:50]
    GS.close()


def test_determine_gene_structure_is_the_drop_in(g23):
    for c in g23['cases'][::9]:
        assert GS.determine_gene_structure(item_of_case(c)) == tuple(c['returned']), c['name']
    GS.close()


def big_batch():
    """20 000 windows of 0 to 3 000 nucleotides and two of 200 000; frame lists, strands and tables mixed; a tenth with planted ORFs"""
    rng = np.random.default_rng(1902)
    items = []
    for k in range(20000):
        frames = FRAME_LISTS[int(rng.integers(0, len(FRAME_LISTS)))]
        if k in (7, 11111):
            seq = random_window(rng, 200000, alphabet='ACCGGGCCA')                # few stops: the walk goes far
            lp, ref_len = int(rng.integers(0, 400)), 150000
        elif k % 10 == 3:
            seq = planted_orf(rng, int(rng.integers(5, 600)), int(rng.integers(0, 300)), int(rng.integers(0, 300)), start=('ATG', 'GTG', 'TTG')[k % 3],
                              stop=('TAA', 'TAG', 'TGA')[k % 3], frame=int(rng.integers(0, 3)) if k % 4 == 0 else 0)
            lp, ref_len = int(rng.integers(0, 400)), int(rng.integers(1, max(2, len(seq))))
        else:
            seq = random_window(rng, int(rng.integers(0, 3001)), alphabet='ACGT' if k % 3 else 'ACCGGGCCA', odd=0.002 if k % 4 == 0 else 0.)
            lp, ref_len = int(rng.integers(0, 400)), int(rng.integers(1, max(2, len(seq))))
        strand = '+-'[k % 2] if reversible(seq) else '+'
        items.append(make_item(k, seq, strand, frames, lp, int(rng.integers(0, 200)), ref_len, 4 if k % 7 == 0 else 11))
    return items


@pytest.fixture(scope='module')
def batch():
    items = big_batch()
    restated = [restate(it) for it in items]
    return items, [r[0] for r in restated], [r[1] for r in restated]


def tables_of(items, N):
    """the library's tables for items in the contig form of one table id, every window a sequence of its own stored as the strand says"""
    stored = [(it[2] if it[1][11] == '+' else rc(it[2])).encode() for it in items]
    length = np.array([len(s) for s in stored])
    flags = np.array([sum(2 << f for f in it[1][14]) | (it[1][11] == '-') for it in items], dtype=np.uint8)
    return (b''.join(stored), np.concatenate([[0], np.cumsum(length)]), np.arange(len(items)), np.zeros(len(items), np.int64), length, flags,
            [it[7] for it in items], [it[8] for it in items], [it[1][12] for it in items])


def test_a_batch_of_20000_windows_equals_the_restatement_in_every_field(N, batch):
    items, want_ret, want_lib = batch
    kinds = {}
    for r in want_ret:
        kinds[r[1].split(':')[0]] = kinds.get(r[1].split(':')[0], 0) + 1
    assert all(kinds.get(t, 0) >= 100 for t in ('CDS', 'nostart', 'nostop', 'premature_stop', 'frameshift')), kinds
    with N.Context(0) as ctx:
        for table in (11, 4):
            part = [k for k, it in enumerate(items) if it[9] == table]
            T = tables_of([items[k] for k in part], N)
            ctx.set_timing(2)
            frame, start_aa, stop_aa, kind = ctx.gene_structure(*T, table4=table == 4)
            ms, up, down = ctx.gene_structure_times()
            ctx.set_timing(0)
            assert frame.dtype == np.int32 and start_aa.dtype == np.uint32 and stop_aa.dtype == np.uint32 and kind.dtype == np.uint8
            got = list(zip(frame.tolist(), start_aa.tolist(), stop_aa.tolist(), kind.tolist()))
            wrong = [(part[j], g, want_lib[part[j]]) for j, g in enumerate(got) if g != tuple(want_lib[part[j]])]
            assert not wrong, (len(wrong), wrong[:5])
            assert ms > 0 and up == len(T[0]) + 32 * len(part) and down == 9 * len(part)
            ctx.gene_structure(*T, table4=table == 4)
            assert ctx.gene_structure_times() == (0., up, down)
    assert GS.gene_structures(items) == want_ret                                # both tables in one list, the items' own windows
    GS.close()


def test_empty_batch_and_refused_calls_leave_the_context_usable(N):
    with N.Context(0) as ctx:
        frame, start_aa, stop_aa, kind = ctx.gene_structure(b'', [0], [], [], [], [], [], [], [])
        assert len(frame) == len(start_aa) == len(stop_aa) == len(kind) == 0
        good = (b'CCATGAAATAACC', [0, 13], [0], [2], [9], [2], [0], [3], [9])
        with pytest.raises(N.PepError) as e:
            ctx.gene_structure(b'ACGT', [0, 4], [0], [2], [3], [2], [0], [0], [9])
        assert '(-2)' in str(e.value) and 'leaves its sequence' in str(e.value)
        with pytest.raises(N.PepError) as e:
            ctx.gene_structure(*good[:5], [1], *good[6:])
        assert '(-2)' in str(e.value) and 'no tried frame' in str(e.value)
        with pytest.raises(ValueError):
            ctx.gene_structure(b'ACGT', [0, 5], [0], [0], [3], [2], [0], [0], [9])
        assert [a.tolist() for a in ctx.gene_structure(*good)] == [[0], [0], [2], [0]]
        # the same window stored reverse-complemented and read backward
        assert [a.tolist() for a in ctx.gene_structure(rc('CCATGAAATAACC').encode(), [0, 13], [0], [2], [9], [3], [0], [3], [9])] == [[0], [0], [2], [0]]


def test_nothing_is_left_on_the_device_after_close(N):
    GS.close()
    before = N.live_resources()
    item = make_item(1, 'ATGAAACCCTAA', '+', [0, 1], 0, 3, 12, 11)
    with N.Context(0) as ctx:
        T = tables_of([item], N)
        assert [a.tolist() for a in ctx.gene_structure(*T)] == [[0], [0], [3], [0]]
        assert N.live_resources()[0] > before[0]
    assert N.live_resources() == before
    assert GS.determine_gene_structure(item) == restate(item)[0]
    assert N.live_resources()[0] > before[0]
    GS.close()
    assert N.live_resources() == before
