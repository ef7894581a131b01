"""K19 (the gene structure of predictions, PEPPAN.py:1193-1229) without a GPU: the g23 fixture recorded from the reference's own
determineGeneStructure against the independent restatement in plain loops (tests/genestruct_helpers.py), its section of
include/peppan_hip.h against _native's limits and codes, the table checks of pep_gene_structure, which need no device, and the host half
of peppan_amd.genestruct - texts and coordinates from hand-made device outputs."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from peppan_amd import genestruct as GS  # noqa: E402  (pure Python: the library is loaded on first use)
from genestruct_helpers import FRAME_LISTS, KINDS, NO_STOP, item_of_case, load_g23, make_item, marks, rc, restate  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


@pytest.fixture(scope='module')
def g23():
    return load_g23()


def test_restatement_equals_every_recorded_case(g23):
    cases = g23['cases']
    assert len(cases) >= 300
    texts, lists, found_in = {}, set(), set()
    for c in cases:
        ret, lib, details = restate(item_of_case(c))
        assert list(ret) == c['returned'], c['name']
        texts[ret[1].split(':')[0]] = texts.get(ret[1].split(':')[0], 0) + 1
        lists.add(tuple(c['frames']))
        if lib[0] >= 0:
            found_in.add(len(details))
    assert all(texts.get(t, 0) >= 10 for t in ('CDS', 'nostart', 'nostop', 'premature_stop', 'frameshift')), texts
    assert lists >= {tuple(f) for f in FRAME_LISTS} and found_in == {1, 2, 3}
    assert {c['strand'] for c in cases} == {'+', '-'} and {c['gtable'] for c in cases} == {4, 11}
    assert {len(c['seq']) for c in cases} >= set(range(6)) and max(len(c['seq']) for c in cases) > 3 * 4097


def test_marks_are_the_marked_start_translation():
    assert marks('ATGGTGTTGTAATAGTGAAAAA-CANCacgtgaC', 0, 11) == 'MMMXXX.-X.X'      # the partial last codon is dropped
    assert marks('ATGGTGTTGTAATAGTGAAAAA-CANCacgtgaC', 0, 4) == 'MMMXX..-X..'
    assert marks('CATGA', 1, 11) == 'M' and marks('CATGA', 2, 11) == 'X' and marks('CA', 2, 11) == '' and marks('', 0, 11) == ''
    assert rc('acgTn-x') == 'NNNACGT'


def test_genestruct_section_of_the_header(N):
    """the K19 section of include/peppan_hip.h cites what it replaces, and its limits and codes are _native's (the prototypes: tests/test_abi.py)"""
    hdr = open(os.path.join(ROOT, 'include', 'peppan_hip.h')).read()
    assert 'PEPPAN.py:1193-1229' in hdr
    assert int(re.search(r'#define PEP_GENESTRUCT_MAX_WINDOW \(1ull << (\d+)\)', hdr).group(1)) == N.GENESTRUCT_MAX_WINDOW.bit_length() - 1 == 31
    assert int(re.search(r'#define PEP_GENESTRUCT_NO_STOP (0x[0-9A-F]+)u', hdr).group(1), 16) == N.GENESTRUCT_NO_STOP == NO_STOP
    for k, name in enumerate(('CDS', 'NOSTART', 'NOSTOP', 'PREMATURE')):
        assert re.search(r'#define PEP_GENESTRUCT_%s %d\b' % (name, k), hdr)
    assert N.GENESTRUCT_KINDS == KINDS


GOOD = dict(seq_off=[0, 100, 100, 350], seq=[0, 2, 2, 1], win_off=[0, 10, 250, 0], win_len=[100, 240, 0, 0], flags=[2, 15, 9, 4], lp=[0, 60, 7, 0],
            allowed_vary=[0, 30, 0, 9], ref_len=[90, 200, 1, 5])
ORDER = ('seq_off', 'seq', 'win_off', 'win_len', 'flags', 'lp', 'allowed_vary', 'ref_len')


def _check(N, code=None, text=None, **change):
    args = dict(GOOD, **change)
    if code is None:
        return N.gene_structure_check(*[args[k] for k in ORDER])
    with pytest.raises(N.PepError) as e:
        N.gene_structure_check(*[args[k] for k in ORDER])
    assert '(%d)' % code in str(e.value) and text in str(e.value), str(e.value)


def test_check_refuses_each_bad_input_with_its_code(N):
    ARG, LIMIT = -2, -3
    _check(N)
    _check(N, seq_off=[0], seq=[], win_off=[], win_len=[], flags=[], lp=[], allowed_vary=[], ref_len=[])       # an empty batch is legal
    _check(N, lp=[2 ** 32 - 1] * 4, allowed_vary=[2 ** 32 - 1] * 4, ref_len=[2 ** 32 - 1] * 4)                 # the full width of every column
    for flags in (2, 4, 6, 8, 10, 12, 14, 3, 15):
        _check(N, flags=[flags] * 4)
    _check(N, ARG, 'seq_off must start at 0', seq_off=[1, 100, 100, 350])
    _check(N, ARG, 'seq_off must be non-decreasing (sequence 1)', seq_off=[0, 100, 99, 350])
    _check(N, ARG, 'prediction 1 names sequence 3 of 3', seq=[0, 3, 2, 1])
    _check(N, ARG, 'the window of prediction 1 leaves its sequence of 250 nucleotides', win_len=[100, 241, 0, 0])
    _check(N, ARG, 'the window of prediction 2 leaves its sequence', win_off=[0, 10, 251, 0])
    _check(N, ARG, 'the window of prediction 3 leaves its sequence of 0 nucleotides', win_len=[100, 240, 0, 1])
    _check(N, ARG, 'the window of prediction 0 leaves its sequence', win_off=np.array([2 ** 64 - 1, 10, 250, 0], dtype=np.uint64), win_len=[2, 240, 0, 0])    # (no wrap-around of off + len)
    _check(N, ARG, 'prediction 2 has no tried frame', flags=[2, 15, 1, 4])
    _check(N, ARG, 'prediction 0 has no tried frame', flags=[0, 15, 9, 4])
    _check(N, ARG, 'prediction 3 has flag bits above bit 3', flags=[2, 15, 9, 20])
    _check(N, ARG, 'ref_len of prediction 1 is 0', ref_len=[90, 0, 1, 5])
    # a window of 2^31 nucleotides: the nucleotides themselves are never read by the check, so none are needed
    big = dict(seq_off=[0, 2 ** 31 + 5], seq=[0, 0], win_off=[0, 3], flags=[2, 2], lp=[0, 0], allowed_vary=[0, 0], ref_len=[9, 9])
    _check(N, win_len=[5, 2 ** 31 - 1], **big)
    _check(N, LIMIT, 'the window of prediction 1 holds 2^31 nucleotides or more', win_len=[5, 2 ** 31], **big)
    _check(N, LIMIT, 'the window of prediction 0 holds 2^31 nucleotides or more', win_len=[2 ** 32 - 1, 5], **big)
    for column in ('seq', 'win_len', 'lp', 'allowed_vary', 'ref_len'):                                         # never reach the library, where they would be cut to 32 bits
        with pytest.raises(ValueError):
            _check(N, **{column: [1, 2 ** 32, 0, 0]})
        with pytest.raises(ValueError):
            _check(N, **{column: [1, -1, 0, 0]})
    with pytest.raises(ValueError):
        _check(N, flags=[2, 256, 9, 4])
    with pytest.raises(ValueError):
        _check(N, lp=[0, 60, 7])
    with pytest.raises(ValueError):
        _check(N, lp=[0.5, 60, 7, 0])


def _device_outputs(libs):
    f, a, z, k = zip(*libs)
    return np.array(f, np.int32), np.array(a, np.uint32), np.array(z, np.uint32), np.array(k, np.uint8)


def test_results_builds_every_text_and_coordinate_from_device_outputs():
    """every kind x frame list x strand, from hand-made outputs of the library: no device"""
    seq = 'A' * 300
    items, libs, want = [], [], []
    for strand in '+-':
        for frames in ([0], [0, 1], [0, 2], [0, 1, 2], [1, 2], [2], [1]):
            for found in frames:                                             # a CDS in each tried frame, codons 7 .. 61
                it = make_item(len(items), seq, strand, frames, 21, 9, 180, 11)
                s2, e2 = it[5], it[6]
                items.append(it)
                libs.append((found, 7, 61, 0 if found == frames[0] else 3))
                want.append((it[0], 'CDS', s2 + 21 + found, s2 + 185 + found) if strand == '+' else (it[0], 'CDS', e2 - 185 - found, e2 - 21 - found))
            for kind, a, z in ((1, 7, 61), (2, 7, NO_STOP), (3, 7, 29), (3, 0, 0)):
                it = make_item(len(items), seq, strand, frames, 21, 9, 180, 11)
                items.append(it)
                libs.append((-1, a, z, kind))
                pct = 'premature_stop:{0:.2f}%'.format((z - a + 1) * 300 / 180) if kind == 3 else None
                if frames[-1] == 0:
                    text = pct or KINDS[kind]
                else:
                    text = pct.replace('premature_stop', 'frameshift') if pct else 'frameshift'
                want.append((it[0], text, it[3], it[4]))
    got = GS.results(items, *_device_outputs(libs))
    assert got == want
    assert {t for _, t, _, _ in got} >= {'CDS', 'nostart', 'nostop', 'frameshift', 'premature_stop:38.33%', 'frameshift:38.33%', 'premature_stop:1.67%', 'frameshift:1.67%'}
    assert all(type(v) is int for r in got for v in r[2:])
    with pytest.raises(ValueError):                                           # no frame, yet the first tried frame a CDS: not something the library returns
        GS.results(items[:1], *_device_outputs([(-1, 7, 61, 0)]))


def test_results_reproduces_the_fixture_from_the_restated_outputs(g23):
    items = [item_of_case(c) for c in g23['cases']]
    got = GS.results(items, *_device_outputs([restate(it)[1] for it in items]))
    assert [list(r) for r in got] == [c['returned'] for c in g23['cases']]


def test_gene_structures_refuses_what_the_library_cannot_hold():
    good = make_item(0, 'ATGAAATAA', '+', [0], 0, 0, 9, 11)
    for change in (dict(frames=[1, 0]), dict(frames=[]), dict(frames=[0, 0]), dict(frames=[3]), dict(lp=-1), dict(lp=2 ** 32), dict(allowed_vary=-3), dict(ref_len=0),
                   dict(lp=1.5)):
        it = make_item(0, 'ATGAAATAA', '+', change.get('frames', [0]), change.get('lp', 0), change.get('allowed_vary', 0), change.get('ref_len', 9), 11)
        with pytest.raises(ValueError):
            GS.gene_structures([good, it])
    with pytest.raises(ValueError):                                           # [s2 - 1, e2) with e2 < s2 - 1
        GS.gene_structures([good[:5] + [10, 5] + good[7:]], genomes={good[1][5]: 'ACGT' * 10})
    assert GS.gene_structures([]) == []
