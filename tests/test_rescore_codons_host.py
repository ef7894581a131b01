"""Rescoring modes 2 and 3 without a GPU: the restatement of tests/rescore_codon_helpers.py + uberBlast.codon_scores_from_counts held to the reference's
recorded values (g21, g05) and to UB.cigar2score, the device-free check entry point, the header, and the routing of RunBlast._rescore_table."""
import copy
import os
import sys

import numpy as np
import pytest
from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rescore_helpers import bad_tables, encode, hit_runs, random_hits  # noqa: E402
from rescore_codon_helpers import load_g21, reference_codon_counts, with_planted  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    """== with nan equal to nan"""
    a, b = float('nan') if a is None else float(a), float('nan') if b is None else float(b)
    return a == b or (a != a and b != b)


def scores(counts, mode):
    from peppan_amd import uberBlast as UB
    iden, score = UB.codon_scores_from_counts(np.array([counts], dtype=np.int64), mode)
    assert iden.dtype == np.float64 and score.dtype == np.float64 and iden.shape == (1,) and score.shape == (1,)
    return iden[0], score[0]


def test_restatement_and_float_end_reproduce_every_recorded_case():
    cases = load_g21()
    assert len(cases) >= 400 and {(c['mode'], c['table_id']) for c in cases} == {(2, 11), (3, 11), (2, 4), (3, 4)}
    n_nan = 0
    for c in cases:
        q, r, first = c['q'].encode(), c['r'].encode(), c['first']
        rs, re = (len(r), 1) if c['rev'] else (1, len(r))
        counts = reference_codon_counts(b'N' * (first - 1) + q, r, first, first - 1 + len(q), rs, re, c['runs'], c['mode'], c['table_id'])
        iden, score = scores(counts, c['mode'])
        assert same(iden, c['out'][0]) and same(score, c['out'][1]), (c, counts, iden, score)
        n_nan += c['out'][0] is None
    assert n_nan >= 5


def test_raw_cigar2score_calls_of_g5():
    raw = [c for c in load_golden('g05_rescore.json')['raw'] if c['mode'] in (2, 3)]
    assert len(raw) == 8
    for c in raw:
        q, r = c['q'].encode(), c['r'].encode()
        counts = reference_codon_counts(b'N' * (c['frame'] - 1) + q, r, c['frame'], c['frame'] - 1 + len(q), 1, len(r), c['cigar'], c['mode'], 11)
        iden, score = scores(counts, c['mode'])
        assert same(iden, c['out'][0]) and same(score, c['out'][1]), (c, counts)


@pytest.mark.parametrize('mode', [2, 3])
def test_equals_cigar2score_on_generated_hits(mode):
    from peppan_amd import uberBlast as UB
    rng = np.random.default_rng(2300 + mode)
    q_seqs, r_seqs, hits, arena, _ = random_hits(rng, 40, 40, 2000)
    q_seqs, r_seqs, hits, arena = with_planted(rng, q_seqs, r_seqs, hits, arena, per_class=6)
    assert len(hits) >= 2000
    q_enc, r_enc = [encode(s) for s in q_seqs], [encode(s) for s in r_seqs]
    n_nan = 0
    with np.errstate(all='ignore'):
        for k, h in enumerate(hits.tolist()):
            i, j, qs, qe, rs, re = h[:6]
            runs, table_id = hit_runs(hits, arena, k), (11, 4)[k % 2]
            want = UB.cigar2score([runs, r_enc[j][rs - 1:re] if rs < re else 4 - r_enc[j][re - 1:rs][::-1], q_enc[i][qs - 1:qe], qs, mode, 6, 1, table_id])
            iden, score = scores(reference_codon_counts(q_enc[i], r_enc[j], qs, qe, rs, re, runs, mode, table_id), mode)
            assert same(iden, want[0]) and same(score, want[1]), (k, h, runs)
            n_nan += iden != iden
    assert n_nan >= 5


def test_float_end_expressions():
    from peppan_amd import uberBlast as UB
    c = np.array([[5, 4, 3, 14, 2, 9, 5], [0, 0, 0, 0, 0, 0, 0]], dtype=np.int64)
    iden, score = UB.codon_scores_from_counts(c, 3)
    n_match = 5 * (9. / 7.) + 4 * (9. / 7.) + 3 * (3. / 7.)
    n_mis = 14 - n_match
    assert iden[0] == n_match / (n_match + n_mis + 9 - 5) and score[0] == n_match * 3 - n_mis * 1 - 2 * (6 - 1) - 9 * 1
    assert iden[1] != iden[1] and score[1] == 0
    iden, score = UB.codon_scores_from_counts(np.array([[5, 7, -13, 0, 2, 9, 5]]), 2, gap_open=11, gap_extend=2)
    assert iden[0] == 15. / (21. + 9 - 5) and score[0] == -13. - 2 * 9. - 9 * 2.
    with pytest.raises(ValueError):
        UB.codon_scores_from_counts(c, 1)


# ---------------------------------------------------------------------------------------------------------------- the check entry point
def offsets(seqs):
    return np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)


def test_check_entry_point():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native as N
    q_seqs, r_seqs, hits, arena, _ = random_hits(np.random.default_rng(9), 12, 12, 120)
    q_off, r_off = offsets(q_seqs), offsets(r_seqs)
    for mode in (2, 3):
        assert N.rescore_codons_check(hits, arena, mode, q_off, r_off) is None
        assert N.rescore_codons_check(hits, arena, mode, q_off, r_off, table_id=4) is None
        assert N.rescore_codons_check(hits[:0], arena[:0], mode, q_off, r_off) is None
        for what, h, cg, n_cigar, text in bad_tables('pep_rescore_codons', q_seqs, r_seqs, hits, arena):
            with pytest.raises(N.PepError, match=r'pep_rescore_codons_check failed \(-2\): %s$' % text):
                N.rescore_codons_check(h, cg[:n_cigar], mode, q_off, r_off)
    assert N.rescore_codons_check(hits, arena, 3, q_off, r_off, tables=None) is None          # mode 3 reads no table
    for mode in (1, 4, 0, -2):
        with pytest.raises(N.PepError, match=r'\(-2\): pep_rescore_codons: mode must be 2 or 3'):
            N.rescore_codons_check(hits, arena, mode, q_off, r_off)
    aa, sub = N.codon_tables(11)
    for tables in (None, (None, sub), (aa, None)):
        with pytest.raises(N.PepError, match=r'\(-2\): pep_rescore_codons: mode 2 needs aa_of_word and sub'):
            N.rescore_codons_check(hits, arena, 2, q_off, r_off, tables=tables)
    for at, value in ((0, 32), (124, 255), (56, 33)):
        spoiled = aa.copy()
        spoiled[at] = value
        with pytest.raises(N.PepError, match=r'\(-2\): pep_rescore_codons: aa_of_word\[%d\] is not below 32' % at):
            N.rescore_codons_check(hits, arena, 2, q_off, r_off, tables=(spoiled, sub))


def test_tables_come_from_the_module():
    from peppan_amd import _native as N, uberBlast as UB, configure
    aa11, sub = N.codon_tables(11)
    aa4, sub4 = N.codon_tables(4)
    assert aa11.dtype == np.uint8 and aa11.shape == (125,) and sub.dtype == np.int8 and sub.shape == (1024,)
    assert np.array_equal(aa11, UB.gtable) and aa4[56] == 22 and aa11[56] != 22 and np.array_equal(np.delete(aa4, 56), np.delete(aa11, 56))
    assert UB.gtable[56] != 22                                                                 # the module's table is not patched
    n = len(configure.blosum62)
    assert np.array_equal(sub[:n], configure.blosum62) and not sub[n:].any() and np.array_equal(sub, sub4)


def test_header_declares_the_entry_points():
    from peppan_amd import _native as N
    hdr = open(os.path.join(ROOT, 'include', 'peppan_hip.h')).read()
    for name in ('pep_rescore_codons', 'pep_rescore_codons_check'):
        assert 'int %s(' % name in hdr and name in N.EXPORTS
    assert 'uberBlast.py:250-269' in hdr and '#define PEP_ABI_VERSION %d' % N.ABI_VERSION in hdr


# ---------------------------------------------------------------------------------------------------------------- routing
class CountsCtx(object):
    """stand-in for peppan_amd._native.Context: rescore_codons from the restatement"""

    def __init__(self, rb):
        self.rb, self.calls = rb, 0

    def rescore_codons(self, h, arena, mode, table_id=11):
        self.calls += 1
        out = np.zeros((len(h), 7), dtype=np.int64)
        for k in range(len(h)):
            out[k] = reference_codon_counts(self.rb.qrySeq[self.rb.q_names[h['q'][k]]], self.rb.refSeq[self.rb.r_names[h['r'][k]]], int(h['qs'][k]), int(h['qe'][k]),
                                            int(h['rs'][k]), int(h['re'][k]), hit_runs(h, arena, k), mode, table_id)
        return out

    def set_query_nt(self, *a):
        pass

    def set_ref_nt(self, *a):
        pass

    def set_target_groups(self, groups):
        assert not groups


def test_rescore_table_takes_the_counts_and_never_the_host_walk(tmp_path, monkeypatch):
    from peppan_amd import uberBlast as UB
    g = load_golden('g05_rescore.json')
    paths = []
    for name, seqs in (('q.fa', g['query']), ('r.fa', g['ref'])):
        paths.append(str(tmp_path / name))
        with open(paths[-1], 'w') as f:
            f.write(''.join('>%s\n%s\n' % (n, s) for n, s in seqs.items()))
    holder = {}
    monkeypatch.setattr(UB, 'get_context', lambda device=None: holder['ctx'])

    def host_walk(*a, **k):
        raise AssertionError('rescore_alignments was called')
    monkeypatch.setattr(UB, 'rescore_alignments', host_walk)
    cases = [c for c in g['cases'] if c['mode'] in (2, 3)]
    assert sorted((c['mode'], c['table_id']) for c in cases) == [(2, 4), (2, 11), (3, 4), (3, 11)]
    for case in cases:
        rb = UB.RunBlast()
        rb.table_id = case['table_id']
        holder['ctx'] = CountsCtx(rb)
        table = np.empty([len(g['table']), len(g['table'][0])], dtype=object)
        for i, row in enumerate(g['table']):
            for j, v in enumerate(row):
                table[i, j] = copy.deepcopy(v)
        out = rb.reScore(paths[1], paths[0], table, case['mode'], case['min_id'], case['table_id'])
        assert holder['ctx'].calls == 1
        assert len(out) == len(case['rows']) > 20
        for got, want in zip(out, case['rows']):
            assert got[15] == want[15] and float(got[2]) == float(want[2]) and float(got[11]) == float(want[11]), (got, want)
            assert [str(got[0]), str(got[1])] + [int(x) for x in got[6:10]] == [str(want[0]), str(want[1])] + want[6:10]
