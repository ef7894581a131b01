"""K7's restatement (tests/rescore_helpers.py) pinned to the reference's recorded values, and the C oracle held to the restatement.  No GPU."""
import os
import sys

import numpy as np
from conftest import load_golden
from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rescore_helpers import assert_coverage, hit_runs, random_hits, reference_counts, reference_identity_score, reference_table  # noqa: E402


def test_restatement_reproduces_every_recorded_mode_1_case():
    g = load_golden('g05_rescore.json')
    cases = [c for c in g['cases'] if c['mode'] == 1]
    assert len(cases) == 2
    for case in cases:
        exp = {r[15]: r for r in case['rows']}
        checked = 0
        for row in g['table']:
            counts = reference_counts(g['query'][row[0]], g['ref'][row[1]], row[6], row[7], row[8], row[9], row[14])
            iden, score = reference_identity_score(counts)
            if row[15] in exp:
                assert iden == exp[row[15]][2] and score == exp[row[15]][11], row[:2]
                checked += 1
            else:
                assert iden < case['min_id'], row[:2]
        assert checked == len(exp) and checked > 20


def test_raw_cigar2score_calls():
    """the four hand-made calls the fixture records: the slices are the whole sequences"""
    g = load_golden('g05_rescore.json')
    raw = [c for c in g['raw'] if c['mode'] == 1]
    assert len(raw) == 4
    for c in raw:
        counts = reference_counts(c['q'], c['r'], 1, len(c['q']), 1, len(c['r']), c['cigar'])
        assert list(reference_identity_score(counts)) == np.round(np.array(c['out']), 3).tolist(), c


def test_oracle_equals_restatement_on_generated_hits():
    """3 200 hits whose classes are counted before anything is compared: the conditions are on the inputs"""
    rng = np.random.default_rng(707)
    q_seqs, r_seqs, hits, arena, cov = random_hits(rng, 40, 40, 3200)
    assert_coverage(cov)
    assert any(len(s) == 0 for s in q_seqs) and any(len(s) == 1 for s in q_seqs) and any(len(s) == 0 for s in r_seqs) and any(len(s) == 1 for s in r_seqs)
    want = reference_table(q_seqs, r_seqs, hits, arena)
    q_enc = [O.nt_encode_rescore(s.decode().upper()) for s in q_seqs]
    r_enc = [O.nt_encode_rescore(s.decode().upper()) for s in r_seqs]
    wrong = []
    for k in range(len(hits)):
        h = hits[k]
        off, n = int(h['cigar_off']), int(h['cigar_runs'])
        got = O.rescore_counts(q_enc[h['q']], r_enc[h['r']], int(h['qs']), int(h['rs']), int(h['re']), arena[off:off + n])
        if got.tolist() != want[k].tolist():
            wrong.append((k, 'one base' if h['rs'] == h['re'] else 'range', hit_runs(hits, arena, k), got.tolist(), want[k].tolist()))
    assert not wrong, (len(wrong), sorted({w[1] for w in wrong}), wrong[:5])
    assert (want[:, 4] > 0).sum() >= 20 and len(set(want[:, 0].tolist())) > 100
