"""Rescoring modes 2 and 3 (K7's codon grid) restated after the reference, a coverage report over a list of hits, and hits planted for the classes the
mode-1 generator of tests/rescore_helpers.py does not reach by itself.

reference_codon_counts does what cigar2score (uberBlast.py:221-269) and its call in RunBlast.reScore (uberBlast.py:397-415) do, in their order: the two aligned
ranges are SLICED out first (the reference range complemented and turned unless rs < re), one block per M or I run is cut out of the slices ([-1] * n opposite
an I run), the blocks are concatenated, [phase:] is taken, the tail is trimmed to a multiple of 3 and the rest reshaped to [-1, 3]; the seven integers are
counted from that array.  No cursor moves through the sequences and no column is looked up by its index, so nothing of the kernel's walk (a cursor per lane
over the runs) is shared with this file.  The two tables are the reference's, as golden g01 records them.  No GPU in here."""
import gzip
import json
import os

import numpy as np

from rescore_helpers import OPS, encode, hit_table, pack_runs, random_bases, revcomp, unpack_runs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
with open(os.path.join(GOLDEN, 'g01_tables.json')) as _f:
    _g01 = json.load(_f)
GTABLE = np.array(_g01['gtable'], dtype=np.int64)                 # word -> amino-acid letter index, table 11 (uberBlast.py:272)
BLOSUM62 = np.array(_g01['blosum62'], dtype=np.int64)             # [qa << 5 | ra] (configure.py:49-87)
PLACE = np.array([25, 5, 1], dtype=np.int64)


def aa_table(table_id):
    t = GTABLE.copy()
    if table_id == 4:
        t[56] = 22                                                # uberBlast.py:223-224
    return t


def load_g21():
    """the recorded calls of the reference's cigar2score: dicts of q, r (the aligned ranges as they lie in their sequences), rev, first (the query's first
    base), runs, mode, table_id, out ([identity, score], nan as None)"""
    with gzip.open(os.path.join(GOLDEN, 'g21_rescore_codons.json.gz')) as f:
        g = json.load(f)
    return [dict(g['alignments'][c['aln']], mode=c['mode'], table_id=c['table_id'], out=c['out']) for c in g['cases']]


def codon_rows(q_seq, r_seq, qs, qe, rs, re, runs):
    """(query codes [n, 3], reference codes [n, 3] with -1 opposite an I column, lengths of the gap runs) - uberBlast.py:226-245, 251-254"""
    q_slice = encode(q_seq)[qs - 1:qe]
    r_codes = encode(r_seq)
    r_slice = r_codes[rs - 1:re] if rs < re else 4 - r_codes[re - 1:rs][::-1]
    length = np.array([n for n, _ in runs], dtype=np.int64)
    kind = np.array([OPS.index(t) for _, t in runs], dtype=np.int64)
    q_begin = np.cumsum(length * (kind != 2)) - length * (kind != 2)
    r_begin = np.cumsum(length * (kind != 1)) - length * (kind != 1)
    q_blk, r_blk = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for n, k, qb, rb in zip(length.tolist(), kind.tolist(), q_begin.tolist(), r_begin.tolist()):
        if k == 0:
            q_blk.append(q_slice[qb:qb + n])
            r_blk.append(r_slice[rb:rb + n])
        elif k == 1:
            q_blk.append(q_slice[qb:qb + n])
            r_blk.append(np.full(n, -1, dtype=np.int64))
    q_aln, r_aln = np.concatenate(q_blk), np.concatenate(r_blk)
    phase = (qs - 1) % 3
    q_aln, r_aln = q_aln[phase:], r_aln[phase:]
    if q_aln.size % 3:
        q_aln, r_aln = q_aln[:-(q_aln.size % 3)], r_aln[:-(r_aln.size % 3)]
    return q_aln.reshape(-1, 3), r_aln.reshape(-1, 3), length[kind != 0]


def reference_codon_counts(q_seq, r_seq, qs, qe, rs, re, runs, mode, table_id=11):
    """the seven integers of one hit: mode 3 (hit0, hit1, hit2, paired, n_gap, b_gap, m_gap), mode 2 (aa_match, codons, sub_sum, 0, n_gap, b_gap, m_gap)"""
    q_aln, r_aln, gaps = codon_rows(q_seq, r_seq, qs, qe, rs, re, runs)
    gap_counts = [int(gaps.size), int(gaps.sum()), int(gaps[gaps > 3].sum())]
    if mode == 3:
        hit = (q_aln == r_aln).sum(axis=0)
        return [int(hit[0]), int(hit[1]), int(hit[2]), int((r_aln >= 0).sum())] + gap_counts
    assert mode == 2
    full = ~(r_aln < 0).any(axis=1)
    table = aa_table(table_id)
    q_aa, r_aa = table[(q_aln[full] * PLACE).sum(axis=1)], table[(r_aln[full] * PLACE).sum(axis=1)]
    return [int((q_aa == r_aa).sum()), int(q_aa.size), int(BLOSUM62[(q_aa << 5) + r_aa].sum()), 0] + gap_counts


def reference_codon_table(q_seqs, r_seqs, hits, arena, mode, table_id=11):
    """reference_codon_counts of every hit -> int64 [n, 7]; every sequence is encoded once"""
    q_enc, r_enc = [encode(s) for s in q_seqs], [encode(s) for s in r_seqs]
    out = np.zeros((len(hits), 7), dtype=np.int64)
    for k, h in enumerate(hits.tolist()):
        out[k] = reference_codon_counts(q_enc[h[0]], r_enc[h[1]], h[2], h[3], h[4], h[5], unpack_runs(arena[h[8]:h[8] + h[6]]), mode, table_id)
    return out


# ---------------------------------------------------------------------------------------------------------------- coverage
CODON_CLASSES = ('phase0', 'phase1', 'phase2', 'ncol_below_phase', 'no_whole_codon', 'tail_1', 'tail_2', 'codon_with_I', 'straddle_M|I', 'straddle_I|M',
                 'straddle_M|D|M', 'leading_I', 'word56_q', 'word56_r', 'x_one_side', 'x_both_sides', 'reverse_with_I', 'reverse_with_D')


def codon_classes(q_seq, r_seq, qs, qe, rs, re, runs):
    """the classes of CODON_CLASSES one hit belongs to, read off its runs and off the codon rows of the restatement"""
    got = set()
    phase = (qs - 1) % 3
    got.add('phase%d' % phase)
    n_col = sum(n for n, t in runs if t != 'D')
    if n_col < phase:
        got.add('ncol_below_phase')
    elif (n_col - phase) // 3 == 0:
        got.add('no_whole_codon')
    if n_col >= phase and (n_col - phase) % 3:
        got.add('tail_%d' % ((n_col - phase) % 3))
    if runs[0][1] == 'I':
        got.add('leading_I')
    ops = {t for _, t in runs}
    if rs >= re and rs != re:
        got.update('reverse_with_' + t for t in 'ID' if t in ops)
    # per column: its op, and whether a D run lies between it and the column in front
    col_op, after_d, d_seen = [], [], False
    for n, t in runs:
        if t == 'D':
            d_seen = d_seen or n > 0
            continue
        for x in range(n):
            col_op.append(t)
            after_d.append(d_seen and len(col_op) > 1)
            d_seen = False
    whole = max(n_col - phase, 0) // 3
    for c in range(whole):
        cols = range(phase + 3 * c, phase + 3 * c + 3)
        o = [col_op[p] for p in cols]
        if 'I' in o:
            got.add('codon_with_I')
        for a, b, p in ((o[0], o[1], cols[1]), (o[1], o[2], cols[2])):
            if a == 'M' and b == 'I':
                got.add('straddle_M|I')
            if a == 'I' and b == 'M':
                got.add('straddle_I|M')
            if a == 'M' and b == 'M' and after_d[p]:
                got.add('straddle_M|D|M')
    q_aln, r_aln, _ = codon_rows(q_seq, r_seq, qs, qe, rs, re, runs)
    full = ~(r_aln < 0).any(axis=1)
    qw, rw = (q_aln[full] * PLACE).sum(axis=1), (r_aln[full] * PLACE).sum(axis=1)
    if (qw == 56).any():
        got.add('word56_q')
    if (rw == 56).any():
        got.add('word56_r')
    qx, rx = (q_aln[full] == 2).any(axis=1), (r_aln[full] == 2).any(axis=1)
    if (qx ^ rx).any():
        got.add('x_one_side')
    if (qx & rx).any():
        got.add('x_both_sides')
    return got


def codon_coverage(q_seqs, r_seqs, hits, arena):
    """hits per class of CODON_CLASSES"""
    cov = dict.fromkeys(CODON_CLASSES, 0)
    q_enc, r_enc = [encode(s) for s in q_seqs], [encode(s) for s in r_seqs]
    for h in hits.tolist():
        for key in codon_classes(q_enc[h[0]], r_enc[h[1]], h[2], h[3], h[4], h[5], unpack_runs(arena[h[8]:h[8] + h[6]])):
            cov[key] += 1
    return cov


def assert_codon_coverage(cov, least=20):
    for key in CODON_CLASSES:
        assert cov[key] >= least, (key, cov[key])


# ---------------------------------------------------------------------------------------------------------------- planted hits
def planted_codon_hits(rng, per_class=24):
    """-> (q_seqs, r_seqs, rows, arena words): hits of the classes random_hits (made for mode 1) reaches rarely or never, every one with its own query and its
    own run words; the reference is one sequence and its reverse complement, a hit lies on either.  Rows are NT_HIT_DTYPE tuples with cigar_off counted from
    the start of the returned words."""
    R = random_bases(rng, 600)
    r_seqs = [R, revcomp(R)]
    q_seqs, rows, arena = [], [], []

    def add(q_body, runs, lo, pad=None):
        """q_body aligned to R[lo:lo + reference bases of runs], behind `pad` unaligned query bases (the phase)"""
        pad = int(rng.integers(0, 6)) if pad is None else pad
        rev = int(rng.integers(0, 2))
        ra = sum(n for n, t in runs if t != 'I')
        assert len(q_body) == sum(n for n, t in runs if t != 'D') and ra >= 1 and lo + ra <= len(R)
        q_seqs.append(random_bases(rng, pad) + q_body + random_bases(rng, int(rng.integers(0, 4))))
        a, b = lo + 1, lo + ra
        if rev:
            a, b = len(R) - a + 1, len(R) - b + 1
        rows.append((len(q_seqs) - 1, rev, pad + 1, pad + len(q_body), a, b, len(runs), 0, len(arena)))
        arena.extend(pack_runs(runs))

    def mutate(s, rate=0.1):
        s = bytearray(s)
        for k in np.flatnonzero(rng.random(len(s)) < rate).tolist():
            s[k] = b'ACGT'[int(rng.integers(0, 4))]
        return bytes(s)

    for i in range(per_class):
        lo = int(rng.integers(0, 300))
        # fewer columns than the phase; columns that reach the phase but hold no whole codon: 1 or 2 M columns, phase 2 / 1 / 0 by turns
        add(R[lo:lo + 1], [[1, 'M']], lo, pad=2 + 3 * (i % 2))
        n = 1 + i % 2
        add(R[lo:lo + n], [[n, 'M']], lo, pad=(0, 1, 2, 4)[i % 4] if n == 2 else (0, 1, 3)[i % 3])
        add(R[lo:lo + 2], [[2, 'M']], lo, pad=1 + 3 * (i % 2))                       # phase 1, two columns: one beyond the phase, no whole codon
        # a leading I run, then M; and M | I | M with the I run inside one codon at every position
        g, m = 1 + i % 5, 5 + i % 7
        add(random_bases(rng, g) + mutate(R[lo:lo + m]), [[g, 'I'], [m, 'M']], lo)
        a, g, b = 1 + i % 7, 1 + i % 4, 4 + i % 5
        add(mutate(R[lo:lo + a]) + random_bases(rng, g) + mutate(R[lo + a:lo + a + b]), [[a, 'M'], [g, 'I'], [b, 'M']], lo)
        # M | D | M with the D run inside a codon
        add(mutate(R[lo:lo + a]) + mutate(R[lo + a + g:lo + a + g + b]), [[a, 'M'], [g, 'D'], [b, 'M']], lo)
        # word 56 = digits 2 1 1 = "NCC" in the query's frame: on the query side, on the reference side (the query then reads the reference's bases
        # where the reference read is N C C on the strand of the hit), on both; a full codon with N on one side and on both
        m = 12 + 3 * (i % 4)
        body = bytearray(R[lo:lo + m])
        body[3:6] = b'NCC'
        add(bytes(body), [[m, 'M']], lo, pad=3 * (i % 2))
        body = bytearray(mutate(R[lo:lo + m]))
        body[6:7] = b'N'
        add(bytes(body), [[m, 'M']], lo, pad=3 * (i % 2))
    # the reference side of word 56 and of N: a reference of its own that carries them, read on either strand
    special = bytearray(random_bases(rng, 300))
    for at in range(9, 290, 30):
        special[at:at + 3] = b'NCC'
        special[at + 15:at + 16] = b'N'
    special = bytes(special)
    r_seqs += [special, revcomp(special)]
    for i in range(2 * per_class):
        at = 9 + 30 * (i % 9)
        m = 27
        lo = at - 3 * (1 + i % 2)                                                    # the query codon grid (pad a multiple of 3) lands on NCC
        q_body = bytearray(special[lo:lo + m])
        if i % 3 == 0:
            q_body[at - lo:at - lo + 3] = b'ACC'                                   # word 56 on the reference side only
        if i % 3 == 1:
            q_body[at + 15 - lo:at + 16 - lo] = b'G'                               # N on the reference side only
        rev = i % 2
        q_seqs.append(random_bases(rng, 3 * (i % 3)) + bytes(q_body) + random_bases(rng, 2))
        pad = 3 * (i % 3)
        a, b = lo + 1, lo + m
        if rev:
            a, b = len(special) - a + 1, len(special) - b + 1
        rows.append((len(q_seqs) - 1, 2 + rev, pad + 1, pad + m, a, b, 1, 0, len(arena)))
        arena.extend(pack_runs([[m, 'M']]))
    return q_seqs, r_seqs, rows, arena


def with_planted(rng, q_seqs, r_seqs, hits, arena, per_class=24):
    """the output of random_hits with planted_codon_hits appended -> (q_seqs, r_seqs, hits, arena)"""
    pq, pr, rows, words = planted_codon_hits(rng, per_class)
    extra = hit_table([(row[0] + len(q_seqs), row[1] + len(r_seqs)) + tuple(row[2:8]) + (row[8] + len(arena),) for row in rows])
    return list(q_seqs) + pq, list(r_seqs) + pr, np.concatenate([hits, extra]), np.concatenate([arena, np.array(words, dtype=np.uint32)])
