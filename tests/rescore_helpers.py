"""Mode-1 rescoring (K7) restated after the reference, and a generator of hits that reach the corners of the kernel's walk.

reference_counts does what cigar2score (uberBlast.py:221-249) and its call in RunBlast.reScore (uberBlast.py:397-415) do, in their order of operations: the
sequences are encoded whole, the two aligned ranges are SLICED out first (the reference range complemented and turned unless rs < re, uberBlast.py:412), the
columns of the M runs are gathered out of the two slices by index and compared with ==, and the gap counts are taken from the list of gap lengths.  Nothing
here moves a cursor through the full sequences - the kernel and the C oracle do, so an error of such a walk (a cursor that moves the wrong way after a gap, a
lane one column off, the strand of a one-base range) cannot be common to both sides of a comparison with this file.  No GPU and no oracle in here."""
import numpy as np

from peppan_amd._native import NT_HIT_DTYPE

# the rescoring alphabet (uberBlast.py:270-271): A 0, C 1, G 3, T 4, every other byte 2 - so that 4 - code is the complement
BASE_CODE = np.full(256, 2, dtype=np.int64)
BASE_CODE[np.frombuffer(b'ACGT', dtype=np.uint8)] = (0, 1, 3, 4)

OPS = 'MID'                                   # op codes 0, 1, 2 of a packed run (len << 2 | op)
M_EDGES = (1, 2, 3, 63, 64, 65, 127, 128, 129)     # around the 64-lane stride of an M run
GAPS = (1, 2, 3, 4, 5, 9, 70)                 # below, at and above the `> 3` of mGap; one longer than a wavefront
OTHER_LETTERS = 'NNNNRYKMSWBDHV-'             # everything that is code 2


def encode(seq):
    """codes of a whole sequence, upper-cased first as the reference's reader does (configure.py:128; encoding: uberBlast.py:403, 405)"""
    if isinstance(seq, np.ndarray):
        return seq                            # encoded already
    if isinstance(seq, str):
        seq = seq.encode('latin-1')
    return BASE_CODE[np.frombuffer(bytes(seq).upper(), dtype=np.uint8)]


def unpack_runs(words):
    """packed runs -> [[length, 'M' | 'I' | 'D'], ...], the form the reference's tables carry"""
    return [[int(w) >> 2, OPS[int(w) & 3]] for w in np.asarray(words).tolist()]


def pack_runs(runs):
    return [(int(n) << 2) | OPS.index(t) for n, t in runs]


def aligned_columns(q_seq, r_seq, qs, qe, rs, re, runs):
    """(query codes, reference codes) of the columns inside M runs, and the lengths of the gap runs in CIGAR order.  Where a run begins inside the two
    slices is the sum of the runs in front of it that use that side (I: query only, D: reference only)"""
    q_slice = encode(q_seq)[qs - 1:qe]
    r_codes = encode(r_seq)
    r_slice = r_codes[rs - 1:re] if rs < re else 4 - r_codes[re - 1:rs][::-1]
    length = np.array([n for n, _ in runs], dtype=np.int64)
    kind = np.array([OPS.index(t) for _, t in runs], dtype=np.int64)
    q_begin = np.cumsum(length * (kind != 2)) - length * (kind != 2)
    r_begin = np.cumsum(length * (kind != 1)) - length * (kind != 1)
    m = kind == 0
    within = np.arange(length[m].sum()) - np.repeat(np.cumsum(length[m]) - length[m], length[m])      # 0 .. n - 1 inside every M run
    return q_slice[np.repeat(q_begin[m], length[m]) + within], r_slice[np.repeat(r_begin[m], length[m]) + within], length[~m]


def reference_counts(q_seq, r_seq, qs, qe, rs, re, runs):
    """(matches, mismatches, gap runs, gap bases, gap bases of the runs longer than 3) of one hit; runs as [[length, 'M' | 'I' | 'D'], ...]"""
    q_cols, r_cols, gaps = aligned_columns(q_seq, r_seq, qs, qe, rs, re, runs)
    matches = int(np.count_nonzero(q_cols == r_cols))
    return matches, int(q_cols.size) - matches, int(gaps.size), int(gaps.sum()), int(gaps[gaps > 3].sum())


def reference_identity_score(counts, gap_open=6, gap_extend=1):
    """(identity, score) in float64, rounded to three decimals by np.round as the reference rounds them (formulas uberBlast.py:249, rounding :413): long gaps
    leave the identity's denominator, a gap run costs gap_open for its first base and gap_extend for every further one"""
    matches, mismatches, gap_runs, gap_bases, long_gap_bases = (int(x) for x in counts)
    identity = float(matches) / (matches + mismatches + gap_bases - long_gap_bases)
    score = 3 * matches - mismatches - (gap_open - gap_extend) * gap_runs - gap_extend * gap_bases
    rounded = np.round(np.array([identity, score], dtype=np.float64), 3)
    return rounded[0], rounded[1]


# ---------------------------------------------------------------------------------------------------------------- generator
_COMP = bytes.maketrans(b'ACGTacgt', b'TGCAtgca')


def revcomp(s):
    return s.translate(_COMP)[::-1]


def _random_seq(rng, n):
    s = bytearray(rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), n).tobytes())
    for _ in range(int(rng.integers(0, 4)) if n > 8 else 0):
        a, k = int(rng.integers(0, n)), int(rng.integers(1, 7))
        kind = int(rng.integers(0, 3))
        if kind == 0:                                                   # a stretch of N, other IUPAC letters and '-'
            s[a:a + k] = ''.join(rng.choice(list(OTHER_LETTERS), len(s[a:a + k]))).encode()
        elif kind == 1:                                                 # a lower-case stretch
            s[a:a + 5 * k] = bytes(s[a:a + 5 * k]).lower()
        else:                                                           # both at once
            s[a:a + k] = ''.join(rng.choice(list('nry-'), len(s[a:a + k]))).encode()
    return bytes(s)


def _mutated(rng, s, rate):
    """substitutions at `rate`, a few short indels; the case of a base and the 'other' letters stay where they are not hit"""
    s = bytearray(s)
    for k in np.flatnonzero(rng.random(len(s)) < rate).tolist():
        s[k] = b'ACGT'[int(rng.integers(0, 4))]
    for _ in range(int(rng.integers(0, 3)) if len(s) > 20 else 0):
        a, k = int(rng.integers(1, len(s) - 1)), int(rng.integers(1, 5))
        if rng.random() < 0.5:
            del s[a:a + k]
        else:
            s[a:a] = rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), k).tobytes()
    return bytes(s)


def _m_len(rng, cap):
    edges = [m for m in M_EDGES if m <= cap]
    if rng.random() < 0.5:
        return int(rng.choice(edges))
    return int(rng.integers(1, min(cap, 300) + 1))


def _make_runs(rng, ql, rl):
    """a CIGAR that consumes at most ql query and rl reference bases, at least one of each inside an M run; gap runs may lead and trail"""
    bq, br = ql, rl
    runs = []

    def gap(must_leave):
        nonlocal bq, br
        t = 'ID'[int(rng.integers(0, 2))]
        room = (bq if t == 'I' else br) - must_leave
        fit = [g for g in GAPS if g <= room]
        if not fit or min(bq, br) < must_leave:
            return
        g = int(rng.choice(fit))
        runs.append([g, t])
        if t == 'I':
            bq -= g
        else:
            br -= g

    if rng.random() < 0.15:
        gap(1)
    for i in range(int(rng.integers(1, 5))):
        if i:
            gap(1)
            if runs[-1][1] == 'M':
                break
        m = _m_len(rng, min(bq, br))
        runs.append([m, 'M'])
        bq, br = bq - m, br - m
        if min(bq, br) < 2:
            break
    if rng.random() < 0.15:
        gap(0)
    return runs


def _consumed(runs):
    return sum(n for n, t in runs if t != 'D'), sum(n for n, t in runs if t != 'I')


COVERAGE_CLASSES = ('forward', 'reverse', 'one_base', 'reverse_with_I', 'reverse_with_D', 'forward_with_I', 'forward_with_D', 'mgap', 'gap_1_or_2', 'leading_gap',
                    'trailing_gap', 'other_q', 'other_r', 'shared_cigar', 'lower_case_q', 'lower_case_r') + tuple(
                        'flush_%s_%s' % (end, strand) for strand in ('forward', 'reverse') for end in ('q_start', 'q_end', 'r_low', 'r_high'))


def random_hits(rng, n_q, n_r, n_hits, max_len=700):
    """-> (q_seqs, r_seqs, hits [NT_HIT_DTYPE], arena uint32, coverage dict).  Sequences are bytes; hit k's runs are
    arena[hits['cigar_off'][k]:][:hits['cigar_runs'][k]].  Built in, not left to luck: M runs of M_EDGES and of random lengths up to 300; I and D runs of
    every length in GAPS, also in front of the first and behind the last M run; both strands at about equal share; hits flush with either end of either
    sequence; one-base reference ranges; references that are copies of queries mutated at rates 0 .. 0.55, on either strand (the share of matching
    columns takes many values); N, other IUPAC letters, '-' and lower-case stretches; empty and one-base sequences; hits that share a CIGAR slice; a
    first cigar_off > 0.  `coverage` counts the hits of every class (assert_coverage holds it to at least 20 hits per class)."""
    assert n_q >= 8 and n_r >= 8
    q_len = rng.integers(1, max_len + 1, n_q)
    q_len[:4] = (max_len, max_len - 1, 130, 65)
    q_seqs = [_random_seq(rng, int(n)) for n in q_len]
    q_seqs[4], q_seqs[5], q_seqs[n_q - 1] = b'', b'g', b''              # empty and one-base sequences: offsets repeat
    rates = (0., 0.01, 0.03, 0.06, 0.1, 0.15, 0.2, 0.3, 0.4, 0.55)
    r_seqs, r_is_rc = [], []
    for j in range(n_r):
        if j % 9 == 8:
            s = _random_seq(rng, int(rng.integers(1, max_len + 1)))
        else:
            s = _mutated(rng, q_seqs[j % n_q], rates[int(rng.integers(0, len(rates)))])[:max_len]
        rc = bool(j % 2)
        r_seqs.append(revcomp(s) if rc else s)
        r_is_rc.append(rc)
    r_seqs[6], r_seqs[7] = b'', b'N'
    q_ok = [i for i, s in enumerate(q_seqs) if len(s)]
    r_ok = [j for j, s in enumerate(r_seqs) if len(s)]

    arena = pack_runs([[7, 'M'], [2, 'I'], [5, 'M']])                   # words no hit refers to: the first cigar_off is not 0
    hits = np.zeros(n_hits, dtype=NT_HIT_DTYPE)
    made = []                                                           # (runs, cigar_off) of the hits so far
    for k in range(n_hits):
        if rng.random() < 0.7:                                          # a reference that is a copy of the query, else any
            j = int(rng.choice(r_ok))
            i = j % n_q if len(q_seqs[j % n_q]) and j % 9 != 8 else int(rng.choice(q_ok))
        else:
            i, j = int(rng.choice(q_ok)), int(rng.choice(r_ok))
        ql, rl = len(q_seqs[i]), len(r_seqs[j])
        runs = off = None
        u = rng.random()
        if u < 0.1 and made:                                            # share the CIGAR slice of an earlier hit, where it fits
            runs, off = made[int(rng.integers(0, len(made)))]
            qa, ra = _consumed(runs)
            if qa > ql or ra > rl:
                runs = off = None
        elif u < 0.14:                                                  # a one-base reference range
            runs = ([[int(rng.choice(GAPS)), 'I']] if rng.random() < 0.3 else []) + [[1, 'M']] + ([[int(rng.choice(GAPS)), 'I']] if rng.random() < 0.3 else [])
            if _consumed(runs)[0] > ql:
                runs = [[1, 'M']]
        if runs is None:
            runs = _make_runs(rng, ql, rl)
        if off is None:
            off = len(arena)
            arena += pack_runs(runs)
        made.append((runs, off))
        qa, ra = _consumed(runs)
        rev = (r_is_rc[j] if rng.random() < 0.85 else not r_is_rc[j])   # mostly the strand on which the copy lies
        place = rng.random()
        qs = 1 if place < 0.2 else ql - qa + 1 if place < 0.4 else int(rng.integers(1, ql - qa + 2))
        place = rng.random()
        if place < 0.2:
            lo = 1
        elif place < 0.4:
            lo = rl - ra + 1
        else:                                                           # on the diagonal of the copy, as far as the reference reaches
            lo = (rl - (qs + qa - 1) + 1) if r_is_rc[j] else qs
            lo = min(max(lo, 1), rl - ra + 1)
        hi = lo + ra - 1
        hits[k] = (i, j, qs, qs + qa - 1, hi if rev else lo, lo if rev else hi, len(runs), 0, off)
    arena = np.array(arena, dtype=np.uint32)

    cov = dict.fromkeys(COVERAGE_CLASSES, 0)
    ratios, m_runs, gap_runs, seen_off = set(), set(), set(), set()
    for h in hits.tolist():
        i, j, qs, qe, rs, re, n_runs, _, off = h
        runs = unpack_runs(arena[off:off + n_runs])
        strand = 'forward' if rs < re else 'reverse' if rs > re else 'one_base'
        cov[strand] += 1
        ops = {t for n, t in runs}
        gaps = [n for n, t in runs if t != 'M']
        if strand != 'one_base':
            for t in 'ID':
                cov['%s_with_%s' % (strand, t)] += t in ops
            cov['flush_q_start_' + strand] += qs == 1
            cov['flush_q_end_' + strand] += qe == len(q_seqs[i])
            cov['flush_r_low_' + strand] += min(rs, re) == 1
            cov['flush_r_high_' + strand] += max(rs, re) == len(r_seqs[j])
        cov['mgap'] += any(g > 3 for g in gaps)
        cov['gap_1_or_2'] += any(g < 3 for g in gaps)
        cov['leading_gap'] += runs[0][1] != 'M'
        cov['trailing_gap'] += runs[-1][1] != 'M'
        cov['shared_cigar'] += off in seen_off
        seen_off.add(off)
        q_cols, r_cols, _ = aligned_columns(q_seqs[i], r_seqs[j], qs, qe, rs, re, runs)
        cov['other_q'] += bool((q_cols == 2).any())
        cov['other_r'] += bool((r_cols == 2).any())
        cov['lower_case_q'] += q_seqs[i][qs - 1:qe] != q_seqs[i][qs - 1:qe].upper()
        cov['lower_case_r'] += r_seqs[j][min(rs, re) - 1:max(rs, re)] != r_seqs[j][min(rs, re) - 1:max(rs, re)].upper()
        ratios.add('%.3f' % (float((q_cols == r_cols).sum()) / q_cols.size))
        m_runs.update(n for n, t in runs if t == 'M')
        gap_runs.update((n, t) for n, t in runs if t != 'M')
    cov['match_ratios'] = len(ratios)
    cov['m_runs'], cov['gap_runs'] = m_runs, gap_runs
    cov['first_cigar_off'] = int(hits['cigar_off'].min()) if n_hits else 0
    return q_seqs, r_seqs, hits, arena, cov


def hit_runs(hits, arena, k):
    off, n = int(hits['cigar_off'][k]), int(hits['cigar_runs'][k])
    return unpack_runs(arena[off:off + n])


def reference_table(q_seqs, r_seqs, hits, arena):
    """reference_counts of every hit -> int64 [n, 5]; every sequence is encoded once"""
    q_enc, r_enc = [encode(s) for s in q_seqs], [encode(s) for s in r_seqs]
    out = np.zeros((len(hits), 5), dtype=np.int64)
    for k, h in enumerate(hits.tolist()):
        out[k] = reference_counts(q_enc[h[0]], r_enc[h[1]], h[2], h[3], h[4], h[5], unpack_runs(arena[h[8]:h[8] + h[6]]))
    return out


def assert_coverage(cov, least=20):
    """the conditions a comparison over random_hits' output relies on: they are on the inputs, so they are checked before anything is compared"""
    for key in COVERAGE_CLASSES:
        assert cov[key] >= least, (key, cov[key])
    assert 0.4 < cov['reverse'] / float(cov['forward'] + cov['reverse']) < 0.6
    assert cov['match_ratios'] >= 30, cov['match_ratios']
    assert cov['m_runs'] >= set(M_EDGES) and max(cov['m_runs']) > 200
    assert cov['gap_runs'] == {(g, t) for g in GAPS for t in 'ID'}
    assert cov['first_cigar_off'] > 0


# ---------------------------------------------------------------------------------------------------------------- what the GPU tests of both kernel families build with
# a base that is neither the one it replaces nor its complement: a planted mismatch is one on either strand, also in a one-base range
OTHER_BASE = bytes.maketrans(b'ACGT', b'CATG')


def load(ctx, q_seqs, r_seqs):
    ctx.set_query_nt(q_seqs, 11)
    ctx.set_ref_nt(r_seqs, 6, 11)


def planted(seq, at):
    s = bytearray(seq)
    s[at:at + 1] = bytes(s[at:at + 1]).translate(OTHER_BASE)
    return bytes(s)


def random_bases(rng, n):
    return rng.choice(np.frombuffer(b'ACGT', dtype=np.uint8), n).tobytes()


def hit_table(rows):
    return np.array(rows, dtype=NT_HIT_DTYPE)


def bad_tables(who, q_seqs, r_seqs, hits, arena):
    """[(what, hits, arena, n_cigar, message)] - every table the check shared by pep_rescore_nt and pep_rescore_codons refuses, made from a good one; `who`,
    the entry point's name, leads the message.  The last one is the victim's own runs behind the arena, the second of them with op code 3."""
    victim = int(np.flatnonzero((hits['rs'] < hits['re']) & (hits['cigar_runs'] >= 3))[1:][0])    # a forward hit of several runs, somewhere among good ones
    assert 0 < victim < len(hits) - 1

    def bad(**fields):
        h = hits.copy()
        for f, v in fields.items():
            h[f][victim] = v
        return h
    v = hits[victim]
    ql, rl = len(q_seqs[v['q']]), len(r_seqs[v['r']])
    index, coords = who + ': hit index out of range', who + ': CIGAR inconsistent with the hit coordinates'
    assert int((hits['cigar_off'] + hits['cigar_runs']).max()) == len(arena)
    spoiled = np.concatenate([arena, np.array(pack_runs(hit_runs(hits, arena, victim)), dtype=np.uint32)])
    spoiled[len(arena) + 1] |= 3
    n = len(arena)
    return [('q', bad(q=len(q_seqs)), arena, n, index), ('r', bad(r=len(r_seqs)), arena, n, index), ('slice', bad(cigar_off=n - 1), arena, n, index),
            ('slice beyond 2^64', bad(cigar_off=2 ** 64 - 1), arena, n, index), ('short arena', hits, arena, n - 1, index),
            ('qs 0', bad(qs=0), arena, n, coords), ('query end', bad(qs=int(v['qs']) + (ql - int(v['qe'])) + 1), arena, n, coords),
            ('re past', bad(rs=int(v['rs']) + (rl - int(v['re'])) + 1, re=rl + 1), arena, n, coords),
            ('rs 0', bad(rs=0, re=int(v['re']) - int(v['rs'])), arena, n, coords), ('re 0', bad(rs=int(v['re']) - int(v['rs']), re=0), arena, n, coords),
            ('span', bad(re=int(v['re']) + 1) if v['re'] < rl else bad(re=int(v['re']) - 1), arena, n, coords),
            ('op 3', bad(cigar_off=n), spoiled, len(spoiled), who + ': unknown CIGAR op')]
