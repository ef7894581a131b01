"""K7's codon grid on the GPU - k7_table<2> and k7_table<3> behind Context.rescore_codons, rescoring modes 2 and 3 - against the slice-by-slice restatement of the reference's
lines in tests/rescore_codon_helpers.py and against rows written down in closed form.  Integers and two float64 values: everything is compared with ==."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rescore_helpers import assert_coverage, bad_tables, hit_runs, hit_table, load, pack_runs, planted, random_bases, random_hits, revcomp  # noqa: E402
from rescore_codon_helpers import assert_codon_coverage, codon_coverage, reference_codon_table, with_planted  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7777
STRIDE_W = 200               # codons of the longest run of test_codon_stride_table


@pytest.fixture(scope='module')
def ctx():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native as N
    with N.Context(0) as c:
        yield c


def assert_rows(got, want, hits, arena):
    assert got.dtype == np.int64 and got.shape == want.shape
    wrong = np.flatnonzero((got != want).any(axis=1))
    assert len(wrong) == 0, (len(wrong), [(int(k), hits[k].tolist(), hit_runs(hits, arena, k), got[k].tolist(), want[k].tolist()) for k in wrong[:5]])


@pytest.fixture(scope='module')
def fuzz_inputs():
    """seed -> (q_seqs, r_seqs, hits, arena): random_hits (made for mode 1) + the planted hits of the classes it reaches rarely; the conditions are
    on the inputs, so they are checked here, before anything is compared"""
    made = {}
    for seed in (71, 72, 73):
        rng = np.random.default_rng(seed)
        q_seqs, r_seqs, hits, arena, cov = random_hits(rng, 40, 40, 3000)
        assert_coverage(cov)
        q_seqs, r_seqs, hits, arena = with_planted(np.random.default_rng(seed + 1000), q_seqs, r_seqs, hits, arena)
        assert_codon_coverage(codon_coverage(q_seqs, r_seqs, hits, arena))
        made[seed] = (q_seqs, r_seqs, hits, arena)
    return made


@pytest.mark.parametrize('table_id', [11, 4])
@pytest.mark.parametrize('mode', [2, 3])
@pytest.mark.parametrize('seed', [71, 72, 73])
def test_fuzz_all_seven_counts(ctx, fuzz_inputs, seed, mode, table_id):
    q_seqs, r_seqs, hits, arena = fuzz_inputs[seed]
    load(ctx, q_seqs, r_seqs)
    got = ctx.rescore_codons(hits, arena, mode, table_id)
    assert_rows(got, reference_codon_table(q_seqs, r_seqs, hits, arena, mode, table_id), hits, arena)


def test_codon_stride_table(ctx):
    """single M runs of phase + 3 w + tail columns, w = 0 .. 200 (the 64-lane trips end at 64 and 128 codons), phase and tail 0 .. 2, both strands; the query
    differs from the reference range in one column, and for every length that column is every column of the run once: 1 092 636 hits.  Mode 3 and the
    integer shape of mode 2 against rows in closed form for every hit; both modes against the restatement for a seeded sample of 8 000 hits and for every
    hit of 63 .. 65 and 127 .. 129 codons at phase 1, tail 2 (the restatement takes 50 us per hit)"""
    from peppan_amd import _native as N
    rng = np.random.default_rng(65)
    W, PAD = STRIDE_W, 37
    span = 2 + 3 * W + 2 + 2                                      # the longest run, started at the largest phase
    G = random_bases(rng, span)
    q_seqs = [planted(G, c) for c in range(span)]
    fwd = random_bases(rng, PAD) + G + random_bases(rng, PAD)
    r_seqs = [fwd, revcomp(fwd)]
    arena = np.array([L << 2 for L in range(span + 1)], dtype=np.uint32)          # the run of L columns is word L
    cols = {k: [] for k in ('q', 'r', 'qs', 'qe', 'rs', 're', 'L', 'w', 'phase', 'x')}
    for w in range(W + 1):
        for phase in range(3):
            for tail in range(3):
                L = phase + 3 * w + tail
                if L == 0:
                    continue
                a = phase                                             # the run covers G[a:a + L]: the query's first base gives the phase
                lo, hi = PAD + a + 1, PAD + a + L
                for rev in (0, 1):
                    x = np.arange(L)
                    cols['q'].append(a + x); cols['x'].append(x)
                    for k, v in (('r', rev), ('qs', a + 1), ('qe', a + L), ('rs', len(fwd) - lo + 1 if rev else lo), ('re', len(fwd) - hi + 1 if rev else hi),
                                 ('L', L), ('w', w), ('phase', phase)):
                        cols[k].append(np.full(L, v))
    cols = {k: np.concatenate(v) for k, v in cols.items()}
    hits = np.zeros(len(cols['q']), dtype=N.NT_HIT_DTYPE)
    for f in ('q', 'r', 'qs', 'qe', 'rs', 're'):
        hits[f] = cols[f]
    hits['cigar_runs'], hits['cigar_off'] = 1, cols['L']
    assert len(hits) == 2 * (27 * W * (W + 1) // 2 + 18 * (W + 1)) and (W != 200 or len(hits) == 1092636)
    w, p = cols['w'], cols['x'] - cols['phase']
    kept = (p >= 0) & (p < 3 * w)
    expect3 = np.zeros((len(hits), 7), dtype=np.int64)
    for k in range(3):
        expect3[:, k] = w - (kept & (p % 3 == k))
    expect3[:, 3] = 3 * w
    load(ctx, q_seqs, r_seqs)
    got3 = ctx.rescore_codons(hits, arena, 3)
    assert_rows(got3, expect3, hits, arena)
    got2 = ctx.rescore_codons(hits, arena, 2, 11)
    assert np.array_equal(got2[:, 1], w) and not got2[:, 3:].any()
    assert np.array_equal(got2[~kept, 0], w[~kept]) and np.all(got2[kept, 0] >= w[kept] - 1)      # only the codon that holds the column can differ
    sample = np.union1d(rng.choice(len(hits), min(8000, len(hits)), replace=False),
                        np.flatnonzero(np.isin(w, (63, 64, 65, 127, 128, 129)) & (cols['phase'] == 1) & (cols['L'] == 1 + 3 * w + 2)))
    sub = hits[sample]
    assert np.array_equal(got3[sample], reference_codon_table(q_seqs, r_seqs, sub, arena, 3))
    assert np.array_equal(got2[sample], reference_codon_table(q_seqs, r_seqs, sub, arena, 2, 11))
    assert np.array_equal(ctx.rescore_codons(sub, arena, 2, 4), reference_codon_table(q_seqs, r_seqs, sub, arena, 2, 4))


def test_run_boundary_table(ctx):
    """aM gI bM and aM gD bM, a = 1 .. 7 and 62 .. 67, g = 1 .. 5 and 70, b = 7, 8, 9, all three phases, both strands: over a and the phase the codon grid
    crosses the gap at each of its three positions.  The query equals the reference inside the M runs except for one column behind the gap."""
    rng = np.random.default_rng(5)
    R = random_bases(rng, 400)
    r_seqs = [R, revcomp(R)]
    q_seqs, rows, arena, expect3, crossing = [], [], [], [], set()
    for a in (1, 2, 3, 4, 5, 6, 7, 62, 63, 64, 65, 66, 67):
        for g in (1, 2, 3, 4, 5, 70):
            for b in (7, 8, 9):
                for kind in 'ID':
                    for phase in range(3):
                        for rev in (0, 1):
                            s = int(rng.integers(0, 40))              # the aligned range is R[s:s + ra]
                            bad = 1 + (a + b + phase) % 4             # the planted column, counted inside the second M run
                            if kind == 'I':
                                q = R[s:s + a] + random_bases(rng, g) + planted(R[s + a:s + a + b], bad)
                                ra, op = a + b, np.array([0] * a + [1] * g + [0] * b)
                                same = np.array([1] * a + [0] * g + [1] * b)
                                same[a + g + bad] = 0
                            else:
                                q = R[s:s + a] + planted(R[s + a + g:s + a + g + b], bad)
                                ra, op = a + g + b, np.array([0] * (a + b))
                                same = np.array([1] * (a + b))
                                same[a + bad] = 0
                            head = random_bases(rng, phase + 3 * int(rng.integers(0, 2)))
                            q_seqs.append(head + q + random_bases(rng, int(rng.integers(0, 4))))
                            lo, hi = s + 1, s + ra
                            rows.append((len(q_seqs) - 1, rev, len(head) + 1, len(head) + len(q), len(R) - lo + 1 if rev else lo, len(R) - hi + 1 if rev else hi,
                                         3, 0, len(arena)))
                            arena += pack_runs([[a, 'M'], [g, kind], [b, 'M']])
                            # closed form, per column of the M and I runs: on the grid or not, its position, matching or not
                            p = np.arange(len(op)) - phase
                            kept = (p >= 0) & (p < 3 * (max(len(op) - phase, 0) // 3))
                            expect3.append([int((kept & (p % 3 == k) & (same == 1)).sum()) for k in range(3)] + [int((kept & (op == 0)).sum()), 1, g, g if g > 3 else 0])
                            crossing.add((kind, (a - phase) % 3))
    assert crossing == {(kind, k) for kind in 'ID' for k in range(3)}
    hits = hit_table(rows)
    arena = np.array(arena, dtype=np.uint32)
    load(ctx, q_seqs, r_seqs)
    got3 = ctx.rescore_codons(hits, arena, 3)
    assert_rows(got3, np.array(expect3, dtype=np.int64), hits, arena)
    assert_rows(got3, reference_codon_table(q_seqs, r_seqs, hits, arena, 3), hits, arena)
    for table_id in (11, 4):
        assert_rows(ctx.rescore_codons(hits, arena, 2, table_id), reference_codon_table(q_seqs, r_seqs, hits, arena, 2, table_id), hits, arena)


@pytest.mark.parametrize('mode', [2, 3])
def test_launch_shapes(ctx, mode):
    q_seqs, r_seqs, hits, arena, _ = random_hits(np.random.default_rng(256), 20, 20, 600)
    load(ctx, q_seqs, r_seqs)
    whole = ctx.rescore_codons(hits, arena, mode)
    assert np.array_equal(whole, reference_codon_table(q_seqs, r_seqs, hits, arena, mode))
    for n in (1, 3, 4, 5, 8, 257):
        for first in (0, 11, len(hits) - n):
            part = ctx.rescore_codons(hits[first:first + n], arena, mode)
            assert part.shape == (n, 7) and np.array_equal(part, whole[first:first + n]), (n, first)
    none = ctx.rescore_codons(hits[:0], arena, mode)
    assert none.shape == (0, 7) and none.dtype == np.int64
    assert ctx.rescore_codons(hits[:0], np.zeros(0, np.uint32), mode).shape == (0, 7)


def nan_equal(a, b):
    return a.shape == b.shape and bool(np.all((a == b) | ((a != a) & (b != b))))


@pytest.mark.parametrize('table_id', [11, 4])
@pytest.mark.parametrize('mode', [2, 3])
def test_float_end_of_the_rescored_table(ctx, mode, table_id):
    from peppan_amd import uberBlast as UB
    from peppan_amd.hittable import HitTable
    rng = np.random.default_rng(413)
    q_seqs, r_seqs, hits, arena, cov = random_hits(rng, 30, 30, 1500)
    q_seqs, r_seqs, hits, arena = with_planted(rng, q_seqs, r_seqs, hits, arena, per_class=6)
    q_names, r_names = ['q%03d' % i for i in range(len(q_seqs))], ['r%03d' % i for i in range(len(r_seqs))]
    rb = UB.RunBlast()
    rb.table_id = table_id
    rb.qrySeq = {n: s.decode().upper() for n, s in zip(q_names, q_seqs)}           # (upper case, as the reader leaves them: the host walk below encodes them as they are)
    rb.refSeq = {n: s.decode().upper() for n, s in zip(r_names, r_seqs)}
    n = len(hits)
    z = np.zeros(n)

    def table():
        return HitTable(list(q_names), list(r_names), hits['q'], hits['r'], z, z, z, z, hits['qs'], hits['qe'], hits['rs'], hits['re'], z, z,
                        [len(q_seqs[i]) for i in hits['q']], [len(r_seqs[j]) for j in hits['r']], arena, hits['cigar_off'], hits['cigar_runs'], rid=np.arange(n))
    with np.errstate(all='ignore'):
        want = [np.round(v, 3) for v in UB.codon_scores_from_counts(reference_codon_table(q_seqs, r_seqs, hits, arena, mode, table_id), mode)]
    assert want[0].dtype == np.float64 and np.isnan(want[0]).sum() >= 5 and len(set(want[0][~np.isnan(want[0])].tolist())) > 100
    T = rb._rescore_table(None, None, table(), mode, None, table_id, cut=False, ctx=ctx)
    assert len(T) == n and T.iden.dtype == np.float64 and T.score.dtype == np.float64
    assert nan_equal(T.iden, want[0]) and nan_equal(T.score, want[1])
    for min_id in (0.5, 0.9, 1.0):
        with np.errstate(all='ignore'):
            keep = np.flatnonzero(want[0] >= min_id)
        assert 0 < len(keep) < n
        cut = rb._rescore_table(None, None, table(), mode, min_id, table_id, cut=True, ctx=ctx)
        assert np.array_equal(cut.rid, keep) and np.array_equal(cut.iden, want[0][keep]) and np.array_equal(cut.score, want[1][keep])

    class HostWalk(object):
        """a context object without rescore_codons: _rescore_table then walks the rows on the host, as it did before K7 counted these modes"""
    with np.errstate(all='ignore'):
        old = rb._rescore_table(None, None, table(), mode, None, table_id, cut=False, ctx=HostWalk())
    assert nan_equal(old.iden, T.iden) and nan_equal(old.score, T.score)


# ---------------------------------------------------------------------------------------------------------------- errors
def test_error_conventions_and_context_stays_usable(ctx):
    from peppan_amd import _native as N
    q_seqs, r_seqs, hits, arena, _ = random_hits(np.random.default_rng(9), 12, 12, 120)
    load(ctx, q_seqs, r_seqs)
    want = {mode: reference_codon_table(q_seqs, r_seqs, hits, arena, mode) for mode in (2, 3)}
    aa, sub = N.codon_tables(11)

    def raw(c, h, cigar, n_cigar, mode, tables):
        out = np.full((max(len(h), 1), 7), SENTINEL, dtype=np.int64)
        t = [None if x is None else N._ptr(x) for x in tables]
        rc = c._lib.pep_rescore_codons(c._h, C.c_uint64(len(h)), N._ptr(h), N._ptr(cigar), C.c_uint64(n_cigar), C.c_int32(mode), t[0], t[1], N._ptr(out))
        return rc, out

    def refused(c, h, cigar, n_cigar, mode, tables, code, text):
        rc, out = raw(c, h, cigar, n_cigar, mode, tables)
        assert rc == code and np.all(out == SENTINEL), text                             # nothing written
        with pytest.raises(N.PepError, match=r'pep_rescore_codons failed \(%d\): %s$' % (code, text)):
            c._check(rc, 'pep_rescore_codons')
        for m in (2, 3):
            assert np.array_equal(c.rescore_codons(hits, arena, m), want[m])            # ... and the context goes on

    for mode in (2, 3):
        for what, h, cg, n_cigar, text in bad_tables('pep_rescore_codons', q_seqs, r_seqs, hits, arena):
            refused(ctx, h, cg, n_cigar, mode, (aa, sub), -2, text)
            if n_cigar == len(cg):
                with pytest.raises(N.PepError, match=text):
                    ctx.rescore_codons(h, cg, mode)
    for mode in (1, 4, 0):
        refused(ctx, hits, arena, len(arena), mode, (aa, sub), -2, 'pep_rescore_codons: mode must be 2 or 3')
        with pytest.raises(N.PepError, match='mode must be 2 or 3'):
            ctx.rescore_codons(hits, arena, mode)
    for tables in ((None, sub), (aa, None), (None, None)):
        refused(ctx, hits, arena, len(arena), 2, tables, -2, 'pep_rescore_codons: mode 2 needs aa_of_word and sub')
    spoiled = aa.copy()
    spoiled[77] = 32
    refused(ctx, hits, arena, len(arena), 2, (spoiled, sub), -2, r'pep_rescore_codons: aa_of_word\[77\] is not below 32')
    rc, out = raw(ctx, hits, arena, len(arena), 3, (None, None))                        # mode 3 reads no table
    assert rc == 0 and np.array_equal(out, want[3])
    rc, out = raw(ctx, hits[:0], arena, len(arena), 2, (aa, sub))                       # n == 0
    assert rc == 0 and np.all(out == SENTINEL)
    # before any nucleotide set was given: a context of its own
    with N.Context(0) as fresh:
        for mode in (2, 3):
            rc, out = raw(fresh, hits, arena, len(arena), mode, (aa, sub))
            assert rc == -4 and np.all(out == SENTINEL)
        with pytest.raises(N.PepError, match=r'pep_rescore_codons failed \(-4\): pep_rescore_codons needs pep_set_query_nt and pep_set_ref_nt first'):
            fresh.rescore_codons(hits, arena, 3)
        fresh.set_query_nt(q_seqs, 11)
        with pytest.raises(N.PepError, match=r'\(-4\)'):
            fresh.rescore_codons(hits, arena, 2)
        fresh.set_ref_nt(r_seqs, 6, 11)
        for mode in (2, 3):
            assert np.array_equal(fresh.rescore_codons(hits, arena, mode), want[mode])
