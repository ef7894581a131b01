"""K7 on the GPU - k7_table<1> behind Context.rescore_nt and k7_hits as the tail of a search (Context.set_nt_match) - against the slice-by-slice
restatement of the reference's lines in tests/rescore_helpers.py.  Integers and two float64 values: everything is compared with ==."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rescore_helpers import (assert_coverage, bad_tables, encode, hit_runs, hit_table, load, pack_runs, planted, random_bases, random_hits,  # noqa: E402
                             reference_counts, reference_identity_score, reference_table, revcomp, unpack_runs)
from rescore_codon_helpers import with_planted  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7777


@pytest.fixture(scope='module')
def ctx():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native as N
    with N.Context(0) as c:
        yield c


@pytest.mark.parametrize('seed', [71, 72, 73])
def test_fuzz_all_five_counts(ctx, seed):
    q_seqs, r_seqs, hits, arena, cov = random_hits(np.random.default_rng(seed), 40, 40, 3000)
    assert_coverage(cov)
    load(ctx, q_seqs, r_seqs)
    got = ctx.rescore_nt(hits, arena)
    want = reference_table(q_seqs, r_seqs, hits, arena)
    assert got.dtype == np.int64 and got.shape == want.shape
    wrong = np.flatnonzero((got != want).any(axis=1))
    assert len(wrong) == 0, (len(wrong), sorted({'one base' if hits['rs'][k] == hits['re'][k] else 'range' for k in wrong.tolist()}),
                             [(int(k), hit_runs(hits, arena, k), got[k].tolist(), want[k].tolist()) for k in wrong[:5]])


def test_lane_stride_table(ctx):
    """single M runs of 1 .. 200 columns, both strands, at the start, in the middle and flush with the end of both sequences; the query differs from the
    reference range in one column, and for every length that column is every column of the run once: 6 x 20 100 hits"""
    rng = np.random.default_rng(64)
    W, PAD = 200, 37
    G = random_bases(rng, W)
    q_seqs = [planted(G, c) for c in range(W)]
    fwd = [G + random_bases(rng, PAD), random_bases(rng, PAD) + G + random_bases(rng, PAD), random_bases(rng, PAD) + G]
    at = (0, PAD, PAD)                                         # where G starts in the three forward references
    r_seqs = fwd + [revcomp(s) for s in fwd]
    arena = np.array([L << 2 for L in range(W + 1)], dtype=np.uint32)          # the run of L columns is word L, shared by every hit of that length
    q_idx, r_idx, qs, qe, rs, re, L_of = [], [], [], [], [], [], []
    for L in range(1, W + 1):
        for place, a in enumerate((0, (W - L) // 2, W - L)):  # the run covers G[a:a + L]
            for rev in (0, 1):
                c = np.arange(a, a + L)
                lo, hi = at[place] + a + 1, at[place] + a + L
                n = len(r_seqs[place])
                q_idx.append(c); r_idx.append(np.full(L, place + 3 * rev)); L_of.append(np.full(L, L))
                qs.append(np.full(L, a + 1)); qe.append(np.full(L, a + L))
                rs.append(np.full(L, n - lo + 1 if rev else lo)); re.append(np.full(L, n - hi + 1 if rev else hi))
    from peppan_amd import _native as N
    L_of = np.concatenate(L_of)
    hits = np.zeros(len(L_of), dtype=N.NT_HIT_DTYPE)
    for f, v in (('q', q_idx), ('r', r_idx), ('qs', qs), ('qe', qe), ('rs', rs), ('re', re)):
        hits[f] = np.concatenate(v)
    hits['cigar_runs'], hits['cigar_off'] = 1, L_of
    assert len(hits) == 6 * W * (W + 1) // 2
    assert ((hits['qs'] == 1) & (hits['rs'] == 1)).any() and ((hits['qe'] == W) & (hits['re'] == W + PAD)).any()               # flush, forward
    assert ((hits['qs'] == 1) & (hits['rs'] == W + PAD)).any() and ((hits['qe'] == W) & (hits['re'] == 1) & (hits['rs'] > 1)).any()      # flush, reverse
    load(ctx, q_seqs, r_seqs)
    got = ctx.rescore_nt(hits, arena)
    expect = np.zeros_like(got)
    expect[:, 0], expect[:, 1] = L_of - 1, 1
    wrong = np.flatnonzero((got != expect).any(axis=1))
    assert len(wrong) == 0, [(hits[k].tolist(), got[k].tolist()) for k in wrong[:5]]
    assert np.array_equal(reference_table(q_seqs, r_seqs, hits, arena), expect)


def test_gap_length_table(ctx):
    """aM gI bM and aM gD bM: the query equals the reference inside the M runs except for one column behind the gap, so a cursor that moves the wrong way,
    or not at all, after the gap run loses nearly all of b's matches"""
    rng = np.random.default_rng(3)
    R = random_bases(rng, 400)
    r_seqs = [R, revcomp(R)]
    q_seqs, rows, arena, expect = [], [], [], []
    for a, b in ((5, 9), (64, 66), (70, 131)):
        for g in (1, 2, 3, 4, 5, 6, 7, 8, 70):
            for kind in 'ID':
                for rev in (0, 1):
                    s = int(rng.integers(0, 40))              # the aligned range is R[s:s + ra]
                    if kind == 'I':
                        q = R[s:s + a] + random_bases(rng, g) + planted(R[s + a:s + a + b], b // 2)
                        ra = a + b
                    else:
                        q = R[s:s + a] + planted(R[s + a + g:s + a + g + b], b // 2)
                        ra = a + g + b
                    head = random_bases(rng, int(rng.integers(0, 4)))
                    q_seqs.append(head + q + random_bases(rng, int(rng.integers(0, 4))))
                    lo, hi = s + 1, s + ra
                    rows.append((len(q_seqs) - 1, rev, len(head) + 1, len(head) + len(q), len(R) - lo + 1 if rev else lo, len(R) - hi + 1 if rev else hi,
                                 3, 0, len(arena)))
                    arena += pack_runs([[a, 'M'], [g, kind], [b, 'M']])
                    expect.append((a + b - 1, 1, 1, g, g if g > 3 else 0))
    hits = hit_table(rows)
    arena = np.array(arena, dtype=np.uint32)
    load(ctx, q_seqs, r_seqs)
    got = ctx.rescore_nt(hits, arena)
    assert got.tolist() == [list(e) for e in expect]
    assert np.array_equal(reference_table(q_seqs, r_seqs, hits, arena), got)


def test_launch_shapes(ctx):
    q_seqs, r_seqs, hits, arena, _ = random_hits(np.random.default_rng(256), 20, 20, 600)
    load(ctx, q_seqs, r_seqs)
    whole = ctx.rescore_nt(hits, arena)
    assert np.array_equal(whole, reference_table(q_seqs, r_seqs, hits, arena))
    for n in (1, 3, 4, 5, 8, 257):
        for first in (0, 11, len(hits) - n):
            part = ctx.rescore_nt(hits[first:first + n], arena)
            assert part.shape == (n, 5) and np.array_equal(part, whole[first:first + n]), (n, first)
    none = ctx.rescore_nt(hits[:0], arena)
    assert none.shape == (0, 5) and none.dtype == np.int64
    assert ctx.rescore_nt(hits[:0], np.zeros(0, np.uint32)).shape == (0, 5)


def test_codes(ctx):
    """every pair of letters as a hit of two columns on either strand: what a letter counts as is read off the restatement's table, the GPU's equals it"""
    letters = 'ACGTNacgtnRY-*7'
    q_seqs = [(x + x).encode() for x in letters]
    r_seqs = [(y + y).encode() for y in letters]
    rows = [(i, j, 1, 2, 2 if rev else 1, 1 if rev else 2, 1, 0, 0) for i in range(len(letters)) for j in range(len(letters)) for rev in (0, 1)]
    hits, arena = hit_table(rows), np.array([2 << 2], dtype=np.uint32)
    load(ctx, q_seqs, r_seqs)
    got = ctx.rescore_nt(hits, arena)
    want = reference_table(q_seqs, r_seqs, hits, arena)
    assert np.array_equal(got, want)
    n = len(letters)
    match = got[:, 0].reshape(n, n, 2)                         # [query letter, reference letter, strand]: 0 or 2
    assert set(match.ravel().tolist()) == {0, 2} and np.array_equal(got[:, 1], 2 - got[:, 0]) and not got[:, 2:].any()
    at = letters.index
    assert match[at('N'), at('N')].tolist() == [2, 2]          # 2 against 2, and against 4 - 2
    for low in 'acgtn':                                        # lower case counts as its upper case
        assert np.array_equal(match[at(low)], match[at(low.upper())]) and np.array_equal(match[:, at(low)], match[:, at(low.upper())])
    for other in 'RY-*7':                                      # every other letter is N's code
        assert np.array_equal(match[at(other)], match[at('N')]) and np.array_equal(match[:, at(other)], match[:, at('N')])
    acgt = [at(x) for x in 'ACGT']
    assert match[np.ix_(acgt, acgt)][:, :, 0].tolist() == (2 * np.eye(4, dtype=int)).tolist()
    assert match[np.ix_(acgt, acgt)][:, :, 1].tolist() == (2 * np.eye(4, dtype=int)[::-1]).tolist()        # A opposite T, C opposite G


def test_float_end_of_the_rescored_table(ctx):
    from peppan_amd import uberBlast as UB
    from peppan_amd.hittable import HitTable
    q_seqs, r_seqs, hits, arena, cov = random_hits(np.random.default_rng(413), 30, 30, 1500)
    q_names, r_names = ['q%03d' % i for i in range(len(q_seqs))], ['r%03d' % i for i in range(len(r_seqs))]
    rb = UB.RunBlast()
    rb.table_id = 11
    rb.qrySeq = {n: s.decode() for n, s in zip(q_names, q_seqs)}
    rb.refSeq = {n: s.decode() for n, s in zip(r_names, r_seqs)}
    n = len(hits)
    z = np.zeros(n)

    def table():
        return HitTable(list(q_names), list(r_names), hits['q'], hits['r'], z, z, z, z, hits['qs'], hits['qe'], hits['rs'], hits['re'], z, z,
                        [len(q_seqs[i]) for i in hits['q']], [len(r_seqs[j]) for j in hits['r']], arena, hits['cigar_off'], hits['cigar_runs'], rid=np.arange(n))
    counts = reference_table(q_seqs, r_seqs, hits, arena)
    want = np.array([reference_identity_score(c) for c in counts])
    assert want.dtype == np.float64 and (counts[:, 4] > 0).sum() >= 20 and len(set(want[:, 0].tolist())) > 100
    T = rb._rescore_table(None, None, table(), 1, None, 11, cut=False, ctx=ctx)
    assert len(T) == n and T.iden.dtype == np.float64 and T.score.dtype == np.float64
    assert np.array_equal(T.iden, want[:, 0]) and np.array_equal(T.score, want[:, 1])
    for min_id in (0.5, 0.9, 1.0):
        keep = np.flatnonzero(want[:, 0] >= min_id)
        assert 0 < len(keep) < n
        cut = rb._rescore_table(None, None, table(), 1, min_id, 11, cut=True, ctx=ctx)
        assert np.array_equal(cut.rid, keep) and np.array_equal(cut.iden, want[keep, 0]) and np.array_equal(cut.score, want[keep, 1])


@pytest.mark.parametrize('mode', [2, 3])
def test_gap_counts_agree_across_the_modes(ctx, mode):
    """k7_table<1> and k7_table<2 | 3> take a hit's gap counts with the same pass: on the fuzz table both files build, columns 2:5 of rescore_nt are
    columns 4:7 of rescore_codons (each side is held to its restatement elsewhere)"""
    rng = np.random.default_rng(413)
    q_seqs, r_seqs, hits, arena, _ = random_hits(rng, 30, 30, 1500)
    q_seqs, r_seqs, hits, arena = with_planted(rng, q_seqs, r_seqs, hits, arena, per_class=6)
    load(ctx, q_seqs, r_seqs)
    gaps = ctx.rescore_nt(hits, arena)[:, 2:5]
    assert len(hits) > 1500 and (gaps[:, 2] > 0).sum() >= 20 and ((gaps[:, 0] > 0) & (gaps[:, 2] == 0)).sum() >= 20
    assert np.array_equal(gaps, ctx.rescore_codons(hits, arena, mode)[:, 4:7])


# ---------------------------------------------------------------------------------------------------------------- k7_hits
@pytest.fixture(scope='module')
def genes_and_contigs():
    """40 genes of 300 - 600 nt and 3 contigs that hold copies of 25 of them each - mutated, with a codon or two deleted and a base triple or two inserted,
    half of them reverse-complemented, some with an N run or a lower-case stretch - between random spacers (which hold stop codons in every frame)"""
    rng = np.random.default_rng(77)
    stops = (b'TAA', b'TAG', b'TGA')

    def gene(n_codons):
        codons = [b'ATG']
        while len(codons) < n_codons - 1:
            c = random_bases(rng, 3)
            if c not in stops:
                codons.append(c)
        return b''.join(codons) + b'TAA'
    genes = [gene(int(rng.integers(100, 201))) for _ in range(40)]

    def copy_of(s):
        s = bytearray(s)
        for k in np.flatnonzero(rng.random(len(s)) < (0., 0.02, 0.04, 0.07)[int(rng.integers(0, 4))]).tolist():
            s[k] = b'ACGT'[int(rng.integers(0, 4))]
        if rng.random() < 0.6:
            a = int(rng.integers(60, len(s) - 60)) // 3 * 3
            del s[a:a + 3 * int(rng.integers(1, 3))]
            b = int(rng.integers(60, len(s) - 60)) // 3 * 3
            s[b:b] = b'GCA' * int(rng.integers(1, 3))
        if rng.random() < 0.3:
            a = int(rng.integers(30, len(s) - 60))
            s[a:a + int(rng.integers(1, 9))] = b'N' * 8
        if rng.random() < 0.3:
            a = int(rng.integers(30, len(s) - 60))
            s[a:a + 25] = bytes(s[a:a + 25]).lower()
        return revcomp(bytes(s)) if rng.random() < 0.5 else bytes(s)
    contigs = []
    for _ in range(3):
        cur = random_bases(rng, int(rng.integers(40, 200)))
        for k in rng.permutation(len(genes))[:25].tolist():
            cur += copy_of(genes[k]) + random_bases(rng, int(rng.integers(40, 200)))
        contigs.append(cur)
    return genes, contigs


@pytest.mark.parametrize('count_on_host', [0, 1])
@pytest.mark.parametrize('tool', [0, 1])
def test_k7_hits_equals_the_restatement(ctx, genes_and_contigs, tool, count_on_host):
    """the count of identical columns the search hands out for hit k against reference_counts over the row pep_table_from_hits makes of hit k: the translated
    tool's template (frames, chunk offsets, runs x 3) and the nucleotide tool's (strands), with the hit count still on the device when the kernel is launched
    (reserved2 = 0) and as a host value (bit 0 set)"""
    from peppan_amd import _native as N
    genes, contigs = genes_and_contigs
    load(ctx, genes, contigs)
    if tool == 0:
        ctx.translate()
        p = N.default_params(40., 25., 10, 5)
    else:
        ctx.use_nt_as_residues(2)
        p = N.nucleotide_params(40., 25.)
    p.reserved2 = count_on_host
    ctx.set_nt_match(True)
    try:
        hits, cig, st = ctx.search(p)
        nt_match = ctx.last_nt_match
    finally:
        ctx.set_nt_match(False)
    tm = ctx.target_meta()
    q_len, r_len = [len(s) for s in genes], [len(s) for s in contigs]
    if tool == 0:
        assert (tm['chunk_off'][hits['t']] > 0).sum() >= 5, 'hits on chunks that do not start their frame'
        cols, arena = N.table_from_hits(0, hits, cig, q_len, r_len, 0, 0, 0, q_meta=ctx.query_meta(), t_meta=tm, nt_match=None)
    else:
        cols, arena = N.table_from_hits(1, hits, cig, q_len, r_len, 0, 0, 0, t_seq=tm['seq'].astype(np.int64), t_rev=tm['frame'] > 3, nt_match=None)
    n = len(hits)
    assert n >= 50 and len(cols['qs']) == n and nt_match is not None and len(nt_match) == n          # no row dropped: row k is hit k
    assert np.array_equal(cols['c_off'], hits['cigar_off'].astype(np.int64))
    assert (cols['ss'] < cols['se']).sum() >= 10 and (cols['ss'] > cols['se']).sum() >= 10 and (cols['c_runs'] > 1).sum() >= 10
    q_enc, r_enc = [encode(s) for s in genes], [encode(s) for s in contigs]
    want = np.zeros(n, dtype=np.int64)
    for k in range(n):
        runs = unpack_runs(arena[int(cols['c_off'][k]):int(cols['c_off'][k]) + int(cols['c_runs'][k])])
        want[k] = reference_counts(q_enc[cols['qi'][k]], r_enc[cols['ri'][k]], int(cols['qs'][k]), int(cols['qe'][k]), int(cols['ss'][k]), int(cols['se'][k]), runs)[0]
    wrong = np.flatnonzero(nt_match.astype(np.int64) != want)
    assert len(wrong) == 0, [(int(k), int(nt_match[k]), int(want[k])) for k in wrong[:5]]
    assert len(set((want * 1000 // np.maximum(cols['aln'], 1)).tolist())) > 10           # (identities of many values)


# ---------------------------------------------------------------------------------------------------------------- errors
def test_error_conventions_and_context_stays_usable(ctx):
    from peppan_amd import _native as N
    q_seqs, r_seqs, hits, arena, _ = random_hits(np.random.default_rng(9), 12, 12, 120)
    load(ctx, q_seqs, r_seqs)
    want = reference_table(q_seqs, r_seqs, hits, arena)

    def raw(c, h, cigar, n_cigar=None):
        out = np.full((len(h), 5), SENTINEL, dtype=np.int64)
        rc = c._lib.pep_rescore_nt(c._h, C.c_uint64(len(h)), N._ptr(h), N._ptr(cigar), C.c_uint64(len(cigar) if n_cigar is None else n_cigar), N._ptr(out))
        return rc, out

    def refused(c, h, cigar, code, text, n_cigar=None):
        rc, out = raw(c, h, cigar, n_cigar)
        assert rc == code and np.all(out == SENTINEL)                                  # nothing written
        with pytest.raises(N.PepError, match=r'pep_rescore_nt failed \(%d\): %s' % (code, text)):
            c._check(rc, 'pep_rescore_nt')
        with pytest.raises(N.PepError, match=text):
            c.rescore_nt(h, cigar[:len(cigar) if n_cigar is None else n_cigar])
        assert np.array_equal(c.rescore_nt(hits, arena), want)                         # ... and the context goes on

    cases = bad_tables('pep_rescore_nt', q_seqs, r_seqs, hits, arena)
    for what, h, cg, n_cigar, text in cases:
        refused(ctx, h, cg, -2, text, n_cigar=n_cigar)
    what, h, _, _, _ = cases[-1]                                                       # the victim's own runs behind the arena: refused with op code 3 ...
    victim = int(np.flatnonzero(h['cigar_off'] != hits['cigar_off'])[0])
    own = arena[int(hits['cigar_off'][victim]):][:int(hits['cigar_runs'][victim])]
    assert what == 'op 3' and np.array_equal(ctx.rescore_nt(h, np.concatenate([arena, own])), want)      # ... and taken as they are
    # before any nucleotide set was given: a context of its own
    with N.Context(0) as fresh:
        rc, out = raw(fresh, hits, arena)
        assert rc == -4 and np.all(out == SENTINEL)
        with pytest.raises(N.PepError, match=r'pep_rescore_nt failed \(-4\): pep_rescore_nt needs pep_set_query_nt and pep_set_ref_nt first'):
            fresh.rescore_nt(hits, arena)
        fresh.set_query_nt(q_seqs, 11)
        with pytest.raises(N.PepError, match=r'\(-4\)'):
            fresh.rescore_nt(hits, arena)
        fresh.set_ref_nt(r_seqs, 6, 11)
        assert np.array_equal(fresh.rescore_nt(hits, arena), want)
