"""K1 on sets of genes: the reference side as a layout launch and a pack launch with one wavefront per gene (k1_ref_layout, k1_pack_ref), the
stop search (k1_ref_chunks) over the frames of more than 1000 characters alone; the query side at the same shapes.  Every packed sequence of
every case is held to the oracle's restatement of the reference - oracle.query_frame, oracle.translate_frames, oracle.ref_chunks - with 6 and
with 3 reference frames, with translation tables 11 and 4; nothing is sampled.  The residues are fetched from the device at the offsets the
host derives from the descriptors, so a packed sequence that the device laid out elsewhere shows as wrong residues; what the seed stage reads
of the layout (pk_off, blk2seq, d_self_t) is held to the oracle by a search over K1's products, and by a search after one side alone was
translated again.

The shapes are the smallest at which those paths can go wrong: lengths 0 - 8 and empty sequences at either end of a set and between two
others; frame lengths on both sides of a multiple of 16 (the padded length follows the chosen frame); lengths around the 1 536-byte window of
the query side and around the 4 608 nucleotides up to which a reference gene is staged whole (GENE_NT); frames of 1000 / 1001 characters and a
stop planted at positions 999, 1000 and 1001 of a frame; stop-free and stop-rich sequences of several chunks; a contig beyond 3 x K1_LONG
nucleotides, which sends the whole set down the path of the long frames, in every order with genes and medium sequences; lower case, N and
'-' anywhere; sets of no and of one sequence on either side."""
import itertools
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GENE_NT = 4608                      # translate.hip: K1_GENE_NT
K1_LONG = 98304                     # translate.hip: characters of a frame (+ 'X') from which it is a long one
COMBOS = [(6, 11), (3, 11), (6, 4), (3, 4)]
RNG = np.random.default_rng(2024)
ACGT = np.frombuffer(b'ACGT', dtype=np.uint8)
NOISY = np.array(list('ACGT' * 12 + 'acgt' * 3 + 'NnRY-'))
_EXPECT = {}                        # (sequence, table) -> what the oracle makes of it, computed once


@pytest.fixture(scope='module')
def ctx():
    from peppan_amd import _native as N
    c = N.Context(0)
    yield c
    c.close()


def plain(n):
    return bytes(RNG.choice(ACGT, size=n))


def noisy(n):
    return ''.join(RNG.choice(NOISY, size=n)).encode()


def stop_free(n):
    """no stop codon in any forward frame (a C can be part of none); the reverse frames have plenty"""
    return plain(n).replace(b'TAA', b'TCA').replace(b'TAG', b'TCG').replace(b'TGA', b'TCA')


def planted(n, frame, pos):
    """stop-free but for one TAA at character `pos` of forward frame `frame`"""
    s = bytearray(stop_free(n))
    at = frame - 1 + 3 * pos
    s[at:at + 3] = b'TAA'
    if at:
        s[at - 1:at] = b'C'         # (no second stop across the planted one's edges)
    s[at + 3:at + 4] = b'C'
    return bytes(s)


def codes(aa):
    from oracle import oracle as O
    return O.aa_codes(aa.replace('-', 'X'))


def expect(seq, table):
    """(chosen query frame, its residues, per frame 1 .. 6 the chunks [(offset, residues)]) of one sequence"""
    from oracle import oracle as O
    key = (seq, table)
    if key not in _EXPECT:
        txt = seq.decode()
        f, aa = O.query_frame(txt, table)
        frames = O.translate_frames(txt, range(1, 7), table)
        _EXPECT[key] = (f, codes(aa), [[(o, codes(c)) for o, c in O.ref_chunks(a)] for a in frames])
    return _EXPECT[key]


def check_query(ctx, seqs, table):
    qm = ctx.query_meta()
    qa, qo = ctx.query_aa()
    assert len(qm) == len(seqs) and len(qo) == len(seqs) + 1
    want = [expect(s, table) for s in seqs]
    assert [int(m['seq']) for m in qm] == list(range(len(seqs)))
    assert [int(m['frame']) for m in qm] == [w[0] for w in want]
    assert [int(m['aa_len']) for m in qm] == [len(w[1]) for w in want]
    assert [int(m['nt_len']) for m in qm] == [len(s) for s in seqs]
    assert np.array_equal(np.diff(qo.astype(np.int64)), [len(w[1]) for w in want])
    for i, w in enumerate(want):
        assert np.array_equal(qa[int(qo[i]):int(qo[i + 1])], w[1]), (table, i, len(seqs[i]))


def check_ref(ctx, seqs, frames, table):
    tm = ctx.target_meta()
    ta, to = ctx.target_aa()
    exp = [(n, f + 1, o, c) for n, s in enumerate(seqs) for f in range(frames) for o, c in expect(s, table)[2][f]]
    got = [(int(m['seq']), int(m['frame']), int(m['chunk_off']), int(m['aa_len'])) for m in tm]
    assert got == [(n, f, o, len(c)) for n, f, o, c in exp], (frames, table)
    assert len(to) == len(exp) + 1 and np.array_equal(np.diff(to.astype(np.int64)), [len(c) for n, f, o, c in exp])
    for i, (n, f, o, c) in enumerate(exp):
        assert np.array_equal(ta[int(to[i]):int(to[i + 1])], c), (frames, table, n, f, o, len(seqs[n]))
    return len(exp)


def run(ctx, q, r):
    """both sides through K1 in all four combinations, every packed sequence compared; returns the number of targets of the last one"""
    n_t = 0
    for frames, table in COMBOS:
        ctx.set_query_nt(q, table)
        ctx.set_ref_nt(r, frames, table)
        ctx.translate(force=True)
        check_query(ctx, q, table)
        n_t = check_ref(ctx, r, frames, table)
    return n_t


def shuffled(seqs):
    return [seqs[i] for i in RNG.permutation(len(seqs))]


# ---- the sets, made once
TINY = [plain(n) for n in range(0, 9)] + [noisy(n) for n in range(1, 9)]
GENES = [plain(int(n)) for n in RNG.integers(150, 1300, 12)]
EDGES = ([plain(n) for n in list(range(43, 52)) + list(range(91, 100)) + list(range(1530, 1542))] +            # frames of 15 - 17, 31 - 33, 510 - 514 characters
         [plain(n) for n in range(GENE_NT - 4, GENE_NT + 6)] + [noisy(n) for n in (47, 96, 1535, 1538, GENE_NT - 1, GENE_NT, GENE_NT + 1)])
CUTS = ([plain(n) for n in range(2998, 3005)] + [stop_free(n) for n in (2999, 3000, 3001, 3003, 3004)] +         # na = 1000 / 1001 / 1002 with and without stops
        [planted(3300, f, p) for f in (1, 2, 3) for p in (999, 1000, 1001)] +
        [stop_free(6200), plain(7000), noisy(7000), stop_free(GENE_NT), stop_free(GENE_NT + 3)])
CONTIG = plain(3 * K1_LONG + 1500)


def test_lengths_0_to_8_and_empty_sequences(ctx):
    """frames of no character make no packed sequence: an empty gene between two others, at the head and at the tail of the set, a set of
    nothing but empty genes (no target at all), every length up to 8"""
    a, b, c = GENES[:3]
    assert run(ctx, [a, b'', b], [a, b'', b]) == run(ctx, [a, b], [a, b])
    run(ctx, [b''] + TINY + [c], [b''] + TINY + [c])
    run(ctx, TINY + [c, b''], [c] + TINY[::-1] + [b''])
    assert run(ctx, [b'', b'', b''], [b'', b'']) == 0
    assert run(ctx, [b'A', b'', b'AC'], [b'', b'A', b'']) == 1
    run(ctx, shuffled(TINY + GENES[:5] + [b''] * 3), shuffled(TINY + GENES[:5] + [b''] * 3))


def test_padding_and_window_edges(ctx):
    """frame lengths on both sides of a multiple of 16, of the query side's window (1 530 - 1 541 nt) and of the staging area of a reference
    gene (GENE_NT): the sequences beyond it are packed by a wavefront per packed sequence in the same launch"""
    assert any(len(s) > GENE_NT for s in EDGES) and any(len(s) == GENE_NT for s in EDGES)
    run(ctx, EDGES, EDGES)
    run(ctx, shuffled(EDGES + GENES), shuffled(EDGES + GENES + TINY))
    run(ctx, [s for s in EDGES if len(s) > GENE_NT], [s for s in EDGES if len(s) > GENE_NT])          # no gene at all on the one-wavefront path


def test_the_single_chunk_limit(ctx):
    """frames of 1000 characters are one chunk whatever their text, frames of 1001 are cut where the reference cuts them: a stop planted at
    characters 999, 1000 and 1001, stop-free sequences (one chunk of up to 2 066 characters), sequences with stops (several chunks)"""
    n_t = run(ctx, CUTS, CUTS)
    assert n_t > 3 * len(CUTS)
    # what the planted stops do to frame 1 (1 100 characters): at 999 it lies in front of the first place a cut may fall - one chunk; at 1000 and 1001 it cuts
    assert [len(expect(CUTS[k], 11)[2][0]) for k in (12, 13, 14)] == [1, 2, 2]
    assert [len(c) for o, c in expect(CUTS[13], 11)[2][0]] == [1001, 99] and [len(c) for o, c in expect(CUTS[14], 11)[2][0]] == [1002, 98]
    assert [len(c) for o, c in expect(CUTS[7], 11)[2][0]] == [1000] and [len(c) for o, c in expect(CUTS[9], 11)[2][0]] == [1001]          # stop-free 2 999 / 3 001 nt
    run(ctx, shuffled(CUTS + GENES[:6] + TINY[:6]), shuffled(CUTS + GENES[:6] + TINY[:6]))


@pytest.mark.parametrize('order', list(itertools.permutations('smc')), ids=''.join)
def test_genes_medium_sequences_and_a_contig(ctx, order):
    """a contig with long frames sends the whole reference set down the path of the long frames, wherever it stands; the query side packs it
    window by window; without it the same set takes the gene path"""
    kinds = dict(s=GENES[:4] + TINY[3:6], m=[CUTS[0], CUTS[13], CUTS[-5], EDGES[-1]], c=[CONTIG])
    seqs = [s for k in order for s in kinds[k]]
    assert (len(CONTIG) + 2) // 3 + 1 > K1_LONG
    run(ctx, seqs, seqs)
    if order[0] == 'c':
        run(ctx, seqs[1:], seqs[1:])                         # and back on the gene path with the same context


def test_no_sequence_and_one_sequence_on_either_side(ctx):
    one_short, one_cut, one_big = GENES[0], CUTS[13], EDGES[-1]
    for q, r in (([], GENES[:3]), (GENES[:3], []), ([], []), ([one_short], GENES[:3]), (GENES[:3], [one_short]), ([one_cut], [one_cut]),
                 ([one_big], [one_big]), ([b''], [one_short]), ([one_short], [b''])):
        run(ctx, q, r)


def test_input_variants_in_any_order(ctx):
    """lower case, N, '-' and unaligned starts: noisy text of every kind of length, in a random order (the sequences start at any byte)"""
    seqs = [noisy(n) for n in list(range(9, 41)) + [333, 1001, 1534, 1537, 1539, 3001, 3004, 3330, GENE_NT - 2, GENE_NT, GENE_NT + 2, 5000, 6150]]
    run(ctx, shuffled(seqs), shuffled(seqs + GENES[:4]))


def _family():
    """about 60 genes of mixed lengths that find each other: members of one family are copies of a root with substitutions"""
    roots = [plain(n) for n in (300, 46, 98, 1002, 1533, 1537, 1540, 2999, 3001, 3004, GENE_NT - 3, GENE_NT, GENE_NT + 3)] + \
        [stop_free(3300), planted(3300, 1, 1000), stop_free(6200), plain(7000)]
    out = []
    for root in roots:
        for _ in range(3):
            s = np.frombuffer(root, dtype=np.uint8).copy()
            hit = RNG.random(len(s)) < 0.05
            s[hit] = RNG.choice(ACGT, size=int(hit.sum()))
            out.append(s.tobytes())
    return out + [b'', plain(5), noisy(900)]


FAMILY = _family()


def _oracle_sets(q, r, frames, table):
    q_aa = [expect(s, table)[1] for s in q]
    t_aa = [c for s in r for f in range(frames) for o, c in expect(s, table)[2][f]]
    return q_aa, t_aa


def _cmp_hits(gh, gc, oh, oc):
    assert len(gh) == len(oh), (len(gh), len(oh))
    for f in ('q', 't', 'q_start', 'q_end', 't_start', 't_end', 'score', 'nm', 'n_ident', 'aln_len', 'cigar_runs', 'bin', 'cigar_off', 'cells'):
        assert np.array_equal(gh[f], oh[f]), f
    assert np.array_equal(gc, oc)


def test_a_search_over_the_products_of_k1(ctx):
    """the seed stage and the alignment passes read pk_off, blk2seq, the lengths and d_self_t as K1 left them on the device: a self-search from
    nucleotides against the oracle's search over the oracle's translations"""
    from peppan_amd import _native as N
    from oracle import oracle as O
    assert 50 <= len(FAMILY) <= 70
    for frames, table in COMBOS:
        ctx.set_query_nt(FAMILY, table)
        ctx.set_ref_nt(FAMILY, frames, table)
        gh, gc, st = ctx.search(N.default_params(45., 25., 10, 5))
        q_aa, t_aa = _oracle_sets(FAMILY, FAMILY, frames, table)
        oh, oc, ost = O.search(q_aa, t_aa, O.default_params(45., 25., 10, 5))
        _cmp_hits(gh, gc, oh, oc)
        assert len(gh) > 2 * len(FAMILY) and st['cells'] == ost['cells']
        check_query(ctx, FAMILY, table)
        check_ref(ctx, FAMILY, frames, table)


def test_one_side_translated_again_after_a_search(ctx):
    """new queries after a search: only the query side runs through K1 again (and then only the reference side); hits, CIGARs and every
    product equal what a fresh context makes of the last sets, and what the oracle makes of them"""
    from peppan_amd import _native as N
    from oracle import oracle as O
    p = N.default_params(45., 25., 10, 5)
    others = FAMILY[7:40][::-1]
    refs2 = FAMILY[20:] + GENES[:3]

    def state(c):
        h, cg, st = c.search(p)
        qa, ta = c.query_aa(), c.target_aa()
        return h, cg, (c.query_meta().tobytes(), c.target_meta().tobytes(), qa[0].tobytes(), qa[1].tobytes(), ta[0].tobytes(), ta[1].tobytes())

    ctx.set_query_nt(FAMILY, 11)
    ctx.set_ref_nt(FAMILY, 6, 11)
    h0, _, _ = ctx.search(p)
    assert len(h0) > 2 * len(FAMILY)
    for q, r, give in ((others, FAMILY, lambda c: c.set_query_nt(others, 11)), (others, refs2, lambda c: c.set_ref_nt(refs2, 6, 11))):
        give(ctx)
        h, cg, rest = state(ctx)
        with N.Context(0) as f:
            f.set_query_nt(q, 11)
            f.set_ref_nt(r, 6, 11)
            fh, fc, frest = state(f)
        assert h.tobytes() == fh.tobytes() and cg.tobytes() == fc.tobytes() and rest == frest
        q_aa, t_aa = _oracle_sets(q, r, 6, 11)
        oh, oc, _ = O.search(q_aa, t_aa, O.default_params(45., 25., 10, 5))
        _cmp_hits(h, cg, oh, oc)
        assert len(h) > len(q)
