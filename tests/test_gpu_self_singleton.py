"""The self-search shortcut for buckets of one entry (seeds.hip: PEP_SELF_SAFE, seed_match, seed_match_stride, self_prepare): a position of a target that
repeats its query, in a block marked safe, whose bucket holds exactly one entry, counts one hit and reads no entry.  Every case compares the default path
with the plain stream (params.reserved[0] = 10; 8 for the nucleotide tool) - hit fields, CIGARs and the seed statistics - and, the sets being small, with
the CPU oracle.  The last test needs no GPU: the numpy count of tools/self_singletons.py against a count with Python integers."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENSE = [a + b + c for a in 'ACGT' for b in 'ACGT' for c in 'ACGT' if a + b + c not in ('TAA', 'TAG', 'TGA')]
HIT_FIELDS = ('q', 't', 'q_start', 'q_end', 't_start', 't_end', 'score', 'nm', 'n_ident', 'aln_len', 'cigar_runs', 'bin', 'cigar_off', 'cells')
STATS = ('query_seeds', 'target_seeds', 'seed_hits', 'candidates', 'pairs', 'tracebacks', 'hits', 'cells')
NT_STATS = STATS[1:]


@pytest.fixture(scope='module')
def ctx():
    from peppan_amd import _native as N
    c = N.Context(0)
    yield c
    c.close()


def _tool():
    spec = importlib.util.spec_from_file_location('self_singletons', os.path.join(ROOT, 'tools', 'self_singletons.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _cmp_hits(gh, gc, oh, oc):
    assert len(gh) == len(oh), (len(gh), len(oh))
    for f in HIT_FIELDS:
        assert np.array_equal(gh[f], oh[f]), f
    assert np.array_equal(gc, oc)


def _codons(rng, n):
    return ''.join(SENSE[i] for i in rng.integers(0, len(SENSE), size=n))


def _gene(rng, n_codons, stop='TAA'):
    """ATG, sense codons, a stop: n_codons codons, so n_codons residues with the stop's X"""
    return ('ATG' + _codons(rng, n_codons - 2) + stop).encode()


def _targets(refs):
    """the oracle's target list of a reference set and, per reference gene, the number of the target its frame 1 starts with"""
    from oracle import oracle as O
    t_aa, first = [], []
    for s in refs:
        first.append(len(t_aa))
        for aa in O.translate_frames(s.decode(), range(1, 7), 11):
            t_aa += [O.aa_codes(c) for o, c in O.ref_chunks(aa)]
    return t_aa, first


def _both(ctx, q, r, make_params, inside=False, oracle=True, again=False):
    """default path against the plain stream on the same sets, then against the oracle; returns the default path's result"""
    from oracle import oracle as O
    out = []
    for flag in (0, 10):
        p = make_params()
        p.reserved[0] = flag
        ctx.set_query_nt(q, 11)
        ctx.set_ref_nt(r, 6, 11)
        if inside:
            ctx.invalidate_translation()                      # K1 inside the search
        out.append(ctx.search(p))
        if again and flag == 0:                               # a second search on the same sets without a new translation
            h2, c2, s2 = ctx.search(p)
            _cmp_hits(h2, c2, out[0][0], out[0][1])
            assert all(s2[k] == out[0][2][k] for k in STATS)
    (h1, c1, s1), (h0, c0, s0) = out
    _cmp_hits(h1, c1, h0, c0)
    for k in STATS:
        assert s1[k] == s0[k], (k, s1[k], s0[k])
    if oracle:
        q_aa = [O.aa_codes(O.query_frame(s.decode(), 11)[1]) for s in q]
        t_aa, first = _targets(r)
        op = O.params_from(make_params())
        oh, oc, ost = O.search(q_aa, t_aa, op)
        _cmp_hits(h1, c1, oh, oc)
        assert s1['candidates'] == ost['candidates']
    return h1, c1, s1


def _default(**kw):
    from peppan_amd import _native as N
    return lambda: N.default_params(45., 25., 10, 5, **kw)


def _loose():
    from peppan_amd import _native as N
    return N.default_params(0., 0., 10, 5)


def _triples(rng, behind, a_end='', n=36):
    """n triples (query A, reference gene, query B).  A = ATG + sense codons + a_end with no stop codon, 40 + i residues: the stretch ends at every phase of
    the 32-byte blocks.  The reference gene is A + behind + 12 sense codons + TAA: its frame 1 repeats A and goes on.  B holds the reference's 8 residues in
    front of the end of A and the 7 behind it between flanks of its own, in frame 1: four windows of '111101110111' and one of '111011010010111', every one of
    them across the end of A, none inside A and none behind it - B meets that target through keys that A does not hold and through nothing else."""
    from oracle import oracle as O
    a_genes, refs, b_genes = [], [], []
    for i in range(n):
        a = 'ATG' + _codons(rng, 39 + i - len(a_end) // 3) + a_end
        ref = a + behind + _codons(rng, 12) + 'TAA'
        while True:
            b = 'ATG' + _codons(rng, 7) + ref[len(a) - 24:len(a) + 21] + _codons(rng, 7) + 'TAA'
            if O.query_frame(b, 11)[0] == 1:
                break
        assert O.query_frame(a, 11)[0] == 1
        a_genes.append(a.encode()); refs.append(ref.encode()); b_genes.append(b.encode())
    return a_genes, refs, b_genes


def _hit_pairs(h):
    return set(zip(h['q'].tolist(), h['t'].tolist()))


@pytest.mark.gpu
def test_overhang_target_goes_on_with_seeding_residues(ctx):
    """The case the safe mark exists for.  The target repeats query A and goes on with seeding residues, so windows that start inside the stretch run over its
    end with keys that are not A's: such a key may sit alone in its bucket (then it is B's, or nobody's and the bucket holds a stranger).  A build that takes
    the bucket of one for the self entry without the mark counts hits that are none (seed_hits) and drops B's.  That the inputs hold such windows is counted
    here on the CPU, for the bucket counts around the library's own choice.  Every B must find the target that starts with its A."""
    from oracle import oracle as O
    rng = np.random.default_rng(501)
    a_genes, refs, b_genes = _triples(rng, '')
    tool, p = _tool(), _loose()
    q_aa = [O.aa_codes(O.query_frame(s.decode(), 11)[1]) for s in a_genes + b_genes]
    t_aa, first = _targets(refs)
    for bits in range(tool.bucket_bits_for(q_aa) - 1, tool.bucket_bits_for(q_aa) + 2):
        alone = 0
        for offs in tool.shapes_of(p):
            keys, valid, owner = tool.seed_table(q_aa, offs, list(p.reduce), int(p.base))
            per_bucket = np.bincount(tool.hash_u64(keys[valid], bits), minlength=1 << bits)
            for i in range(len(refs)):
                tk, tv, town = tool.seed_table([t_aa[first[i]]], offs, list(p.reduce), int(p.base))
                ql = len(q_aa[i])
                over = np.arange(max(0, ql - offs[-1]), ql)                     # windows that start inside the stretch and end behind it
                over = over[tv[over]]
                alone += int((per_bucket[tool.hash_u64(tk[over], bits)] == 1).sum())
        assert alone >= 100, (bits, alone)
    h, c, st = _both(ctx, a_genes + b_genes, refs, _loose)
    pairs = _hit_pairs(h)
    for i in range(len(refs)):
        assert (i, first[i]) in pairs and (len(refs) + i, first[i]) in pairs, i


@pytest.mark.gpu
@pytest.mark.parametrize('behind,a_end', [('TAA', ''), ('NNN', ''), ('', 'GNT'), ('GCTNNN', ''), ('ANG', 'NCA')])
def test_stop_or_ambiguous_residue_at_the_end_of_the_stretch(ctx, behind, a_end):
    """the residue behind the stretch is a stop or an ambiguous codon (X, which never seeds), A itself ends in one, the X lies one residue further on, or on
    both sides: the contiguous windows end there, the spaced shapes step over a single X - whatever the mark says, the table and the counts are the plain
    stream's and the oracle's"""
    rng = np.random.default_rng(502)
    a_genes, refs, b_genes = _triples(rng, behind, a_end)
    h, c, st = _both(ctx, a_genes + b_genes, refs, _loose)
    t_aa, first = _targets(refs)
    pairs = _hit_pairs(h)
    assert all((i, first[i]) in pairs for i in range(len(refs)))
    if a_end == '' and behind in ('TAA', 'NNN'):
        # one X behind the stretch: B still meets the target, through the windows of the spaced shapes that step over it - a stop codon alone makes no stretch safe
        assert all((len(refs) + i, first[i]) in pairs for i in range(len(refs)))


@pytest.mark.gpu
def test_buckets_that_are_not_singletons(ctx):
    """duplicate queries, an exact repeat inside a gene longer than the longest shape, families of four, and a random set of 200 genes whose index holds
    buckets of one entry, of several equal keys and of foreign keys side by side (0.25 - 0.5 entries per bucket)"""
    from peppan_amd import synth
    rng = np.random.default_rng(503)
    names, fam = synth.make_genes(48, 300, seed=21)
    fam = [bytes(s) for s in fam]
    fam[10] = fam[11]
    fam[12] = fam[11]
    seg = _codons(rng, 24)
    fam[13] = ('ATG' + _codons(rng, 20) + seg + _codons(rng, 15) + seg + _codons(rng, 9) + 'TAA').encode()
    fam[14] = ('ATG' + seg * 4 + 'TAA').encode()
    h, c, st = _both(ctx, fam, fam, _default())
    assert len(h) > 100
    names, rnd = synth.make_genes(200, 360, seed=22, family=1)
    h, c, st = _both(ctx, [bytes(s) for s in rnd], [bytes(s) for s in rnd], _default())
    assert len(h) >= 200


@pytest.mark.gpu
def test_edges_of_the_marking(ctx):
    """proteins of 31 .. 65 residues (the last block partial, exactly full, absent), a gene shorter than a shape, an empty one, a gene read in frame 2, a gene
    beyond 1 000 codons (its target is not its query: nothing marked), reference sets that differ in order, a base, a gene and number, partial query sets"""
    from peppan_amd import synth
    rng = np.random.default_rng(504)
    seqs = [_gene(rng, n) for n in (31, 32, 33, 63, 64, 65, 47, 48, 49, 16, 17)]
    seqs += [b'ATGAAATAA', b'', b'C' + _gene(rng, 80), _gene(rng, 1402), b'ATGTAATAGTGA' + _gene(rng, 70)[12:]]
    seqs += [bytes(s) for s in synth.make_genes(24, 270, seed=23)[1]]
    h, c, st = _both(ctx, seqs, seqs, _default())
    assert len(h) >= 30
    other = list(seqs); other[20] = seqs[21]
    base = list(seqs); base[3] = seqs[3][:40] + (b'A' if seqs[3][40:41] != b'A' else b'C') + seqs[3][41:]
    for q, r in ((seqs, other), (seqs, base), (seqs, seqs[::-1]), (seqs, seqs[:-1]), (seqs, seqs + [seqs[0]]), (seqs[:9], seqs), (seqs[14:30], seqs)):
        _both(ctx, q, r, _default())


@pytest.mark.gpu
def test_shapes_and_build_paths(ctx):
    """four shapes; the plain index build; a second search without a new translation; K1 inside the search"""
    from peppan_amd import _native as N, synth
    seqs = [bytes(s) for s in synth.make_genes(120, 300, seed=24)[1]]
    h, c, st = _both(ctx, seqs, seqs, _default(sensitive=True), again=True)

    def plain_build():
        p = N.default_params(45., 25., 10, 5)
        p.reserved[2] = 1
        return p
    h1, c1, st1 = _both(ctx, seqs, seqs, plain_build)
    h2, c2, st2 = _both(ctx, seqs, seqs, _default(), inside=True, again=True)
    _cmp_hits(h1, c1, h2, c2)
    assert all(st1[k] == st2[k] for k in STATS) and len(h2) > 300


@pytest.mark.gpu
def test_nucleotide_tool_self_search(ctx):
    """seed_match_stride in the tool's own layout (forward strands, then reverse complements: the forward strand of reference gene g is query g): a probe in
    a safe block whose 14-mer bucket holds one entry counts the 17-mers it owns and reads no entry.  Exact runs of 13 .. 22 bases of other genes planted at
    every phase of the stride, an ambiguous stretch, duplicates, a tiny and an empty gene; references that differ in a gene, a base, a length, order and number"""
    from peppan_amd import _native as N, synth
    from oracle import oracle as O
    rng = np.random.default_rng(505)
    names, seqs = synth.make_genes(260, 0, seed=78)
    seqs = [bytearray(x) for x in seqs]
    n = 0
    for ln in range(13, 23):
        for ph in range(4):
            src, dst = seqs[200 + n % 40], seqs[40 + n]
            at, to = int(rng.integers(1, len(src) - ln - 1)), 60 + 4 * int(rng.integers(0, 10)) + ph
            dst[to:to + ln] = src[at:at + ln]
            for x, y in ((to - 1, at - 1), (to + ln, at + ln)):          # the bases right outside the run differ from the source's
                dst[x] = b'ACGT'[(b'ACGT'.index(src[y]) + 1) % 4]
            n += 1
    seqs = [bytes(x) for x in seqs]
    seqs[5] = seqs[5][:200] + b'NNNN' + seqs[5][204:]
    seqs[6] = seqs[7]
    seqs[8] = b'ACGTACGTACGTACGTAC'
    seqs[9] = b''
    other = list(seqs); other[20] = seqs[21]
    base = list(seqs); base[30] = seqs[30][:40] + (b'A' if seqs[30][40:41] != b'A' else b'C') + seqs[30][41:]
    longer = list(seqs); longer[41] = seqs[41] + b'ACGTTGCA'
    first = None
    for ref in (seqs, other, base, longer, seqs[::-1], seqs[:-3], seqs + [seqs[0]]):
        res = {}
        for flag in (0, 8):
            p = N.nucleotide_params(70., 25.)
            p.reserved[0] = flag
            ctx.set_query_nt(seqs, 11); ctx.set_ref_nt(ref, 6, 11); ctx.use_nt_as_residues(2)
            gh, gc, st = ctx.search(p)
            res[flag] = (gh.tobytes(), gc.tobytes()) + tuple(st[k] for k in NT_STATS)      # (query_seeds: the stride matcher's index holds 14-mers, the plain one 17-mers)
        assert res[0] == res[8], (len(ref), res[0][2:], res[8][2:])
        first = first or res[0]
    rc = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
    codes = [O.nt_codes(x.upper()) for x in seqs]
    p = N.nucleotide_params(70., 25.)
    ms = np.array([O.min_score(len(c), p.dbsize, p.max_evalue, p.ka_lambda, p.ka_k) for c in codes], dtype=np.int32)
    oh, oc, ost = O.search(codes, codes + [rc[c[::-1]] for c in codes], O.params_from(p), min_scores=ms)
    _cmp_hits(np.frombuffer(first[0], dtype=N.HIT_DTYPE), np.frombuffer(first[1], dtype=np.uint32), oh, oc)
    assert first[2 + NT_STATS.index('candidates')] == ost['candidates'] and first[2 + NT_STATS.index('seed_hits')] > 50000


def test_singleton_count_of_the_tool_equals_a_brute_force_count():
    """tools/self_singletons.py: the numpy count (the library's key and hash_u64 restated) against one position at a time with Python integers, 20 genes with a
    duplicate, a family and a gene that is not its own target; small and large bucket counts, so that shared buckets occur"""
    from peppan_amd import _native as N, synth
    tool = _tool()
    seqs = [bytes(s) for s in synth.make_genes(20, 240, seed=25)[1]]
    seqs[3] = seqs[4]
    seqs[5] = b'C' + seqs[5]
    prots, is_self = tool.query_proteins(seqs)
    assert sum(is_self) >= 15 and not all(is_self)
    p = N.default_params(45., 25., 10, 5)
    assert tool.shapes_of(p) == [[k for k, ch in enumerate(s) if ch == '1'] for s in N.DEFAULT_SHAPES]
    seen = set()
    for offs in tool.shapes_of(p):
        for bits in (10, 12, tool.bucket_bits_for(prots)):
            fast = tool.count_shape(prots, is_self, offs, list(p.reduce), int(p.base), bits)
            assert fast == tool.count_shape_brute(prots, is_self, offs, list(p.reduce), int(p.base), bits), (offs, bits)
            assert 0 < fast[1] <= fast[2] <= fast[0]
            seen.add(fast[1] < fast[2])
    assert True in seen                                    # at 2^10 buckets unique keys share buckets
