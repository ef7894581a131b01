"""The state of a context's two packed sequence sets ("State of the sequence sets"): a context that reached its current sets by any
route gives what a fresh context gives when handed only those last sets - the hit table and the CIGAR arena, the statistics that
test_k1_inside_the_search_equals_translate_in_front compares, the meta records and the packed residues of both sides, byte for byte.  The fresh
context translates in front of its search (translate(), or use_nt_as_residues for the nucleotide tool): what the parity tests hold to the oracle.

Inputs: twelve random genes of 150 - 600 nt with start and stop codon, one of 3 306 nt (a reference frame of two chunks: K1's chunk tables and
target_meta's chunk offsets matter), an empty one and one of 2 nt; the proteins of the first five for the residue routes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PEP_ERR_ARG, PEP_ERR_STATE = -2, -4
KEYS = ('candidates', 'pairs', 'tracebacks', 'hits', 'cells', 'query_residues', 'target_residues', 'query_seeds', 'target_seeds', 'seed_hits')
PARTS = ('hits', 'cigar', 'stats', 'query_meta', 'target_meta', 'query_aa', 'target_aa')
AA = 'ACDEFGHIKLMNPQRSTVWY'


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


def make_genes():
    rng = np.random.default_rng(20)
    sense = [a + b + c for a in 'ACGT' for b in 'ACGT' for c in 'ACGT' if a + b + c not in ('TAA', 'TAG', 'TGA')]

    def gene(n_codons):
        return ('ATG' + ''.join(sense[i] for i in rng.integers(0, len(sense), n_codons)) + 'TAA').encode()

    genes = [gene(int(n)) for n in rng.integers(48, 199, 12)]       # 150 .. 600 nt
    genes.append(gene(1100))                                        # 3 306 nt: 1 102 residues per frame, two chunks
    genes += [b'', b'AT']
    assert all(150 <= len(g) <= 600 for g in genes[:12]) and len(genes[12]) > 3003
    return genes


GENES = make_genes()
A, R = GENES, GENES
B = GENES[3:9]                                      # fewer queries than A
R2 = GENES[::-1]
GROUPS = [0] * 5 + [1] * 5 + [2] * 5
GROUPS2 = [0] * 8 + [1] * 7
FRESH = {}                                          # what the fresh contexts gave, computed once per set of inputs


def real(seqs):
    return sum(1 for s in seqs if len(s) >= 50)


def state(ctx, params, n_real):
    """one search and everything a caller can see of the sets afterwards; n_real: the queries that must have found something (every
    non-degenerate one finds at least itself in these sets) - no comparison of trivially empty tables"""
    h, c, st = ctx.search(params)
    assert len(np.unique(h['q'])) >= n_real and (n_real == 0 or len(c) >= len(h) > 0), (len(h), len(c), n_real)
    qa, ta = ctx.query_aa(), ctx.target_aa()
    return dict(hits=h.tobytes(), cigar=c.tobytes(), stats=tuple(st[k] for k in KEYS), query_meta=ctx.query_meta().tobytes(),
                target_meta=ctx.target_meta().tobytes(), query_aa=(qa[0].tobytes(), qa[1].tobytes()), target_aa=(ta[0].tobytes(), ta[1].tobytes()))


def same(got, want, what):
    for part in PARTS:
        assert got[part] == want[part], (what, part)


def fresh(N, key, give, params, n_real, front='translate'):
    """a fresh context handed only the last sets (give), translated in front of its search"""
    if key not in FRESH:
        with N.Context(0) as f:
            give(f)
            if front == 'translate':
                f.translate()
            else:
                f.use_nt_as_residues(front)
            FRESH[key] = state(f, params, n_real)
    return FRESH[key]


def give_nt(q, r, groups=None):
    def give(ctx):
        ctx.set_query_nt(q, 11)
        ctx.set_ref_nt(r, 6, 11)
        if groups is not None:
            ctx.set_target_groups(groups)
    return give


def proteins(N, params):
    """the translations of the first five genes, as K1 made them"""
    codes, off = fresh(N, 'A,R', give_nt(A, R), params, real(A))['query_aa']
    codes, off = np.frombuffer(codes, dtype=np.uint8), np.frombuffer(off, dtype=np.uint64)
    return [codes[int(off[i]):int(off[i + 1])].copy() for i in range(5)]


def give_aa(q, r_aa=None, r_nt=None):
    def give(ctx):
        ctx.set_query_aa(q)
        if r_aa is not None:
            ctx.set_ref_aa(r_aa)
        else:
            ctx.set_ref_nt(r_nt, 6, 11)
    return give


def gapped_pair():
    """8 proteins in linclust's alphabet, the last one the first with two residues cut out of its middle (test_gpu_workspace_sharing.py): at 0.9
    identity only the gapped stage can accept that pair"""
    rng = np.random.default_rng(47)
    idx = [rng.integers(0, 20, int(rng.integers(62, 119))) for _ in range(7)]
    cut = len(idx[0]) // 2
    idx.append(np.concatenate([idx[0][:cut], idx[0][cut + 2:]]))
    return [p.astype(np.uint8) for p in idx]


def takeover(ctx):
    rep, st = ctx.linclust(gapped_pair(), 0.9, 0.8, base=20, k=5, m=20)
    print('linclust representatives: %r, stats %r' % (rep.tolist(), st))
    assert st['accepted'] >= 1 and rep[7] == rep[0]             # the gapped stage ran and took the context's sets over


def test_k1_inside_the_search_equals_translate_in_front(N):
    p = N.default_params(45., 25., 10, 5)
    want = fresh(N, 'A,R', give_nt(A, R), p, real(A))
    with N.Context(0) as ctx:
        give_nt(A, R)(ctx)
        same(state(ctx, p, real(A)), want, 'K1 inside the search, the reference side taken late')
        ctx.set_query_nt(B, 11)                                  # only the query side is replaced
        same(state(ctx, p, real(B)), fresh(N, 'B,R', give_nt(B, R), p, real(B)), 'new queries, the reference side kept')
        ctx.set_ref_nt(R2, 6, 11)                                # only the reference side
        same(state(ctx, p, real(B)), fresh(N, 'B,R2', give_nt(B, R2), p, real(B)), 'new reference set, the queries kept')
    with N.Context(0) as ctx:
        ctx.set_timing(2)                                        # the search translates through pep_translate
        give_nt(A, R)(ctx)
        same(state(ctx, p, real(A)), want, 'set_timing(2)')
    with N.Context(0) as ctx:
        give_nt(A, R, GROUPS)(ctx)                               # target groups: no side is left queued
        same(state(ctx, p, real(A)), fresh(N, 'A,R,groups', give_nt(A, R, GROUPS), p, real(A)), 'set_target_groups')


def test_new_queries_leave_the_reference_side_readable(N):
    """fewer queries given after a search: the reference side's tables are built without a look at the query side, whose own are refused
    until it is translated again"""
    p = N.default_params(45., 25., 10, 5)
    want = fresh(N, 'B,R', give_nt(B, R), p, real(B))
    with N.Context(0) as ctx:
        give_nt(A, R)(ctx)
        h, _, _ = ctx.search(p)
        assert len(np.unique(h['q'])) >= real(A)
        ctx.set_query_nt(B, 11)
        ta = ctx.target_aa()
        assert ctx.target_meta().tobytes() == want['target_meta'] and (ta[0].tobytes(), ta[1].tobytes()) == want['target_aa']
        with pytest.raises(N.PepError, match=r'failed \(%d\)' % PEP_ERR_STATE):
            ctx.query_meta()
        same(state(ctx, p, real(B)), want, 'the search after the getters')


def test_source_changes(N):
    p = N.default_params(45., 25., 10, 5)
    prots = proteins(N, p)
    nt_nt = fresh(N, 'A,R', give_nt(A, R), p, real(A))
    with N.Context(0) as ctx:
        give_aa(prots, r_aa=prots)(ctx)
        same(state(ctx, p, 5), fresh(N, 'P,P', give_aa(prots, r_aa=prots), p, 5), 'residues on both sides')
        give_nt(A, R)(ctx)
        same(state(ctx, p, real(A)), nt_nt, 'residues, then nucleotides on both sides')
        ctx.set_query_aa(prots)
        same(state(ctx, p, 5), fresh(N, 'P,R', give_aa(prots, r_nt=R), p, 5), 'residue queries, the nucleotide reference kept')
        ctx.set_query_nt(A, 11)
        same(state(ctx, p, real(A)), nt_nt, 'and back')


def test_the_nucleotide_tool_and_the_translated_search_in_turn(N):
    p, pn = N.default_params(45., 25., 10, 5), N.nucleotide_params(70., 25.)
    with N.Context(0) as ctx:
        give_nt(A, R)(ctx)
        ctx.use_nt_as_residues(2)
        first = state(ctx, pn, real(A))
        same(first, fresh(N, 'nucl A,R 2', give_nt(A, R), pn, real(A), front=2), 'use_nt_as_residues(2)')
        ctx.translate()                                          # K1 reruns by itself: the packed sets held base codes
        same(state(ctx, p, real(A)), fresh(N, 'A,R', give_nt(A, R), p, real(A)), 'the translated search on the same sets')
        ctx.use_nt_as_residues(2)
        same(state(ctx, pn, real(A)), first, 'the kept layout')
        ctx.set_target_groups(GROUPS2)
        ctx.use_nt_as_residues(2)
        same(state(ctx, pn, real(A)), fresh(N, 'nucl A,R,groups2 2', give_nt(A, R, GROUPS2), pn, real(A), front=2), 'target groups changed')
        ctx.use_nt_as_residues(1)
        same(state(ctx, pn, real(A)), fresh(N, 'nucl A,R,groups2 1', give_nt(A, R, GROUPS2), pn, real(A), front=1), 'strands 1 after 2')


def test_k9_takes_the_sets_over(N):
    p = N.default_params(45., 25., 10, 5)
    prots = proteins(N, p)
    with N.Context(0) as ctx:
        give_nt(A, R)(ctx)
        before = state(ctx, p, real(A))
        takeover(ctx)
        after = state(ctx, p, real(A))                           # nucleotide sources: K1 runs again by itself
        same(after, before, 'the search after linclust')
        same(after, fresh(N, 'A,R', give_nt(A, R), p, real(A)), 'the search after linclust')
    with N.Context(0) as ctx:
        give_aa(prots, r_aa=prots)(ctx)
        takeover(ctx)
        with pytest.raises(N.PepError, match=r'failed \(%d\)' % PEP_ERR_STATE):
            ctx.search(p)                                        # residue sources: the sets have to be given again
        give_aa(prots, r_aa=prots)(ctx)
        same(state(ctx, p, 5), fresh(N, 'P,P', give_aa(prots, r_aa=prots), p, 5), 'the sets given again')


def test_failures_on_the_way(N):
    p = N.default_params(45., 25., 10, 5)
    want = fresh(N, 'A,R', give_nt(A, R), p, real(A))
    with N.Context(0) as ctx:
        ctx.set_query_nt(A, 11)
        with pytest.raises(N.PepError, match=r'failed \(%d\)' % PEP_ERR_STATE):
            ctx.search(p)                                        # queries only
        ctx.set_ref_nt(R, 6, 11)
        same(state(ctx, p, real(A)), want, 'the reference set given after the failure')
        ctx.invalidate_translation()
        bad = N.default_params(45., 25., 10, 5)
        bad.n_shapes = 0
        with pytest.raises(N.PepError, match=r'failed \(%d\)' % PEP_ERR_ARG):
            ctx.search(bad)
        same(state(ctx, p, real(A)), want, 'the valid search after the refused one')


@pytest.mark.parametrize('q, r', [([], R), (A, [])], ids=['no queries', 'no reference'])
def test_an_empty_side(N, q, r):
    p = N.default_params(45., 25., 10, 5)
    key = 'empty %d,%d' % (len(q), len(r))
    want = fresh(N, key, give_nt(q, r), p, 0)
    assert want['stats'][KEYS.index('hits')] == 0 and want['hits'] == b''
    with N.Context(0) as ctx:
        give_nt(q, r)(ctx)
        same(state(ctx, p, 0), want, 'K1 inside the search')
        ctx.translate(force=True)
        same(state(ctx, p, 0), want, 'translate() in front')
