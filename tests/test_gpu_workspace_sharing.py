"""The one workspace slot with a lifetime beyond a call: PEP_WS_HITS_OUT, the hit table a search leaves on the device (search_on_device).  Every
stand-alone call borrows slots of the same pep_ctx::ws and is held below that one by a static_assert; this test pins what those asserts are for, on
the public Python API alone.

    1. context A: search() -> the expected (hits, cigar)
    2. context B, same sets: search_on_device() counts as many
    3. on B, once each: components, overlaps, sha1 + dedup, allele_diff, group_verdicts(detail=True), pair_support, alleles, gene_ingroups and
       rescore_nt (set_query_nt / set_ref_nt upload nucleotides into buffers of their own and queue no search) - checked only to return
    4. result_to_host() on B is A's table byte for byte, and components_of_search labels as it did before step 3
    5. linclust on B runs pep_extend, which rewrites the slot: the table left by a search_on_device is refused with the library's state error
       (PEP_ERR_STATE, -4) by result_to_host and by components_of_search, and neither returns anything
    6. the sets uploaded again (the gapped stage of linclust takes the context's sequence sets over), search() on B is A's table again

Step 5 searches on the device once more before it clusters: result_to_host in step 4 gave the first result a host copy of its own, which the library
rightly keeps handing out whatever happens to the device afterwards; only a result that was never fetched has nothing but the slot.

The sets are 8 proteins of 60 to 120 residues: seven random ones and the first again with two residues cut out of its middle.  Without gaps that
copy matches its original on half of any diagonal, so linclust at 0.9 identity can accept the pair only through its gapped stage - the call of
pep_extend that step 5 is about.  Should the pair not get there, no table is rewritten and step 5 fails."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import similar_helpers as SH  # noqa: E402
import small_kernel_cases as K  # noqa: E402
from divergence_helpers import pack_codes, verdict_table  # noqa: E402

pytestmark = pytest.mark.gpu

PEP_ERR_STATE = -4
AA = 'ACDEFGHIKLMNPQRSTVWY'


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


def proteins(seed):
    """-> (codes letter - 'A' for the search, codes in linclust's alphabet ACDEFGHIKLMNPQRSTVWY)"""
    rng = np.random.default_rng(seed)
    idx = [rng.integers(0, 20, int(rng.integers(62, 119))) for _ in range(7)]
    cut = len(idx[0]) // 2
    idx.append(np.concatenate([idx[0][:cut], idx[0][cut + 2:]]))
    assert all(60 <= len(p) <= 120 for p in idx)
    letters = np.frombuffer(AA.encode(), dtype=np.uint8) - 65
    return [letters[p].astype(np.uint8) for p in idx], [p.astype(np.uint8) for p in idx]


def small_calls(N, ctx):
    """step 3: every stand-alone call that borrows slots of the shared workspace, once, on a handful of rows"""
    from peppan_amd import orthofilter as OF
    c = K.components_cases()[0]
    ctx.components(c['n'], c['a'], c['b'])
    c = K.overlaps_cases()[0]
    ctx.overlaps(c['contig'], c['start'], c['end'], c['rid'], c['ovl_l'], c['ovl_p'])
    texts = [b'ATGAAA', b'', b'ATGAAA', b'ATGAAC' * 20]
    ctx.dedup([len(t) for t in texts], ctx.sha1(texts))
    a, b, far = np.full(305, 1), np.full(305, 1), np.full(305, 3)
    b[:2], b[298:] = 2, 0
    packed, row_off, row_len, index = verdict_table([pack_codes(np.stack([a, b, far]))], [305])
    ctx.allele_diff(packed, row_off, row_len, index, 3)
    gd = OF.gd_table({(1, 3): (0.01, 0.1), (2, 3): (0.01, 0.1)}, 0.002, 3)
    ctx.group_verdicts(packed, row_off, row_len, index, [np.array([1, 2, 3])], [False], gd, 0.002, detail=True)
    sets = {}
    for case in SH.load_g24()['cases']:
        if case['probes'] and not any(p.get('n', 0) > 32768 for p in case['probes']):
            sets.setdefault(SH.params_key(case['params']), []).append(case)
    cases = min(sets.values(), key=lambda cs: sum(len(x['table']) for x in cs))
    rows, cigar, off, gq, gr, _ = SH.k14_inputs(cases)
    ctx.pair_support(rows, cigar, off, gq, gr, N.support_limits(cases[0]['params']))
    c = K.alleles_cases()[0]
    ctx.alleles(c['contigs'], c['rows'], c['cigar'], c['grp_off'], c['grp_qlen'], c['gtable'])
    ctx.gene_ingroups([1, 2], [9000, 8000], [100, 90], [0, 2], OF.gd_table({(1, 2): (0.01, 0.1)}, 0.002, 3), 0.005, 8800.)
    bases = b'ACGTTGCAAGCTTAGGCATC' * 3
    ctx.set_query_nt([bases], 11)
    ctx.set_ref_nt([bases], 6, 11)
    nt_hit = np.array([(0, 0, 1, 60, 1, 60, 1, 0, 0)], dtype=N.NT_HIT_DTYPE)
    ctx.rescore_nt(nt_hit, np.array([60 << 2], dtype=np.uint32))


def test_only_a_search_rewrites_the_table_a_search_left_on_the_device(N):
    prots, clust_codes = proteins(47)
    params = N.default_params()
    node_of_target = 8 + np.arange(8) % 4

    def load(ctx):
        ctx.set_query_aa(prots)
        ctx.set_ref_aa(prots)

    with N.Context(0) as a, N.Context(0) as b:
        load(a)
        hits, cigar, _ = a.search(params)                                   # 1
        assert len(hits) >= 8 + 2 and len(cigar) > len(hits)               # every protein finds itself, the cut copy and its original find each other with a gap
        load(b)
        n_hits, n_cigar = b.search_on_device(params)[:2]                    # 2
        assert (n_hits, n_cigar) == (len(hits), len(cigar))
        labels = b.components_of_search(16, node_of_target)
        small_calls(N, b)                                                   # 3
        got_hits, got_cigar = b.result_to_host()                            # 4
        assert got_hits.tobytes() == hits.tobytes() and got_cigar.tobytes() == cigar.tobytes()
        assert np.array_equal(b.components_of_search(16, node_of_target), labels)
        load(b)                                                             # 5 (a table nobody has fetched)
        assert b.search_on_device(params)[:2] == (len(hits), len(cigar))
        rep, _ = b.linclust(clust_codes, 0.9, 0.8, base=20, k=5, m=20)
        print('linclust representatives: %r' % (rep.tolist(),))
        for fetch in (b.result_to_host, lambda: b.components_of_search(16, node_of_target)):
            with pytest.raises(N.PepError, match=r'failed \(%d\)' % PEP_ERR_STATE):
                fetch()
        load(b)                                                             # 6
        again_hits, again_cigar, _ = b.search(params)
        assert again_hits.tobytes() == hits.tobytes() and again_cigar.tobytes() == cigar.tobytes()
