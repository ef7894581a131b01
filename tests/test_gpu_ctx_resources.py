"""What a context takes from the GPU it gives back: pep_live_resources (bytes of device buffers, bytes of pinned host buffers, HIP events the library
holds in the process) before a context is made, while it lives and after pep_ctx_destroy.

The context is driven through every corner that owns something: the phase timers' events, the staging areas of uploads and of the hit table, K10 over
a device-resident hit table (pep_ctx::uf_nodes), K1's events and pinned areas, K7's match counts behind a search, the nucleotide tool's sets, K16's
triangles and leaders.  Until the buffers released themselves, pep_ctx_destroy freed from a hand-written list that had lost uf_nodes: this test would
have ended 4 * 1.25 * (n_targets + 1) bytes, rounded up to 256, above its baseline - 256 bytes for the 8 targets used here.

The one thing the sequence does not reach is pin_down: the detail copy of a 3-row group is 24 bytes of triangle and 12 of leaders, far below the
64 KiB from which a download is staged, and the input is not inflated to get there.

Other modules' contexts may be alive in the process, so everything is held against the baseline taken first, never against zero."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from divergence_helpers import pack_codes, verdict_table  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


def proteins(seed):
    """8 random proteins of 60 to 120 residues (codes: letter - 'A')"""
    rng = np.random.default_rng(seed)
    aa = np.frombuffer(b'ARNDCQEGHILKMFPSTWYV', dtype=np.uint8) - 65
    return [aa[rng.integers(0, 20, int(rng.integers(60, 121)))].astype(np.uint8) for _ in range(8)]


def test_a_closed_context_leaves_nothing_behind(N):
    from peppan_amd import orthofilter as OF, synth
    before = N.live_resources()
    ctx = N.Context(0)
    try:
        # phase timer events, pin_stage, d_zero, sort and scan state
        prots = proteins(41)
        ctx.set_timing(2)
        ctx.set_query_aa(prots)
        ctx.set_ref_aa(prots)
        hits, cig, st = ctx.search(N.default_params())
        assert len(hits) >= 8                              # every protein finds itself
        # uf_nodes: K10 as the tail of a search, then over the table the search left on the device (with another node map: uploaded again)
        ctx.set_grouping(16, np.arange(8, 16))
        n_hits = ctx.search_on_device(N.default_params())[0]
        assert n_hits == len(hits)
        labels = ctx.components_of_search(16, 8 + np.arange(8) % 4)
        assert len(labels) == 16
        ctx.set_grouping(0)
        # K1's events and pinned areas, the upload staging area (one reference sequence beyond 64 KiB), K7's counts behind the search
        names, genes = synth.make_genes(8, 300, seed=3)
        rng = np.random.default_rng(42)
        contig = bytearray(np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, 70000)].tobytes())
        contig[1000:1000 + len(genes[0])] = genes[0]
        ctx.set_query_nt(genes, 11)
        ctx.set_ref_nt(genes + [bytes(contig)], 6, 11)
        ctx.translate()
        ctx.set_nt_match(True)
        hits, cig, st = ctx.search(N.default_params(45., 25., 10, 5))
        assert len(hits) >= 8 and ctx.last_nt_match is not None and len(ctx.last_nt_match) == len(hits)
        ctx.set_nt_match(False)
        # the nucleotide tool's sets (NuclSide)
        ctx.use_nt_as_residues(2)
        hits, cig, st = ctx.search(N.nucleotide_params(60., 20.))
        assert len(hits) >= 8
        # K16: one group of 3 rows - two that differ in 2 of 298 columns and a third far from both, so the group is divergent, a pair lies beyond its
        # bound, and triangle and leaders are made and fetched
        a, b, far = np.full(305, 1), np.full(305, 1), np.full(305, 3)
        b[:2], b[298:] = 2, 0
        packed, row_off, row_len, index = verdict_table([pack_codes(np.stack([a, b, far]))], [305])
        gd = OF.gd_table({(1, 3): (0.01, 0.1), (2, 3): (0.01, 0.1)}, 0.002, 3)
        (verdict, tri, leader), = ctx.group_verdicts(packed, row_off, row_len, index, [np.array([1, 2, 3])], [False], gd, 0.002, detail=True)
        assert verdict == 2 and tri.shape == (3, 2) and len(leader) == 3
        during = N.live_resources()
        print('live resources (device bytes, pinned bytes, events): before %r, during %r' % (before, during))
        assert all(d > b0 for d, b0 in zip(during, before)), (before, during)
    finally:
        ctx.close()                                        # (frees the result search_on_device left in its keeping, then the context)
    after = N.live_resources()
    print('live resources after close: %r' % (after,))
    assert after == before


def test_a_staged_result_is_copied_out_before_its_context_goes(N):
    """pep_search leaves the hit table in the context's pinned staging area (the result holds views); ~pep_ctx gives a result that is still alive its own
    copy BEFORE pin_stage is released.  Through the C entry points: Context.close() frees the result it keeps before it destroys the context."""
    lib = N.load_library()
    before = N.live_resources()
    ctx = N.Context(0)
    prots = proteins(43)
    ctx.set_query_aa(prots)
    ctx.set_ref_aa(prots)
    p = N.default_params()
    want_hits, want_cigar, st = ctx.search(p)              # the same search, copied out while the context lives
    r = C.c_void_p()
    assert lib.pep_search(ctx._h, C.byref(p), C.byref(r)) == 0
    try:
        ctx.close()
        assert N.live_resources() == before
        nh, nc = C.c_uint64(), C.c_uint64()
        assert lib.pep_result_size(r, C.byref(nh), C.byref(nc)) == 0
        assert nh.value == len(want_hits) >= 8 and nc.value == len(want_cigar) > 0
        hits, cigar = np.empty(nh.value, dtype=N.HIT_DTYPE), np.empty(nc.value, dtype=np.uint32)
        assert lib.pep_result_copy(r, N._ptr(hits), N._ptr(cigar)) == 0
        assert np.array_equal(hits, want_hits) and np.array_equal(cigar, want_cigar)
    finally:
        lib.pep_result_free(r)


def test_the_six_call_records_do_not_share_a_slot(N):
    """pep_call_times keeps one record per kernel of K15 - K20 in the context.  Each of the six calls runs once, at the smallest shape that launches its
    kernels, on one context with every phase timed; then all six records are read: the byte counts are those the kernel's own test states for the shape, the
    slots a kernel fills are >= 0, every slot and byte count it does not use is exactly 0 - a kernel writing into another's record would show in one of
    them - and a second K19 call leaves the other five records bit for bit as they were.  The eight records of K21 - K26, whose calls this context never made, read
    zeros up to selector 13 = PEP_CALL_COUNT - 1; a bad selector (14 among them) or a null record is refused on a live context too."""
    from peppan_amd import orthofilter as OF
    lib = N.load_library()
    gd = OF.gd_table({(1, 2): (0.01, 0.1)}, 0.002, 3)
    packed, row_off, row_len, index = verdict_table([pack_codes(np.array([[1, 2, 3], [1, 2, 4]]))], [3])
    with N.Context(0) as ctx:
        ctx.set_timing(2)
        ctx.allele_diff(packed, row_off, row_len, index, 3)
        (verdict, tri, leader), = ctx.group_verdicts(packed, row_off, row_len, index, [np.array([1, 2])], [False], gd, 0.002, detail=True)
        ctx.gene_ingroups([1, 2], [9000, 8000], [100, 90], [0, 2], gd, 0.005, 8800.)
        has_conflict, _, conf_off, _, walk_off, _ = ctx.synteny_pairs([0, 2], [1, 2], [0, 1, 2], [5, 5], 2)
        assert not has_conflict[0] and conf_off[-1] == walk_off[-1] == 0          # (two genomes: no conflict pair, so the emit pass has nothing to do)
        ctx.gene_structure(b'ATGAAA', [0, 6], [0], [0], [6], [2], [0], [0], [6])
        ctx.rarefaction_curves(N.pack_presence([[True], [False]]), 1, [[1, 0]])
        ctx.profile_pairs([[1], [2]])
        # (slots in use, bytes to the device, bytes to the host); K16: a byte per group and the word of flags, and the detail of a verdict-2 group: a pair and two leaders
        want = {N.CALL_ALLELE_DIFF: (3, 0, 0), N.CALL_GROUP_VERDICTS: (4, 0, 1 + 4 + (8 + 2 * 4 if verdict == 2 else 0)), N.CALL_GENE_INGROUPS: (2, 0, 2 + 8 * 1),
                N.CALL_SYNTENY_PAIRS: (3, 0, 12 * 1 + 12), N.CALL_GENE_STRUCTURE: (1, 6 + 32 * 1, 9 * 1), N.CALL_PARSER: (2, 2 * 1 * 4, 2 * 2 * 2 * 4)}
        assert sorted(want) == list(range(N.CALL_KIMURA_PAIRS))          # (the six selectors of K15 - K20)
        records = {which: ctx.call_times(which) for which in want}
        for which, (used, up, down) in want.items():
            ms, to_device, to_host = records[which]
            print('call %d: ms %r, bytes to the device %d, to the host %d' % (which, ms.tolist(), to_device, to_host))
            assert len(ms) == N.CALL_MS == 8 and (ms[:used] >= 0).all() and ms[used:].tolist() == [0.] * (8 - used), (which, ms.tolist())
            assert (to_device, to_host) == (up, down), which
        ctx.gene_structure(b'ATGAAA', [0, 6], [0], [0], [6], [2], [0], [0], [6])
        for which in want:
            if which != N.CALL_GENE_STRUCTURE:
                ms, to_device, to_host = ctx.call_times(which)
                assert (ms.tobytes(), to_device, to_host) == (records[which][0].tobytes(),) + records[which][1:], which
        assert ctx.gene_structure_times()[1:] == (38, 9)
        out = N.CallTimes()
        for which, record in ((-1, C.byref(out)), (N.CALL_COUNT, C.byref(out)), (0, None)):
            assert lib.pep_call_times(ctx._h, which, record) == -2          # PEP_ERR_ARG
        assert N.CALL_COUNT == 14
        for which in range(N.CALL_KIMURA_PAIRS, N.CALL_COUNT):
            assert lib.pep_call_times(ctx._h, which, C.byref(out)) == 0 and bytes(out) == bytes(80), which
