"""K23 on the GPU (csrc/cdsgenes.hip: the verdict and the digest of every annotated CDS, the per-gene work of iter_readGFF PEPPAN.py:117-182, checkPseu
:992-1010 and addGenes :1013-1021): the drop-ins against what the reference's own functions returned for every case of tests/golden/g26_gffgenes.json.gz,
and Context.cds_genes / cds_verdicts on synthetic windows against the restatement of tests/gffgenes_helpers.py and hashlib.

The tolerance is zero: codes, digests, texts, names and their order are compared with ==.

Shapes.  The verdict kernel walks chunks of 64 codons = 192 nucleotides, the digest kernel blocks of 64 bytes whose padding changes at 55 / 56 and 63 /
64 (119 / 120, ..): the sweep takes every length 0 .. 200 and the chunk and block borders near 384, 576 and 4096, on both strands, with the window at the
contig's first byte, at its last byte and in its middle, a start and a stop codon of either strand directly outside both ends.  The placement test puts
an X, an M and a '-' codon at the first two and last two codons and around codons 64 and 128."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gffgenes_helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu

LEFT, RIGHT = 'TTACATTAAATG', 'ATGTAACATTTA'              # a stop and a start of either strand directly outside the window


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


@pytest.fixture(scope='module')
def GG(N):
    from peppan_amd import gffgenes
    yield gffgenes
    gffgenes.close()


@pytest.fixture(scope='module')
def ctx(N):
    with N.Context(0) as c:
        yield c


@pytest.fixture(scope='module')
def fx(tmp_path_factory):
    fx = H.load()
    fx['dir'] = str(tmp_path_factory.mktemp('gff'))
    H.write_files(fx, fx['dir'])
    return fx


@pytest.fixture
def there(fx, monkeypatch):
    monkeypatch.chdir(fx['dir'])
    return fx


def mask_of(N, letters):
    return sum(N.CDS_ALLOW[ch] for ch in set(letters))


def expected(texts, strands, gtable, min_cds, incomplete):
    """(codes, digests) of windows as they stand in their contigs: the restatement and hashlib; 6 where the restatement raises"""
    codes, digests = [], []
    for text, rev in zip(texts, strands):
        s = H.rc(text) if rev else text
        try:
            code = H.check_pseu(s, gtable, min_cds, incomplete)
        except IndexError:
            code = 6
        codes.append(code)
        digests.append(hashlib.sha1(s.encode()).digest() if code == 0 else bytes(20))
    return codes, digests


def run_windows(ctx, contigs, windows, strands, gtable, min_cds, mask):
    """contigs: texts; windows: (contig, offset, length) -> (codes, digests as bytes)"""
    off = np.concatenate([[0], np.cumsum([len(c) for c in contigs])])
    code, digest = ctx.cds_genes(''.join(contigs).encode(), off, [w[0] for w in windows], [w[1] for w in windows], [w[2] for w in windows], strands, min_cds, mask,
                                 table4=gtable == 4)
    return code.tolist(), [bytes(d) for d in digest]


# ---- 1. the fixture
def test_every_read_case_is_the_reference_s_dictionaries(GG, there):
    for c in there['read']:
        params = dict(min_cds=c['min_cds'], incompleteCDS=c['incomplete'])
        if c['error']:
            with pytest.raises(AssertionError):
                GG.readGFF(c['entry'], c['feature'], c['gtable'], params)
            continue
        seq, cds = GG.readGFF(c['entry'], c['feature'], c['gtable'], params)
        assert seq == c['seq'] and list(seq) == list(c['seq']), c['name']
        assert cds == c['cds'] and list(cds) == list(c['cds']), c['name']
        assert all(type(v[5]) is int and type(v[6]) is str for v in cds.values())


def test_several_files_in_one_call_equal_one_call_each(GG, there):
    entries = ['synth.gff', 'second.v2.gff', 'zipped.gff.gz', 'pair.gff,pair.fna', 'names.gff']
    params = dict(min_cds=30, incompleteCDS='')
    seq, cds = {}, {}
    for e in entries:
        s, c = GG.readGFF(e, 'CDS', 11, params)
        seq.update(s)
        cds.update(c)
    for batch_bytes in (GG.DEFAULT_BATCH_BYTES, 1, 9000):                # (one batch; a batch per file; batches cut where the contigs pass 9 kB)
        s, c = GG.readGFF(entries, 'CDS', 11, params, batch_bytes=batch_bytes)
        assert s == seq and c == cds and list(s) == list(seq) and list(c) == list(cds), batch_bytes
    recorded = {}
    for name in ("synth.gff '' 11 30", "second.v2.gff '' 11 30", 'gz'):
        recorded.update([c for c in there['read'] if c['name'] == name][0]['cds'])
    assert all(cds[k] == v for k, v in recorded.items()) and len(recorded) > 100


def test_every_gene_file_case_is_the_reference_s_dictionary(GG, there):
    for c in there['genes']:
        genes, error = {k: list(v) for k, v in c['before'].items()}, None
        try:
            assert GG.addGenes(genes, c['gene_file'], c['gtable'], dict(min_cds=c['min_cds'], incompleteCDS=c['incomplete'])) is genes
        except IndexError:
            error = 'IndexError'
        assert error == c['error'] and genes == c['genes'] and list(genes) == list(c['genes']), c['name']


def test_every_checkpseu_case(GG, there):
    groups = {}
    for text, incomplete, gtable, min_cds, want in there['pseu']:
        groups.setdefault((incomplete, gtable, min_cds), []).append((text, 6 if want == 'IndexError' else want))
    assert len(groups) >= 32
    for (incomplete, gtable, min_cds), rows in groups.items():
        codes, digests = GG.cds_verdicts([t for t, _ in rows], ['+'] * len(rows), gtable, min_cds, incomplete)
        assert codes.tolist() == [w for _, w in rows], (incomplete, gtable, min_cds)
        assert [bytes(d) for d in digests] == [hashlib.sha1(t.encode()).digest() if w == 0 else bytes(20) for t, w in rows]


# ---- 2. the length sweep
def test_length_sweep_on_both_strands_at_three_places(N, ctx):
    rng = np.random.default_rng(23)
    lengths = list(range(0, 201)) + list(range(380, 391)) + list(range(570, 581)) + list(range(4090, 4101))
    contigs, windows, strands, texts = [], [], [], []
    for L in lengths:
        w = ''.join(rng.choice(list('ACGT'), L).tolist())
        if L >= 6 and L % 3 == 0:                           # a gene, so that code 0 occurs without a waiver: a start, no inner stop, a stop
            inner = ''.join('TCA' if w[k:k + 3] in H.STOPS else w[k:k + 3] for k in range(3, L - 3, 3))
            w = 'GTG' + inner + 'TAG'
        for rev in (0, 1):
            v = H.rc(w) if rev else w
            for contig, at in ((v + RIGHT, 0), (LEFT + v, len(LEFT)), (LEFT + v + RIGHT, len(LEFT))):
                windows.append((len(contigs), at, L))
                contigs.append(contig)
                strands.append(rev)
                texts.append(v)
    for incomplete, min_cds in (('', 0), ('sife', 0), ('f', 1), ('e', 100)):
        got = run_windows(ctx, contigs, windows, strands, 11, min_cds, mask_of(N, incomplete))
        want = expected(texts, strands, 11, min_cds, incomplete)
        for k, (w, code) in enumerate(zip(windows, want[0])):
            if code == 6:                                   # no codon at all: the header's answer, as if no codon were M or X
                want[0][k] = 0 if incomplete == 'sife' else 3
                want[1][k] = hashlib.sha1(b'').digest() if incomplete == 'sife' else bytes(20)
        assert got[0] == want[0], (incomplete, min_cds)
        assert got[1] == want[1], (incomplete, min_cds)
        if incomplete == '':
            assert sum(c == 0 for c in got[0]) > 400 and {1, 2} & set(got[0]) == {2}
        if incomplete == 'sife':
            assert set(got[0]) == {0}


# ---- 3. one codon placed
def test_x_m_and_gap_codons_at_the_borders_under_every_mask_and_table(N, ctx):
    n = 200
    plain, gene = ['CCC'] * n, ['ATG'] + ['CCC'] * (n - 2) + ['TAA']
    texts = [''.join(plain), ''.join(gene)]
    for base in (plain, gene):
        for codon in ('TAA', 'TGA', 'ANC', 'ATG', 'A-C', '-NN'):
            for at in (0, 1, n - 2, n - 1, 63, 64, 65, 127, 128):
                texts.append(''.join(base[:at] + [codon] + base[at + 1:]))
    texts = texts + texts
    strands = [0] * (len(texts) // 2) + [1] * (len(texts) // 2)
    windows = [(k, len(LEFT), 3 * n) for k in range(len(texts))]
    contigs = [LEFT + t + RIGHT for t in texts]
    seen = set()
    for gtable in (11, 4):
        for incomplete in H.MASKS:
            got = run_windows(ctx, contigs, windows, strands, gtable, 0, mask_of(N, incomplete))
            want = expected(texts, strands, gtable, 0, incomplete)
            assert got[0] == want[0], (gtable, incomplete)
            assert got[1] == want[1], (gtable, incomplete)
            seen |= set(got[0])
    assert seen == {0, 3, 4, 5}


# ---- 4. a large batch
_CODE = np.full(256, 4, np.uint8)
_CODE[[ord(c) for c in 'ACGT']] = [0, 1, 2, 3]
_CODE[ord('-')] = 5
_STOP = {11: np.isin(np.arange(64), [48, 50, 56]), 4: np.isin(np.arange(64), [48, 50])}
_START = np.isin(np.arange(64), [14, 46, 62])


def check_pseu_numpy(text, gtable, min_cds, incomplete):
    """H.check_pseu with the codons classified by numpy (held to H.check_pseu on a part of the batch below)"""
    if len(text) < min_cds:
        return 1
    if len(text) % 3 and 'f' not in incomplete:
        return 2
    if not text:
        return 6
    c = _CODE[np.frombuffer(text.encode() + b'??'[:-len(text) % 3], np.uint8)].reshape(-1, 3)
    gap, bad = (c == 5).any(1), (c >= 4).any(1)
    idx = (c[:, 0] & 3) * 16 + (c[:, 1] & 3) * 4 + (c[:, 2] & 3)
    is_m, is_x = ~bad & _START[idx], ~gap & (bad | _STOP[gtable][idx])
    if not is_m[0] and 's' not in incomplete:
        return 3
    if not is_x[-1] and 'e' not in incomplete:
        return 4
    if is_x[:-1].any() and 'i' not in incomplete:
        return 5
    return 0


_RC_FAST = str.maketrans({chr(c): 'TGCA'['ACGT'.index(chr(c))] if chr(c) in 'ACGT' else 'N' for c in range(128)})


def rc_fast(text):
    """H.rc for the large batch (held to H.rc on a part of it below)"""
    return text.upper().translate(_RC_FAST)[::-1]


def big_batch():
    rng = np.random.default_rng(2300)
    letters = np.frombuffer(b'ACGT', np.uint8)
    odd = np.frombuffer(b'N-RYacgtn*', np.uint8)
    texts = []
    for k in range(20002):
        L = 199998 + 3 * (k - 20000) if k >= 20000 else int(rng.integers(0, 3001))
        a = letters[rng.integers(0, 4, L)].copy()
        if k % 2 and L >= 6:                                # every other one a gene up to its last codon: a start, no stop in frame, a stop
            body = a[:L - L % 3].reshape(-1, 3)
            t = body[:, 0] == ord('T')
            body[t & (((body[:, 1] == ord('A')) & ((body[:, 2] == ord('A')) | (body[:, 2] == ord('G')))) | ((body[:, 1] == ord('G')) & (body[:, 2] == ord('A')))), 0] = ord('C')
            body[0] = list(b'TTG')
            body[-1] = list(b'TGA' if k % 4 == 1 else b'TAA')
        if k % 5 == 0 and L:                                # a small rate of odd characters
            at = rng.integers(0, L, 1 + L // 400)
            a[at] = odd[rng.integers(0, len(odd), len(at))]
        texts.append(a.tobytes().decode())
    strands = rng.integers(0, 2, len(texts)).tolist()
    return texts, strands


def test_big_batch_of_mixed_windows(GG):
    texts, strands = big_batch()
    # the genes were made for the forward strand: hand their reverse complement over where the strand says '-'
    given = [t.upper() for t in texts]
    windows = [rc_fast(t) if rev and k % 2 else t for k, (t, rev) in enumerate(zip(given, strands))]
    seen = set()
    parts = {(11, 120, ''): [k for k in range(len(texts)) if k % 3 == 0], (4, 0, 'fi'): [k for k in range(len(texts)) if k % 3 == 1],
             (11, 0, 'sife'): [k for k in range(len(texts)) if k % 3 == 2]}
    for (gtable, min_cds, incomplete), part in parts.items():
        codes, digests = GG.cds_verdicts([windows[k] for k in part], ['-' if strands[k] else '+' for k in part], gtable, min_cds, incomplete)
        read = [rc_fast(windows[k]) if strands[k] else windows[k] for k in part]
        want = [check_pseu_numpy(t, gtable, min_cds, incomplete) for t in read]
        for t in read[:150]:
            try:
                slow = H.check_pseu(t, gtable, min_cds, incomplete)
            except IndexError:
                slow = 6
            assert slow == check_pseu_numpy(t, gtable, min_cds, incomplete) and rc_fast(t) == H.rc(t)
        assert codes.tolist() == want, (gtable, min_cds, incomplete)
        assert [bytes(d) for d in digests] == [hashlib.sha1(t.encode()).digest() if c == 0 else bytes(20) for t, c in zip(read, want)]
        assert want.count(0) > 500, want.count(0)
        seen |= set(want)
    assert max(len(t) for t in texts) == 200001 and seen == {0, 1, 2, 3, 4, 5, 6}


# ---- 5. nothing to do
def test_empty_calls(GG, ctx, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with open('bare.gff', 'w') as out:
        out.write('##gff-version 3\n##FASTA\n>c1\nACGTAC\n>c2\n')
    with open('headless.gff', 'w') as out:
        out.write('c1\ts\tCDS\t1\t9\t.\t+\t0\tID=a\nc1\ts\tCDS\t1\t9\t.\t-\t0\tID=b\n')
    params = dict(min_cds=0, incompleteCDS='')
    assert GG.readGFF('bare.gff', 'CDS', 11, params) == ({'bare:c1': ['bare.gff', 'ACGTAC'], 'bare:c2': ['bare.gff', '']}, {})
    seq, cds = GG.readGFF(['headless.gff'], 'CDS', 11, params)
    assert seq == {} and cds == {'headless:a': ['headless.gff', 'headless:c1', 1, 9, '+', 6, ''], 'headless:b': ['headless.gff', 'headless:c1', 1, 9, '-', 6, '']}
    assert GG.readGFF([], 'CDS', 11, params) == ({}, {})
    codes, digests = GG.cds_verdicts([], [], 11, 0, '')
    assert codes.shape == (0,) and digests.shape == (0, 20)
    codes, digests = GG.cds_verdicts(['', 'ATGTAA', ''], ['+', '-', '-'], 11, 0, 'sife')
    assert codes.tolist() == [6, 0, 6] and bytes(digests[1]) == hashlib.sha1(b'TTACAT').digest()
    code, digest = ctx.cds_genes(b'ACGT', [0, 4], [], [], [], [])
    assert len(code) == 0 and digest.shape == (0, 20)
    code, digest = ctx.cds_genes(b'', [0], [], [], [], [], 5, 15, table4=True)
    assert len(code) == 0


# ---- 6. the limits
def test_limits_are_refused_with_their_message_and_the_context_goes_on(N, ctx):
    with pytest.raises(N.PepError, match=r'\(-2\).*the window of CDS 1 leaves its contig of 4 bytes'):
        ctx.cds_genes(b'ACGTACGT', [0, 4, 8], [0, 1], [0, 2], [4, 3], [0, 0])
    with pytest.raises(N.PepError, match=r'\(-2\).*the strand byte of CDS 0 is 2'):
        ctx.cds_genes(b'ACGT', [0, 4], [0], [0], [4], [2])
    with pytest.raises(N.PepError, match=r'\(-2\).*mask 16 has bits beyond the four'):
        ctx.cds_genes(b'ACGT', [0, 4], [0], [0], [4], [0], 0, 16)
    with pytest.raises(N.PepError, match=r'\(-2\).*CDS 0 names contig 1 of 1'):
        ctx.cds_genes(b'ACGT', [0, 4], [1], [0], [4], [0])
    # a window of 2^31 bytes in a contig of 2^33, at an offset beyond 32 bits: refused by the tables alone, no byte of a contig is asked for
    off, one = np.array([0, 1 << 33], np.uint64), np.zeros(1, np.uint32)
    at, length, strand = np.array([(1 << 32) + 7], np.uint64), np.array([1 << 31], np.uint32), np.zeros(1, np.uint8)
    out = np.zeros(20, np.uint8)
    with pytest.raises(N.PepError, match=r'\(-3\).*the window of CDS 0 holds 2\^31 bytes or more'):
        ctx._call('pep_cds_genes', None, N._ptr(off), 1, 1, N._ptr(one), N._ptr(at), N._ptr(length), N._ptr(strand), 0, 0, 0, N._ptr(out), N._ptr(out))
    # 2^32 CDS: refused before a table is looked through (a column of 2^32 entries that takes no memory)
    column = np.broadcast_to(np.uint8(0), (1 << 32,))
    with pytest.raises(ValueError, match=r'2\^32 CDS'):
        ctx.cds_genes(b'ACGT', [0, 4], column, column, column, column)
    with pytest.raises(ValueError):
        ctx.cds_genes(b'ACGT', [0, 5], [0], [0], [4], [0])
    with pytest.raises(ValueError):
        ctx.cds_genes(b'ACGT', [0, 4], [0], [0], [4], [0], min_cds=(1 << 31) + 1)
    code, digest = ctx.cds_genes(b'ATGTAA', [0, 6], [0, 0], [0, 0], [6, 6], [0, 1])
    assert code.tolist() == [0, 3] and bytes(digest[0]) == hashlib.sha1(b'ATGTAA').digest() and bytes(digest[1]) == bytes(20)
    assert not ctx.call_times(N.CALL_CDS_GENES, total=True)[0].any() and not ctx.call_times(N.CALL_CDS_GENES)[0].any()
