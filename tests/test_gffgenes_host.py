"""K23 (the GFF front end: iter_readGFF PEPPAN.py:117-182, checkPseu :992-1010, addGenes :1013-1021) without a GPU: the restatement of
tests/gffgenes_helpers.py against what the reference's own functions returned for the committed fixture (tests/golden/g26_gffgenes.json.gz, made by
tests/golden/make_golden_gffgenes.py), the host parse and the window resolution of peppan_amd.gffgenes against the fixture, its text builder against
hashlib and the restatement, the device-free checks of pep_cds_genes, and the K23 section of the header against _native's constants.

The tolerance is zero: names, their order, coordinates, codes, texts and digests are compared with ==."""
import ctypes as C
import hashlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gffgenes_helpers as H  # noqa: E402
import test_abi as ABI  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEP_ERR_ARG, PEP_ERR_LIMIT = -2, -3


@pytest.fixture(scope='module')
def N():
    import __graft_entry__ as G
    G.build()
    from peppan_amd import _native
    return _native


@pytest.fixture(scope='module')
def fx(tmp_path_factory):
    fx = H.load()
    fx['dir'] = str(tmp_path_factory.mktemp('gff'))
    H.write_files(fx, fx['dir'])
    assert len(fx['read']) == 17 and len(fx['genes']) == 5 and len(fx['pseu']) == 567
    return fx


@pytest.fixture
def there(fx, monkeypatch):
    monkeypatch.chdir(fx['dir'])              # (the fixture's file names are relative, and they are part of the recorded dictionaries)
    return fx


def test_restated_checkpseu_is_the_reference_on_every_case(fx):
    seen = set()
    for text, incomplete, gtable, min_cds, want in fx['pseu']:
        try:
            got = H.check_pseu(text, gtable, min_cds, incomplete)
        except IndexError:
            got = 'IndexError'
        assert got == want, (text, incomplete, gtable, min_cds)
        seen.add((frozenset(incomplete), gtable))
    assert len(seen) == 32                                  # all 16 subsets of sife under both tables


def test_restated_parse_is_the_reference_on_every_case(there):
    for c in there['read']:
        if c['error']:
            with pytest.raises(AssertionError):
                H.read_gff(c['entry'], c['feature'], c['gtable'], c['min_cds'], c['incomplete'])
            continue
        seq, cds = H.read_gff(c['entry'], c['feature'], c['gtable'], c['min_cds'], c['incomplete'])
        assert seq == c['seq'] and list(seq) == list(c['seq']), c['name']
        assert cds == c['cds'] and list(cds) == list(c['cds']), c['name']


def test_restated_addgenes_is_the_reference_on_every_case(there):
    for c in there['genes']:
        genes, error = {k: list(v) for k, v in c['before'].items()}, None
        try:
            assert H.add_genes(genes, c['gene_file'], c['gtable'], c['min_cds'], c['incomplete']) is genes
        except IndexError:
            error = 'IndexError'
        assert error == c['error'] and genes == c['genes'] and list(genes) == list(c['genes']), c['name']


def test_host_parse_and_windows_are_the_reference_s(there):
    """contigs, gene names in order, coordinates; the window gives the recorded text, its digest and - through the restated checkPseu - the recorded code;
    no window exactly where the reference ended in code 6"""
    from peppan_amd import gffgenes as GG
    for c in there['read']:
        if c['error']:
            with pytest.raises(AssertionError):
                GG.read_gff_file(c['entry'], c['feature'], c['gtable'], c['min_cds'], c['incomplete'])
            continue
        f = GG.read_gff_file(c['entry'], c['feature'], c['gtable'], c['min_cds'], c['incomplete'])
        assert f.fname == c['entry'].split(',')[0]
        assert [(k, [f.fname, v.decode()]) for k, v in f.contigs.items()] == list(c['seq'].items()), c['name']
        assert [g[0] for g in f.genes] == list(c['cds']), c['name']
        for gname, cname, start, end, strand, window in f.genes:
            want = c['cds'][gname]
            assert [f.fname, cname, start, end, strand] == want[:5], (c['name'], gname)
            if window is None:
                assert want[5:] == [6, ''], (c['name'], gname)
                continue
            lo, n = window
            assert 0 <= lo and lo + n <= len(f.contigs[cname]) and n == len(f.contigs[cname][slice(start - 1, end)])
            text = GG._text(f.contigs[cname], lo, n, strand == '-')
            code = H.check_pseu(text, c['gtable'], c['min_cds'], c['incomplete'])
            assert text == (H.rc(f.contigs[cname].decode()[lo:lo + n]) if strand == '-' else f.contigs[cname].decode()[lo:lo + n])
            if code:
                assert want[5:] == [code, ''], (c['name'], gname)
            else:
                assert want[5:] == [int(hashlib.sha1(text.encode()).hexdigest(), 16), text], (c['name'], gname)


def test_reverse_complement_table_is_rc_on_every_byte():
    from peppan_amd import gffgenes as GG
    every = bytes(range(128))                               # (rc() upper-cases first, and so does the table)
    assert GG._text(every, 0, len(every), True) == H.rc(every.decode()) and len(GG._RC) == 256 and set(GG._RC[128:]) == {ord('N')}
    assert GG._text(b'AACGTN-R', 1, 6, True) == 'NNACGT' and GG._text(b'AACGTN-R', 1, 6, False) == 'ACGTN-'


def test_parameters_as_the_library_takes_them(N):
    from peppan_amd import gffgenes as GG
    assert [GG._mask(m) for m in ('', 's', 'i', 'f', 'e', 'sife', 'efis', 'xyz')] == [0, 1, 2, 4, 8, 15, 15, 0]
    # len < min_cds for integer lengths, also for the float the reference's command line gives
    assert [GG._min_cds(v) for v in (-5, 0, 0.5, 120., 120.25, 1 << 40)] == [0, 0, 1, 120, 121, 1 << 31]
    for v in (-5, 0, 0.5, 120., 120.25):
        assert all((n < v) == (n < GG._min_cds(v)) for n in range(0, 130))


def test_a_character_outside_ascii_is_refused(tmp_path, monkeypatch):
    from peppan_amd import gffgenes as GG
    monkeypatch.chdir(tmp_path)
    with open('odd.gff', 'w', encoding='utf-8') as out:
        out.write('c1\ts\tCDS\t1\t9\t.\t+\t0\tID=a\n##FASTA\n>c1\nATGAAAßTAA\n')
    with pytest.raises(ValueError):
        GG.read_gff_file('odd.gff')
    with pytest.raises(ValueError):
        GG.cds_verdicts(['ATGı'], ['+'], 11, 0, '')


def check(N, contig_off, contig, win_off, win_len, strand, mask=0):
    msg = C.create_string_buffer(512)
    cols = [np.array(contig_off, dtype=np.uint64), np.array(contig, dtype=np.uint32), np.array(win_off, dtype=np.uint64), np.array(win_len, dtype=np.uint32),
            np.array(strand, dtype=np.uint8)]
    rc = N.load_library().pep_cds_genes_check(N._ptr(cols[0]), len(cols[0]) - 1, len(cols[1]), *[N._ptr_or_null(c) for c in cols[1:]], mask, msg, len(msg))
    return rc, msg.value.decode()


def test_every_refusal_of_the_device_free_check(N):
    assert check(N, [0, 10, 30], [0, 1, 1], [0, 0, 20], [10, 20, 0], [0, 1, 0], 15) == (0, '')
    assert check(N, [0], [], [], [], []) == (0, '') and check(N, [0, 0], [0], [0], [0], [1]) == (0, '')
    rc, msg = check(N, [0, 10, 30], [0, 1], [0, 1], [10, 20], [0, 0])
    assert rc == PEP_ERR_ARG and 'the window of CDS 1 leaves its contig of 20 bytes' in msg
    rc, msg = check(N, [0, 10, 30], [0, 1], [11, 0], [0, 20], [0, 0])
    assert rc == PEP_ERR_ARG and 'the window of CDS 0 leaves its contig of 10 bytes' in msg
    rc, msg = check(N, [0, 10], [0, 0], [0, 0], [10, 10], [0, 2])
    assert rc == PEP_ERR_ARG and 'the strand byte of CDS 1 is 2' in msg
    rc, msg = check(N, [0, 10], [0], [0], [10], [0], 16)
    assert rc == PEP_ERR_ARG and 'mask 16 has bits beyond the four' in msg
    rc, msg = check(N, [0, 10], [0, 1], [0, 0], [10, 10], [0, 0])
    assert rc == PEP_ERR_ARG and 'CDS 1 names contig 1 of 1' in msg
    rc, msg = check(N, [0, 10, 5], [0], [0], [1], [0])
    assert rc == PEP_ERR_ARG and 'non-decreasing (contig 1)' in msg
    rc, msg = check(N, [3, 10], [0], [0], [1], [0])
    assert rc == PEP_ERR_ARG and 'must start at 0' in msg
    # the limits: a window of 2^31 bytes inside a contig of 2^33 (nothing is allocated: the contigs are not read), an offset beyond 32 bits
    rc, msg = check(N, [0, 1 << 33], [0], [0], [1 << 31], [0])
    assert rc == PEP_ERR_LIMIT and 'the window of CDS 0 holds 2^31 bytes or more' in msg
    assert check(N, [0, 1 << 33], [0, 0], [0, (1 << 33) - 5], [(1 << 31) - 1, 5], [0, 1]) == (0, '')
    lib = N.load_library()
    assert lib.pep_cds_genes_check(None, 0, 0, None, None, None, None, 0, None, 0) == PEP_ERR_ARG
    with pytest.raises(N.PepError, match=r'\(-2\).*leaves its contig'):
        N.cds_genes_check([0, 4], [0], [2], [3], [0])
    with pytest.raises(ValueError):
        N.cds_genes_check([0, 4], [0], [-1], [3], [0])
    with pytest.raises(ValueError):
        N.cds_genes_check([0, 4], [0, 0], [1], [3], [0])
    assert N.cds_genes_check([0, 4], [0], [1], [3], [1], mask=15) is None


def test_null_context_is_an_argument_error(N):
    restype, *argtypes = N.SIGNATURES['pep_cds_genes']
    assert restype is C.c_int and argtypes[0] is C.c_void_p
    assert N.load_library().pep_cds_genes(*[None if t is C.c_void_p else t(0) for t in argtypes]) == PEP_ERR_ARG


def test_gffgenes_section_of_the_header(N):
    """the K23 section of include/peppan_hip.h declares its two functions in this order, cites what it replaces, and its limits and mask bits are _native's (the
    prototypes: tests/test_abi.py)"""
    hdr = open(os.path.join(ROOT, 'include', 'peppan_hip.h')).read()
    names = [name for _, name, _ in ABI._header_prototypes()]
    own = ['pep_cds_genes_check', 'pep_cds_genes']
    assert names[names.index(own[0]):][:len(own)] == own == [name for name in N.SIGNATURES if name in own]
    for define, value in (('PEP_CDS_MAX_WINDOW', N.CDS_MAX_WINDOW), ('PEP_CDS_MAX_ITEMS', N.CDS_MAX_ITEMS)):
        assert re.search(r'#define %s \(1u(?:ll)? << (\d+)\)' % define, hdr).group(1) == str(value.bit_length() - 1)
    for letter, define in (('s', 'NO_START'), ('i', 'INNER_STOP'), ('f', 'FRAMESHIFT'), ('e', 'NO_STOP')):
        assert int(re.search(r'#define PEP_CDS_ALLOW_%s (\d+)\b' % define, hdr).group(1)) == N.CDS_ALLOW[letter]
    assert int(re.search(r'#define PEP_ABI_VERSION (\d+)', hdr).group(1)) == N.ABI_VERSION
    assert 'PEPPAN.py:117-182' in hdr and ':992-1010' in hdr
