#!/usr/bin/env python3
"""Generate tests/golden/g19_allele_diff.json.gz by IMPORTING the reference's Python (build machine only: needs /root/reference).

    python tests/golden/make_golden_allele_diff.py

The same kind of shim as make_golden.py: stub `numba` / `ete3` packages and no-op aligner tools on PATH, then `import PEPPAN`.
Every case is a seeded gene group given as base-5 packed rows (the .seq store's form) plus its ref_len; the expected values are
PEP.compare_seq and PEP.compare_seqX (PEPPAN.py:296-316) over PEP.decodeSeq and the masking of filt_per_group (:332-333), stored as
the packed upper triangle and the first / last row.  Only DATA is written - none of the reference's source text.

Cases: n in {1, 2, 3, 17, 64, 65} x ref_len in {1, 2, 3, 63, 64, 65, 191, 192, 193, 1000, 1002}, n = 130 with ref_len in
{1, 64, 193, 1002}; from three rows on, row 1 is all gaps and the last row repeats row 0; every row carries random digits past ref_len
where its last byte has room for them; groups of 17 rows and more also give a sub-group taken by index (the :354-360 pattern).
"""
import base64, gzip, json, os, stat, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'


def build_shim():
    root = tempfile.mkdtemp(prefix='peppan_shim_')
    os.makedirs(os.path.join(root, 'bin'))
    for t in ('mmseqs', 'makeblastdb', 'diamond', 'blastn'):
        p = os.path.join(root, 'bin', t)
        with open(p, 'w') as f:
            f.write('#!/bin/sh\nexit 0\n')
        os.chmod(p, os.stat(p).st_mode | stat.S_IEXEC | stat.S_IXGRP | stat.S_IXOTH)
    for pkg, body in (('numba', 'def jit(*a, **k):\n    if len(a) == 1 and callable(a[0]) and not k:\n        return a[0]\n    return lambda f: f\n'),
                      ('ete3', 'class Tree(object):\n    pass\n')):
        os.makedirs(os.path.join(root, 'py', pkg))
        with open(os.path.join(root, 'py', pkg, '__init__.py'), 'w') as f:
            f.write(body)
    os.makedirs(os.path.join(root, 'cwd'))
    return root


SHIM = build_shim()
os.environ['PATH'] = os.path.join(SHIM, 'bin') + os.pathsep + os.environ['PATH']
sys.path[:0] = [os.path.join(SHIM, 'py'), os.path.join(REF, 'modules'), REF]
os.chdir(os.path.join(SHIM, 'cwd'))

import numpy as np                       # noqa: E402
if not hasattr(np.lib.npyio, 'format'):  # numpy >= 2 dropped this alias of np.lib.format; the reference's MapBsn spells it the old way
    np.lib.npyio.format = np.lib.format
import PEPPAN as PEP                     # noqa: E402


def make_group(rng, n, ref_len):
    """packed rows uint8[n, ceil(ref_len / 3)]: a random ancestor, per row a gap rate and a divergence, garbage digits past ref_len"""
    s = -(-ref_len // 3)
    anc = rng.integers(1, 5, ref_len)
    codes = np.zeros((n, 3 * s), dtype=np.int64)
    for r in range(n):
        row = anc.copy()
        mut = rng.random(ref_len) < rng.uniform(0, 0.3)
        row[mut] = rng.integers(1, 5, int(mut.sum()))
        row[rng.random(ref_len) < rng.uniform(0, 0.5)] = 0
        codes[r, :ref_len] = row
    if n >= 3:
        codes[1, :ref_len] = 0
        codes[n - 1, :ref_len] = codes[0, :ref_len]
    codes[:, ref_len:] = rng.integers(0, 5, (n, 3 * s - ref_len))
    return (codes[:, :s] * 25 + codes[:, s:2 * s] * 5 + codes[:, 2 * s:]).astype(np.uint8)


def reference_seqs(packed, ref_len):
    """PEPPAN.py:332-333"""
    seqs = np.array([45, 65, 67, 71, 84], dtype=np.uint8)[PEP.decodeSeq(packed)][:, :ref_len]
    seqs[np.isin(seqs, [65, 67, 71, 84], invert=True).reshape(seqs.shape)] = 0
    return seqs


def expected(seqs):
    n = seqs.shape[0]
    diff = PEP.compare_seq(seqs, np.zeros(shape=[n, n, 2], dtype=int))
    diffX = PEP.compare_seqX(seqs, np.zeros(shape=[n, n, 2], dtype=int))
    assert not diff[np.tril_indices(n)].any()
    assert n <= 2 or not diffX[1:-1].any()
    iu = np.triu_indices(n, 1)
    return dict(tri=diff[iu[0], iu[1]].tolist(), edge=[diffX[0].tolist(), diffX[n - 1].tolist()])


def main():
    rng = np.random.default_rng(20190)
    lens = (1, 2, 3, 63, 64, 65, 191, 192, 193, 1000, 1002)
    shapes = [(n, L) for n in (1, 2, 3, 17, 64, 65) for L in lens] + [(130, L) for L in (1, 64, 193, 1002)]
    cases = []
    for n, L in shapes:
        packed = make_group(rng, n, L)
        seqs = reference_seqs(packed, L)
        case = dict(name='n%d_L%d' % (n, L), n=n, ref_len=L, rows=base64.b64encode(packed.tobytes()).decode(), sub=None)
        case.update(expected(seqs))
        if n >= 17:
            index = sorted(rng.choice(n, size=int(rng.integers(2, 7)), replace=False).tolist())
            case['sub'] = dict(index=index, **expected(seqs[index]))
        cases.append(case)
    out = os.path.join(HERE, 'g19_allele_diff.json.gz')
    with gzip.GzipFile(out, 'wb', mtime=0) as f:
        f.write(json.dumps(dict(source='PEPPAN.py:296-316 over :318-324, :332-333', cases=cases), separators=(',', ':')).encode())
    print(out, os.path.getsize(out), 'bytes,', len(cases), 'cases')


if __name__ == '__main__':
    main()
