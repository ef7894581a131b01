#!/usr/bin/env python3
"""Generate tests/golden/g21_rescore_codons.json.gz by IMPORTING the reference's Python (build machine only: needs /root/reference).

    python tests/golden/make_golden_rescore_codons.py

The same kind of shim as make_golden.py: stub `numba` / `ete3` packages and no-op aligner tools on PATH, then `import uberBlast`.
Every alignment is a seeded hit of tests/rescore_helpers.random_hits (sequences of at most 400 nt) or one planted by
tests/rescore_codon_helpers.planted_codon_hits; it is stored as the two aligned ranges as they lie in their sequences, the strand, the
query's first base and the runs.  The expected values are the reference's own cigar2score (uberBlast.py:221-269) in modes 2 and 3, fed as
RunBlast.reScore feeds it (:402-412: upper-cased text through nucEncoder, the reference range complemented and turned on the reverse
strand).  Every table-11 call is made before the first table-4 call: the reference patches its module-level table for good (:223-224).
Only DATA is written - none of the reference's source text.  nan is stored as null.
"""
import gzip, json, math, os, stat, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
ROOT = os.path.dirname(os.path.dirname(HERE))


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
import uberBlast as UBR                  # noqa: E402  (the reference's)

sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from rescore_helpers import encode, random_hits, unpack_runs                                                     # noqa: E402
from rescore_codon_helpers import CODON_CLASSES, codon_classes, with_planted                                      # noqa: E402


def ref_codes(text):
    """readFastq upper-cases (configure.py:128), reScore encodes (uberBlast.py:403, 405)"""
    return UBR.nucEncoder[np.array(list(text.upper())).view(UBR.asc2int)] if text else np.zeros(0, dtype=int)


def call(aln, mode, table_id):
    r = ref_codes(aln['r'])
    with np.errstate(all='ignore'):
        out = UBR.cigar2score([aln['runs'], 4 - r[::-1] if aln['rev'] else r, ref_codes(aln['q']), aln['first'], mode, 6, 1, table_id])
    return [None if math.isnan(float(v)) else float(v) for v in out]


def main():
    rng = np.random.default_rng(2100)
    q_seqs, r_seqs, hits, arena, _ = random_hits(rng, 12, 12, 260, max_len=400)
    q_seqs, r_seqs, hits, arena = with_planted(rng, q_seqs, r_seqs, hits, arena, per_class=5)
    alns, cov = [], dict.fromkeys(CODON_CLASSES, 0)
    for h in hits.tolist():
        i, j, qs, qe, rs, re, n_runs, _, off = h
        runs = unpack_runs(arena[off:off + n_runs])
        lo, hi = min(rs, re), max(rs, re)
        alns.append(dict(q=q_seqs[i][qs - 1:qe].decode(), r=r_seqs[j][lo - 1:hi].decode(), rev=not rs < re, first=qs, runs=runs))
        for key in codon_classes(encode(q_seqs[i]), encode(r_seqs[j]), qs, qe, rs, re, runs):
            cov[key] += 1
    assert all(cov[k] >= 5 for k in CODON_CLASSES), cov
    assert max(len(a['q']) for a in alns) <= 400 and max(len(a['r']) for a in alns) <= 400
    cases = []
    for table_id in (11, 4):                                  # table 4 last: from its first call on the reference's table stays patched
        for mode in (2, 3):
            for k, a in enumerate(alns):
                cases.append(dict(aln=k, mode=mode, table_id=table_id, out=call(a, mode, table_id)))
    changed = sum(1 for c, d in zip(cases[:len(alns)], cases[2 * len(alns):3 * len(alns)]) if c['out'] != d['out'])
    n_nan = sum(1 for c in cases if c['out'][0] is None)
    assert changed >= 5 and n_nan >= 5, (changed, n_nan)
    out = os.path.join(HERE, 'g21_rescore_codons.json.gz')
    with gzip.GzipFile(out, 'wb', mtime=0) as f:
        f.write(json.dumps(dict(source='uberBlast.py:221-269 fed as :402-412', alignments=alns, cases=cases), separators=(',', ':')).encode())
    print(out, os.path.getsize(out), 'bytes,', len(alns), 'alignments,', len(cases), 'cases,', changed, 'differ under table 4,', n_nan, 'nan;', cov)


if __name__ == '__main__':
    main()
