#!/usr/bin/env python3
"""Generate tests/golden/g25_parser.json.gz by IMPORTING the reference's Python (build machine only).

    python tests/golden/make_golden_parser.py

The shim of make_golden_synteny.py, taken by importing that module: it puts the reference on the path (its ete3 stub is all PEPPAN_parser needs beside
scipy).  Every case is a seeded synthetic pan-genome, some of them written as a small GFF text and read by the reference's getOrtho.  Recorded per case:
the input, the seed, the genome orders the reference walked (seen by wrapping np.random.shuffle: its list of genomes after every shuffle), its `curves`
array (seen by wrapping np.mean, the one place it is handed over), the text of <prefix>_content.curve, and for writeCGAV the two texts, the profile
matrix and getDistance's matrix as hex floats; plus getDistance on a few hand-made profile matrices.  Only DATA is written, none of the reference's source
text.  Replaying the seed on an index array must give the recorded orders, the restatement of tests/parser_helpers.py is held to every case, and the
conditions the fixture is pinned by are asserted at the end.
"""
import gzip, json, os, sys, tempfile, warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_synteny import np                            # noqa: E402  (the shim; also puts tests/ and the reference on the path)
import scipy                                                  # noqa: E402
import PEPPAN_parser as REF                                   # noqa: E402
from parser_helpers import (gff_of_groups, groups_as_lists, groups_of_presence, presence_of_groups, random_presence, random_profiles, restate_curves,   # noqa: E402
                            restate_pairs)

OUT = tempfile.mkdtemp(prefix='peppan_g25_')


def read(path):
    with open(path) as f:
        return f.read()


def run_curve(groups, seed, n_iter, pseudogene):
    """the reference's writeCurve under a seed -> (orders it walked, its curves, the file's text)"""
    seen = {'orders': [], 'index': None, 'curves': None}
    real_shuffle, real_mean = np.random.shuffle, np.mean

    def shuffle(x):
        if seen['index'] is None:                                            # the list before its first shuffle: genome k of groups.values() at place k
            seen['index'] = {id(m): k for k, m in enumerate(x)}
        real_shuffle(x)
        seen['orders'].append([seen['index'][id(m)] for m in x])

    def mean(a, *args, **kwargs):
        if isinstance(a, np.ndarray) and a.ndim == 3:
            seen['curves'] = a.copy()
        return real_mean(a, *args, **kwargs)

    prefix = os.path.join(OUT, 'curve%d' % seed)
    np.random.seed(seed)
    np.random.shuffle, np.mean = shuffle, mean
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            summary = REF.writeCurve(prefix, groups, pseudogene, n_iter)
    finally:
        np.random.shuffle, np.mean = real_shuffle, real_mean
    assert not summary.any() and summary.shape == (len(groups), 2, 5)
    # the same seed on an index array, shuffled in place again and again
    np.random.seed(seed)
    index = np.arange(len(groups))
    for t in range(n_iter):
        np.random.shuffle(index)
        assert index.tolist() == seen['orders'][t], ('orders', seed, t)
    assert len(seen['orders']) == n_iter and seen['curves'].shape == (len(groups), n_iter, 2)
    return seen['orders'], seen['curves'], read(prefix + '_content.curve')


def run_cgav(groups, pCore, tag):
    prefix = os.path.join(OUT, 'cgav_%s' % tag)
    REF.writeCGAV(prefix, groups, pCore)
    profile = read(prefix + '_CGAV.profile')
    rows = [[int(v) for v in line.split('\t')[1:] if v] for line in profile.splitlines()[1:]]        # (no gene reaches pCore: a bare tab)
    dist = REF.getDistance(np.array(rows))
    return dict(pCore=pCore, profile_text=profile, dist_text=read(prefix + '_CGAV.dist'), profiles=rows, dist_hex=[[float(v).hex() for v in row] for row in dist])


def edge_presence():
    """12 genomes x 70 genes: genome 0 carries every gene, genome 1 one gene (gene 0), gene 0 is in every genome, gene 69 only in genome 0; genomes 2 and 3 share
    nothing but gene 0 and carry all but gene 69 between them"""
    rng = np.random.default_rng(2501)
    P = random_presence(rng, 12, 70, core=0.1, shell=0.5)
    P[:, 0] = 1
    P[0, :] = 1
    P[1, :] = 0
    P[1, 0] = 1
    P[1:, 69] = 0
    P[1:, 64:69] = 0
    P[4, 64:69] = 1
    P[2, 1:69] = np.arange(1, 69) % 2
    P[3, 1:69] = 1 - P[2, 1:69]
    return P


def main():
    rng = np.random.default_rng(25000)
    cases, pairs = [], []

    def add(name, groups, seed, n_iter, pseudogene, pCore, gff=None, no_pseudogene=None):
        orders, curves, text = run_curve(groups, seed, n_iter, pseudogene)
        presence = presence_of_groups(groups)
        assert restate_curves(presence, orders) == curves.tolist(), name
        case = dict(name=name, groups=groups_as_lists(groups), seed=seed, n_iter=n_iter, pseudogene=pseudogene, orders=orders, curves=curves.tolist(), curve_text=text,
                    mean_size=float(np.mean([sum(r) for r in presence])).hex(), cgav=run_cgav(groups, pCore, name))
        if gff is not None:
            case.update(gff=gff, no_pseudogene=no_pseudogene)
        s, p = restate_pairs(case['cgav']['profiles'])
        want = [[0. if i == j else float(-np.log((s[i][j] + 0.5) / (p[i][j] + 1.))) for j in range(len(s))] for i in range(len(s))]
        assert [[v.hex() for v in row] for row in want] == case['cgav']['dist_hex'], name
        cases.append(case)

    # through a GFF text and the reference's getOrtho, with and without the pseudogene lines
    text = gff_of_groups(groups_of_presence(random_presence(rng, 23, 149), rng))
    path = os.path.join(OUT, 'small.gff')
    with open(path, 'w') as f:
        f.write(text)
    for no_pseudogene, n_iter in ((False, 50), (True, 129)):
        groups = REF.getOrtho(path, no_pseudogene)
        add('gff_%s' % ('cds' if no_pseudogene else 'all'), {g: dict(v) for g, v in groups.items()}, 2511 + n_iter, n_iter, not no_pseudogene, 90 if no_pseudogene else 40, gff=text, no_pseudogene=no_pseudogene)
    add('wide', groups_of_presence(random_presence(rng, 40, 300, core=0.3, shell=0.2), rng), 2513, 130, True, 50)
    add('edges', groups_of_presence(edge_presence(), rng), 2514, 37, True, 50)
    add('tiny_default_n_iter', groups_of_presence(random_presence(rng, 4, 6, core=0.4, shell=0.4), rng), 2515, 1000, True, 0)

    def add_pairs(name, profiles):
        profiles = np.array(profiles)
        dist = REF.getDistance(profiles)
        s, p = restate_pairs(profiles.tolist())
        want = -np.log((np.array(s) + 0.5) / (np.array(p) + 1.))
        np.fill_diagonal(want, 0.)
        assert np.array_equal(want, dist), name
        pairs.append(dict(name=name, profiles=profiles.tolist(), shared=s, presence=p, dist_hex=[[float(v).hex() for v in row] for row in dist]))

    prof = random_profiles(rng, 17, 33)
    prof[3] = 0                                                              # a row of zeros
    prof[5] = -prof[6]                                                       # a row of negatives
    prof[8] = prof[7]                                                        # identical rows
    add_pairs('random_17x33', prof)
    add_pairs('one_gene', [[1], [1], [2], [0], [-1]])
    add_pairs('one_profile', [[3, 1, 4, 1, 5]])
    big = random_profiles(rng, 9, 21).astype(np.int64)
    big[big == 1] = 2 ** 40 + 1
    big[big == 2] = 2 ** 40 + 1 + 2 ** 32                                    # equal to the one above in its low 32 bits
    big[big == -1] = -2 ** 35
    big[big == 3] = 2 ** 32 + 3                                              # 3 in its low 32 bits, 4 stays 4
    add_pairs('beyond_int32', big)

    # what the fixture is pinned by
    edges = next(c for c in cases if c['name'] == 'edges')
    P = np.array(presence_of_groups({g: {grp: dict(cp) for grp, cp in og} for g, og in edges['groups']}))
    per_genome, per_gene = P.sum(1), P.sum(0)
    assert per_genome.max() == P.shape[1] and per_genome.min() == 1, 'a genome with every gene and a genome with one'
    assert (per_gene == len(P)).sum() == 1 and (per_gene == 1).sum() >= 1, 'one gene in every genome, a gene in exactly one'
    C = np.array(edges['curves'])
    assert C[:, :, 1].min() == 1 and (C[-1, :, 1] == 1).all() and (C[-1, :, 0] == P.shape[1]).all(), 'core never drops below the gene every genome has'
    early = [t for t, o in enumerate(edges['orders']) if {2, 3} <= set(o[:4])]
    assert early and all(C[3, t, 0] >= P.shape[1] - 1 and C[3, t, 1] == 1 for t in early), 'orders whose AND empties and whose OR all but fills within four steps'
    for c in cases:
        C = np.array(c['curves'])
        assert (np.diff(C[:, :, 0], axis=0) >= 0).all() and (np.diff(C[:, :, 1], axis=0) <= 0).all(), c['name']
        assert len(c['curve_text'].splitlines()) == 8 + len(c['groups'])
    assert {c['n_iter'] for c in cases} >= {37, 50, 129, 130, 1000} and {c['pseudogene'] for c in cases} == {True, False}
    assert any(len(c['groups'][0][1]) % 64 for c in cases)
    first = pairs[0]
    assert float.fromhex(first['dist_hex'][3][0]) == -np.log(0.5) and float.fromhex(first['dist_hex'][5][6]) == -np.log(0.5), 'rows of zeros and of negatives'
    assert first['shared'][7][8] == first['presence'][7][8] > 0, 'identical rows'
    assert max(max(abs(v) for v in row) for row in pairs[3]['profiles']) >= 2 ** 40
    assert any(c['cgav']['profiles'] and 0 in sum(c['cgav']['profiles'], []) for c in cases)
    out = os.path.join(HERE, 'g25_parser.json.gz')
    with gzip.GzipFile(out, 'wb', mtime=0) as f:
        f.write(json.dumps(dict(source='PEPPAN_parser.py:37-61, 63-115, 145-179 (getOrtho, writeCurve, writeCGAV, getDistance)', scipy=scipy.__version__,
                                numpy=np.__version__, cases=cases, pairs=pairs), separators=(',', ':')).encode())
    print(out, os.path.getsize(out), 'bytes;', len(cases), 'cases,', len(pairs), 'profile matrices; scipy', scipy.__version__)
    assert os.path.getsize(out) < 300 << 10


if __name__ == '__main__':
    main()
