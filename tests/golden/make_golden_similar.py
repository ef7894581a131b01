#!/usr/bin/env python3
"""Generate tests/golden/g24_similar_edges.json.gz by IMPORTING the reference's Python (build machine only: needs the reference checkout).

    python tests/golden/make_golden_similar.py

The same shim as make_golden_synteny.py; PEP.uberBlast, PEP.pool and PEP.params are patched the way g10_g11_g12() of make_golden.py patches
them, and the reference's own PEP.get_similar_pairs (PEPPAN.py:194-294) runs once per case of tests/similar_helpers.py in a temporary
directory of the case's own.  Only DATA is written - the canned table, gene lengths, priorities, params, the exemplar file and clust.npy
before and after, the returned pairs - none of the reference's source text.  Everything is seeded: two runs write the same bytes.  The
conditions each case was built for are asserted at the end on what the reference returned.
"""
import copy, gzip, json, os, sys, tempfile

from make_golden_synteny import PEP, np            # the shim: stub tools on PATH, numba / ete3 stand-ins, the reference on sys.path
import similar_helpers as H

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(case):
    rec = case.record()
    d = tempfile.mkdtemp(prefix='g24_')
    cl = os.path.join(d, 'p.clust.exemplar')
    with open(cl, 'w') as f:
        f.write(rec['exemplar_in'])
    npy = os.path.join(d, 'p.clust.npy')
    np.save(npy, np.array(rec['clust_npy_in'], dtype=int))
    tab = H.object_table(rec['table'])
    params = dict(rec['params'], clust=cl)
    PEP.uberBlast = lambda argv, pool=None: copy.deepcopy(tab)
    PEP.pool = None
    PEP.params = params
    res = PEP.get_similar_pairs(cl, H.priorities_of(rec), params)
    rec.update(pairs=[[int(x) for x in r] for r in res.tolist()], exemplar_out=open(cl).read(),
               clust_npy_out=[[int(x) for x in r] for r in np.load(npy, allow_pickle=True).tolist()])
    return rec


def check(g):
    by = {c['name']: c for c in g['cases']}
    out = lambda c: {p['tag']: d for p, d in zip(c['probes'], H.decode(c))}
    kind = lambda v: v if v in ('none', 'zero') else 'value'
    pairs = lambda c: {(a, b): v for a, b, v in c['pairs']}
    about = lambda v, w: w - 1 <= v <= w          # (int() of a mean of equal identities may fall one short of identity * 10000)
    names = lambda c: {int(l[1:]) for l in c['exemplar_out'].split('\n') if l.startswith('>')}
    for c in g['cases']:
        for p, d in zip(c['probes'], H.decode(c)):
            assert p['expect'] is None or p['expect'] == kind(d), (c['name'], p, d)
        edge = [r[2] for r in c['clust_npy_out']]
        assert len(set(edge)) == len(edge), c['name']                     # the order of clust.npy is defined
    # gates
    o = out(by['gate_len'])
    assert (kind(o['n30']), o['n29'], kind(o['n31'])) == ('value', 'none', 'value'), o
    for name, short, at in (('gate_prop_0.4_203', 27, 28), ('gate_prop_0.28_300', 28, 29), ('gate_prop_0.57_300', 56, 57)):
        o = out(by[name])
        ql = int(name.rsplit('_', 1)[1])
        for sl in (ql, ql + 60):
            assert o['n%d_sl%d' % (short, sl)] == 'none' and kind(o['n%d_sl%d' % (at, sl)]) == 'value', (name, o)
    n_id = 0
    for c in g['cases']:
        if c['name'].startswith('gate_identity_'):
            mi, o = c['params']['match_identity'], out(c)
            ns = sorted({p['n'] for p in c['probes']})
            for n in ns:
                assert o['n%d_%s' % (n, mi)] == 'none' and kind(o['n%d_%s' % (n, round(mi + 0.001, 3))]) == 'value' and o['n%d_%s' % (n, round(mi - 0.001, 3))] == 'none', o
            assert ns[0] == 1 and ns[1] >= 64 and mi * 10000 != round(mi * 10000)
            n_id += 1
    assert n_id == 2
    for which in range(3):
        o = out(by['need_%d_len' % which])
        assert (kind(o['n30']), o['n29'], o['n10'], o['n9']) == ('value', 'zero', 'zero', 'none'), o
        o = out(by['need_%d_prop' % which])
        assert (kind(o['n30']), o['n29'], o['n6'], o['n5']) == ('value', 'zero', 'zero', 'none'), o
    o = out(by['gate_20x'])
    assert [kind(o['ql%d_sl%d' % x]) for x in ((2000, 100), (2000, 101), (100, 2000), (101, 2000), (1980, 99), (99, 1980), (1981, 99), (99, 1981), (1979, 99), (99, 1979))] == \
        ['none', 'value', 'none', 'value', 'none', 'none', 'none', 'none', 'value', 'value'], o
    # frames: only the closing row counts where the frames differ, unless incomplete CDSs are allowed
    o0, o1 = out(by['frames_none']), out(by['frames_f'])
    closing = o0['5_5_1M']
    assert closing == o1['5_5_1M'] and kind(closing) == 'value'
    for qs in (4, 5, 6):
        for ss in (4, 5, 6):
            t = '%d_%d_30M' % (qs, ss)
            assert (o0[t] != closing) == (qs % 3 == ss % 3) and o1[t] != closing, (t, o0[t], o1[t])
    assert sum(o0[t] != o1[t] for t in o0) >= 12 and len({v for v in o1.values()}) >= 10
    # several rows
    for k in (2, 3, 6, 49):
        o = out(by['rows%d' % k])
        assert len({o[t] for t in ('descending', 'ascending', 'shuffled', 'shuffled2')}) >= 2, o
        assert kind(o['early']) == 'value' and o['undecided'] == 'none'
    # the ordered pass
    c = by['ordered']
    n, p, alive, clu = c['notes'], pairs(c), names(c), c['clust_npy_out']
    a, b = n['judged49']; assert (a, b) in p and {a, b} <= alive
    a, b, x = n['killed50']; assert b not in alive and (a, b) not in p and (b, x) not in p and about(p[(a, x)], 7300)
    a, x, y = n['self50']; assert a not in alive and about(p[(a, x)], 7400) and (a, y) not in p
    a, b, x = n['settled_by_victim']; assert b not in alive and about(p[(a, b)], 7700) and (b, x) not in p
    a, b, b2, x = n['absorbed_while_pending']; assert a not in alive and about(p[(a, b)], 7900) and [b2, a, 9510] in clu and (a, x) not in p and about(p[(b, x)], 8300)
    a, b, x = n['absorbed_ref']; assert b not in alive and [a, b, 9520] in clu and (b, x) not in p and about(p[(a, x)], 8600)
    a, r = n['ref_only']; assert r not in alive and about(p[(a, r)], 6100)
    assert n['skipped_only'][0] in alive
    a, b = n['conflict_first']; assert p[(a, b)] == -2
    a, b, x = n['conflict_after']; assert p[(a, b)] == -2 and list(p).index((a, b)) < list(p).index((a, x))
    a, b = n['zero_blocks']; assert (a, b) not in p and {a, b} <= alive
    a, b = n['not_saved']; assert (a, b) in p and b in alive
    a, b = n['not_split']; assert (a, b) not in p and b not in alive
    z, a = n['last_group']; assert about(p[(a, z)], 6900) and c['table'][-1][:2] == [str(z), str(a)]
    c = by['ordered_last50']
    x, a = c['notes']['last50']; assert a not in names(c) and c['table'][-1][:2] == [str(x), str(a)]
    c = by['string_order']
    assert [r[0] for r in c['table']][::3] == ['10', '100', '9'] and list(pairs(c)) == [(10, 100), (9, 10), (9, 100)] and all(about(pairs(c)[k], w) for k, w in (((9, 10), 7000), ((10, 100), 7200), ((9, 100), 7100)))
    # the row-local tests
    for c in g['cases']:
        if c['family'] != 'rowlocal':
            continue
        p, alive = pairs(c), names(c)
        lab = {l['tag']: (l['a'], l['b']) for l in c['labels']}
        conflict = lambda t: p.get(lab[t]) == -2
        gone = lambda t, k: lab[t][k] not in alive
        ci = c['params']['clust_identity']
        assert gone('iden_%s' % ci, 0) and not gone('iden_%s' % round(ci - 0.0001, 4), 0) and gone('iden_%s' % (0.9999 if ci > 0.5 else 0.57), 0)
        assert [int(ci * 10000.), int((0.9999 if ci > 0.5 else 0.57) * 10000.)] == [r[2] for r in c['clust_npy_out'] if r[1] in (lab['iden_%s' % ci][0], lab['iden_%s' % (0.9999 if ci > 0.5 else 0.57)][0])][::-1]
        for L in (300, 290):
            for t in ('qa', 'sa'):
                assert not conflict('%s_%d_-1' % (t, L)) and conflict('%s_%d_1' % (t, L))
            assert not gone('absq_%d_-1' % L, 0) and gone('absq_%d_1' % L, 0) and not gone('absr_%d_-1' % L, 1) and gone('absr_%d_1' % L, 1)
        assert not gone('equal_prio_fails', 0) and not gone('equal_prio_fails', 1) and not gone('equal_qa_fails', 0) and not gone('equal_qa_fails', 1)
        assert [gone('prio_q_%d_%d' % x, 0) for x in ((0, 0), (1, 0), (0, 1), (2, 2))] == [True, True, False, True]
        assert [gone('prio_r_%d_%d' % x, 1) for x in ((0, 0), (1, 0), (0, 1), (2, 2))] == [True, False, True, True]
        assert conflict('head_shift') and lab['head_tail_shift'] not in p and not gone('head_tail_shift', 0) and p[lab['tail_shift_only']] > 0
    # at the exact products the comparison is the float one: 0.81 * 300 = 243.00000000000003 is not reached by 243 positions
    c = by['rowlocal_0.9_0.81']
    lab = {l['tag']: (l['a'], l['b']) for l in c['labels']}
    assert pairs(c).get(lab['qa_300_0']) is None and pairs(c).get(lab['sa_300_0']) is None
    c = by['rowlocal_0.9_0.8']
    lab = {l['tag']: (l['a'], l['b']) for l in c['labels']}
    assert pairs(c)[lab['qa_300_0']] == -2 and pairs(c)[lab['sa_300_0']] == -2
    # what the fixture is pinned by (tests/test_similar_host.py asserts the same from the file)
    f = H.fixture_figures(g)
    print(f)
    H.assert_figures(f)


def main():
    g = dict(source='PEPPAN.py:194-294 (get_similar_pairs, get_similar)', cases=[run_case(c) for c in H.all_cases()])
    g = json.loads(json.dumps(g))
    check(g)
    # the restatement agrees with the reference on every case
    for c in g['cases']:
        got, kept, edges = H.restate_pass(c['table'], H.priorities_of(c), c['params'])
        text, clu = H.expected_files(c, kept, edges)
        assert got == c['pairs'] and text == c['exemplar_out'] and clu == c['clust_npy_out'], c['name']
    out = os.path.join(HERE, H.FIXTURE)
    with gzip.GzipFile(out, 'wb', mtime=0) as f:
        f.write(json.dumps(g, separators=(',', ':')).encode())
    print(out, os.path.getsize(out), 'bytes;', len(g['cases']), 'cases,', sum(len(c['table']) for c in g['cases']), 'rows')
    assert os.path.getsize(out) < 700 << 10


if __name__ == '__main__':
    main()
