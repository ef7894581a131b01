#!/usr/bin/env python3
"""Generate tests/golden/g27_outalleles.json.gz by RUNNING the reference's own write_output (build machine only: needs /root/reference).

    python tests/golden/make_golden_outalleles.py

The shim of make_golden_synteny.py; PEP.pool2 is replaced by an object whose imap_unordered records every toRun item before it maps the reference's own
determineGeneStructure over them.  The allele pass (PEPPAN.py:1391-1472) is observed without editing the reference: a trace function on write_output's frame
copies the table when line 1391 is about to run (the table as it stands at :1390) and when line 1473 is (the table the pass left), and takes the `alleles`
dictionary - both levels in insertion order - when the function returns.  params['min_cds'] = 0 and untrusted = [0, 0.] keep the rest of write_output running.
Only DATA is written - inputs and recorded results - none of the reference's source text.  The cases are built by tests/outalleles_helpers.py; the small ones
are stored with their tables, the two-batch case with its seed and the reference's results alone.  The restatement of that file is held to every case here,
and the conditions the fixture is pinned by are asserted at the end.
"""
import copy
import gzip
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_golden_synteny as SHIM       # noqa: E402  (builds the shim, puts the reference on the path, imports it as SHIM.PEP)
import numpy as np                       # noqa: E402
import outalleles_helpers as H           # noqa: E402

PEP = SHIM.PEP
FIRST_LINE, AFTER_LINE = 1391, 1473
TWO_BATCH_SEED = 27102
CODE = PEP.write_output.__code__


def plain(v):
    """numpy scalars and arrays as plain Python values"""
    if isinstance(v, (list, tuple, np.ndarray)):
        return [plain(x) for x in v]
    if isinstance(v, np.integer):
        return int(v)
    if isinstance(v, np.floating):
        return float(v)
    return v


class RecordingPool(object):
    def __init__(self):
        self.items = []

    def imap_unordered(self, fn, items):
        out = []
        for it in items:
            got = fn(it)
            self.items.append(dict(pid=int(it[0]), s=int(it[3]), e=int(it[4]), s2=int(it[5]), e2=int(it[6]), lp=int(it[7]), allowed_vary=int(it[8]),
                                   cds=got[1], start=int(got[2]), stop=int(got[3])))
            out.append(got)
        return out


def run_reference(inputs):
    """write_output on one case -> dict(before, after, alleles, sent)"""
    seen = {}

    def local_trace(frame, event, arg):
        if event == 'line' and frame.f_lineno == FIRST_LINE and 'before' not in seen:
            seen['before'] = [plain(list(r)) for r in frame.f_locals['prediction']]
        elif event == 'line' and frame.f_lineno == AFTER_LINE:
            seen['after'] = [plain(list(r)) for r in frame.f_locals['prediction']]
        elif event == 'return':
            seen['alleles'] = {g: dict(a) for g, a in frame.f_locals.get('alleles', {}).items()}
        return local_trace

    def global_trace(frame, event, arg):
        return local_trace if frame.f_code is CODE else None

    where = tempfile.mkdtemp(prefix='outalleles_')
    path = os.path.join(where, 'in.Prediction')
    with open(path, 'w') as f:
        for r in inputs['rows']:
            f.write('\t'.join(str(x) for x in r) + '\n')
    pool = RecordingPool()
    PEP.pool2 = pool
    PEP.params['min_cds'] = 0
    sys.settrace(global_trace)
    try:
        PEP.write_output(os.path.join(where, 'out'), path, inputs['genomes'], inputs['clust_ref'], inputs['encodes'], copy.deepcopy(inputs['old_prediction']),
                         inputs['pseudogene'], [0, 0.], inputs['gtable'])
    finally:
        sys.settrace(None)
    assert set(seen) == {'before', 'after', 'alleles'}, sorted(seen)
    seen['sent'] = pool.items
    return seen


def held(inputs, got):
    """the restatement against what the reference did"""
    table = copy.deepcopy(got['before'])
    alleles, rows = H.restate(table, inputs['genomes'], inputs['encodes'], inputs['clust_ref'], inputs['pseudogene'], inputs['gtable'])
    assert table == got['after'], next((a, b) for a, b in zip(table, got['after']) if a != b)
    assert alleles == got['alleles'] and list(alleles) == list(got['alleles'])
    for g in alleles:
        assert list(alleles[g].items()) == list(got['alleles'][g].items()), g
    assert sorted(i for i, r in enumerate(rows) if r and r['sent']) == sorted(x['pid'] for x in got['sent'])
    for x in got['sent']:
        r = rows[x['pid']]
        assert (r['s2'], r['e2'], r['lp']) == (x['s2'], x['e2'], x['lp']), x
    return rows


def neighbour_walk(table, i):
    """(rows of the same contig inside the look range, misc_feature rows among them, whether the chosen one is not the nearest candidate)"""
    row = table[i]
    rng = range(i + 1, min(i + 5, len(table))) if row[11] == '+' else range(i - 1, max(i - 5, 0) - 1, -1)
    walked, misc, candidates = 0, 0, []
    for j in rng:
        if table[j][5] != row[5]:
            break
        walked += 1
        if table[j][15] == 'misc_feature':
            misc += 1
        else:
            candidates.append(j)
    return walked, misc, len(candidates) > 1, j_changed(table, i, rng)


def j_changed(table, i, rng):
    return any(table[j][5] != table[i][5] for j in rng)


def main():
    out = dict(note='recorded from the reference write_output by make_golden_outalleles.py; data only', small=[], two_batch=None)
    hit = set()
    for name, make, seed in H.SMALL_CASES:
        case = H.small_case(name)
        inputs = case.inputs()
        got = run_reference(inputs)
        rows = held(inputs, got)
        before, alleles = got['before'], got['alleles']
        out['small'].append(dict(name=name, genomes={str(k): list(v) for k, v in inputs['genomes'].items()}, encodes=inputs['encodes'],
                                 clust_ref={str(k): v for k, v in inputs['clust_ref'].items()}, pseudogene=inputs['pseudogene'], gtable=inputs['gtable'],
                                 before=before, after=got['after'], alleles=[[g, list(a.items())] for g, a in alleles.items()], sent=got['sent']))
        # ---- which of the conditions the fixture is pinned by this case meets
        enc, ref = inputs['encodes'], inputs['clust_ref']
        for i, (row, info) in enumerate(zip(before, rows)):
            if info is None:
                hit.add('skipped')
                continue
            g = row[0]
            seeded = g in enc and enc[g] in ref
            if seeded and info['id'] == '1' and info['allele'] == ref[enc[g]]:
                hit.add('seed reused')
            hit.add('seeded gene' if seeded else 'gene without a seed' if g in enc else 'gene not in encodes')
            if row[4]:
                hit.add('secondary')
            if '/' in g:
                hit.add('slash name')
            vary = int(row[12] * (1 - inputs['pseudogene']) + 0.01)
            length = row[10] - row[9] + 1
            if info['kind'] == 'fragment':
                hit.add('fragment by column 1' if row[1] > 1 else 'fragment by length')
                if row[1] <= 1 and length == row[12] - vary - 1:
                    hit.add('fragment one short')
                continue
            if length == row[12] - vary:
                hit.add('intact at the fragment threshold')
            clean = row[4] == '' and row[7] == 1 and row[8] == row[12]
            if clean and info['id'].startswith('t'):
                hit.add('t inherited by a clean row')
            if not clean and not info['id'].startswith('t') and info['id'] != '1':
                hit.add('plain id inherited by a t row')
            if not clean and info['id'] == '1':
                hit.add('seed id on a t row')
            base = g.rsplit('/', 2)[0]
            if enc[base] in ref:
                x = inputs['pseudogene'] * len(ref[enc[base]])
                if info['kind'] == 'structural_variation' and len(info['allele']) + 1 >= x:
                    hit.add('structural variation one short')
                if info['kind'] == 'intact' and len(info['allele']) - 1 < x:
                    hit.add('no structural variation at the threshold')
            walked, misc, not_nearest, changed = neighbour_walk(before, i)
            hit.add('%s %d walked' % (row[11], walked))
            if misc:
                hit.add('misc in between ' + row[11])
            if not_nearest:
                hit.add('not the nearest ' + row[11])
            if changed:
                hit.add('contig change ' + row[11])
            if len(info['allele']) < length:
                hit.add('negative rp')
            if info['s2'] == 1 and row[9] > 1:
                hit.add('clipped at the start')
            if row[9] == info['s2'] and row[11] == '+':
                hit.add('no room at the start')
            if info['e2'] - row[10] < 3 and row[13] - row[10] < 60:
                hit.add('clipped at the end')
            hit.add('strand ' + row[11])
            if len(info['allele']) in (55, 56, 63, 64, 119, 120):
                hit.add('span %d %s' % (len(info['allele']), row[11]))
            for ch, label in (('N', 'N'), ('R', 'R')):
                text = inputs['genomes'][enc[row[5]]][1][row[9] - 1:row[10]]
                if ch in text:
                    hit.add('%s on %s' % (label, row[11]))
                if text != text.upper():
                    hit.add('lower case on ' + row[11])
        per_gene = {}
        for row in before:
            if row[15] != 'misc_feature':
                per_gene[row[0]] = per_gene.get(row[0], 0) + 1
        for g, n in per_gene.items():
            if n in (64, 65):
                hit.add('gene with %d rows' % n)
            if len(alleles[g]) >= 300:
                hit.add('gene with 300 alleles')
        homes = {}
        for row, info in zip(before, rows):
            if info is not None:
                homes.setdefault((row[0], info['allele']), set()).add(row[5])
        if any(len(v) > 1 for v in homes.values()):
            hit.add('one allele on several contigs')

    # ---- the two-batch case: its seed and the reference's results, not its rows
    case = H.two_batch_case(TWO_BATCH_SEED)
    inputs = case.inputs()
    got = run_reference(inputs)
    assert got['before'] == H.table_of(case), 'the two-batch rows are no fixed points of the front end'
    assert len(got['before']) >= H.BATCH + 6
    rows = held(inputs, got)
    stale = {i: r[9] for i, r in enumerate(got['before'])}
    moved = 0
    for i in range(H.BATCH, H.BATCH + 5):
        row = got['before'][i]
        if row[11] == '-' and rows[i] is not None and rows[i]['kind'] != 'fragment':
            table = copy.deepcopy(got['before'])
            one = H.restate(table, inputs['genomes'], inputs['encodes'], inputs['clust_ref'], inputs['pseudogene'], inputs['gtable'], batch=len(table))[1][i]
            if one['s2'] != rows[i]['s2']:
                moved += 1
    assert moved >= 1, 'no head row whose s2 differs between the updated and the stale column 9'
    out['two_batch'] = dict(seed=TWO_BATCH_SEED, n_rows=len(got['before']), heads_moved=moved, pseudogene=inputs['pseudogene'], gtable=inputs['gtable'],
                            cols=[[r[9], r[10], r[13], r[15]] for r in got['after']], alleles=[[g, [[len(s), i] for s, i in a.items()]] for g, a in got['alleles'].items()],
                            allele_sha1=H.allele_digest(got['alleles']), sent=len(got['sent']))

    wanted = {'skipped', 'seed reused', 'seeded gene', 'gene without a seed', 'gene not in encodes', 'secondary', 'slash name', 'fragment by column 1', 'fragment by length',
              'fragment one short', 'intact at the fragment threshold', 't inherited by a clean row', 'plain id inherited by a t row', 'seed id on a t row',
              'structural variation one short', 'no structural variation at the threshold', 'negative rp', 'clipped at the start', 'clipped at the end',
              'strand +', 'strand -', 'N on +', 'N on -', 'R on +', 'R on -', 'lower case on +', 'lower case on -', 'gene with 64 rows', 'gene with 65 rows',
              'gene with 300 alleles', 'one allele on several contigs', 'misc in between +', 'misc in between -', 'not the nearest +', 'not the nearest -',
              'contig change +', 'contig change -'}
    wanted |= {'+ %d walked' % k for k in range(5)} | {'- %d walked' % k for k in range(6)}
    wanted |= {'span %d %s' % (n, st) for n in (55, 56, 63, 64, 119, 120) for st in '+-'}
    assert wanted <= hit, sorted(wanted - hit)
    out['hit'] = sorted(hit)
    path = os.path.join(HERE, 'g27_outalleles.json.gz')
    with gzip.GzipFile(path, 'wb', mtime=0) as f:
        f.write(json.dumps(out, sort_keys=True).encode())
    print(path, os.path.getsize(path), 'bytes;', sum(len(c['before']) for c in out['small']), 'small rows')


if __name__ == '__main__':
    main()
