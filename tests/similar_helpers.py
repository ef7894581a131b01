"""Shared by tests/golden/make_golden_similar.py, tests/test_similar_host.py and tests/test_gpu_similar.py: the pass of get_similar_pairs
(PEPPAN.py:194-294) at its edges.

    Case / the *_cases builders   canned all-vs-all tables shaped like pairs_table of make_golden.py builds them (names as strings, rows sorted by
                                  columns [0, 1, 11]), one family of edges per builder; random_case mixes the same row makers freely
    load_g24                      the recorded fixture (the reference's own get_similar_pairs on every case)
    decode                        get_similar's outcome per probed pair, read back from the recorded pairs alone
    restate_pass                  the whole pass once more in plain loops and dictionaries, written from the behaviour; it calls neither the
                                  oracle's pair_support nor _classify_rows nor the library, so it is a third opinion
    k14_inputs                    the groups of the probed pairs as K14 takes them, without going through pep_similar_scan

How get_similar's three outcomes become visible.  get_similar is a nested function; a None and a 0 both leave nothing in the returned pairs.
For a probed pair (a, b), a < b, the table also holds a group (b, a) of ONE clean full-length in-frame row of identity 1.0 (the sentinel; every
probe row's identity is below 1, so no probe can return 10000).  The dictionary's first-writer-wins rule then separates the three:
    the pairs hold (a, b)'s own value    that value
    nothing for the key                  0     ((a, b) wrote 0, which blocked (b, a) and was filtered from the result)
    the pairs hold 10000                 None  ((a, b) wrote nothing, (b, a) was judged)
The length test of PEPPAN.py:199-200 is symmetric in the two genes, so a sentinel cannot show it: probes of kind 'length_gate' carry none,
their rows are far above every other gate (a 0 is impossible), and a missing key means None."""
import gzip, json, math, os, re
import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURE = 'g24_similar_edges.json.gz'
SENTINEL, SENTINEL_VALUE = 1.0, 10000
BASE = dict(noDiamond=False, match_identity=0.5, match_frag_len=50, n_thread=2, match_frag_prop=0.25, gtable=11,
            clust_identity=0.9, clust_match_prop=0.8, incompleteCDS='', match_len=250., match_len1=100., match_len2=400.,
            match_prop=0.5, match_prop1=0.8, match_prop2=0.4)
LOW = dict(clust_identity=1.5, match_identity=0.01, match_len=3., match_len1=3., match_len2=3., match_prop=1e-6, match_prop1=1e-6, match_prop2=1e-6)
TREE_N = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130, 136, 137, 255, 256, 257, 264, 265, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097)
TREE_IDEN = (0.57, 0.7, 0.813, 0.931)
TREE_BUFFER = (8191, 8192, 8193, 8200, 8320, 12000, 16385, 20000)          # around and beyond numpy's reduction buffer of 8192 elements
TREE_LONG = 40000                    # more than 32 768 covered positions


def runs_of(cigar):
    return [(int(n), t) for n, t in re.findall(r'(\d+)([A-Z])', cigar)]


def up3(n):
    return n + (-n) % 3


class Case(object):
    """one canned table: genes (id -> length), rows in the order they were added (the score column keeps that order inside a (query,
    reference) group), priorities, the probed pairs"""

    def __init__(self, name, family, first_id=1000, **params):
        self.name, self.family, self.params = name, family, dict(BASE, **params)
        self.genes, self.prio, self.rows, self.probes = {}, {}, [], []
        self.next_id = first_id
        self.clust_npy_in = [[1, 2, 10000], [3, 4, 9950]]
        self.labels, self.notes = [], {}

    def gene(self, length, prio=0, self_row=True, gid=None):
        g = self.next_id if gid is None else gid
        assert g not in self.genes
        self.next_id = max(self.next_id, g + 1)
        self.genes[g], self.prio[g] = length, [prio, -length, g]
        if self_row:
            self.row(g, g, 1.0, 1, 1, '%dM' % length)
        return g

    def pair(self, la, lb=None, pa=0, pb=0):
        a = self.gene(la, pa)
        return a, self.gene(la if lb is None else lb, pb)

    def row(self, q, r, iden, qs, ss, cigar, reverse=False):
        """an alignment that starts at query position qs; ss is its first reference column (the larger end on the reverse strand)"""
        runs = runs_of(cigar)
        qe = qs + sum(n for n, t in runs if t in 'MI') - 1
        rspan = sum(n for n, t in runs if t in 'MD')
        se = ss - rspan + 1 if reverse else ss + rspan - 1
        assert 1 <= qs and qs <= qe + 1 and qe <= self.genes[q] and 1 <= min(ss, se) and max(ss, se) <= self.genes[r], (q, r, qs, qe, ss, se)
        self.rows.append([q, r, iden, qs, qe, ss, se, cigar])

    def full(self, q, r, iden):
        """one clean in-frame row over the whole of the shorter gene"""
        self.row(q, r, iden, 1, 1, '%dM' % min(self.genes[q], self.genes[r]))

    def probe(self, a, b, tag, expect, sentinel=True, **extra):
        assert a < b
        if sentinel:
            self.full(b, a, SENTINEL)
        self.probes.append(dict(a=a, b=b, tag=tag, expect=expect, kind='sentinel' if sentinel else 'length_gate', **extra))

    def label(self, a, b, tag):
        self.labels.append(dict(a=a, b=b, tag=tag))

    def table(self):
        out = [[str(q), str(r), iden, qe - qs + 1, 0, 0, qs, qe, ss, se, 0.0, float(k), self.genes[q], self.genes[r], cigar, k]
               for k, (q, r, iden, qs, qe, ss, se, cigar) in enumerate(self.rows)]
        out.sort(key=lambda x: (x[0], x[1], x[11]))
        return out

    def exemplar(self):
        return ''.join('>%d\n%s\n' % (g, ('ACGT' * (L // 4 + 1))[:L]) for g, L in self.genes.items())

    def record(self):
        return dict(name=self.name, family=self.family, params=self.params, genes=[[g, L] for g, L in self.genes.items()], table=self.table(),
                    priorities={str(g): p for g, p in self.prio.items()}, clust_npy_in=self.clust_npy_in, exemplar_in=self.exemplar(), probes=self.probes, labels=self.labels,
                    notes=self.notes)


# ------------------------------------------------------------------------------------------------------------------ the families
def tree_cases():
    """one forward in-frame row of constant identity over n positions, gates so low that the first M run decides: the value is
    int(np.mean([v] * n) * 10000), and the summation tree is all that stands between it and its neighbour"""
    c = Case('tree', 'tree', **LOW)
    for v in TREE_IDEN:
        for n in TREE_N:
            a, b = c.pair(up3(n) + 3)
            c.row(a, b, v, 1, 1, '%dM' % n if n > 1 else '1M1D')             # (a row of one reference column has ss == se and is never judged)
            c.probe(a, b, 'n%d' % n, 'value', n=n, iden=v)
    for v in TREE_IDEN[:2]:
        for n in TREE_BUFFER:
            a, b = c.pair(up3(n) + 3)
            c.row(a, b, v, 1, 1, '%dM' % n)
            c.probe(a, b, 'n%d' % n, 'value', n=n, iden=v)
    a, b = c.pair(up3(TREE_LONG) + 3)
    c.row(a, b, 0.57, 1, 1, '%dM' % TREE_LONG)
    c.probe(a, b, 'long', 'value', n=TREE_LONG, iden=0.57)
    return [c]


def _slots(c, a, b, order, idens, step=30, length=45):
    """rows of `length` positions at slots of `step`: neighbours overlap, every row owns positions no other row has"""
    for k, slot in enumerate(order):
        c.row(a, b, idens[k], 1 + step * slot, 1 + step * slot, '%dM' % length)


def rows_cases():
    """several rows per group, the decision only after the last one (match_len* = 3 x all covered positions): last writer wins on the
    overlaps, and rows that come later in the table cover positions in front of earlier ones"""
    out = []
    for k in (2, 3, 6, 49):
        total = 30 * (k - 1) + 45
        c = Case('rows%d' % k, 'rows', clust_identity=1.5, match_identity=0.3, match_len=3. * total, match_len1=3. * total, match_len2=3. * total,
                 match_prop=1e-6, match_prop1=1e-6, match_prop2=1e-6)
        rng = np.random.default_rng(2400 + k)
        idens = [round(0.6 + 0.007 * j, 3) for j in range(k)]
        for tag, order in (('descending', list(range(k))[::-1]), ('ascending', list(range(k))), ('shuffled', rng.permutation(k).tolist()),
                           ('shuffled2', rng.permutation(k).tolist())):
            a, b = c.pair(up3(total) + 3)
            _slots(c, a, b, order, idens if tag != 'shuffled2' else idens[::-1])
            c.probe(a, b, tag, 'value', n_rows=k)
        # gaps inside the rows: the same slots, every second row with an insertion and a deletion of 3 that cancel
        a, b = c.pair(up3(total) + 3)
        for j, slot in enumerate(list(range(k))[::-1]):
            c.row(a, b, idens[j], 1 + 30 * slot, 1 + 30 * slot, '45M' if j % 2 else '12M3I15M3D15M')
        c.probe(a, b, 'gapped', None, n_rows=k)                # inserted positions that no neighbour covers stay uncovered: the gate is then never met
        # decided by its first row although the later rows would change the mean
        a, b = c.pair(up3(total) + 93)
        c.row(a, b, 0.8, 1, 1, '%dM' % (total + 30))
        for j in range(k - 1):
            c.row(a, b, 0.6, 1 + 30 * j, 1 + 30 * j, '45M')
        c.probe(a, b, 'early', 'value', n_rows=k)
        # never decided
        a, b = c.pair(up3(total) + 3)
        _slots(c, a, b, list(range(k - 1))[::-1], idens)
        c.probe(a, b, 'undecided', 'none', n_rows=k - 1)
        out.append(c)
    return out


def gates_cases():
    out = []
    tiny = dict(match_prop=1e-6, match_prop1=1e-6, match_prop2=1e-6)
    # len * 3 against min(match_len*)
    c = Case('gate_len', 'gates', clust_identity=1.5, match_identity=0.3, match_len=120., match_len1=90., match_len2=150., **tiny)
    for n in (30, 29, 31):                                                           # 90 nucleotides open the gate, and need = min(120, 90, 150) is met with it
        a, b = c.pair(300)
        c.row(a, b, 0.7, 1, 1, '%dM' % n)
        c.probe(a, b, 'n%d' % n, None, n=n)
    out.append(c)
    # len * 3 against min(match_prop*) * ql with products that are inexact in binary: 0.4 * 203 = 81.2, 0.28 * 300 = 84.00000000000001 (28 positions
    # make 84: short of it), 0.57 * 300 = 170.99999999999997 (57 positions make 171)
    for prop, ql, at in ((0.4, 203, 28), (0.28, 300, 28), (0.57, 300, 57)):
        c = Case('gate_prop_%s_%d' % (prop, ql), 'gates', clust_identity=1.5, match_identity=0.3, match_len=3., match_len1=3., match_len2=3.,
                 match_prop=prop + 0.1, match_prop1=prop + 0.2, match_prop2=prop)
        for n in (at - 1, at, at + 1):
            for sl in (ql, ql + 60):
                a = c.gene(ql)
                b = c.gene(sl)
                c.row(a, b, 0.7, 1, 1, '%dM' % n)
                c.probe(a, b, 'n%d_sl%d' % (n, sl), None, n=n)
        out.append(c)
    # ave against match_identity * 10000: 0.57 * 10000 = 5699.999999999999 and int() of it is 5699, below the threshold; 0.343 * 10000 = 3430.0000000000005 lies
    # above its integer
    for mi in (0.57, 0.343):
        c = Case('gate_identity_%s' % mi, 'gates', **dict(LOW, match_identity=mi))
        exact = [n for n in (300, 256, 128, 64) if float(np.mean([mi] * n)) == mi][0]
        for n in (1, exact):
            for v in (mi, round(mi + 0.001, 3), round(mi - 0.001, 3)):
                a, b = c.pair(up3(n) + 3)
                c.row(a, b, v, 1, 1, '%dM' % n if n > 1 else '1M1D')
                c.probe(a, b, 'n%d_%s' % (n, v), None, n=n, iden=v)
        out.append(c)
    # need: the binding (match_len, match_prop) pair asks for 90 nucleotides, through its length (the other two ask for 0.9 x 300, and open the gate at
    # 30 nucleotides) or through its proportion (0.25 x 360; the other two ask for 300, and open the gate at 0.05 x 360 = 18)
    for which in range(3):
        for via in ('len', 'prop'):
            L = 300 if via == 'len' else 360
            p = dict(clust_identity=1.5, match_identity=0.3)
            for k, sfx in enumerate(('', '1', '2')):
                if k == which:
                    p['match_len' + sfx], p['match_prop' + sfx] = (90., 0.05) if via == 'len' else (3., 0.25)
                else:
                    p['match_len' + sfx], p['match_prop' + sfx] = (30., 0.9) if via == 'len' else (300., 0.05)
            c = Case('need_%d_%s' % (which, via), 'gates', **p)
            for n in (30, 29, 10, 9) if via == 'len' else (30, 29, 6, 5):
                a, b = c.pair(L)
                c.row(a, b, 0.7, 1, 1, '%dM' % n)
                c.probe(a, b, 'n%d' % n, None, n=n)
            out.append(c)
    # 20 * min(ql, sl) <= max(ql, sl): ql from column 12, sl from column 13, in both orders
    c = Case('gate_20x', 'gates', **LOW)
    for ql, sl in ((2000, 100), (2000, 101), (100, 2000), (101, 2000), (1980, 99), (99, 1980), (1981, 99), (99, 1981), (1979, 99), (99, 1979)):
        a = c.gene(ql)
        b = c.gene(sl)
        c.row(a, b, 0.7, 1, 1, '60M')
        c.probe(a, b, 'ql%d_sl%d' % (ql, sl), None, sentinel=False)
    out.append(c)
    return out


FRAME_ROWS = [(qs, ss, '30M') for qs in (4, 5, 6) for ss in (4, 5, 6)] + [
    # I and D runs of 1, 2 and 3 that move the two frames apart and back together in mid-row
    (4, 4, '12M1I12M2I12M'), (4, 4, '12M1D12M2D12M'), (4, 4, '12M3I12M'), (4, 4, '12M3D12M'), (4, 4, '12M1I12M1D12M'), (4, 4, '12M2D12M2I12M'),
    (5, 5, '13M2I11M1I12M'), (6, 6, '11M1D13M1I12M'), (4, 5, '12M1I12M'), (4, 6, '12M2I12M3D9M'), (5, 4, '12M1D12M3I6M'),
    # M runs of 1 and 2, shorter than the offset to the next codon start
    (5, 5, '1M1I1D24M'), (5, 5, '2M1I1D24M'), (6, 6, '1M2I2D21M'), (5, 5, '1M'), (5, 5, '2M'), (6, 6, '1M'), (5, 5, '2M3I1M3D2M30M'), (4, 4, '1M'), (4, 4, '1M3D'), (5, 5, '1M3D'), (6, 6, '2M3D'), (4, 4, '2M1I2M1D20M'),
    # rows that begin with an I run, and with a D run
    (4, 4, '3I30M'), (4, 4, '1I30M'), (4, 4, '2I30M'), (4, 4, '3D30M'), (4, 4, '1D30M'), (4, 4, '2D30M'), (5, 6, '1I30M'), (6, 5, '1D30M'),
]


def frames_cases():
    """the row under test (identity 0.9) lies inside positions 1 .. 99 and can never open the gate (match_len* = 300 = 3 x 100 positions); a closing row
    (identity 0.6) of exactly 100 positions behind it does, so the mean tells how many positions the row under test covered"""
    out = []
    for cds in ('', 'f'):
        c = Case('frames_%s' % (cds or 'none'), 'frames', clust_identity=1.5, match_identity=0.3, match_len=300., match_len1=300., match_len2=300.,
                 match_prop=1e-6, match_prop1=1e-6, match_prop2=1e-6, incompleteCDS=cds)
        for qs, ss, cigar in FRAME_ROWS:
            a, b = c.pair(210)
            c.row(a, b, 0.9, qs, ss, cigar)
            c.row(a, b, 0.6, 100, 100, '100M')
            c.probe(a, b, '%d_%d_%s' % (qs, ss, cigar), 'value', qs=qs, ss=ss, cigar=cigar)
        out.append(c)
    return out


def ordered_cases():
    """scan and resolve (PEPPAN.py:236-276) with the usual parameters; genes of 240 nucleotides, for which a full row is judged a value (720 >= 192)
    and a row of 45 positions a 0 (135 opens the gate at 100 and 96, and misses the need of 192)"""
    c = Case('ordered', 'ordered')
    L = 240
    note = {}

    def many(a, b, n, iden=0.7, start=0):
        for k in range(start, start + n):
            c.row(a, b, round(iden + 0.001 * (k % 50), 3), 1 + 3 * (k % 40), 1 + 3 * (k % 40), '90M')
    # exactly 49 forward rows: judged.  Exactly 50: the reference gene is a repeat, and its later rows are ignored on either side
    a, b = c.pair(L); many(a, b, 49); note['judged49'] = [a, b]
    a, b = c.pair(L); many(a, b, 50); x = c.gene(L); c.full(b, x, 0.71); c.full(x, b, 0.72); c.full(a, x, 0.73); note['killed50'] = [a, b, x]
    # 50 self rows kill the gene; the row that settles them names the gene, has passed the presence tests already and is still judged
    a = c.gene(L, self_row=False); many(a, a, 50); x = c.gene(L); c.full(a, x, 0.74); y = c.gene(L); c.full(a, y, 0.75); c.full(y, a, 0.76)
    note['self50'] = [a, x, y]
    # 50 rows (a, b) settled by the row (b, a): b dies, and (b, a) is judged all the same
    a, b = c.pair(L); many(a, b, 50); c.full(b, a, 0.77); x = c.gene(L); c.full(b, x, 0.78); note['settled_by_victim'] = [a, b, x]
    # a is absorbed by a later row while the pending group (a, b) names it: the group is still judged; a's and b2's later rows are ignored
    a = c.gene(L); b = c.gene(L); b2 = c.gene(L); x = c.gene(L)
    c.full(a, b, 0.79); c.full(a, b2, 0.951); c.full(a, x, 0.81); c.full(x, a, 0.82); c.full(x, b, 0.83)
    note['absorbed_while_pending'] = [a, b, b2, x]
    # the reference is absorbed (longer query, priorities equal): rows that name it later are ignored
    a = c.gene(L + 3); b = c.gene(L); x = c.gene(L)
    c.row(a, b, 0.952, 1, 1, '%dM' % L); c.full(b, x, 0.84); c.full(x, b, 0.85); c.full(a, x, 0.86); note['absorbed_ref'] = [a, b, x]
    # a gene that is only ever a reference is dropped; a gene whose only rows are skipped rows stays
    a = c.gene(L); r_only = c.gene(L, self_row=False); c.full(a, r_only, 0.61); note['ref_only'] = [a, r_only]
    dead_q = note['absorbed_while_pending'][0]
    s = c.gene(L, self_row=False); c.full(s, dead_q, 0.62); c.full(s, note['killed50'][1], 0.63); note['skipped_only'] = [s]
    # a conflict written before the pair's forward group blocks get_similar; one written after a value overwrites it
    a, b = c.pair(L); c.row(a, b, 0.953, 1, L, '%dM' % L, reverse=True); c.full(a, b, 0.64); c.full(b, a, 0.65); note['conflict_first'] = [a, b]
    a, b = c.pair(L); x = c.gene(L); c.full(a, b, 0.66); c.full(a, x, 0.661); c.row(b, a, 0.954, 1, L, '%dM' % L, reverse=True); note['conflict_after'] = [a, b, x]
    # (a, b) returns 0 and blocks (b, a)
    a, b = c.pair(L); c.row(a, b, 0.67, 1, 1, '45M'); c.full(b, a, 0.68); note['zero_blocks'] = [a, b]
    # reverse-strand rows and rows with ss == se never enter the group: 49 forward rows stay 49 ...
    a, b = c.pair(L); many(a, b, 20); c.row(a, b, 0.7, 1, L, '%dM' % L, reverse=True); c.row(a, b, 0.7, 10, 10, '1M'); many(a, b, 29, start=20)
    c.row(a, b, 0.7, 1, L, '90M', reverse=True); note['not_saved'] = [a, b]
    # ... and a reverse-strand row between the forward rows does not split them: 25 + 25 are 50
    a, b = c.pair(L); many(a, b, 25); c.row(a, b, 0.7, 1, L, '90M', reverse=True); many(a, b, 25, start=25); note['not_split'] = [a, b]
    # the last group of the table is settled after the loop
    a = c.gene(L); z = c.gene(L, self_row=False); c.full(z, a, 0.69); note['last_group'] = [z, a]
    c.notes = note
    out = [c]
    # the same, with the last group one of 50 rows; ids whose string order is not their numeric order
    c = Case('ordered_last50', 'ordered')
    a = c.gene(L); x = c.gene(L, self_row=False); many(x, a, 50)
    c.notes = dict(last50=[x, a])
    out.append(c)
    c = Case('string_order', 'ordered', first_id=9)
    g9, g10 = c.gene(L), c.gene(L)
    g100 = c.gene(L, gid=100)
    c.full(g10, g9, 0.7); c.full(g9, g10, 0.8); c.full(g100, g9, 0.71); c.full(g9, g100, 0.81); c.full(g10, g100, 0.72); c.full(g100, g10, 0.82)
    c.notes = dict(ids=[9, 10, 100])
    out.append(c)
    return out


def rowlocal_cases():
    """classify (PEPPAN.py:241-260): every threshold at equality and one unit short, the branch structure, the priorities"""
    out = []
    for ci, cover in ((0.9, 0.81), (0.9, 0.8), (0.5, 0.81)):
        c = Case('rowlocal_%s_%s' % (ci, cover), 'rowlocal', clust_identity=ci, clust_match_prop=cover, match_identity=0.3)
        k = [0]

        def near():                                            # identities at and above clust_identity, no two alike
            k[0] += 1
            return round(ci + 0.0007 * k[0], 4)
        root = math.sqrt(cover)
        # iden exactly clust_identity, and just below
        for v in (ci, round(ci - 0.0001, 4), 0.9999 if ci > 0.5 else 0.57):
            a, b = c.pair(300); c.full(a, b, v); c.label(a, b, 'iden_%s' % v)
        for L in (300, 290):
            # conflict through qa (the reference twice as long) and through sa (the query twice as long), on the reverse strand
            for d in (-1, 0, 1):
                n = int(round(cover * L)) + d
                a = c.gene(L); b = c.gene(2 * L); c.row(a, b, near(), 1, n, '%dM' % n, reverse=True); c.label(a, b, 'qa_%d_%d' % (L, d))
                a = c.gene(2 * L); b = c.gene(L); c.row(a, b, near(), 1, n, '%dM' % n, reverse=True); c.label(a, b, 'sa_%d_%d' % (L, d))
            # absorption of the query (ql <= sl, qa against sqrt * sl) and of the reference (ql > sl, sa against sqrt * ql); tails in frame
            for d in (-1, 0, 1):
                n = int(round(root * L)) + d
                a, b = c.pair(L); c.row(a, b, near(), 1, 1, '%dM' % n); c.label(a, b, 'absq_%d_%d' % (L, d))
                a = c.gene(L); b = c.gene(L - 3); c.row(a, b, near(), 1, 1, '%dM' % n); c.label(a, b, 'absr_%d_%d' % (L, d))
        # ql == sl takes the first branch only: when it fails on the priority, or on qa with sa long enough, the row falls through
        a, b = c.pair(300, pa=0, pb=1); c.full(a, b, near()); c.label(a, b, 'equal_prio_fails')
        n = int(root * 300) + 1
        a, b = c.pair(300); c.row(a, b, near(), 1, 1, '%dM3D%dM' % (n - 103, 100)); c.label(a, b, 'equal_qa_fails')
        # priorities: ties, and either side of a tie, in both branches
        for pa, pb in ((0, 0), (1, 0), (0, 1), (2, 2)):
            a, b = c.pair(297, 300, pa, pb); c.row(a, b, near(), 1, 1, '297M'); c.label(a, b, 'prio_q_%d_%d' % (pa, pb))
            a, b = c.pair(300, 297, pa, pb); c.row(a, b, near(), 1, 1, '297M'); c.label(a, b, 'prio_r_%d_%d' % (pa, pb))
        # head frame shifted, tail frame equal: a conflict.  Head and tail shifted: neither
        a = c.gene(301); b = c.gene(300); c.row(a, b, near(), 2, 1, '270M'); c.label(a, b, 'head_shift')
        a, b = c.pair(300); c.row(a, b, near(), 2, 1, '270M'); c.label(a, b, 'head_tail_shift')
        a = c.gene(301); b = c.gene(300); c.row(a, b, near(), 1, 1, '270M'); c.label(a, b, 'tail_shift_only')
        out.append(c)
    return out


def all_cases():
    return tree_cases() + rows_cases() + gates_cases() + frames_cases() + ordered_cases() + rowlocal_cases()


def random_case(rng, k):
    """30 to 60 genes and the row makers of the families above on random pairs of them, genes shared between pairs"""
    c = Case('random%d' % k, 'random', incompleteCDS=('', 'f')[k % 2], match_identity=(0.5, 0.6)[k // 2 % 2])
    ids = [c.gene(int(rng.choice([150, 240, 240, 243, 300, 303, 450, 600])), prio=int(rng.integers(0, 3))) for _ in range(int(rng.integers(30, 61)))]
    near = [0]
    for _ in range(int(rng.integers(60, 120))):
        a, b = (int(x) for x in rng.choice(ids, 2, replace=False))
        m = min(c.genes[a], c.genes[b])
        what = rng.choice(['full', 'full', 'short', 'group', 'group', 'near', 'near', 'reverse', 'shift', 'many'], p=[.2, .1, .1, .15, .1, .1, .1, .08, .05, .02])
        iden = round(float(rng.uniform(0.5, 0.89)), 3)
        if what == 'full':
            c.full(a, b, iden)
        elif what == 'short':
            c.row(a, b, iden, 1 + int(rng.integers(0, 6)), 1 + int(rng.integers(0, 6)), '%dM' % int(rng.integers(20, 80)))
        elif what == 'group':
            for j in range(int(rng.integers(2, 7))):
                s = 1 + int(rng.integers(0, m - 100))
                c.row(a, b, round(float(rng.uniform(0.5, 0.89)), 3), s, s + int(rng.choice([0, 0, 0, 3, 1])),
                      str(rng.choice(['90M', '30M3I30M3D24M', '40M1I40M', '20M2D60M1D10M', '96M'])))
        elif what == 'near':
            near[0] += 1
            c.row(a, b, round(0.9 + 0.0001 * near[0], 4), 1, 1, '%dM' % (m - 3 * int(rng.integers(0, 12))))
        elif what == 'reverse':
            near[0] += 1
            n = m - int(rng.integers(0, 80))
            c.row(a, b, round(0.9 + 0.0001 * near[0], 4), 1, n, '%dM' % n, reverse=True)
        elif what == 'shift':
            near[0] += 1
            c.row(a, b, round(0.9 + 0.0001 * near[0], 4), 2, 1, '%dM' % (m - 3))
        else:
            for j in range(int(rng.integers(48, 53))):
                c.row(a, b, iden, 1 + 3 * (j % 10), 1 + 3 * (j % 10), '90M')
    return c


# ------------------------------------------------------------------------------------------------------------------ fixture, decoder
def load_g24():
    with gzip.open(os.path.join(GOLDEN, FIXTURE), 'rt') as f:
        return json.load(f)


def object_table(rows):
    tab = np.empty([len(rows), 16], dtype=object)
    for i, r in enumerate(rows):
        for j, v in enumerate(r):
            tab[i, j] = v
    return tab


def priorities_of(case):
    return {int(k): v for k, v in case['priorities'].items()}


def decode(case):
    """per probed pair of a recorded case: 'none', 'zero' or the value get_similar returned for it (see the module's docstring)"""
    got = {(a, b): v for a, b, v in case['pairs']}
    out = []
    for p in case['probes']:
        v = got.get((p['a'], p['b']))
        if p['kind'] == 'sentinel':
            out.append('zero' if v is None else 'none' if v == SENTINEL_VALUE else v)
        else:
            out.append('none' if v is None else v)
    return out


def running_sum_value(n, v):
    """what a left-to-right sum would make of n positions of identity v"""
    s = 0.
    for _ in range(n):
        s += v
    return int(s / n * 10000)


def unbuffered_value(n, v):
    """what ONE pairwise summation over all n positions of identity v would make (numpy sums buffers of 8192 elements pairwise and adds
    the buffers' sums up from left to right: beyond 8192 positions that is another sum)"""
    def pairwise(m):
        if m < 8:
            return running(m)
        if m <= 128:
            r = [running(m // 8)] * 8
            s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
            for _ in range(m % 8):
                s += v
            return s
        left = m // 2 - (m // 2) % 8
        return pairwise(left) + pairwise(m - left)

    def running(m):
        s = 0.
        for _ in range(m):
            s += v
        return s
    return int(pairwise(n) / n * 10000)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def _row_local(q, r, row, rank, near_identity, cover, root):
    iden = float(row[2])
    qs, qe, ss, se, ql, sl = (float(row[k]) for k in (6, 7, 8, 9, 12, 13))
    action = 'ordinary'
    if q != r and iden >= near_identity:
        head, tail = qs % 3 == ss % 3, (ql - qe) % 3 == (sl - se) % 3
        if ss > se or (tail and not head):
            if qe - qs + 1 >= cover * ql or abs(se - ss) + 1 >= cover * sl:
                action = 'conflict'
        elif ss < se and head and tail:
            if ql <= sl:
                if qe - qs + 1 >= root * sl and rank[q][0] >= rank[r][0]:
                    action = 'absorb_query'
            elif abs(se - ss) + 1 >= root * ql and rank[q][0] <= rank[r][0]:
                action = 'absorb_ref'
    return action, ss < se, int(iden * 10000.)


def _judge(group, params):
    """one group of forward rows of a pair -> None | 0 | int(mean * 10000)"""
    ql, sl = int(group[0][12]), int(group[0][13])
    if 20 * min(ql, sl) <= max(ql, sl):
        return None
    lens = [params['match_len'], params['match_len1'], params['match_len2']]
    props = [params['match_prop'], params['match_prop1'], params['match_prop2']]
    any_frame = 'f' in params['incompleteCDS']
    cover = {}
    for row in group:
        qpos, rpos, iden = int(row[6]), int(row[8]), row[2]
        for n, t in runs_of(row[14]):
            if t == 'I':
                qpos += n
            elif t != 'M':
                rpos += n
            else:
                if any_frame or qpos % 3 == rpos % 3:
                    first = qpos
                    while first % 3 != 1:                  # the next codon start at or behind qpos
                        first += 1
                    for p in range(first, qpos + n):
                        cover[p] = iden
                qpos += n
                rpos += n
                nt = 3 * len(cover)
                if nt >= min(lens) and nt >= min(props) * ql:
                    ave = int(np.mean(list(cover.values())) * 10000)
                    if ave >= params['match_identity'] * 10000:
                        need = min(max(l, p * min(ql, sl)) for l, p in zip(lens, props))
                        return ave if nt >= need else 0
    return None


def restate_pass(table, priorities, params, trace=None):
    """get_similar_pairs over a table (rows as lists, in table order) -> (pairs [[a, b, value]] in dictionary order without the zeros, the set of
    names that stay in the exemplar file, the absorbed edges [kept, dropped, int(identity * 10000)] in table order).  trace (a dict): 'rows' gets
    (action, forward, int(identity * 10000), fate) per row, 'judged' (query, reference, rows, outcome) per group handed to get_similar"""
    root = math.sqrt(params['clust_match_prop'])
    dead, asked, found, edges, pending = set(), set(), {}, [], []
    rows_t, judged_t = [], []

    def settle():
        if not pending:
            return
        q, r = int(pending[0][0]), int(pending[0][1])
        if len(pending) >= 50:
            dead.add(r)
            judged_t.append((q, r, len(pending), 'repeat'))
        elif q != r:
            key = (min(q, r), max(q, r))
            if key in found:
                judged_t.append((q, r, len(pending), 'blocked'))
            else:
                v = _judge(pending, params)
                if v is not None:
                    found[key] = v
                judged_t.append((q, r, len(pending), 'none' if v is None else 'zero' if v == 0 else v))
        del pending[:]

    for row in table:
        q, r = int(row[0]), int(row[1])
        action, forward, iden4 = _row_local(q, r, row, priorities, params['clust_identity'], params['clust_match_prop'], root)
        if q not in dead:
            asked.add(q)
        if q in dead or r in dead:
            fate = 'dead'
        elif action == 'conflict':
            found[(min(q, r), max(q, r))] = -2
            fate = action
        elif action == 'absorb_query':
            edges.append([r, q, iden4])
            dead.add(q)
            fate = action
        elif action == 'absorb_ref':
            edges.append([q, r, iden4])
            dead.add(r)
            fate = action
        elif not forward:
            fate = 'not_forward'
        else:
            if pending and (int(pending[0][0]), int(pending[0][1])) != (q, r):
                settle()
            pending.append(row)
            fate = 'saved'
        rows_t.append((action, forward, iden4, fate))
    settle()
    if trace is not None:
        trace.update(rows=rows_t, judged=judged_t)
    return [[a, b, v] for (a, b), v in found.items() if v != 0], asked - dead, edges


def expected_files(case_or_record, kept, edges):
    """the exemplar text and clust.npy rows the pass leaves behind, from the restatement's kept names and absorbed edges (identities of the
    edges are distinct by construction, so the descending order is defined)"""
    text = ''.join('>%s\n%s\n' % (name, seq) for name, seq in re.findall(r'>(\S+)\n(\S*)\n', case_or_record['exemplar_in']) if int(name) in kept)
    clu = [list(x) for x in case_or_record['clust_npy_in']] + [list(e) for e in edges]
    return text, sorted(clu, key=lambda x: -x[2]) if edges else [list(x) for x in case_or_record['clust_npy_in']]


def run_product(case, where, monkeypatch, ctx):
    """PL.get_similar_pairs over a case's canned table -> (pairs, exemplar text, clust.npy rows)"""
    import copy
    from peppan_amd import pipeline as PL
    os.makedirs(str(where), exist_ok=True)
    cl = os.path.join(str(where), 'p.clust.exemplar')
    with open(cl, 'w') as f:
        f.write(case['exemplar_in'])
    npy = os.path.join(str(where), 'p.clust.npy')
    np.save(npy, np.array(case['clust_npy_in'], dtype=int))
    tab = object_table(case['table'])
    monkeypatch.setattr(PL, 'uberBlast', lambda argv, pool=None, as_table=False: copy.deepcopy(tab))
    res = PL.get_similar_pairs(cl, priorities_of(case), dict(case['params'], clust=cl), ctx=ctx)
    with open(cl) as f:
        return res.tolist(), f.read(), np.load(npy, allow_pickle=True).tolist()


def tally_random(case, tally):
    """what happened on a table, by the restatement's trace: get_similar's outcomes, absorptions in either direction, conflicts, repeat kills"""
    trace = {}
    restate_pass(case['table'], priorities_of(case), case['params'], trace)
    for q, r, n, o in trace['judged']:
        if o != 'blocked':
            tally[o if o in ('none', 'zero', 'repeat') else 'value'] += 1
    for action, forward, iden4, fate in trace['rows']:
        if fate in ('absorb_query', 'absorb_ref', 'conflict'):
            tally[fate] += 1


# ------------------------------------------------------------------------------------------------------------------ K14's inputs
def k14_inputs(cases, order=None):
    """the forward rows of every probed pair (a, b) of the cases (all of one params set), one group per probe in table order, as pep_pair_support
    takes them -> (rows, cigar arena, group offsets, query lengths, reference lengths, the decoded outcomes as K14 reports them).  order: a
    permutation of the groups"""
    from peppan_amd import _native as N
    groups, want = [], []
    for case in cases:
        by_pair = {}
        for row in case['table']:
            if row[8] < row[9]:
                by_pair.setdefault((row[0], row[1]), []).append(row)
        for p, d in zip(case['probes'], decode(case)):
            groups.append(by_pair.get((str(p['a']), str(p['b'])), []))
            want.append(N.SUPPORT_NONE if d == 'none' else 0 if d == 'zero' else d)
    if order is not None:
        groups, want = [groups[k] for k in order], [want[k] for k in order]
    rows, cigar, off, gq, gr = [], [], [0], [], []
    for g in groups:
        for row in g:
            runs = [(n << 2) | 'MID'.index(t) for n, t in runs_of(row[14])]
            rows.append((row[6], row[8], len(runs), 0, len(cigar), row[2]))
            cigar += runs
        off.append(len(rows))
        gq.append(g[0][12] if g else 30)
        gr.append(g[0][13] if g else 30)
    return (np.array(rows, dtype=N.SUPPORT_ROW_DTYPE), np.array(cigar, dtype=np.uint32), np.array(off, dtype=np.uint64), np.array(gq, dtype=np.uint32),
            np.array(gr, dtype=np.uint32), np.array(want, dtype=np.int32))


def params_key(params):
    return json.dumps({k: params[k] for k in sorted(params) if k.startswith('match_') or k == 'incompleteCDS'}, sort_keys=True)


# ------------------------------------------------------------------------------------------------------------------ what the fixture is pinned by
def fixture_figures(g):
    """the counts that make the fixture worth having, from the recorded data alone"""
    f = dict(none=0, zero=0, value=0, tree_pairs=0, tree_running_sum_differs=0, tree_unbuffered_differs=0, tree_longest=0, group_sizes=set(), absorbed=0, conflicts=0, cases=len(g['cases']))
    for case in g['cases']:
        for p, d in zip(case['probes'], decode(case)):
            f[d if d in ('none', 'zero') else 'value'] += 1
            if case['family'] == 'tree':
                f['tree_pairs'] += 1
                f['tree_longest'] = max(f['tree_longest'], p['n'])
                f['tree_running_sum_differs'] += running_sum_value(p['n'], p['iden']) != d
                f['tree_unbuffered_differs'] += p['n'] > 8192 and unbuffered_value(p['n'], p['iden']) != d
        size = {}
        for row in case['table']:
            if row[8] < row[9] and row[0] != row[1]:
                size[row[0], row[1]] = size.get((row[0], row[1]), 0) + 1
        f['group_sizes'] |= set(size.values())
        f['absorbed'] += len(case['clust_npy_out']) - len(case['clust_npy_in'])
        f['conflicts'] += sum(v == -2 for a, b, v in case['pairs'])
    return f


def assert_figures(f):
    """the bounds are counts of what the builders above lay out, not of what came back: the short side of every gate, the undecided groups and the
    off-frame rows make 30 and more None outcomes, the need edges 12 zeros (two per binding pair and route), the tree alone 125 values; the
    row-local and ordered cases hold 30 and more absorbing rows and 15 and more conflicts.  At least 20 tree pairs must tell np.mean's
    summation from a running sum, at least 4 its buffers of 8192 elements from one pairwise sum over everything"""
    assert f['none'] >= 30 and f['zero'] >= 12 and f['value'] >= 250, f
    assert f['tree_pairs'] >= 3 * len(TREE_N) + 1 and f['tree_running_sum_differs'] >= 20 and f['tree_unbuffered_differs'] >= 4 and f['tree_longest'] > 32768, f
    assert {2, 3, 6, 49, 50} <= f['group_sizes'], f
    assert f['absorbed'] >= 30 and f['conflicts'] >= 15, f
