"""The allele pass of write_output (PEPPAN.py:1391-1472) restated in plain Python over lists, strings and dictionaries, for the tests of K24.  It shares nothing
with csrc/outalleles.hip or peppan_amd/outalleles.py: alleles are dictionary keys, windows are cut out as strings and sliced with Python's own slices, batches
are walked one after another with the write-back between them.  It is held to every case of tests/golden/g27_outalleles.json.gz, which was recorded from the
reference itself, and the GPU tests are held to it.  Also here: the builders of that fixture's cases - the two-batch case is regenerated from its recorded
seed, the fixture holds only what the reference made of it."""
import gzip
import hashlib
import json
import os

import numpy as np

import genestruct_helpers as GS

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'g27_outalleles.json.gz')
BATCH = 10000
PAIR = {'A': 'T', 'T': 'A', 'G': 'C', 'C': 'G', 'N': 'N'}


def load():
    with gzip.open(FIXTURE, 'rt') as f:
        return json.load(f)


def dictionaries_of(case):
    """(genomes, encodes, clust_ref) of a stored case: JSON turned their integer keys into strings"""
    return {int(k): tuple(v) for k, v in case['genomes'].items()}, case['encodes'], {int(k): v for k, v in case['clust_ref'].items()}


def reverse_complement(text):
    out = []
    for ch in reversed(text.upper()):
        out.append(PAIR.get(ch, 'N'))
    return ''.join(out)


def toward_zero_3(x):
    """3 * int(x / 3) for integers, without the float"""
    q = abs(x) // 3 * 3
    return q if x >= 0 else -q


def structure_on_cpu(item):
    """determineGeneStructure as tests/genestruct_helpers.py restates it -> (pid, cds, start, stop)"""
    return GS.restate(item)[0]


def restate(prediction, genomes, encodes, clust_ref, pseudogene, gtable, structure=structure_on_cpu, batch=BATCH):
    """prediction: the table at :1390 as a list of 17-entry lists; mutated as the reference mutates it (columns 9, 10, 13, 15).
    -> (alleles: gene -> {sequence: id} in insertion order; rows: per row None when skipped, else dict(kind, s2, e2, lp, allele, id, sent))"""
    alleles = {}
    for row in prediction:
        name = row[0]
        if row[15] == 'misc_feature' or name in alleles:
            continue
        alleles[name] = {}
        if name in encodes and encodes[name] in clust_ref:
            alleles[name][clust_ref[encodes[name]]] = '1'
    seen = [None] * len(prediction)
    for lo in range(0, len(prediction), batch):
        hi = min(lo + batch, len(prediction))
        items = []
        for i in range(lo, hi):
            row = prediction[i]
            name, part, second, contig, q_lo, q_hi, s, e, strand, ref_len, contig_len = row[0], row[1], row[4], row[5], row[7], row[8], row[9], row[10], row[11], row[12], row[13]
            if row[15] == 'misc_feature' or name == '':
                row[13] = '%s:t0:%s-%s:%s-%s' % (name, q_lo, q_hi, s, e)
                continue
            vary = int(ref_len * (1 - pseudogene) + 0.01)
            text = genomes[encodes[contig]][1]
            known = alleles[name]
            info = dict(sent=False)
            if part > 1 or e - s + 1 < ref_len - vary:
                info.update(kind='fragment', s2=s, e2=e, lp=0)
                allele = text[s - 1:e]
                if strand != '+':
                    allele = reverse_complement(allele)
                fresh = 't%d' % (len(known) + 1)
                row[15] = 'pseudogene=fragment:{0:.2f}%'.format((e - s + 1) * 100 / ref_len)
            else:
                other = None
                if strand == '+':
                    for j in range(i + 1, min(i + 5, len(prediction))):
                        if prediction[j][5] != contig:
                            break
                        if prediction[j][15] != 'misc_feature':
                            other = prediction[j]
                    right = toward_zero_3(other[10] + 300 - e) if other is not None else 600 + ref_len - q_hi
                    e2 = e + min(toward_zero_3(contig_len - e), right)
                    s2 = s - min(toward_zero_3(s - 1), 60 + q_lo - 1)
                    window = text[s2 - 1:e2]
                    lp, rp = s - s2, e2 - e
                else:
                    for j in range(i - 1, max(i - 5, 0) - 1, -1):
                        if prediction[j][5] != contig:
                            break
                        if prediction[j][15] != 'misc_feature':
                            other = prediction[j]
                    left = toward_zero_3(s - other[9] + 300) if other is not None else 600 + ref_len - q_hi
                    s2 = s - min(toward_zero_3(s - 1), left)
                    e2 = e + min(toward_zero_3(contig_len - e), 60 + q_lo - 1)
                    window = reverse_complement(text[s2 - 1:e2])
                    lp, rp = e2 - e, s - s2
                allele = window[lp:len(window) - rp]
                clean = second == '' and q_lo == 1 and q_hi == ref_len
                fresh = ('%d' if clean else 't%d') % (len(known) + 1)
                info.update(kind='intact', s2=s2, e2=e2, lp=lp)
                base = name.rsplit('/', 2)[0]
                if encodes[base] in clust_ref and len(allele) < pseudogene * len(clust_ref[encodes[base]]):
                    info['kind'] = 'structural_variation'
                    row[15] = 'pseudogene=structural_variation:{0:.2f}%'.format(100. * len(allele) / len(clust_ref[encodes[base]]))
                else:
                    info['sent'] = True
                    items.append([i, row, window, s, e, s2, e2, lp, vary, gtable])
            if allele not in known:
                known[allele] = fresh
            info.update(allele=allele, id=known[allele])
            seen[i] = info
            if second:
                row[13] = '%s:(%s)%s:%s-%s:%s-%s' % (name, second.rsplit(':', 1)[-1], known[allele], q_lo, q_hi, s, e)
            else:
                row[13] = '%s:%s:%s-%s:%s-%s' % (name, known[allele], q_lo, q_hi, s, e)
        for item in items:
            pid, cds, start, stop = structure(item)
            prediction[pid][9], prediction[pid][10] = start, stop
            if cds != 'CDS':
                prediction[pid][15] = 'pseudogene=' + cds
    return alleles, seen


def expected_ids(prediction_before, seen, clust_ref, encodes):
    """what K24's arrays must be for a restated table: per row (class 0 .. 3, s2, e2, lp, allele length, first row of its class or -1 / -2, rank, t flag)"""
    kinds = {'fragment': 1, 'intact': 2, 'structural_variation': 3}
    first_of = {}
    out = []
    for i, (row, info) in enumerate(zip(prediction_before, seen)):
        if info is None:
            out.append((0, 0, 0, 0, 0, -2, 0, 0))
            continue
        name = row[0]
        if name not in first_of:
            first_of[name] = {}
            if name in encodes and encodes[name] in clust_ref:
                first_of[name][clust_ref[encodes[name]]] = -1
        first = first_of[name].setdefault(info['allele'], i)
        tid = info['id']
        out.append((kinds[info['kind']], info['s2'], info['e2'], info['lp'], len(info['allele']), first, int(tid.lstrip('t')), 1 if tid.startswith('t') else 0))
    return out


def allele_digest(alleles):
    """one SHA-1 over every gene, sequence and id in insertion order: the two-batch case's sequences are regenerated, not stored"""
    h = hashlib.sha1()
    for g, a in alleles.items():
        h.update(('>' + g + '\n').encode())
        for s, i in a.items():
            h.update((s + '\t' + i + '\n').encode())
    return h.hexdigest()


# ---- building cases.  A case is what write_output is given: the rows of a Prediction file, genomes, encodes, clust_ref, old predictions.

SAFE = [a + b + c for a in 'ACGT' for b in 'ACGT' for c in 'ACGT' if a + b + c not in ('ATG', 'GTG', 'TTG', 'TAA', 'TAG', 'TGA')]


def safe_codons(rng, n):
    """n codons that are neither a start nor a stop"""
    return ''.join(SAFE[k] for k in rng.integers(0, len(SAFE), n))


def random_dna(rng, n, alphabet='ACGT'):
    return ''.join(alphabet[k] for k in rng.integers(0, len(alphabet), n))


class Case(object):
    """collects contigs, genes and predictions; `inputs()` gives write_output's arguments, the Prediction file as rows of 15 values"""

    def __init__(self, pseudogene=0.8, gtable=11):
        self.pseudogene, self.gtable = pseudogene, gtable
        self.contigs, self.encodes, self.clust_ref, self.rows, self.old = {}, {}, {}, [], {}
        self.next_id, self.next_tag = 1, 1

    def name(self, text):
        if text not in self.encodes:
            self.encodes[text] = self.next_id
            self.next_id += 1
        return self.encodes[text]

    def contig(self, name, text):
        self.name(name)
        self.contigs[name] = text

    def gene(self, name, representative=None, encoded=True):
        if encoded:
            gid = self.name(name)
            if representative is not None:
                self.clust_ref[gid] = representative

    def predict(self, gene, contig, s, e, strand, q_lo=1, q_hi=None, ref_len=None, second=None, tag=None, cigar=None):
        """one line of the Prediction file: the region [s, e] (1-based, inclusive) of `contig`; second None: the gene itself (emptied at :1388)"""
        ref_len = e - s + 1 if ref_len is None else ref_len
        q_hi = ref_len if q_hi is None else q_hi
        if tag is None:
            tag, self.next_tag = 'T%06d' % self.next_tag, self.next_tag + 1
        a, b = (s, e) if strand == '+' else (e, s)
        self.rows.append([gene, 0, tag, contig, gene if second is None else second, contig, 99.5, q_lo, q_hi, a, b, strand, ref_len, len(self.contigs[contig]),
                          cigar or '%dM' % (e - s + 1)])

    def old_gene(self, contig, name, s, e, strand, code):
        """an entry of old_prediction: code 0 a kept CDS, 1 .. 6 a misc_feature with its reason"""
        self.old.setdefault(contig, []).append([name, s, e, strand, code])

    def inputs(self):
        genomes = {self.encodes[c]: ('genome', text) for c, text in self.contigs.items()}
        old = {c: sorted([list(g) for g in genes], key=lambda g: g[1]) for c, genes in self.old.items()}
        return dict(rows=self.rows, genomes=genomes, encodes=dict(self.encodes), clust_ref=dict(self.clust_ref), old_prediction=old, pseudogene=self.pseudogene, gtable=self.gtable)


def orf(rng, codons, first='ATG', last='TAA'):
    return first + safe_codons(rng, codons - 2) + last


def lay_out(case, rng, contig, genes, gap=(70, 90), lead=70, tail=70):
    """a contig made of random stretches with the given texts in between -> the 1-based (s, e) of each"""
    parts, at, spans = [random_dna(rng, lead)], lead, []
    for k, text in enumerate(genes):
        parts.append(text)
        spans.append((at + 1, at + len(text)))
        at += len(text)
        fill = tail if k == len(genes) - 1 else int(rng.integers(gap[0], gap[1] + 1))
        parts.append(random_dna(rng, fill))
        at += fill
    case.contig(contig, ''.join(parts))
    return spans


def case_seeds(rng):
    """seeds, the t prefix, the secondary gene, names with /n, fragments and structural variation at their thresholds"""
    c = Case()
    rep = orf(rng, 34)                                                  # 102 nt
    other = orf(rng, 34)
    var1 = rep[:30] + ('A' if rep[30] != 'A' else 'C') + rep[31:]
    var2 = rep[:45] + ('A' if rep[45] != 'A' else 'C') + rep[46:]
    c.gene('gs', rep)                                                   # seeded
    c.gene('gn')                                                        # encoded, no representative
    c.gene('gx', encoded=False)                                         # not in encodes: fragments only, :1460 would raise for an intact row
    c.gene('sec', other)
    texts = [rep, var1, rep, var1, var2, var2, other, rep[:80], rep[:79], var1[:82], var1[:81], other, other[:60], rep, var2]
    spans = lay_out(c, rng, 'ctgA', texts)
    spans_b = lay_out(c, rng, 'ctgB', [reverse_complement(rep), reverse_complement(var1), reverse_complement(var2), other, rep, reverse_complement(other)])
    p = c.predict
    p('gs', 'ctgA', *spans[0], '+')                                     # the seed itself: id 1
    p('gs', 'ctgA', *spans[1], '+', second='sec:77')                    # a new allele first met by a secondary row: t2 ...
    p('gs', 'ctgA', *spans[2], '+', second='sec:80')                    # ... a t-row of the seed's allele stays 1
    p('gs', 'ctgA', *spans[3], '+')                                     # ... and a clean row of that allele inherits the t
    p('gs', 'ctgA', *spans[4], '+')                                     # clean first: 3
    p('gs', 'ctgA', *spans[5], '+', second='sec:78')                    # ... inherited without t by a secondary row
    p('sec', 'ctgA', *spans[6], '+')
    p('gs', 'ctgA', *spans[7], '+', ref_len=100)                        # 80 = 100 - 20: intact, and 80 < 0.8 * 102 = 81.6: structural variation
    p('gs', 'ctgA', *spans[8], '+', ref_len=100)                        # 79: a fragment by length
    p('gs/2', 'ctgA', *spans[9], '+', ref_len=90, second='gs/3')        # /n names; 82 >= 81.6: no structural variation; second emptied at :1388
    p('gs/2', 'ctgA', *spans[10], '+', ref_len=90, second='gs/3')       # 81 < 81.6: structural variation
    p('gn', 'ctgA', *spans[11], '+')                                    # a gene without a seed
    p('gx', 'ctgA', *spans[12], '+', ref_len=102)                       # a gene not in encodes: a fragment
    p('gs', 'ctgA', *spans[13], '+', tag='SHARED')                      # column 1 becomes 2: fragments by column 1
    p('gs', 'ctgB', *spans_b[0], '-', tag='SHARED')
    p('gs', 'ctgB', *spans_b[1], '-')
    p('gs', 'ctgB', *spans_b[2], '-', second='sec:79')
    p('gn', 'ctgB', *spans_b[3], '+')
    p('gs/2', 'ctgB', *spans_b[4], '+', second='gs/3')
    p('sec', 'ctgB', *spans_b[5], '-')
    p('gs', 'ctgA', *spans[14], '+')
    return c


def case_neighbours(rng):
    """0 .. 4 rows ahead and 0 .. 5 behind, misc_feature rows in between, contig changes, the nested neighbour, windows clipped at both contig ends"""
    c = Case()
    rep = orf(rng, 30)
    c.gene('ga', rep)
    c.gene('gb', orf(rng, 30))
    for k, n_genes in enumerate((1, 2, 3, 7, 12, 9)):
        name = 'nb%02d' % k
        texts = [rep if rng.random() < .5 else reverse_complement(rep) for _ in range(n_genes)]
        spans = lay_out(c, rng, name, texts, gap=(40, 140), lead=(2, 3, 0, 64, 61, 70)[k], tail=(1, 2, 0, 61, 59, 70)[k])
        strands = ['+' if texts[j] == rep else '-' for j in range(n_genes)]
        if k == 4:
            strands = ['+'] * 6 + ['-'] * 6
        if k == 5:
            strands = ['-'] * 5 + ['+'] * 4
        for j, (s, e) in enumerate(spans):
            c.predict('ga' if j % 3 else 'gb', name, s, e, strands[j])
        if k >= 3:                                                      # old annotations between the predictions: misc_feature rows of the table
            for j in range(0, n_genes - 1, 2):
                gap_lo, gap_hi = spans[j][1] + 5, spans[j + 1][0] - 5
                if gap_hi - gap_lo >= 12:
                    c.old_gene(name, 'old:%s_%d' % (name, j), gap_lo, gap_lo + 11, '+', 1 + j % 5)
    # the nested neighbour: a long gene with a short one inside, far from its end
    long_gene = orf(rng, 240)                                           # 720 nt
    c.gene('glong')                                                     # (no representative: no structural-variation test, the short window goes to K19)
    inner = orf(rng, 20)
    c.gene('ginner', inner)
    text = random_dna(rng, 90) + long_gene[:120] + inner + long_gene[180:] + random_dna(rng, 400)
    c.contig('nested', text)
    c.predict('glong', 'nested', 91, 90 + 720, '+')
    c.predict('ginner', 'nested', 91 + 120, 90 + 180, '+')
    return c


def case_bytes(rng):
    """N and R on both strands, lower case, the SHA-1 padding edges"""
    c = Case()
    texts, plan = [], []
    for n in (55, 56, 63, 64, 119, 120):
        base = random_dna(rng, n)
        c.gene('len%d' % n, base)
        for strand in '+-':
            texts.append(base if strand == '+' else reverse_complement(base))
            plan.append(('len%d' % n, strand))
    odd = orf(rng, 30)
    c.gene('godd', odd)
    for strand, base in (('+', odd), ('-', reverse_complement(odd))):   # what the contig holds; on '-' R and N, and both cases, are one allele
        variants = (base, base[:40] + 'N' + base[41:], base[:40] + 'R' + base[41:], base[:20] + base[20:50].lower() + base[50:])
        for text in variants + variants[1:]:
            texts.append(text)
            plan.append(('godd', strand))
    spans = lay_out(c, rng, 'bytes', texts)
    for (gene, strand), (s, e) in zip(plan, spans):
        c.predict(gene, 'bytes', s, e, strand)
    return c


def case_many(rng):
    """one gene with 64 rows, one with 65, one with 300 distinct alleles; identical alleles across contigs and genomes"""
    c = Case()
    plans = []
    for gene, n_rows, n_distinct in (('g64', 64, 5), ('g65', 65, 7), ('g300', 300, 300)):
        rep = orf(rng, 12)                                              # 36 nt
        c.gene(gene, rep)
        variants = [rep]
        while len(variants) < n_distinct:
            k = int(rng.integers(3, 33))
            v = rep[:k] + random_dna(rng, 1) + rep[k + 1:]
            v = v[:int(rng.integers(3, 30))] + random_dna(rng, 2) + v[int(rng.integers(3, 30)) + 2:] if n_distinct > 50 else v
            v = (v + rep)[:36]
            if v not in variants:
                variants.append(v)
        order = list(range(n_distinct)) + [int(x) for x in rng.integers(0, n_distinct, n_rows - n_distinct)]
        rng.shuffle(order)
        plans += [(gene, variants[k], '+' if rng.random() < .5 else '-') for k in order]
    rng.shuffle(plans)
    per = (len(plans) + 3) // 4
    for k in range(4):
        chunk = plans[k * per:(k + 1) * per]
        spans = lay_out(c, rng, 'many%d' % k, [t if st == '+' else reverse_complement(t) for _, t, st in chunk], gap=(61, 75))
        for (gene, _, strand), (s, e) in zip(chunk, spans):
            c.predict(gene, 'many%d' % k, s, e, strand)
    return c


SMALL_CASES = (('seeds', case_seeds, 2701), ('neighbours', case_neighbours, 2702), ('bytes', case_bytes, 2703), ('many', case_many, 2704))


def small_case(name):
    for label, make, seed in SMALL_CASES:
        if label == name:
            return make(np.random.default_rng(seed))
    raise KeyError(name)


TWO_BATCH_ROWS = 10008


def two_batch_case(seed):
    """10 008 predictions over 8 contigs, so that the reference writes determineGeneStructure's results back once inside the table.  Genes are 90 nt between 60 nt
    of codons that are neither start nor stop; a third of the genes begin with CTG and have their ATG two codons upstream, a third two codons downstream, so
    that determineGeneStructure moves their starts.  The rows around index 10 000 are fixed: five moved '+' rows in front of five '-' rows.
    Every row is a fixed point of write_output's front end (setInFrame, merging), so `table_of` gives the table at :1390 without the reference."""
    rng = np.random.default_rng(seed)
    c = Case()
    genes = []
    for g in range(300):
        kind = g % 3                                                    # 0 starts where predicted, 1 two codons upstream, 2 two codons downstream
        body = safe_codons(rng, 27)
        text = ('ATG' + body + 'CAA' if kind == 0 else 'CTG' + body + 'CAA' if kind == 1 else 'CTGCAAATG' + body[:75]) + 'TAA'
        text = text[:87] + 'TAA'
        name = 'tb%03d' % g
        c.gene(name, text if g % 5 else None)
        genes.append((name, text, kind))
    per = TWO_BATCH_ROWS // 8
    planned = []
    for k in range(8):
        parts, at = [], 0
        for j in range(per):
            i = k * per + j
            g = int(rng.integers(0, 300))
            strand = '+' if rng.random() < .5 else '-'
            if 9995 <= i < 10000:
                g, strand = 3 * int(rng.integers(0, 100)) + 1, '+'
            elif 10000 <= i < 10005:
                strand = '-'
            name, text, kind = genes[g]
            if rng.random() < .3:                                       # a variant allele
                p = 3 * int(rng.integers(3, 27))
                text = text[:p] + SAFE[int(rng.integers(0, len(SAFE)))] + text[p + 3:]
            up = safe_codons(rng, 18) + ('ATG' + safe_codons(rng, 1) if kind == 1 else safe_codons(rng, 2))
            down = safe_codons(rng, 20)
            slot = up + text + down if strand == '+' else reverse_complement(up + text + down)
            parts.append(slot)
            s = at + 61
            planned.append((name, 'tbc%d' % k, s, s + 89, strand))
            at += len(slot)
        c.contig('tbc%d' % k, ''.join(parts))
    for name, contig, s, e, strand in planned:
        c.predict(name, contig, s, e, strand)
    return c


def table_of(case):
    """the table at :1390 for a case whose rows are all fixed points of the front end (no old predictions, distinct tags, rows in order of contig and start)"""
    table = []
    for i, r in enumerate(case.rows):
        s, e = (r[9], r[10]) if r[11] == '+' else (r[10], r[9])
        table.append([r[0], 1, i + 1, r[3], '' if r[4].rsplit('/', 2)[0] == r[0].rsplit('/', 2)[0] else r[4], r[5], r[6], r[7], r[8], s, e, r[11], r[12], r[13], [0], 'CDS', ''])
    return table


def as_object_table(rows):
    """a list of rows as the 2-D object array write_output works on (column 14 stays a list)"""
    table = np.empty((len(rows), 17), dtype=object)
    for i, r in enumerate(rows):
        for k in range(17):
            table[i, k] = r[k]
    return table
