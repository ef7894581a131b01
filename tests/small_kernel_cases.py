"""What the K10-K13 edge tests compare against, and the hand-built cases they run (tests/test_small_kernels_host.py, tests/test_gpu_small_kernels.py).
Pure Python / numpy: no GPU, no ctypes, no code shared with the kernels or with oracle/align_oracle.c.

    restate_alleles     iter_map_bsn (PEPPAN.py:814-833) and the packing (PEPPAN.py:851-852) on strings, statement for statement
    restate_components  a dictionary union-find; every node is labelled with the smallest id of its component
    restate_overlaps    oracle.overlaps_sweep, which already is tab2overlaps line by line
    restate_dedup       oracle.dedup, which already is the loop of writeGenes

Every comparison made with these is ==.  The case builders return lists of dicts with a 'name'; the names say what a case is built for, and
tests/test_small_kernels_host.py asserts that each is what its name says."""
import re

import numpy as np

from oracle.oracle import dedup as restate_dedup, overlaps_sweep as restate_overlaps  # noqa: F401  (plain Python, no library is loaded)

LOCUS_DTYPE = np.dtype([('contig', '<u4'), ('q_start', '<u4'), ('rs', '<u4'), ('re', '<u4'), ('cigar_runs', '<u4'), ('group', '<u4'), ('cigar_off', '<u8')])

# ---------------------------------------------------------------------------------------------------------------------------------------
# K12
# ---------------------------------------------------------------------------------------------------------------------------------------
_COMPLEMENT = {'A': 'T', 'T': 'A', 'G': 'C', 'C': 'G', 'N': 'N'}
_BASE_CONV = np.zeros(255, dtype=np.uint8)
_BASE_CONV[(np.array(['A', 'C', 'G', 'T']).view(np.uint32),)] = (1, 2, 3, 4)


def _rc(seq):
    return ''.join([_COMPLEMENT.get(s, 'N') for s in reversed(seq.upper())])


def restate_alleles(contigs, rows, cigar, grp_off, grp_qlen, gtable=11, detail=False):
    """-> (in_frame int64[n], orf int64[n], packed uint8[sum ceil(ql / 3)]) as Context.alleles returns them; with detail=True a fourth
    item: per row (ms, sc, stop codon indices).  A row is forward when rs < re and reverse otherwise - one base (rs == re) is reverse, as
    `if tab[8] < tab[9] else rc(...)` has it."""
    stop = ['TAG', 'TAA', 'TGA'] if gtable != 4 else ['TAA', 'TAG']
    seq = [c.decode() if isinstance(c, (bytes, bytearray)) else c for c in contigs]
    in_frame, orf, packed, seen = [], [], [], []
    for g in range(len(grp_qlen)):
        gene = np.zeros(int(grp_qlen[g]), dtype=np.uint8)
        for r in range(int(grp_off[g]), int(grp_off[g + 1])):
            row = rows[r]
            contig, q_start, rs, re_ = int(row['contig']), int(row['q_start']), int(row['rs']), int(row['re'])
            text = ''.join('%d%s' % (int(c) >> 2, 'MID'[int(c) & 3]) for c in cigar[int(row['cigar_off']):int(row['cigar_off']) + int(row['cigar_runs'])])
            matchedSeq = seq[contig][rs - 1:re_] if rs < re_ else _rc(seq[contig][re_ - 1:rs])
            ms, i, f, sc = [], 0, 0, [0, 0, 0]
            for s, t in re.findall(r'(\d+)([A-Z])', text):
                s = int(s)
                if t == 'M':
                    ms.append(matchedSeq[i:i + s])
                    i += s
                    sc[f] += s
                elif t == 'D':
                    i += s
                    f = (f - s) % 3
                else:
                    ms.append('-' * s)
                    f = (f + s) % 3
            ms = ''.join(ms)
            at = np.where([c in stop for c in re.findall('...', ms)])[0]
            sc2 = np.max(np.diff(np.concatenate([[0], at * 3, [len(ms)]])))
            x = _BASE_CONV[np.array(list(ms)).view(np.uint32)]
            gene[q_start - 1:q_start + len(x) - 1] = x
            in_frame.append(np.max(sc))
            orf.append(sc2)
            seen.append((ms, sc, at.tolist()))
        s = int(np.ceil(len(gene) / 3))
        packed.append((gene[:s] * 25 + gene[s:2 * s] * 5 + np.concatenate([gene, np.zeros(-gene.shape[0] % 3, dtype=int)])[2 * s:]).astype(np.uint8))
    out = (np.array(in_frame, dtype=np.int64), np.array(orf, dtype=np.int64), np.concatenate(packed) if packed else np.zeros(0, np.uint8))
    return out + (seen,) if detail else out


def random_loci(rng, n_groups, contig_len=20000, n_contigs=3):
    """random K12 input: contigs with N runs and planted stops, groups of 1-3 rows with indels, both strands"""
    contigs = []
    for c in range(n_contigs):
        s = rng.choice(list(b'ACGT'), contig_len).astype(np.uint8)
        for _ in range(6):
            p = int(rng.integers(0, contig_len - 40)); s[p:p + int(rng.integers(1, 30))] = ord('N')
        for p in rng.integers(0, contig_len - 3, 300):
            s[p:p + 3] = list(rng.choice([b'TAA', b'TAG', b'TGA']))
        contigs.append(s.tobytes())
    rows, cigar, grp_off, grp_qlen = [], [], [0], []
    for g in range(n_groups):
        ql = int(rng.integers(60, 2500))
        q_at = 1
        for k in range(int(rng.choice([1, 1, 1, 2, 3]))):
            if q_at > ql - 30:
                break
            qs = max(1, q_at - int(rng.integers(0, 20)) * (k > 0))
            budget = ql - qs + 1
            runs, q_used, r_used = [], 0, 0
            while q_used < budget:
                m = int(min(budget - q_used, rng.integers(1, 400)))
                runs.append((m, 0)); q_used += m; r_used += m
                if q_used >= budget or rng.random() < 0.3:
                    break
                op = int(rng.choice([1, 2])); n = int(rng.integers(1, 8))
                if op == 1:
                    n = min(n, budget - q_used)
                    if n == 0:
                        break
                    q_used += n
                else:
                    r_used += n
                runs.append((n, op))
            if runs[-1][1] == 2:
                r_used -= runs[-1][0]; runs.pop()
            c = int(rng.integers(0, n_contigs))
            lo = int(rng.integers(1, contig_len - r_used))
            rs, re_ = (lo, lo + r_used - 1) if rng.random() < 0.5 else (lo + r_used - 1, lo)
            rows.append((c, qs, rs, re_, len(runs), g, len(cigar)))
            cigar += [(n << 2) | op for n, op in runs]
            q_at = qs + q_used
        grp_off.append(len(rows)); grp_qlen.append(ql)
    return contigs, np.array(rows, dtype=LOCUS_DTYPE), np.array(cigar, dtype=np.uint32), np.array(grp_off, dtype=np.uint64), np.array(grp_qlen, dtype=np.uint32)


def _base_contigs():
    """three contigs of about 700 nt over A, C and G alone: without T neither strand holds a stop codon, so a case has the stops it plants
    and no others.  The last one matters: the kernel's nt buffer ends where it ends."""
    rng = np.random.default_rng(12)
    return [bytes(rng.choice(list(b'ACG'), n).astype(np.uint8)) for n in (701, 697, 703)]


_CONTIGS = _base_contigs()
STRANDS = (('fwd', '+'), ('rev', '-'))


class _Groups(object):
    """one K12 input in the making: row() adds a row to the open group, close() ends the group, plant() writes the contig under a row"""

    def __init__(self, gtable=11):
        self.contigs = [bytearray(c) for c in _CONTIGS]
        self.rows, self.runs, self.cigar, self.grp_off, self.grp_qlen, self.gtable = [], [], [], [0], [], gtable
        self.expect = {}

    def row(self, contig, lo, runs, strand, q_start=1):
        """runs: [(n, 'M' | 'I' | 'D')]; lo: the smaller contig coordinate (1-based) -> the row's index"""
        rcons = sum(n for n, op in runs if op != 'I')
        hi = lo + rcons - 1
        assert 1 <= lo and hi <= len(self.contigs[contig]) and rcons >= 1
        rs, re_ = (lo, hi) if strand == '+' else (hi, lo)
        self.rows.append((contig, q_start, rs, re_, len(runs), len(self.grp_qlen), len(self.cigar)))
        self.runs.append(runs)
        self.cigar += [(n << 2) | 'MID'.index(op) for n, op in runs]
        return len(self.rows) - 1

    def close(self, ql):
        for r in range(self.grp_off[-1], len(self.rows)):
            span = sum(n for n, op in self.runs[r] if op != 'D')
            assert ql >= 3 and self.rows[r][1] >= 1 and self.rows[r][1] - 1 + span <= ql          # what pep_k12_alleles validates
        self.grp_off.append(len(self.rows))
        self.grp_qlen.append(ql)
        return self

    def plant(self, r, col, text):
        """write the contig so that the aligned string of row r reads `text` from column `col` on ('-' stands for a column of an I run)"""
        contig, _, rs, re_ = self.rows[r][:4]
        where, at, i = {}, 0, 0                             # column of an M run -> offset in the matched sequence
        for n, op in self.runs[r]:
            if op == 'M':
                where.update((at + k, i + k) for k in range(n))
            if op != 'D':
                at += n
            if op != 'I':
                i += n
        for k, ch in enumerate(text):
            if ch == '-':
                assert col + k not in where and col + k < at
            elif rs < re_:
                self.contigs[contig][rs - 1 + where[col + k]] = ord(ch)
            else:
                self.contigs[contig][rs - 1 - where[col + k]] = ord(_COMPLEMENT[ch])

    def case(self, name, **expect):
        return dict(name=name, contigs=[bytes(c) for c in self.contigs], rows=np.array(self.rows, dtype=LOCUS_DTYPE), cigar=np.array(self.cigar, dtype=np.uint32),
                    grp_off=np.array(self.grp_off, dtype=np.uint64), grp_qlen=np.array(self.grp_qlen, dtype=np.uint32), gtable=self.gtable, expect=expect)


def _tables(text):
    """every case that involves TGA runs under both genetic tables"""
    return (11, 4) if 'TGA' in text or 'TCA' in text else (11,)


def _is_stop(text, gtable):
    return text in ('TAA', 'TAG') or (text == 'TGA' and gtable != 4)


def alleles_cases():
    """-> [dict(name, contigs, rows, cigar, grp_off, grp_qlen, gtable, expect)]; expect holds what the case was built to give, worked out by
    hand from its construction (orf / in_frame per row), never from a restatement"""
    out = []
    one = lambda name, contig, lo, runs, strand, ql=None, q_start=1, gtable=11, **expect: out.append(  # noqa: E731
        _one_row(name, contig, lo, runs, strand, ql, q_start, gtable, expect))
    last = [len(c) for c in _CONTIGS]
    for tag, strand in STRANDS:
        # ---- contig edges
        one('edge/first-base-of-contig/' + tag, 0, 1, [(40, 'M')], strand)
        one('edge/last-base-of-contig/' + tag, 1, last[1] - 39, [(40, 'M')], strand)
        one('edge/whole-contig/' + tag, 1, 1, [(last[1], 'M')], strand)
        one('edge/last-contig-last-base/' + tag, 2, last[2] - 39, [(30, 'M'), (3, 'I'), (10, 'M')], strand)
        one('edge/last-contig-last-base-one-column/' + tag, 2, last[2], [(1, 'M')], strand)
        # ---- M runs around the 64-lane stride
        for n in (1, 63, 64, 65, 128, 129):
            one('mrun/%d/alone/%s' % (n, tag), n % 3, 20 + n, [(n, 'M')], strand, in_frame=[n])
            one('mrun/%d/between-gaps/%s' % (n, tag), n % 3, 3 + n, [(n, 'M'), (1, 'D'), (n, 'M'), (1, 'I'), (n, 'M')], strand, in_frame=[2 * n], frames=[[2 * n, 0, n]])
        # ---- I and D runs around the stride; len % 3 takes 1 (64), 2 (65) and 0 (66); the frame with the most M columns is not frame 0
        for n, op, frames in ((64, 'I', (7, 100, 20)), (65, 'I', (7, 20, 100)), (64, 'D', (7, 20, 100)), (65, 'D', (7, 100, 20)), (66, 'D', (127, 0, 0)),
                              (66, 'I', (127, 0, 0))):
            one('indel/%d%s/%s' % (n, op, tag), 0, 11, [(7, 'M'), (n, op), (100, 'M'), (n, op), (20, 'M')], strand, in_frame=[max(frames)], frames=[list(frames)])
        one('frame/1-has-most-M/' + tag, 1, 30, [(5, 'M'), (1, 'I'), (30, 'M')], strand, in_frame=[30], frames=[[5, 30, 0]])
        one('frame/2-has-most-M/' + tag, 1, 30, [(5, 'M'), (1, 'D'), (30, 'M')], strand, in_frame=[30], frames=[[5, 0, 30]])
        one('frame/0-then-2-then-1/' + tag, 2, 30, [(5, 'M'), (2, 'I'), (30, 'M'), (2, 'I'), (40, 'M')], strand, in_frame=[40], frames=[[5, 40, 30]])
        one('frame/back-to-0/' + tag, 2, 30, [(5, 'M'), (2, 'D'), (9, 'M'), (2, 'I'), (4, 'M')], strand, in_frame=[9], frames=[[9, 9, 0]])
        # ---- row spans without a codon, and with one or two columns beyond the last codon
        for runs, span in (([(1, 'M')], 1), ([(2, 'M')], 2), ([(1, 'M'), (1, 'I')], 2), ([(3, 'M')], 3), ([(4, 'M')], 4), ([(5, 'M')], 5), ([(2, 'D')], 0),
                           ([(64, 'M')], 64), ([(194, 'M')], 194)):
            one('span/%d-columns-%s/%s' % (span, ''.join('%d%s' % r for r in runs), tag), 0, 300, runs, strand, ql=200, q_start=4, orf=[span])
    # ---- stop codons in frame: 66 codons and two columns; codons 63 and 64 are the two sides of the ballot window's edge
    where = (('codon-0', 200, (0,)), ('codon-63', 200, (63,)), ('codon-64', 200, (64,)), ('last-full-codon', 200, (65,)), ('two-adjacent-63-64', 200, (63, 64)),
             ('two-adjacent-10-11', 200, (10, 11)), ('stop-then-row-end', 198, (65,)), ('codons-0-and-64', 200, (0, 64)))
    for name, span, codons in where:
        for text in ('TAA', 'TAG', 'TGA'):
            for gtable in (11, 4):
                for tag, strand in STRANDS:
                    g = _Groups(gtable)
                    r = g.row(1, 50, [(span, 'M')], strand)
                    for cd in codons:
                        g.plant(r, 3 * cd, text)
                    cuts = [0] + ([3 * cd for cd in codons] if _is_stop(text, gtable) else []) + [span]
                    out.append(g.close(span).case('stop/%s/%s/%s/gtable%d' % (name, text, tag, gtable), orf=[max(b - a for a, b in zip(cuts, cuts[1:]))],
                                                  stops=[list(codons) if _is_stop(text, gtable) else []]))
    # ---- a stop joined across a D run is one (the contig base drops out of the aligned string); everything after this is none
    for text in ('TAA', 'TGA'):
        for gtable in _tables(text):
            for tag, strand in STRANDS:
                g = _Groups(gtable)
                r = g.row(0, 100, [(31, 'M'), (1, 'D'), (40, 'M')], strand)
                g.plant(r, 30, text)
                out.append(g.close(71).case('stop/joined-across-D/%s/%s/gtable%d' % (text, tag, gtable), orf=[41 if _is_stop(text, gtable) else 71]))
                for shift in (1, 2):                        # one base out of frame, at the window's edge
                    g = _Groups(gtable)
                    r = g.row(1, 50, [(200, 'M')], strand)
                    g.plant(r, 3 * 63 + shift, text)
                    out.append(g.close(200).case('nonstop/out-of-frame-by-%d/%s/%s/gtable%d' % (shift, text, tag, gtable), orf=[200], stops=[[]]))
                g = _Groups(gtable)
                r = g.row(0, 100, [(31, 'M'), (1, 'I'), (40, 'M')], strand)
                g.plant(r, 30, text[0] + '-' + text[1:])
                out.append(g.close(72).case('nonstop/split-by-I/%s/%s/gtable%d' % (text, tag, gtable), orf=[72], stops=[[]]))
    # ---- the text of a stop that begins in the row's last one or two columns and goes on in the next row of the table (whose codes lie
    # right behind in the kernel's buffer): there is no codon behind the last full one
    for span in (64, 65, 196, 197):
        for text in ('TAA', 'TGA'):
            for gtable in _tables(text):
                for tag, strand in STRANDS:
                    g = _Groups(gtable)
                    r0 = g.row(0, 100, [(span, 'M')], strand)
                    r1 = g.row(1, 100, [(30, 'M')], strand, q_start=span + 1)
                    g.plant(r0, span - span % 3, text[:span % 3])
                    g.plant(r1, 0, text[span % 3:])
                    out.append(g.close(span + 30).case('nonstop/stop-text-across-the-row-end/%d-columns/%s/%s/gtable%d' % (span, text, tag, gtable),
                                                       orf=[span, 30], stops=[[], []]))
    for text in ('TNA', 'TAN', 'NAA', 'TGN', 'NGA', 'NNN'):
        for tag, strand in STRANDS:
            g = _Groups()
            r = g.row(2, 200, [(90, 'M')], strand)
            g.plant(r, 30, text)
            out.append(g.close(90).case('nonstop/with-N/%s/%s' % (text, tag), orf=[90], stops=[[]]))
    # ---- the forward strand's text decides nothing on the reverse strand: TTA, CTA and TCA read TAA, TAG and TGA there
    for text, back in (('TTA', 'TAA'), ('CTA', 'TAG'), ('TCA', 'TGA')):
        for gtable in _tables(text):
            for tag, strand in STRANDS:
                g = _Groups(gtable)
                g.contigs[0][312:315] = text.encode()        # 0-based 312 .. 314; the row covers 1-based 301 .. 330
                g.row(0, 301, [(30, 'M')], strand)           # forward: columns 12 .. 14 (codon 4); reverse: offsets 329 - 314 = 15 .. 17 (codon 5)
                stop = strand == '-' and _is_stop(back, gtable)
                out.append(g.close(30).case('forward-text/%s/%s/gtable%d' % (text, tag, gtable), orf=[15 if stop else 30], stops=[[5] if stop else []]))
    # ---- packing: gene lengths around ql % 3 and s = 64; a row that ends on the gene's last position
    for ql in (3, 4, 5, 191, 192, 193, 195):
        for tag, strand in STRANDS:
            one('pack/gene-%d/covered/%s' % (ql, tag), ql % 3, 100, [(ql, 'M')], strand)
            if ql > 5:
                one('pack/gene-%d/first-and-last-open/%s' % (ql, tag), ql % 3, 100, [(ql - 2, 'M')], strand, ql=ql, q_start=2)
    for tag, strand in STRANDS:
        one('pack/row-ends-on-gene-end/' + tag, 1, 7, [(20, 'M'), (4, 'I'), (36, 'M')], strand, ql=100, q_start=41)
    # ---- packing: what covers what (rows alternate strands; the first row's strand names the case)
    other = {'+': '-', '-': '+'}
    for tag, strand in STRANDS:
        g = _Groups()
        g.row(0, 40, [(50, 'M')], strand, q_start=11)
        g.row(1, 90, [(50, 'M')], other[strand], q_start=101)
        out.append(g.close(200).case('cover/open-head-tail-and-hole/' + tag))
        g = _Groups()
        g.row(0, 40, [(100, 'M')], strand, q_start=1)
        g.row(1, 90, [(10, 'M'), (20, 'I'), (10, 'M')], other[strand], q_start=51)
        out.append(g.close(120).case('cover/later-insert-columns-overwrite-bases/' + tag))
        g = _Groups()
        g.row(2, 40, [(150, 'M')], strand, q_start=1)
        g.row(0, 90, [(31, 'M')], other[strand], q_start=50)
        out.append(g.close(150).case('cover/later-row-inside-earlier/' + tag))
        g = _Groups()
        g.row(0, 40, [(50, 'M')], strand, q_start=1)
        g.row(1, 90, [(21, 'M')], other[strand], q_start=60)
        g.row(2, 300, [(81, 'M')], strand, q_start=40)
        out.append(g.close(130).case('cover/middle-row-hidden-by-last/' + tag))
        g = _Groups()
        g.row(0, 40, [(50, 'M')], strand, q_start=1)
        g.close(60).close(100)
        g.row(2, 600, [(50, 'M')], other[strand], q_start=3)
        out.append(g.close(52).case('cover/empty-group-between-two/' + tag))
    for ql in (3, 100, 193):
        out.append(_Groups().close(ql).case('cover/only-an-empty-group/gene-%d' % ql))
    rng = np.random.default_rng(300)
    g = _Groups()
    for k in range(300):
        runs = [[(int(rng.integers(3, 10)), 'M')], [(2, 'M'), (int(rng.integers(1, 4)), 'I'), (3, 'M')], [(4, 'M'), (2, 'D'), (2, 'M')]][k % 3]
        span = sum(n for n, op in runs if op != 'D')
        g.row(k % 3, int(rng.integers(1, 680)), runs, '+-'[int(rng.integers(0, 2))], q_start=int(rng.integers(1, 600 - span + 2)))
    out.append(g.close(600).case('cover/one-group-of-300-short-rows'))
    # ---- several groups of different gene lengths in one call: the offsets of the packed bytes and of the rows' codes
    g = _Groups()
    for k, ql in enumerate((3, 191, 4, 192, 5, 193, 195, 64)):
        g.row(k % 3, 10 + 7 * k, [(ql, 'M')], '+-'[k % 2])
        g.close(ql)
    out.append(g.case('pack/eight-groups-in-one-call'))
    assert len({c['name'] for c in out}) == len(out)
    return out


def _one_row(name, contig, lo, runs, strand, ql, q_start, gtable, expect):
    g = _Groups(gtable)
    g.row(contig, lo, runs, strand, q_start)
    span = sum(n for n, op in runs if op != 'D')
    return g.close(max(3, q_start - 1 + span) if ql is None else ql).case(name, **expect)


# ---------------------------------------------------------------------------------------------------------------------------------------
# K11
# ---------------------------------------------------------------------------------------------------------------------------------------
def overlaps_cap(n):
    """the pair buffer of Context.overlaps's first call; a table with more pairs is called a second time"""
    return max(1024, 4 * n)


def overlaps_cases():
    """-> [dict(name, contig, start, end, rid, ovl_l, ovl_p, pairs)], rows sorted by (contig, start, end); pairs: the number of pairs the
    case is built to report (None where it is not worked out by hand)"""
    out = []

    def add(name, rows, ovl_l, ovl_p, pairs=None, rid=None):
        rows = sorted(rows)
        contig, start, end = (np.array([r[k] for r in rows], dtype=dt) for k, dt in ((0, np.int32), (1, np.int64), (2, np.int64)))
        rid = np.arange(len(rows), dtype=np.int64)[::-1].copy() if rid is None else np.asarray(rid, dtype=np.int64)
        out.append(dict(name=name, contig=contig, start=start, end=end, rid=rid, ovl_l=float(ovl_l), ovl_p=float(ovl_p), pairs=pairs))

    # ---- exact thresholds, each on the side of the first and of the second interval.  In doubles 0.6 * 5 and 0.1 * 30 are 3.0 (an overlap of 3
    # is reported) and 0.28 * 25 is 7.000000000000001 (an overlap of 7 is not, though 7 / 25 is 0.28)
    add('threshold/0.6x5-is-3.0/first-interval', [(0, 100, 104), (0, 102, 200)], 300, 0.6, 1)
    add('threshold/0.1x30-is-3.0/first-interval', [(0, 100, 129), (0, 127, 400)], 300, 0.1, 1)
    add('threshold/0.28x25-is-above-7/first-interval', [(0, 100, 124), (0, 118, 400)], 300, 0.28, 0)
    add('threshold/0.6x5-is-3.0/second-interval', [(0, 100, 1000), (0, 998, 1002)], 300, 0.6, 1)
    add('threshold/0.1x30-is-3.0/second-interval', [(0, 100, 1000), (0, 998, 1027)], 300, 0.1, 1)
    add('threshold/0.28x25-is-above-7/second-interval', [(0, 100, 1000), (0, 994, 1018)], 300, 0.28, 0)
    add('threshold/overlap-equals-ovl_l', [(0, 1, 100), (0, 71, 200)], 30, 0.9, 1)
    add('threshold/overlap-one-below-ovl_l', [(0, 1, 100), (0, 72, 200)], 30, 0.9, 0)
    # ---- geometry
    add('geometry/identical-intervals', [(0, 50, 90)] * 3 + [(1, 50, 90)] * 2, 300, 0.6, 4)
    add('geometry/nested', [(0, 1, 1000), (0, 10, 20), (0, 400, 500), (0, 990, 1000)], 300, 0.6, 3)
    add('geometry/start-equals-end-of-the-first', [(0, 10, 50), (0, 50, 90)], 1, 1.5, 1)
    add('geometry/start-one-past-the-end', [(0, 10, 50), (0, 51, 90)], 1, 0., 0)
    # ---- contig changes on the block edge (rows 255 / 256) and the scan tile edge (2047 / 2048): every row overlaps its next two
    n = 2100
    rows = [(0 if i < 256 else (1 if i < 2048 else 2), 10 * i, 10 * i + 25) for i in range(n)]
    add('contig-change/at-rows-256-and-2048', rows, 300, 0., sum(min(2, hi - 1 - i) for lo, hi in ((0, 256), (256, 2048), (2048, n)) for i in range(lo, hi)))
    # ---- one row's count spans scan tiles
    add('long-first-interval/3000-successors', [(0, 1, 10 ** 6)] + [(0, 10 + 40 * i, 40 + 40 * i) for i in range(3000)], 300, 0.6, 3000)
    # ---- pair-count paths
    add('pairs/none-at-all', [(0, 100 * i, 100 * i + 50) for i in range(700)], 300, 0.6, 0)
    add('pairs/600-mutual-overlaps-exceed-the-first-buffer', [(0, 1 + i, 5000 + i) for i in range(600)], 300, 0.6, 600 * 599 // 2)
    # ---- value ranges
    base = 3 * 10 ** 9
    add('range/start-around-3e9', [(0, base, base + 104), (0, base + 102, base + 400), (0, base + 300, base + 2 ** 31), (1, base, base + 10)], 3, 0.6, 2)
    add('range/rid-above-2-to-32', [(0, 1, 100), (0, 50, 150), (0, 60, 70)], 10, 0.6, 3, rid=[2 ** 32 + 5, 2 ** 40, 2 ** 62 + 1])
    add('range/ovl_p-0', [(0, 1, 100), (0, 100, 200), (0, 200, 300), (0, 301, 400)], 300, 0., 2)
    add('range/ovl_p-1.5', [(0, 1, 100), (0, 2, 100), (0, 71, 300), (0, 272, 400)], 30, 1.5, 3)
    assert len({c['name'] for c in out}) == len(out)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# K10
# ---------------------------------------------------------------------------------------------------------------------------------------
def restate_components(n, a, b):
    """a dictionary union-find -> uint32[n], every node labelled with the smallest id of its component"""
    parent = {}

    def find(x):
        while parent.get(x, x) != x:
            x = parent[x]
        return x

    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
        for z in (x, y):                                    # shorten what was walked (the labels do not depend on it)
            while parent.get(z, z) != z:
                parent[z], z = min(rx, ry), parent[z]
    label = list(range(n))
    for i in range(n):                                      # a parent is smaller than its child: its label is final when the child is reached
        label[i] = label[parent.get(i, i)]
    return np.array(label, dtype=np.uint32)


def components_cases():
    """-> [dict(name, n, a, b)].  n stays at 20 000 or below on purpose: the kernel has no path compression, a path graph can leave a
    parent chain as deep as n, and uf_flatten then walks it from every node - quadratic work, milliseconds at this size and not beyond."""
    rng = np.random.default_rng(10)
    out = []
    add = lambda name, n, a, b: out.append(dict(name=name, n=n, a=np.asarray(a, dtype=np.uint32), b=np.asarray(b, dtype=np.uint32)))  # noqa: E731
    n = 20000
    i = np.arange(n - 1)
    add('path/edges-ascending', n, i, i + 1)
    add('path/edges-descending', n, i[::-1] + 1, i[::-1])
    p = rng.permutation(n - 1)
    add('path/edges-shuffled', n, p, p + 1)
    add('star/on-node-0', n, np.zeros(n - 1), i + 1)
    add('star/on-the-largest-id', n, np.full(n - 1, n - 1), i)
    add('edges/every-edge-a-self-loop', 5000, np.arange(5000), np.arange(5000))
    add('edges/one-edge-5000-times', 300, np.full(5000, 299), np.full(5000, 7))
    a, b = rng.integers(0, 3000, 4000), rng.integers(0, 3000, 4000)
    add('edges/both-orientations', 3000, np.concatenate([a, b]), np.concatenate([b, a]))
    add('mixed/giant-component-and-isolated-nodes', n, 2 * rng.integers(0, n // 2, 60000), 2 * rng.integers(0, n // 2, 60000))
    left, right = np.repeat(np.arange(40), 40), 100 + np.tile(np.arange(40), 40)
    add('mixed/complete-bipartite-40x40', 200, right, left)
    for nn in (255, 256, 257):
        for m in (255, 256, 257):
            add('size/n-%d-m-%d' % (nn, m), nn, rng.integers(0, nn, m), rng.integers(0, nn, m))
    add('size/no-edges', 257, [], [])
    assert len({c['name'] for c in out}) == len(out) and max(c['n'] for c in out) <= 20000
    return out


def hits_case():
    """components_of_hits: edges (q + q_base, node_of_target[t]).  -> dict(n, q, t, q_base, maps): maps is A, B, A with B differing from A in
    its last entry alone, and the last target is in the table, so the labels of B differ from those of A"""
    rng = np.random.default_rng(11)
    n_q, n_t, q_base = 300, 700, 5
    q, t = rng.integers(0, n_q, 500), rng.integers(0, n_t, 500)
    t[-1] = n_t - 1
    map_a = rng.integers(0, n_q + q_base, n_t).astype(np.uint32)
    map_a[-1] = 0
    map_b = map_a.copy()
    map_b[-1] = 1
    return dict(n=n_q + q_base, q=q.astype(np.uint32), t=t.astype(np.uint32), q_base=q_base, maps=[map_a, map_b, map_a.copy()])


# ---------------------------------------------------------------------------------------------------------------------------------------
# K13
# ---------------------------------------------------------------------------------------------------------------------------------------
def dedup_slot(run, digest, n):
    """where the probe of key (run, digest) starts in pep_dedup's table of n genes, and the table's mask: the hash of dedup.hip restated so
    that a case can put a probe chain across the end of the table; it reads digest words 0 and 1 and the run id, nothing else.
    A copy: the collide cases cross the wrap only as long as this matches slot_of and the table sizing of dedup.hip, and no test can
    tell when it no longer does (the keys still collide, wherever the chain starts) - change the two together."""
    bits = 4
    while (1 << bits) < 2 * n:
        bits += 1
    mask, m64 = (1 << bits) - 1, (1 << 64) - 1
    d0, d1 = (int.from_bytes(bytes(digest[k:k + 4]), 'big') for k in (0, 4))
    x = ((d0 << 32) | d1) ^ ((run * 0x9E3779B97F4A7C15) & m64)
    x ^= x >> 31
    x = (x * 0xBF58476D1CE4E5B9) & m64
    x ^= x >> 29
    return x & 0xFFFFFFFF & mask, mask


def _digests(rng, n):
    return rng.integers(0, 256, (n, 20)).astype(np.uint8)


def dedup_cases():
    """-> [dict(name, lengths, digests, rep)]; rep: what the case is built to give, by hand (None where it is not worked out)"""
    rng = np.random.default_rng(13)
    out = []
    add = lambda name, lengths, digests, rep=None: out.append(dict(name=name, lengths=np.asarray(lengths, dtype=np.uint32),  # noqa: E731
                                                                   digests=np.ascontiguousarray(digests, dtype=np.uint8), rep=rep))
    # ---- 3000 keys that share the run and digest words 0 and 1 - all that the hash reads - and differ in words 2 to 4; the last two differ
    # in the digest's last byte alone; then three true duplicates.  The head is chosen so that the chain starts 100 slots before the table's
    # end and goes on through (pos + 1) & mask.
    n = 3003
    head = None
    for k in range(1 << 20):
        cand = np.frombuffer(k.to_bytes(8, 'big'), dtype=np.uint8)
        slot, mask = dedup_slot(0, cand, n)
        if slot == mask - 100:
            head = cand
            break
    assert head is not None, 'no digest head within 2^20 candidates starts its probe 100 slots before the end of the table'
    d = np.zeros((n, 20), dtype=np.uint8)
    d[:, :8] = head
    for i in range(2999):
        d[i, 8 + 4 * (i % 3):12 + 4 * (i % 3)] = np.frombuffer((i // 3 + 1).to_bytes(4, 'big'), dtype=np.uint8)      # one of words 2, 3, 4 differs, the others are 0
    d[2999] = d[2998]
    d[2999, 19] ^= 1
    d[3000], d[3001], d[3002] = d[0], d[1500], d[2999]
    add('collide/3000-keys-share-the-hashed-words', np.full(n, 300), d, list(range(3000)) + [0, 1500, 2999])
    two = np.zeros((2, 20), dtype=np.uint8)
    two[:] = _digests(rng, 1)
    two[1, 19] ^= 0x80
    add('collide/two-keys-differ-in-the-last-byte', [30, 30], two, [0, 1])
    # ---- each duplicate sits in front of a distinct key that probes past it
    d = np.zeros((600, 20), dtype=np.uint8)
    d[:, :8] = head
    d[:, 16:20] = np.frombuffer((np.arange(600) // 2).astype('>u4').tobytes(), dtype=np.uint8).reshape(600, 4)
    add('collide/duplicate-then-a-key-probing-past-it', np.full(600, 90), d, [i - i % 2 for i in range(600)])
    # ---- table size steps and scan tile edges
    for n in (8, 9, 2048, 2049, 4097):
        add('distinct/%d-keys' % n, np.full(n, 33), _digests(rng, n), list(range(n)))
    # ---- run ids
    add('runs/every-gene-a-new-length', 10 + np.arange(2500), np.tile(_digests(rng, 1), (2500, 1)), list(range(2500)))
    d3 = _digests(rng, 2)[[0, 1, 0]]
    add('runs/length-re-opened-30-33-30', [30, 33, 30], d3, [0, 1, 2])
    add('runs/alternating-lengths-5000', np.where(np.arange(5000) % 2 == 0, 30, 33), np.tile(_digests(rng, 1), (5000, 1)), list(range(5000)))
    pool = _digests(rng, 7)
    pick = rng.integers(0, 7, 5000)
    lengths = np.repeat([36, 33, 36, 30, 33], 1000)
    add('runs/five-runs-of-1000-over-7-digests', lengths, pool[pick])
    add('identical/3000-genes', np.full(3000, 30), np.tile(_digests(rng, 1), (3000, 1)), [0] * 3000)
    assert len({c['name'] for c in out}) == len(out)
    return out
