"""determineGeneStructure (PEPPAN.py:1193-1229) restated in plain Python loops over strings, for the tests of K19.  It shares nothing with
csrc/genestruct.hip or peppan_amd/genestruct.py: characters are compared one by one, positions are searched by counting.  It is held to every
case of tests/golden/g23_genestruct.json.gz, which was recorded from the reference itself, and the GPU tests are held to it."""
import gzip
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FRAME_LISTS = ([0], [0, 1], [0, 2], [0, 1, 2], [1, 2], [2])
KINDS = ('CDS', 'nostart', 'nostop', 'premature_stop')
NO_STOP = 0xFFFFFFFF
STOPS = {11: ('TAA', 'TAG', 'TGA'), 4: ('TAA', 'TAG')}
STARTS = ('ATG', 'GTG', 'TTG')
COMPLEMENT = {'A': 'T', 'T': 'A', 'C': 'G', 'G': 'C'}


def load_g23():
    with gzip.open(os.path.join(HERE, 'golden', 'g23_genestruct.json.gz'), 'rt') as f:
        return json.load(f)


_RC = bytes(COMPLEMENT.get(chr(k).upper(), 'N').encode()[0] if k < 128 else ord('N') for k in range(256))


def rc(seq):
    """the reference's rc() (modules/configure.py:152-154): upper-cased, reversed, complemented, everything else N"""
    return seq.encode('ascii', 'replace').translate(_RC)[::-1].decode()


def mark_of(codon, stops):
    """one upper-cased codon -> M a start, X a stop or a codon with a character outside ACGT, - a codon with a '-', . the rest"""
    if '-' in codon:
        return '-'
    for ch in codon:
        if ch not in 'ACGT':
            return 'X'
    if codon in stops:
        return 'X'
    return 'M' if codon in STARTS else '.'


class Marks(dict):
    """codon -> its mark under one table; a codon is judged when it is first met"""
    def __init__(self, table):
        dict.__init__(self)
        self.stops = STOPS[table]

    def __missing__(self, codon):
        self[codon] = m = mark_of(codon, self.stops)
        return m


_MARKS = {4: Marks(4), 11: Marks(11)}


def marks(seq, frame, gtable):
    """one character per whole codon of the frame (the partial last codon is dropped)"""
    seq = seq.upper()
    codons = [seq[k:k + 3] for k in range(frame, frame + 3 * max(0, (len(seq) - frame) // 3), 3)]
    return ''.join(map(_MARKS[4 if gtable == 4 else 11].__getitem__, codons))


def first(text, what, lo, hi):
    for k in range(max(lo, 0), min(hi, len(text))):
        if text[k] == what:
            return k
    return -1


def last(text, what, lo, hi):
    for k in range(min(hi, len(text)) - 1, max(lo, 0) - 1, -1):
        if text[k] == what:
            return k
    return -1


def one_frame(text, lp, allowed_vary, ref_len):
    """the search of :1201-1216 over the marks of one frame -> dict(kind, start, stop, by, moves, broken)"""
    a, b, n = lp // 3, (lp + allowed_vary) // 3, len(text)
    s0, s1 = first(text, 'M', a, b), last(text, 'M', 0, a)
    kind, by = 0, 's0' if s0 >= 0 else 's1'
    start = s0 if s0 >= 0 else s1
    if start < 0:
        kind, start, by = 1, a, 'none'
    stop = first(text, 'X', start, n)
    first_stop = stop
    moves, broken = 0, False
    while 0 <= stop < b:
        m = first(text, 'M', stop, b)
        if m < 0:
            broken = True
            break
        start, moves = m, moves + 1
        stop = first(text, 'X', start, n)
    if stop < 0:
        kind = 2
    elif (stop - start + 1) * 3 < ref_len - allowed_vary:
        kind = 3
    return dict(kind=kind, start=start, stop=stop, by=by, moves=moves, broken=broken, first_stop=first_stop, s0=s0, s1=s1, a=a, b=b, n=n,
                slack=(stop - start + 1) * 3 - (ref_len - allowed_vary) if stop >= 0 else None)


def restate(item):
    """item = [pid, pred, seq, s, e, s2, e2, lp, allowed_vary, gtable] -> (what the reference returns, what the library returns, the frames' details)
    = ((pid, cds, start, stop), (frame, start_aa, stop_aa, kind), [one_frame(...) per tried frame until the first CDS])"""
    pid, pred, seq, s, e, s2, e2, lp, allowed_vary, gtable = item
    details = []
    for f in pred[14]:
        d = one_frame(marks(seq, f, gtable), lp, allowed_vary, pred[12])
        details.append(d)
        if d['kind'] == 0:
            if pred[11] == '+':
                ret = (pid, 'CDS', s2 + 3 * d['start'] + f, s2 + 3 * d['stop'] + 2 + f)
            else:
                ret = (pid, 'CDS', e2 - 3 * d['stop'] - 2 - f, e2 - 3 * d['start'] - f)
            return ret, (f, d['start'], d['stop'], details[0]['kind']), details
    d = details[0]
    text = KINDS[d['kind']]
    if d['kind'] == 3:
        text = 'premature_stop:{0:.2f}%'.format((d['stop'] - d['start'] + 1) * 300 / pred[12])
    if pred[14][-1] > 0:
        text = text.replace('premature_stop', 'frameshift') if d['kind'] == 3 else 'frameshift'
    return (pid, text, s, e), (-1, d['start'], d['stop'] if d['stop'] >= 0 else NO_STOP, d['kind']), details


def make_item(pid, seq, strand, frames, lp, allowed_vary, ref_len, gtable, s2=None):
    """an item as write_output builds it (:1465): pred carries only the fields determineGeneStructure reads; coordinates consistent with the window"""
    s2 = 1000 + 7 * pid if s2 is None else s2
    e2 = s2 + len(seq) - 1
    pred = [''] * 16
    pred[5], pred[11], pred[12], pred[14] = 'contig%d' % (pid % 3), strand, ref_len, list(frames)
    s, e = (s2 + lp, e2 - 3) if strand == '+' else (s2 + 3, e2 - lp)
    return [pid, pred, seq, s, e, s2, e2, lp, allowed_vary, gtable]


def item_of_case(c):
    pred = [''] * 16
    pred[5], pred[11], pred[12], pred[14] = c['contig'], c['strand'], c['ref_len'], list(c['frames'])
    return [c['pid'], pred, c['seq'], c['s'], c['e'], c['s2'], c['e2'], c['lp'], c['allowed_vary'], c['gtable']]


def random_window(rng, length, alphabet='ACGT', odd=0.):
    seq = np.frombuffer(alphabet.encode(), dtype=np.uint8)[rng.integers(0, len(alphabet), length)]
    if odd and length:
        hit = rng.random(length) < odd
        seq = np.where(hit, np.frombuffer(b'N-nRacgt', dtype=np.uint8)[rng.integers(0, 8, length)], seq)
    return seq.astype(np.uint8).tobytes().decode()


def planted_orf(rng, codons, lead, tail, start='ATG', stop='TAA', frame=0):
    """`lead` random nucleotides without stops or starts in frame, a start codon, codons - 2 plain codons, a stop, `tail` random nucleotides"""
    plain = ['GCT', 'GAA', 'CTC', 'AAA', 'GGC', 'CCA', 'ACC', 'GAT']
    body = ''.join(plain[k] for k in rng.integers(0, len(plain), max(codons - 2, 0)))
    front = ''.join(plain[k] for k in rng.integers(0, len(plain), lead // 3 + 1))[:lead]
    return random_window(rng, frame) + front + start + body + stop + random_window(rng, tail)


def reversible(seq):
    """whether a window is its own double reverse complement: upper-case ACGTN alone"""
    return set(seq) <= set('ACGTN')


def contig_form(items, rng, pad=37):
    """the windows of `items` embedded in longer contigs -> (items with seq None and s2 / e2 pointing into their contig, {contig: sequence}).  A '-' item's
    window is stored reverse-complemented, so that reading it backward gives the item's seq again - which needs a window of ACGTN upper case alone; others stay '+'"""
    contigs, out = {}, []
    for it in items:
        pid, pred, seq, s, e, s2, e2, lp, allowed_vary, gtable = it
        assert pred[11] == '+' or reversible(seq), 'a - window must be its own double reverse complement'
        name = pred[5]
        have = contigs.setdefault(name, [random_window(rng, pad)])
        at = sum(len(p) for p in have)
        have.append(seq if pred[11] == '+' else rc(seq))
        have.append(random_window(rng, int(rng.integers(0, pad))))
        shift = at + 1 - s2
        out.append([pid, pred, None, s + shift, e + shift, s2 + shift, e2 + shift, lp, allowed_vary, gtable])
    return out, {k: ''.join(v) for k, v in contigs.items()}


def shifted_back(ret, item, moved):
    """the tuple of a moved item in the coordinates of the original one"""
    d = moved[5] - item[5]
    return (ret[0], ret[1], ret[2] - d, ret[3] - d)
