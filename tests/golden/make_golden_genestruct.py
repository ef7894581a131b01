#!/usr/bin/env python3
"""Generate tests/golden/g23_genestruct.json.gz by IMPORTING the reference's Python (build machine only).

    python tests/golden/make_golden_genestruct.py

The shim of make_golden_synteny.py, taken by importing that module: it puts the reference on the path and imports it as PEP.  Every case goes through
PEP.determineGeneStructure (PEPPAN.py:1193-1229) as an item [pid, pred, seq, s, e, s2, e2, lp, allowed_vary, gtable]; recorded are the inputs and the
returned tuple.  Only DATA is written, none of the reference's source text.  The restatement of tests/genestruct_helpers.py is held to every case, and
the conditions the fixture is pinned by are asserted at the end.
"""
import gzip, json, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_synteny import PEP, np                      # noqa: E402  (the shim; also puts tests/ on the path)
from genestruct_helpers import FRAME_LISTS, make_item, planted_orf, random_window, rc, restate   # noqa: E402

PLAIN = ['GCT', 'GAA', 'CTC', 'AAA', 'GGC', 'CCA', 'ACC', 'GAT']
SPELL = {'M': 'ATG', 'V': 'GTG', 'L': 'TTG', 'X': 'TAA', 'Z': 'TAG', 'O': 'TGA', 'N': 'ANC', '-': 'A-C', 'n': 'acn', 'm': 'atg', 'x': 'taa'}


def spell(rng, marks, tail=''):
    """a window whose frame 0 reads as `marks`: . a plain codon, M V L the three starts, X Z O the three stops, N a codon with an N, - one with a '-',
    m x n lower case; `tail`: 0 to 2 more nucleotides"""
    return ''.join(SPELL[ch] if ch in SPELL else PLAIN[int(rng.integers(0, len(PLAIN)))] for ch in marks) + tail


def constructed(rng):
    """(name, seq, frames, lp, allowed_vary, ref_len, gtable) of the hand-made cases"""
    C = []
    body = '.' * 30
    for st in 'MVL':                                                          # a clean CDS with each start codon (both strands: see main)
        C.append(('clean_' + SPELL[st], spell(rng, '.....' + st + body + 'X...'), [0], 15, 9, 96, 11))
    C.append(('s0_over_s1', spell(rng, '.M...M' + body + 'X..'), [0], 12, 9, 96, 11))
    C.append(('rfind_only', spell(rng, 'M.M....' + body + 'X..'), [0], 15, 9, 96, 11))
    C.append(('nostart_kept', spell(rng, '.....' + body + 'X..'), [0], 15, 9, 96, 11))
    C.append(('nostart_nostop', spell(rng, '.....' + body + '...'), [0], 15, 9, 96, 11))
    C.append(('nostart_premature', spell(rng, '..........X' + body), [0], 15, 9, 96, 11))
    C.append(('relocated_once', spell(rng, '..M.X..M' + body + 'X..'), [0], 6, 30, 96, 11))
    C.append(('relocated_thrice', spell(rng, '..M.XM.ZV.OL' + body + 'X..'), [0], 6, 36, 96, 11))
    C.append(('stop_at_b_minus_1', spell(rng, '..M........X' + body), [0], 6, 30, 40, 11))          # b = 12: the loop looks for an M in [11, 12) and breaks
    C.append(('stop_at_b_minus_1_premature', spell(rng, '..M........X' + body), [0], 6, 30, 96, 11))
    C.append(('stop_at_b', spell(rng, '..M.........X' + body), [0], 6, 30, 40, 11))                # stop = 12 = b: the loop is not entered
    C.append(('a_beyond_end', spell(rng, '..M....X..'), [0], 60, 9, 30, 11))
    C.append(('a_beyond_end_no_m', spell(rng, '.......X..'), [0, 1], 60, 9, 30, 11))
    C.append(('b_beyond_end', spell(rng, '..M....X..'), [0], 3, 90, 100, 11))
    C.append(('b_beyond_end_relocated', spell(rng, 'M.X.M..X.M'), [0], 0, 90, 100, 11))
    C.append(('span_equal', spell(rng, '.....M' + body + 'X...'), [0], 15, 9, 105, 11))              # (36 - 5 + 1) * 3 = 96 = 105 - 9
    C.append(('span_one_codon_short', spell(rng, '.....M' + body + 'X...'), [0], 15, 9, 108, 11))
    C.append(('n_in_codon_is_stop', spell(rng, '..M...N' + body + 'X'), [0], 6, 9, 96, 11))
    C.append(('n_in_start_region', spell(rng, 'N.M' + body + 'X'), [0], 6, 9, 96, 11))
    C.append(('gap_codon_is_nothing', spell(rng, '..M..-..' + body + 'X..'), [0], 6, 9, 96, 11))
    C.append(('gap_and_n', spell(rng, '..M..-N.' + body + 'X..'), [0, 1, 2], 6, 9, 96, 11))
    C.append(('lower_case', spell(rng, '..m' + body + 'x..').lower(), [0], 6, 9, 96, 11))
    C.append(('lower_case_n', spell(rng, '..m...n' + body + 'x..'), [0, 2], 6, 9, 96, 11))
    for table in (11, 4):
        C.append(('tga_table%d' % table, spell(rng, '..M' + '.' * 10 + 'O' + '.' * 19 + 'X..'), [0], 6, 9, 96, table))
        C.append(('tga_only_table%d' % table, spell(rng, '..M' + body + 'O..'), [0, 1], 6, 9, 96, table))
    # M and X at codons 63, 64, 65 of a frame, and around 4 096
    for edge in (64, 4096):
        for d in (-1, 0, 1):
            k = edge + d
            C.append(('start_at_%d' % k, spell(rng, '.' * k + 'M' + body + 'X..'), [0], 3 * k, 9, 96, 11))
            C.append(('stop_at_%d' % k, spell(rng, '..M' + '.' * (k - 3) + 'X..'), [0], 6, 9, 3 * (k - 1), 11))
            C.append(('rfind_at_%d' % k, spell(rng, '.' * k + 'M...' + body + 'X..'), [0], 3 * k + 6, 6, 96, 11))
            C.append(('relocated_at_%d' % k, spell(rng, '.' * (k - 2) + 'M.X.M' + body + 'X..'), [0], 3 * k - 6, 30, 96, 11))
            C.append(('frame1_at_%d' % k, 'C' + spell(rng, '.' * k + 'M' + body + 'X..'), [1], 3 * k, 9, 96, 11))
            C.append(('frame2_at_%d' % k, 'CA' + spell(rng, '.' * k + 'M' + '.' * (k if edge == 64 else 30) + 'X..', 'GC'), [0, 2], 3 * k, 9, 96, 11))
    # window lengths 0 to 8 under every frame list: every residue of the length mod 3 per frame, frames without a codon
    for length in range(9):
        for frames in FRAME_LISTS:
            C.append(('length_%d' % length, random_window(rng, length), frames, int(rng.integers(0, 7)), int(rng.integers(0, 7)), int(rng.integers(1, 12)), 11))
    for length in (30, 31, 32):
        for frames in FRAME_LISTS:
            C.append(('length_%d' % length, spell(rng, 'M' + '.' * 8 + 'X', 'AC'[:length - 30]), frames, 0, 6, 30, 11))
    # a CDS in the second and in the third tried frame; all frames failing, with and without a premature first frame
    for frames in FRAME_LISTS:
        for f in range(3):
            C.append(('orf_in_frame%d' % f, planted_orf(rng, 40, 12, 20, frame=f), frames, 12, 9, 120, 11))
            C.append(('short_orf_in_frame%d' % f, planted_orf(rng, 12, 12, 60, frame=f), frames, 12, 9, 120, 11))
        C.append(('nothing', spell(rng, '.' * 50), frames, 12, 9, 120, 11))
    return C


def seeded(rng):
    """random windows: plain, with odd characters, with planted ORFs; all frame lists, both tables"""
    C = []
    for k in range(240):
        frames = FRAME_LISTS[int(rng.integers(0, len(FRAME_LISTS)))]
        table = 4 if k % 5 == 0 else 11
        kind = k % 4
        if kind == 0:
            seq = random_window(rng, int(rng.integers(0, 700)))
        elif kind == 1:
            seq = random_window(rng, int(rng.integers(0, 700)), odd=0.01)
        else:
            seq = planted_orf(rng, int(rng.integers(5, 200)), int(rng.integers(0, 90)), int(rng.integers(0, 120)), start=('ATG', 'GTG', 'TTG')[k % 3],
                              stop=('TAA', 'TAG', 'TGA')[k % 3], frame=int(rng.integers(0, 3)) if k % 8 < 3 else 0)
        lp = int(rng.integers(0, 120))
        C.append(('seeded_%d' % kind, seq, frames, lp, int(rng.integers(0, 60)), int(rng.integers(1, max(2, len(seq)))), table))
    return C


def main():
    rng = np.random.default_rng(23000)
    cases, seen = [], {}

    def note(key):
        seen[key] = seen.get(key, 0) + 1

    for pid, (name, seq, frames, lp, allowed_vary, ref_len, gtable) in enumerate(constructed(rng) + seeded(rng)):
        strand = '+-'[pid % 2]
        if strand == '-' and rc(rc(seq)) != seq:
            # a '-' window reaches the function reverse-complemented (:1449): upper case, N for everything else.  '-' and lower case stay on '+'
            strand = '+'
        item = make_item(pid, seq, strand, frames, lp, allowed_vary, ref_len, gtable)
        got = PEP.determineGeneStructure(item)
        ret = [int(got[0]), str(got[1]), int(got[2]), int(got[3])]
        mine, lib, details = restate(item)
        assert list(mine) == ret, (name, pid, ret, mine)
        cases.append(dict(name='%s_%d' % (name, pid), pid=pid, contig=item[1][5], strand=strand, ref_len=ref_len, frames=list(frames), seq=seq, s=item[3], e=item[4],
                          s2=item[5], e2=item[6], lp=lp, allowed_vary=allowed_vary, gtable=gtable, returned=ret))
        # what the fixture is pinned by
        d = details[0]
        text = ret[1].split(':')[0]
        note(('text', text))
        note(('frames', tuple(frames), 'found' if text == 'CDS' else 'failed'))
        if text == 'CDS':
            note(('strand', strand, seq[3 * d['start'] + frames[0]:3 * d['start'] + frames[0] + 3].upper()) if len(details) == 1 else ('found in tried frame', len(details)))
        else:
            note(('all fail', 'premature first' if d['kind'] == 3 else 'other first', 'one frame' if len(frames) == 1 else 'several'))
        for d in details:
            note(('by', d['by'], 'M below a too' if d['s1'] >= 0 else ''))
            note(('kind', d['by'], d['kind']))
            note(('moves', min(d['moves'], 3)))
            if d['broken']:
                note(('broken at', 'b-1' if d['stop'] == d['b'] - 1 else 'below'))
            if d['first_stop'] == d['b'] and d['moves'] == 0:
                note('stop at b')
            if d['a'] > d['n']:
                note('a beyond end')
            if d['b'] > d['n'] >= d['a']:
                note('b beyond end')
            if d['slack'] in (0, -3):
                note(('slack', d['slack'], d['kind']))
            for k in (63, 64, 65, 4095, 4096, 4097):
                if d['start'] == k and d['by'] != 'none':
                    note(('M at', k))
                if d['stop'] == k:
                    note(('X at', k))
        note(('length', len(seq)) if len(seq) < 9 else ('length mod 3', len(seq) % 3, tuple(frames)))
        up = seq.upper()
        if 'N' in up:
            note('N')
        if '-' in seq:
            note('gap')
        if seq != up:
            note('lower case')
        if 'TGA' in up and text != 'nostop':
            note(('TGA', gtable))
    print(len(cases), 'cases')
    for k in sorted(seen, key=str):
        print('  ', k, seen[k])
    need = [('text', t) for t in ('CDS', 'nostart', 'nostop', 'premature_stop', 'frameshift')]
    need += [('strand', s, c) for s in '+-' for c in ('ATG', 'GTG', 'TTG')]
    need += [('by', 's0', 'M below a too'), ('by', 's1', 'M below a too'), ('kind', 'none', 1), ('kind', 'none', 2), ('kind', 'none', 3), ('moves', 1), ('moves', 3),
             ('broken at', 'b-1'), 'stop at b', 'a beyond end', 'b beyond end', ('slack', 0, 0), ('slack', -3, 3), ('found in tried frame', 2), ('found in tried frame', 3),
             ('all fail', 'premature first', 'several'), ('all fail', 'other first', 'several'), ('all fail', 'premature first', 'one frame'),
             ('all fail', 'other first', 'one frame'), 'N', 'gap', 'lower case', ('TGA', 11), ('TGA', 4)]
    need += [('frames', tuple(f), r) for f in FRAME_LISTS for r in ('found', 'failed')]
    need += [('length', k) for k in range(6)] + [('length mod 3', r, tuple(f)) for r in range(3) for f in FRAME_LISTS]
    need += [(w, k) for w in ('M at', 'X at') for k in (63, 64, 65, 4095, 4096, 4097)]
    missing = [k for k in need if not seen.get(k)]
    assert not missing, missing
    by_name = {c['name'].rsplit('_', 1)[0]: c for c in cases}
    assert by_name['tga_table11']['returned'][1].startswith('premature_stop') and by_name['tga_table4']['returned'][1] == 'CDS'
    assert by_name['n_in_codon_is_stop']['returned'][1].startswith('premature_stop') and by_name['gap_codon_is_nothing']['returned'][1] == 'CDS'
    assert by_name['lower_case']['returned'][1] == 'CDS' and by_name['stop_at_b']['returned'][1] == 'CDS' and by_name['stop_at_b_minus_1']['returned'][1] == 'CDS'
    assert 300 <= len(cases) <= 900 and sum(len(c['seq']) < 1000 for c in cases) > 0.8 * len(cases)
    out = os.path.join(HERE, 'g23_genestruct.json.gz')
    with gzip.GzipFile(out, 'wb', mtime=0) as f:
        f.write(json.dumps(dict(source='PEPPAN.py:1193-1229 (determineGeneStructure)', cases=cases), separators=(',', ':')).encode())
    print(out, os.path.getsize(out), 'bytes')
    assert os.path.getsize(out) < 700 << 10


if __name__ == '__main__':
    main()
