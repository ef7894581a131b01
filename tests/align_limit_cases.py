"""Hand-built searches that put the two alignment passes (csrc/sw.hip: sw_score_kernel, sw_trace_kernel, sw_trace_retry_kernel) on, one
below and one above every limit at which they choose another sweep, and a restatement of that dispatch arithmetic in plain Python.
tests/test_align_limit_cases_host.py holds every case to what its name says (with the oracle's own counters and the full-matrix
optimum of oracle/full_sw.py), tests/test_gpu_align_limits.py compares the GPU with the oracle on each.

THIS FILE CANNOT SEE sw.hip.  Every constant below names the line it restates; whoever moves a limit in sw.hip moves the constant here,
and the census of the host test then shows whether the cases still stand on both sides of it (every limit is covered from two below to
two above, so a limit that moves by one without this file being told still has cases on both sides).

The sweeps a candidate can take (side()):

    score pass     pk16            two candidates per wavefront, packed 16-bit, windows staged once         (sw_two_pk16<false>)
                   pk16_chunked    the same in chunks of SCORE_CHUNK blocks, the launch of the long pairs   (sw_two_pk16<true>)
                   s32_lds         one candidate per wavefront in 32 bits, residues staged                  (sw_one<true, false>)
                   s32_global      the same, residues read from global memory                               (sw_one<false, false>)
    traceback pass pk16x4          four sub-bands per wavefront, packed 16-bit                              (sw_four_pk16_trace<false>)
                   pk16x4_chunked  the same in chunks of TRACE_CHUNK blocks                                 (sw_four_pk16_trace<true>)
                   s32_lds / s32_global   trace_slow_path: the sub-band in 32 bits, then the full band if the alignment left it
                   a `+retry` behind a packed sweep: the alignment left its sub-band, the pair went on the defer list and
                   sw_trace_retry_kernel swept its full band (the oracle counts exactly these and the slow path's as `full_band`)

The case families (a case: name, family, q, t, params, pairs; every builder draws from a seed fixed by the case's name):

    eligibility/    fits16 crossed: a W-rich BLOSUM62 query of 2960 .. 2963 residues (and one far beyond) against four targets, the same with
                    255 .. 258 residues under a table whose W/W entry is 127, such an item of four with ONE ineligible pair, and searches
                    of 2 .. 5 one-candidate pairs with exactly one ineligible member (mixed items in both passes)
    half_word_edge/ W/W = 127 and -128 everywhere else, gap costs from (0, 1) to (255, 255), pairs of the largest eligible length
    staging/        block counts around nb_limit of both passes and around the `fits` test, with and without a long bystander that
                    switches split_long on, and pairs of k chunks and k chunks + 1 block of both chunked sweeps
    step_counter/   nucleotide pairs (reward 1), four a search, whose longest sub-band has 2038 .. 2041 blocks, and a search of 20 000 bases
    tails/          1, 2, 3, 5, 6 and 7 active candidates, all eligible and with one ineligible member
    sub_band_exit/  items of four with 0, 1, 3 and 4 pairs that leave their sub-band, straight and transposed, and one long enough
                    for the chunked launch"""
import functools
import zlib

import numpy as np

# ---------------------------------------------------------------------------------------------------------------- the constants
BIN_W, DIAG_OFF, BAND, BAND_LEAD = 64, 1 << 23, 128, 32      # align_oracle.c:44-47; sw.hip cand_geom: dlo = bin * 64 - (1 << 23) - 32
SUB_LANES = 32                   # sw.hip:61        lanes of a sub-band (two diagonals each)
PK_BIAS = 128                    # sw.hip:251       the packed score pass carries H + PK_BIAS
FITS16_SLACK = 64                # sw.hip:285       fits16: min(Lq, Lt) * max_sub + 64 + PK_BIAS < 32767
HALF_WORD = 32767
LEN_BUCKETS = 1024               # sw.hip:31        the order is by min(blocks, LEN_BUCKETS - 1), longest first
LDS_CAP = 8192                   # sw.hip:968       staging area per wavefront, capped
LDS_LONG_SCORE = 3072            # sw.hip:1068      staging area of the long score launch
STEP_GATE = 2040                 # sw.hip:699       the four-candidate sweep takes items of fewer blocks only (16-bit step counter)
SCORE_WIN_PAD, TRACE_WIN_PAD = 80, SUB_LANES + 16           # sw.hip:303-304 / 466-467   window = 8 * blocks + pad entries of two bytes
S32_WIN_PAD = 72                 # sw.hip:618, 633  the 32-bit sweep stages two windows of 8 * blocks + 72 entries
PACK_MIN_BYTES = 4 * 2 * 88      # sw.hip:610       can_pack needs a staging area of at least this
TRACE_LONG_MIN_BYTES = 8 * 2 * (SUB_LANES + 24)             # sw.hip:699  the chunked four-candidate sweep needs at least this

W, P_, A_ = 22, 15, 0            # residue codes: letter - 'A'
AA20 = np.frombuffer(b'ARNDCQEGHILKMFPSTWYV', dtype=np.uint8) - 65
NOT_W = AA20[AA20 != W]


def round8(x):
    return (x + 7) & ~7


# ---------------------------------------------------------------------------------------------------------------- the restatement
def band_dlo(bin_):
    return bin_ * BIN_W - DIAG_OFF - BAND_LEAD


def bin_of(d):
    return (d + DIAG_OFF) // BIN_W


def band_geom(Lq, Lt, dlo, width):
    """sw.hip:65 band_geom -> (a0, 16-step blocks) of the band [dlo, dlo + width) of an Lq x Lt matrix"""
    dl, dh = max(dlo, -(Lq - 1)), min(dlo + width - 1, Lt - 1)
    s_lo = 0 if (dl <= 0 <= dh) else (dl if dl > 0 else -dh)
    s0 = s_lo - ((s_lo - dlo) & 1)
    a0 = (s0 - dlo) // 2
    nblk = 0
    if dl <= dh:
        dstar = min(max(Lt - Lq, dl), dh)
        s_hi = 2 * min(Lq - 1, Lt - 1 - dstar) + dstar
        nblk = (s_hi - s0 + 1 + 15) // 16
    return a0, nblk


def cand_blocks(Lq, Lt, bin_):
    """sw.hip:801 sw_prep: the 16-step blocks of a candidate's full band"""
    return band_geom(Lq, Lt, band_dlo(bin_), BAND)[1]


def cand_cells(Lq, Lt, bin_):
    """sw.hip:801 sw_prep / align_oracle.c banded_sw: in-band in-matrix cells of a candidate"""
    dlo = band_dlo(bin_)
    dl, dh = max(dlo, -(Lq - 1)), min(dlo + BAND - 1, Lt - 1)
    return sum(min(Lq, Lt - d) + min(0, d) for d in range(dl, dh + 1))


def sub_band_first_lane(end_lane):
    """sw.hip:62"""
    return min(max(end_lane - SUB_LANES // 2, 0), 64 - SUB_LANES)


def sub_geom(Lq, Lt, bin_, end_lane):
    """sw.hip:438 sub_geom -> (first diagonal, a0, blocks) of the sub-band around the lane the score was met in"""
    dlo = band_dlo(bin_) + 2 * sub_band_first_lane(end_lane)
    a0, nblk = band_geom(Lq, Lt, dlo, 2 * SUB_LANES)
    return dlo, a0, nblk


def table(name):
    """the 32 x 32 substitution tables of the cases, [q * 32 + t] as the parameter blocks hold them (None: the block's own default)"""
    if name == 'blosum62':
        return None
    if name == 'edge':                                   # W/W = 127, everything else -128 (row / column 31, the padding code, included)
        s = np.full((32, 32), -128, dtype=np.int8)
        s[W, W] = 127
        return s.reshape(-1)
    if name == 'nucl1':                                  # the nucleotide tool's table with the reward set to 1
        s = np.full((32, 32), -64, dtype=np.int8)
        s[:5, :5] = -3
        s[np.arange(4), np.arange(4)] = 1
        return s.reshape(-1)
    raise KeyError(name)


def max_sub(params):
    """sw.hip:1059-1060: the largest table entry, at least 1"""
    return max(1, int(np.frombuffer(bytes(params.sub), dtype=np.int8).max()))


def fits16(Lq, Lt, msub):
    """sw.hip:285"""
    return min(Lq, Lt) * msub + FITS16_SLACK + PK_BIAS < HALF_WORD


def staging(max_q, max_t, trace):
    """sw.hip:964-982 pep_sw_run with the packed passes on (use_lds = 1, reserved[1] = 0) -> lds_res_bytes, split_long, nb_limit and the
    chunk of the pass's chunked sweep (sw.hip:303 with the long score launch's staging area, sw.hip:466)"""
    max_blk = (max_q + max_t) // 16 + 2
    want = 2 * 2 * round8(8 * max_blk + SCORE_WIN_PAD)
    want4 = 8 * 2 * round8(8 * max_blk + TRACE_WIN_PAD)
    need = max(want4, 2 * want) if trace else 2 * want
    lds = min(LDS_CAP, (need + 255) & ~255)
    split_long = (want4 if trace else 2 * want) > lds
    nb_limit = 0
    if not trace and split_long:
        entries = lds // (4 * 2)
        nb_limit = min((entries - 87) // 8 if entries > 88 else 0, LEN_BUCKETS - 2)
    if trace:
        entries = lds // (8 * 2)
        nb_limit = min((entries - SUB_LANES - 16) // 8 - 1 if entries > SUB_LANES + 16 + 8 else 0, LEN_BUCKETS - 2)
    if trace:
        chunk = (lds // 16 - TRACE_WIN_PAD) // 8
    else:
        chunk = (min(lds, LDS_LONG_SCORE) // 8 - SCORE_WIN_PAD) // 8
    return dict(lds_res_bytes=lds, split_long=split_long, nb_limit=nb_limit, chunk=max(1, chunk))


def _s32(nb, lds):
    """sw.hip:618-620, 633-640: the 32-bit sweep stages its two windows when they fit"""
    return 's32_lds' if 2 * 2 * round8(8 * nb + S32_WIN_PAD) <= lds else 's32_global'


def _score_sweeps(cands, st, tie):
    """sw.hip:592 sw_score_kernel over the candidates in the length order; tie = +1 / -1: the two extreme orders inside a length bucket"""
    n = len(cands)
    order = sorted(range(n), key=lambda k: (-min(cands[k]['nblk'], LEN_BUCKETS - 1), tie * cands[k]['eligible'], tie * k))
    n_long = sum(1 for c in cands if c['nblk'] > st['nb_limit'])
    w_long = min((n + 1) // 2, (n_long + 1) // 2) if st['split_long'] else 0
    out = [None] * n
    for w in range((n + 1) // 2):
        c0, c1 = order[2 * w], order[min(2 * w + 1, n - 1)]
        long_ = w < w_long
        lds = min(st['lds_res_bytes'], LDS_LONG_SCORE) if long_ else st['lds_res_bytes']
        nbm = max(cands[c0]['nblk'], cands[c1]['nblk'])
        can_pack = cands[c0]['eligible'] and cands[c1]['eligible'] and lds >= PACK_MIN_BYTES
        fits = 4 * 2 * round8(8 * nbm + SCORE_WIN_PAD) <= lds
        for c in (c0, c1):
            if long_ and can_pack:
                out[c] = 'pk16_chunked'
            elif not long_ and can_pack and fits:
                out[c] = 'pk16'
            else:
                out[c] = _s32(cands[c]['nblk'], lds) + ('' if can_pack else ('+mixed' if cands[c]['eligible'] else ''))
    return out


def _trace_sweeps(traced, st, tie):
    """sw.hip:648 sw_trace_kernel over the traced pairs in the length order (the order is by the blocks of the FULL band, sw_prep)"""
    n = len(traced)
    order = sorted(range(n), key=lambda k: (-min(traced[k]['nblk'], LEN_BUCKETS - 1), tie * traced[k]['eligible'], tie * traced[k]['nblk_sub'], tie * k))
    n_long = sum(1 for c in traced if c['nblk'] > st['nb_limit'])
    lds = st['lds_res_bytes']
    out = [None] * n
    parts = [(order[:n_long], 4 if st['split_long'] else 1, st['split_long']), (order[n_long:], 4, False)]
    for members, span, chunked in parts:
        for k in range(0, len(members), span):
            item = members[k:k + span]
            packed = len(item) == 4 and all(traced[c]['eligible'] for c in item)
            if packed:
                nb = max(traced[c]['nblk_sub'] for c in item)
                room = lds >= TRACE_LONG_MIN_BYTES if chunked else 8 * 2 * round8(8 * nb + TRACE_WIN_PAD) <= lds
                packed = room and nb < STEP_GATE
            for c in item:
                if packed:
                    out[c] = ('pk16x4_chunked' if chunked else 'pk16x4') + ('+retry' if traced[c]['leaver'] else '')
                else:
                    mixed = len(item) == 4 and traced[c]['eligible'] and not all(traced[x]['eligible'] for x in item)
                    out[c] = _s32(traced[c]['nblk'], lds) + ('+mixed' if mixed else '') + ('+full' if traced[c]['leaver'] else '')
    return out


def side(case):
    """-> dict(score=[...], trace=[...], staging_score, staging_trace): per candidate of the score pass and per traced pair of the
    traceback pass its geometry (blocks, eligibility, above nb_limit) and the sweep it must take, from the lengths, the table and the
    planted diagonals alone.  `+mixed`: an eligible candidate that takes the 32-bit sweep because a member of its item is not eligible.
    A sweep is None where the two extreme orders inside a length bucket disagree (the kernel's order there is whatever its atomics give)."""
    msub = max_sub(oracle_params(case))
    max_q, max_t = max(len(s) for s in case['q']), max(len(s) for s in case['t'])
    sts, stt = staging(max_q, max_t, False), staging(max_q, max_t, True)
    cands = []
    for q, t, b in candidates(case):
        Lq, Lt = len(case['q'][q]), len(case['t'][t])
        nb = cand_blocks(Lq, Lt, b)
        cands.append(dict(q=q, t=t, bin=b, nblk=nb, eligible=fits16(Lq, Lt, msub), long=sts['split_long'] and nb > sts['nb_limit']))
    traced = []
    for p in case['pairs']:
        Lq, Lt = len(case['q'][p['q']]), len(case['t'][p['t']])
        b = p['bin']
        end_lane = (p['d_end'] - band_dlo(b)) >> 1
        sdlo, _, nbs = sub_geom(Lq, Lt, b, end_lane)
        nb = cand_blocks(Lq, Lt, b)
        leaver = not all(sdlo <= d < sdlo + 2 * SUB_LANES for d in p['diags'])
        traced.append(dict(q=p['q'], t=p['t'], bin=b, nblk=nb, nblk_sub=nbs, eligible=fits16(Lq, Lt, msub), long=nb > stt['nb_limit'], leaver=leaver))
    for rows, fn, st in ((cands, _score_sweeps, sts), (traced, _trace_sweeps, stt)):
        a, b = fn(rows, st, 1), fn(rows, st, -1)
        for row, x, y in zip(rows, a, b):
            row['sweep'] = x if x == y else None
    return dict(score=cands, trace=traced, staging_score=sts, staging_trace=stt)


# ---------------------------------------------------------------------------------------------------------------- parameter blocks
def _fill(p, case):
    """the fields a case sets, on an oracle or a native parameter block (both name them alike)"""
    par = case['params']
    if par['kind'] == 'nucl':                            # peppan_amd._native.nucleotide_params, field by field
        p.gap_open, p.gap_ext, p.n_shapes, p.base = 6, 2, 1, 4
        for s in range(4):
            p.weight[s] = 17 if s == 0 else 0
        for i in range(32):
            p.offs[0][i] = i if i < 17 else 0
            p.reduce[i] = i if i < 4 else 0xFF
        p.ungapped_min, p.xdrop, p.ext_right, p.ext_left, p.stage1_min, p.hsp_mode = 40, 16, 40, 24, 0, 1
        p.top_k, p.n_splits, p.min_id_pct, p.min_qcov_pct = 1000, 1, 0., 0.
    if 'gap' in par:
        p.gap_open, p.gap_ext = par['gap']
    tab = table(par['table'])
    if tab is not None:
        for x in range(1024):
            p.sub[x] = int(tab[x])
    for x, v in par.get('raise', ()):                    # single entries set on top of the table: ((q code, t code), value)
        p.sub[x[0] * 32 + x[1]] = v
    for code in par.get('never_seeds', ()):              # residues taken out of the reduced alphabet: no seed window may hold one
        p.reduce[code] = 0xFF
    return p


NUCL_KA = dict(dbsize=5e6, max_evalue=1e-2, ka_lambda=0.625, ka_k=0.41)      # peppan_amd._native.nucleotide_params


def oracle_params(case):
    from oracle import oracle as O
    return _fill(O.default_params(0., 0., 10, 5), case)


def native_params(case, **kw):
    """the same search for Context.search; kw: use_lds, forced32 (reserved[1]), exact (reserved2 bit 0)"""
    from peppan_amd import _native as N
    p = N.nucleotide_params() if case['params']['kind'] == 'nucl' else N.default_params(0., 0., 10, 5)
    _fill(p, case)
    p.use_lds = kw.get('use_lds', 1)
    p.reserved[1] = 1 if kw.get('forced32') else 0
    p.reserved2 = 1 if kw.get('exact') else 0
    return p


def min_scores(case):
    from oracle import oracle as O
    if case['params']['kind'] == 'nucl':
        return np.array([O.min_score(len(s), NUCL_KA['dbsize'], NUCL_KA['max_evalue'], NUCL_KA['ka_lambda'], NUCL_KA['ka_k']) for s in case['q']], dtype=np.int32)
    return np.array([O.min_score(len(s)) for s in case['q']], dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------- the builders
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _indel_pair(base, cuts, fill):
    """base with indels: cuts = [(position in base, g)], g > 0: g residues of `fill` inserted into the target, g < 0: into the query.
    -> (q, t, diagonals of the aligned stretches in order)"""
    q, t, diags, d, last = [], [], [0], 0, 0
    for pos, g in cuts:
        q.append(base[last:pos]); t.append(base[last:pos])
        (t if g > 0 else q).append(fill(abs(g)))
        d += g
        diags.append(d)
        last = pos
    q.append(base[last:]); t.append(base[last:])
    return np.concatenate(q).astype(np.uint8), np.concatenate(t).astype(np.uint8), diags


def _winning_bin(diags, dense):
    """the candidate that wins a pair: the lowest bin among its candidates whose band holds every planted diagonal (equal scores: the lowest
    bin is kept, align_oracle.c step 4).  A pair has a candidate in the bin of every diagonal that carries seeds - every bin, if it is W-rich"""
    lo, hi = min(diags), max(diags)
    bins = range(bin_of(lo) - 2, bin_of(hi) + 1) if dense else sorted(set(bin_of(d) for d in diags))
    for b in bins:
        if band_dlo(b) <= lo and hi < band_dlo(b) + BAND:
            return b
    raise ValueError('no candidate band holds the diagonals %r' % (diags,))


def _pair(case, q, t, diags, dense=False, qi=None):
    """adds one planted pair to a case.  diags: the diagonals its seeds lie on (dense: every diagonal with 12 residues of overlap - W-rich
    pairs seed everywhere); qi: the query is one the case has already"""
    if qi is None:
        case['q'].append(q)
        qi = len(case['q']) - 1
    case['t'].append(t)
    case['pairs'].append(dict(q=qi, t=len(case['t']) - 1, diags=list(diags), d_end=diags[-1], bin=_winning_bin(diags, dense), dense=dense))


def _case(name, table_='blosum62', kind='protein', **par):
    return dict(name=name, family=name.split('/')[0], q=[], t=[], pairs=[], params=dict(kind=kind, table=table_, **par))


def candidates(case):
    """the (q, t, bin) the seed stage must nominate: the bins of the planted diagonals of every pair (of every diagonal with an overlap of at
    least 12 residues - the shorter seed shape - where the pair is W-rich).  The host test holds the oracle's candidate count and cell total to it."""
    out = set()
    for p in case['pairs']:
        Lq, Lt = len(case['q'][p['q']]), len(case['t'][p['t']])
        ds = range(-(Lq - 12), Lt - 12 + 1) if p['dense'] else p['diags']
        out |= set((p['q'], p['t'], bin_of(d)) for d in ds)
    return sorted(out)


def _rand(rng, n, alphabet=AA20):
    return alphabet[rng.integers(0, len(alphabet), n)].astype(np.uint8)


def _len_for_blocks(nb, g, rem=8):
    """Lq of a pair (Lq, Lq + g) in the band of diagonal 0 with nb blocks: 2 * Lq - 1 + g steps = 16 * nb - rem"""
    steps = 16 * nb - rem
    L = (steps + 1 - g) // 2
    assert cand_blocks(L, L + g, bin_of(0)) == nb, (nb, g, L)
    return L


def _random_pair(case, rng, L, g, pos=None, alphabet=AA20, transposed=False, **kw):
    """a random sequence of L residues against itself with g random residues inserted (into the target; into the query when transposed - the
    target then gets nothing, and the pair lies on the diagonals 0 and -g)"""
    base = _rand(rng, L, alphabet)
    q, t, diags = _indel_pair(base, [(L // 2 if pos is None else pos, -g if transposed else g)], lambda n: _rand(rng, n, alphabet))
    _pair(case, q, t, diags, **kw)


def _w_rich(rng, L, every=97):
    """W with another residue every `every` positions (the same in both members of a pair): scores stay within a few hundred of L * W/W"""
    s = np.full(L, W, dtype=np.uint8)
    at = np.arange(every // 2, L, every)
    s[at] = _rand(rng, len(at), NOT_W)
    return s


def _variant(base, pos, g, fill):
    """a target for the query `base`: g > 0: g residues of `fill` inserted at pos, g < 0: the -g residues from pos on left out.
    -> (target, the diagonals of the two aligned stretches)"""
    if g > 0:
        return np.concatenate([base[:pos], fill(g), base[pos:]]).astype(np.uint8), [0, g]
    return np.concatenate([base[:pos], base[pos - g:]]).astype(np.uint8), [0, g]


def _one_query(case, base, variants, fill, dense=True):
    """one query and one target per (pos, g) of variants: as many (q, t) pairs, each with one candidate selected and traced"""
    case['q'].append(base)
    for pos, g in variants:
        t, diags = _variant(base, pos, g, fill)
        _pair(case, base, t, diags, dense=dense, qi=len(case['q']) - 1)


def _anchored(rng, L):
    """W with four anchors of 20 residues other than W at L/5 .. 4L/5"""
    s = np.full(L, W, dtype=np.uint8)
    for k in (1, 2, 3, 4):
        s[k * L // 5:k * L // 5 + 20] = _rand(rng, 20, NOT_W)
    return s


def _eligibility_cases():
    """fits16 looks at min(Lq, Lt) and the largest table entry.  A W-rich query against four targets that carry an insertion each (all at least
    as long as the query: min = Lq) is an item of four of the traceback pass, and its candidates - a W-rich pair seeds on every diagonal - are
    pairs of the score pass, all on one side of the rule; the scores stand a few hundred below Lq * W/W"""
    out = []
    ins = lambda L: [(L // 2 + 5, 7), (L // 3, 3), (2 * L // 3, 11), (L // 2 - 40, 5)]
    fill = lambda n: np.full(n, P_, np.uint8)
    # BLOSUM62: min(Lq, Lt) <= 2961 is eligible (2961 * 11 + 192 = 32763 < 32767 <= 2962 * 11 + 192); 3100: scores above the half word.
    # 3 000 W against 3 000 W is nine million seed hits a shape; here W is taken out of the reduced alphabet and four anchors of 20 other
    # residues, one on either side of every insertion, carry the seeds: one candidate a pair
    for L in (2960, 2961, 2962, 2963, 3100):
        c = _case('eligibility/blosum62_w_rich_%d' % L, never_seeds=(W,))
        _one_query(c, _anchored(_rng(c['name']), L), ins(L), fill, dense=False)
        out.append(c)
    # W/W raised to 127: min(Lq, Lt) <= 256 is eligible (256 * 127 + 192 = 32704 < 32767 <= 257 * 127 + 192); 300: scores above the half word
    for L in (255, 256, 257, 258, 300):
        c = _case('eligibility/w127_w_rich_%d' % L, **{'raise': (((W, W), 127),)})
        _one_query(c, _w_rich(_rng(c['name']), L, 61), ins(L), fill)
        out.append(c)
    # the same with ONE ineligible pair in the item: a query one residue beyond the limit, three targets that lack a few residues (min = Lt, eligible)
    # and one that carries an insertion (min = Lq)
    for name, L, every, kw in (('blosum62', 2962, 97, {'raise': (), 'never_seeds': (W,)}), ('w127', 257, 61, {'raise': (((W, W), 127),)})):
        c = _case('eligibility/%s_w_rich_item_with_one_ineligible' % name, **kw)
        base = _w_rich(_rng(c['name']), L, every) if kw['raise'] else _anchored(_rng(c['name']), L)
        _one_query(c, base, [(L // 2 + 5, 7), (L // 3, -3), (2 * L // 3, -6), (L // 2 - 40, -5)], fill, dense=bool(kw['raise']))
        c['order_dependent'] = True                       # its candidates of equal block count differ in eligibility: which ones share a wavefront is the kernel's choice
        out.append(c)
    # 2 .. 5 one-candidate pairs under W/W = 127, exactly one of them not eligible (257 residues: ordinary residues, the rule looks at the
    # length and the table only); it is the longest, so it opens the order and shares its item with eligible candidates in both passes
    for n in (2, 3, 4, 5):
        c = _case('eligibility/mixed_%d_one_ineligible' % n, **{'raise': (((W, W), 127),)})
        rng = _rng(c['name'])
        _random_pair(c, rng, 257, 9, alphabet=NOT_W)
        for k in range(n - 1):
            _random_pair(c, rng, 256 - 8 * k, 5 + k, alphabet=NOT_W)
        out.append(c)
    return out


HALF_WORD_GAPS = ((11, 1), (0, 1), (255, 1), (1, 255), (255, 255))


def _half_word_cases():
    """W/W = 127, -128 elsewhere: only W/W columns score, every other column costs 128, so walking THROUGH an insertion of g residues on one
    diagonal costs 255 a residue (the column and the W it displaces) where the table leaves the flanks shift-invariant (all W), and 255 for
    every residue other than W in a flank that the shift puts out of register.  A gap of g costs open + g * extend.  The query is 256
    residues, the largest eligible length; each flank carries as many P at uneven distances as make the gap of the LONG insertion the
    cheaper way through (none where extend = 1 and the insertion alone decides).  Four targets a query: a short (1) and a long insertion
    (19; 4 where extend = 255, beyond which no score near the half word is left), each at two places"""
    out = []
    for go, ge in HALF_WORD_GAPS:
        short, long_ = 1, (19 if ge == 1 else 4)
        need = max(0 if go + g * ge < 255 * g else (go + g * ge) // 255 + 1 for g in (short, long_))
        c = _case('half_word_edge/gap_%d_%d' % (go, ge), 'edge', gap=(go, ge))
        base = np.full(256, W, dtype=np.uint8)
        for flank in (0, 128):
            base[flank + np.array([9, 23, 31, 52, 59, 77, 90, 101, 118])[:need]] = P_
        _one_query(c, base, [(128, short), (128, long_), (107, short), (140, long_)], lambda n: np.full(n, A_, np.uint8))
        out.append(c)
    c = _case('half_word_edge/gap_11_1_beyond_the_half_word', 'edge', gap=(11, 1))      # 300 W: not eligible, scores of 38 000
    _one_query(c, np.full(300, W, dtype=np.uint8), [(150, 1), (150, 19), (107, 1), (140, 19)], lambda n: np.full(n, A_, np.uint8))
    out.append(c)
    return out


BYSTANDER = 2000                 # a sequence on both sides that shares nothing with the pairs: longest query + longest target >= 1872 / 912


def _bystander(case):
    """a long sequence of X on either side: it seeds nothing (X has no reduced letter) and only raises the set's longest lengths, which is
    what sizes the staging area and switches split_long on"""
    case['q'].append(np.full(BYSTANDER, 23, np.uint8)); case['t'].append(np.full(BYSTANDER, 23, np.uint8))


def _block_case(name, blocks, bystander, gs=(5, 9, 13, 17)):
    """four one-candidate pairs (an item of the traceback pass, two of the score pass) with the given block counts"""
    c = _case(name)
    rng = _rng(name)
    for nb, g in zip(blocks, gs):
        _random_pair(c, rng, _len_for_blocks(nb, g), g)
    if bystander:
        _bystander(c)
    return c


def _staging_cases():
    out = []
    sc, tr = staging(2 * BYSTANDER, 0, False), staging(2 * BYSTANDER, 0, True)
    # nb_limit of the traceback pass (57 at 8 KiB) and of the score pass (117), the `fits` test of the score pass (118 blocks at 8 KiB);
    # the sub-band of a pair never has more blocks than its band (test_sub_band_never_outgrows_its_band), so the fourth limit - one block more -
    # is covered by the same block counts: nb_limit + 1 is the count that still fits the staging area
    fits_limit = (LDS_CAP // 8 - SCORE_WIN_PAD) // 8
    around = sorted(set(range(tr['nb_limit'] - 2, tr['nb_limit'] + 4)) | set(range(sc['nb_limit'] - 2, fits_limit + 3)))
    for nb in around:
        for by in (False, True):                           # (pairs of 117 blocks and more switch split_long on by themselves: side() says what each case is)
            out.append(_block_case('staging/four_pairs_of_%d_blocks%s' % (nb, '_long_bystander' if by else ''), [nb] * 4, by))
    # items that straddle a limit: the order is by decreasing block count, so the first item / pair holds the longer ones
    out.append(_block_case('staging/trace_limit_straddled', [tr['nb_limit'] + 2, tr['nb_limit'] + 1, tr['nb_limit'], tr['nb_limit'] - 1], True))      # two and two: tails on both sides
    out.append(_block_case('staging/trace_limit_four_and_four', [tr['nb_limit'] + k for k in (2, 2, 1, 1, 0, 0, -1, -1)], True, gs=(5, 7, 9, 11, 13, 15, 17, 19)))
    out.append(_block_case('staging/score_limit_straddled', [sc['nb_limit'] + 2, sc['nb_limit'] + 1, sc['nb_limit'], sc['nb_limit'] - 1], True))
    c = _case('staging/five_long_three_short')             # 5 above the traceback limit: an item of four in chunks and a tail of one in 32 bits
    rng = _rng(c['name'])
    for k, nb in enumerate([tr['nb_limit'] + x for x in (9, 8, 7, 6, 5, -5, -5, -5)]):
        _random_pair(c, rng, _len_for_blocks(nb, 4 + k), 4 + k)
    _bystander(c)
    out.append(c)
    # chunk multiples: k chunks and k chunks + 1 block.  Traceback pass: 58 blocks a chunk, k = 1, 2, 3.  Score pass: 38 blocks a chunk in the long
    # launch, which takes pairs above 117 blocks only - one, two and three chunks never reach it (built all the same: side() shows them in the plain
    # sweep), so k = 4, 5, 6 are the first multiples the chunked score sweep sees
    for which, chunk, ks in (('trace', tr['chunk'], (1, 2, 3)), ('score', sc['chunk'], (1, 2, 3, 4, 5, 6))):
        for k in ks:
            for extra in (0, 1):
                nb = k * chunk + extra
                out.append(_block_case('staging/%s_chunks_%d_plus_%d' % (which, k, extra), [nb] * 4, True))
    return out


NT4 = np.arange(4, dtype=np.uint8)


def _step_counter_cases():
    """nucleotide pairs under reward 1: eligible up to 32 574 bases, so only the gate `blocks < 2040` of the four-candidate sweep decides.  One
    query and four targets a search (one item of the long launch), each target with an insertion of its own length g: 2 * Lq - 1 + g steps.
    The item's block count is its longest member's"""
    out = []
    for name, Lq, gs, top in (('step_counter/item_of_2038', 16300, (3, 5, 7, 9), 2038), ('step_counter/item_of_2039', 16300, (3, 5, 7, 11), 2039),
                              ('step_counter/item_of_2040', 16300, (3, 5, 7, 27), 2040), ('step_counter/item_of_2041', 16308, (3, 5, 7, 27), 2041),
                              ('step_counter/item_of_20000_bases', 20000, (3, 5, 7, 9), 2501)):
        c = _case(name, 'nucl1', 'nucl')
        rng = _rng(name)
        _one_query(c, _rand(rng, Lq, NT4), [((k + 1) * Lq // 5, g) for k, g in enumerate(gs)], lambda n: _rand(rng, n, NT4), dense=False)
        assert max(cand_blocks(Lq, Lq + g, bin_of(0)) for g in gs) == top, name
        out.append(c)
    return out


def _tail_cases():
    out = []
    for n in (1, 2, 3, 5, 6, 7):
        for inel in (False, True):
            c = _case('tails/%d_active%s' % (n, '_one_ineligible' if inel else ''), **{'raise': (((W, W), 127),)})
            rng = _rng(c['name'])
            for k in range(n):
                L = 270 if (inel and k == 0) else 250 - 9 * k
                _random_pair(c, rng, L, 4 + k, alphabet=NOT_W)
            out.append(c)
    return out


def _sub_band_cases():
    """two flanks of 150 residues around g extra residues: the alignment starts on diagonal 0 and ends on diagonal g (-g transposed); the sub-band
    is the 64 diagonals around the end: [g - 32, g + 31] for an even g in the band of diagonal 0, so g <= 33 stays inside and g >= 34 needs the full
    band; a transposed pair is won by the band one bin lower, [-96, 31], where the sub-band around -g is [-g - 32, -g + 31] for an even g and
    one lower for an odd one: g <= 30 stays, g >= 31 leaves"""
    out = []
    leave = (36, 40, 60, 34)
    for n_leave in (0, 1, 3, 4):
        for tp in (False, True):
            c = _case('sub_band_exit/%d_of_4_leave%s' % (n_leave, '_transposed' if tp else ''))
            rng = _rng(c['name'])
            stay = (30, 29, 30, 28) if tp else (30, 33, 30, 33)
            gs = list(leave[:n_leave]) + list(stay[:4 - n_leave])
            for k, g in enumerate(gs):
                _random_pair(c, rng, 300 + 6 * k, g, pos=150 + 3 * k, transposed=tp)
            out.append(c)
    for tp in (False, True):                               # every g once more, straight and transposed: one pair a search (a tail of one, the 32-bit sweep)
        for g in (30, 31, 33, 34, 36, 40, 60):
            c = _case('sub_band_exit/alone_g%d%s' % (g, '_transposed' if tp else ''))
            _random_pair(c, _rng(c['name']), 300, g, pos=150, transposed=tp)
            out.append(c)
    c = _case('sub_band_exit/long_enough_for_the_chunked_launch')       # flanks of 500: 63 blocks, four pairs, two of them leave
    rng = _rng(c['name'])
    for g in (40, 30, 60, 33):
        _random_pair(c, rng, 1000, g, pos=500)
    out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(_eligibility_cases() + _half_word_cases() + _staging_cases() + _step_counter_cases() + _tail_cases() + _sub_band_cases())


@functools.lru_cache(maxsize=None)
def full_matrix_scores():
    """(query bytes, target bytes, table, gap costs) -> the optimum of the whole matrix (oracle/full_sw.py), for every planted pair, each
    distinct pair once"""
    from oracle import full_sw as F
    out = {}
    for fam in sorted(set(c['family'] for c in cases())):
        if fam == 'step_counter':
            # pairs of 16 000 bases: fullsw_align keeps the whole matrix (gigabytes each); score_matrix keeps a column and takes up to 32 targets
            # of a query for the price of one, so every query of the family meets every target of the family in one call
            group = [c for c in cases() if c['family'] == fam]
            qs = [c['q'][0] for c in group]
            ts = [t for c in group for t in c['t']]
            m = F.score_matrix(qs, ts, oracle_params(group[0]))
            at = 0
            for k, c in enumerate(group):
                for pr in c['pairs']:
                    out[pair_key(c, pr)] = int(m[k, at + pr['t']])
                at += len(c['t'])
            continue
        for c in cases():
            if c['family'] == fam:
                p = oracle_params(c)
                for pr in c['pairs']:
                    if pair_key(c, pr) not in out:
                        out[pair_key(c, pr)] = int(F.align(c['q'][pr['q']], c['t'][pr['t']], p)[0].score)
    return out


def pair_key(case, pr):
    par = case['params']
    return (case['q'][pr['q']].tobytes(), case['t'][pr['t']].tobytes(), par['table'], par.get('raise', ()), par.get('gap', None), par['kind'])


@functools.lru_cache(maxsize=None)
def oracle_results():
    """name -> (hits, cigar, stats, trace_counts) of oracle.search on every case, computed once and shared"""
    from oracle import oracle as O
    out = {}
    for c in cases():
        O.trace_counts(True)
        h, cg, st = O.search(c['q'], c['t'], oracle_params(c), min_scores=min_scores(c))
        out[c['name']] = (h, cg, st, O.trace_counts(True))
    return out
