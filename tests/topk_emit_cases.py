"""Searches built where topk_emit (trace.hip: top-k, compaction, hit records, CIGAR runs and single linkage in one launch) can go wrong: a tile
of 256 selected pairs, its look-back over the tiles in front of it, the records and runs it stages, the staging area of pack_out behind it.
No GPU in here: the builders use the oracle alone (the counters of its searches say where a case stands), tests/test_topk_emit_cases.py
proves every case is where its name says, tests/test_gpu_topk_emit.py holds the kernels to the oracle on them.

A case: dict(name, q, t - lists of residue-code arrays -, par - what the parameter blocks are made of -, group - None or the arguments of
pep_set_grouping -, and what the builder planted, for the host test)."""
import functools
import zlib

import numpy as np

TILE = 256                        # selected pairs per tile of topk_emit
BAND = 128                        # diagonals of a band
AA = np.frombuffer(b'ARNDCQEGHILKMFPSTWYV', dtype=np.uint8) - 65
FIELDS = ('q', 't', 'q_start', 'q_end', 't_start', 't_end', 'score', 'nm', 'n_ident', 'aln_len', 'cigar_runs', 'bin', 'cigar_off', 'cells')
NEVER = 1e-200                    # max_evalue at which no pair of these sets reaches its query's score threshold


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def band_dlo(b):
    return int(b) * 64 - (1 << 23) - 32


# ---------------------------------------------------------------------------------------------------------------- cells of a band
def cells_loop(Lq, Lt, dlo):
    """in-matrix cells of the diagonals dlo .. dlo + 127 (d = j - i) of an Lq x Lt matrix, one diagonal at a time (what emit's lanes add up)"""
    n = 0
    for d in range(max(dlo, -(Lq - 1)), min(dlo + BAND - 1, Lt - 1) + 1):
        n += min(Lq - 1, Lt - 1 - d) - max(0, -d) + 1
    return n


def cells_closed(Lq, Lt, dlo):
    """the same in closed form (pep_band_cells of common.h, restated): diagonal d holds min(Lq, Lt - d) + min(0, d) cells"""
    dl, dh = max(dlo, -(Lq - 1)), min(dlo + BAND - 1, Lt - 1)
    if dl > dh:
        return 0
    tri = lambda a, b: 0 if b < a else (a + b) * (b - a + 1) // 2
    k = Lt - Lq
    flat_hi, slope_lo = min(dh, k), max(dl, k + 1)
    total = (flat_hi - dl + 1) * Lq if flat_hi >= dl else 0
    if slope_lo <= dh:
        total += (dh - slope_lo + 1) * Lt - tri(slope_lo, dh)
    return total + tri(dl, min(dh, -1))


def cells_closed_grid(lq, lt, dlo):
    """cells_closed over numpy arrays (int64), for the exhaustive comparison"""
    lq, lt, dlo = (np.asarray(x, dtype=np.int64) for x in (lq, lt, dlo))
    dl, dh = np.maximum(dlo, -(lq - 1)), np.minimum(dlo + BAND - 1, lt - 1)
    tri = lambda a, b: np.where(b < a, 0, (a + b) * (b - a + 1) // 2)
    k = lt - lq
    flat_hi, slope_lo = np.minimum(dh, k), np.maximum(dl, k + 1)
    total = np.where(flat_hi >= dl, (flat_hi - dl + 1) * lq, 0)
    total = total + np.where(slope_lo <= dh, (dh - slope_lo + 1) * lt - tri(slope_lo, dh), 0)
    total = total + tri(dl, np.minimum(dh, -1))
    return np.where(dl > dh, 0, total)


def cells_loop_grid(lq, lt, dlo):
    """cells_loop over numpy arrays: the 128 diagonals one after another"""
    lq, lt, dlo = (np.asarray(x, dtype=np.int64) for x in (lq, lt, dlo))
    dl, dh = np.maximum(dlo, -(lq - 1)), np.minimum(dlo + BAND - 1, lt - 1)
    total = np.zeros(np.broadcast(lq, lt, dlo).shape, dtype=np.int64)
    for x in range(BAND):
        d = dlo + x
        total += np.where((d >= dl) & (d <= dh), np.minimum(lq - 1, lt - 1 - d) - np.maximum(0, -d) + 1, 0)
    return total


def clipping(hit, q, t):
    """(the band of a hit leaves the matrix below its first diagonal - at the left / top -, beyond its last)"""
    dlo = band_dlo(hit['bin'])
    return dlo < -(len(q[int(hit['q'])]) - 1), dlo + BAND - 1 > len(t[int(hit['t'])]) - 1


# ---------------------------------------------------------------------------------------------------------------- parameter blocks
def native_params(case):
    from peppan_amd import _native as N
    par = case['par']
    if par['kind'] == 'nucl':
        return N.nucleotide_params(par['min_id'], par['min_qcov'], top_k=par['top_k'], hsp_mode=par['hsp_mode'])
    return N.default_params(par['min_id'], par['min_qcov'], par['top_k'], par['n_splits'], max_evalue=par.get('max_evalue', 1.))


def _oracle_search(q, t, par, top_k=None, filters=True):
    """the oracle on (q, t) with the case's parameters; top_k / filters: the same search with another cut-off, without the identity and cover filters.
    par['groups'] (a batch of reference sets in one search, pep_set_target_groups: the sizes of the sets, which follow each other in t): every set
    searched alone and the tables merged - what the batch is defined to give"""
    from oracle import oracle as O
    if par.get('groups'):
        one = {k: v for k, v in par.items() if k != 'groups'}
        parts, first = [], 0
        for n in par['groups']:
            parts.append((first, _oracle_search(q, t[first:first + n], one, top_k, filters)))
            first += n
        assert first == len(t)
        hits = np.concatenate([h for _, (h, _, _) in parts])
        hits['t'] += np.concatenate([np.full(len(h), f, dtype=np.uint32) for f, (h, _, _) in parts])
        runs = np.concatenate([c for _, (_, c, _) in parts])
        src = hits['cigar_off'] + np.concatenate([np.full(len(h), x, dtype=np.uint64) for x, (_, (h, _, _)) in
                                                   zip(np.cumsum([0] + [len(c) for _, (_, c, _) in parts[:-1]]), parts)]).astype(np.uint64)
        order = np.lexsort((hits['t'], hits['q']))
        hits, src = hits[order], src[order]
        off = np.concatenate([[0], np.cumsum(hits['cigar_runs'], dtype=np.uint64)]).astype(np.uint64)
        cig = np.concatenate([runs[int(a):int(a) + int(n)] for a, n in zip(src, hits['cigar_runs'])] + [np.zeros(0, np.uint32)]).astype(np.uint32)
        hits['cigar_off'] = off[:-1]
        return hits, cig, {k: sum(st[k] for _, (_, _, st) in parts) for k in parts[0][1][2]}
    if par['kind'] == 'nucl':
        from peppan_amd import _native as N
        n = N.nucleotide_params(par['min_id'] if filters else 0., par['min_qcov'] if filters else 0., top_k=par['top_k'] if top_k is None else top_k, hsp_mode=par['hsp_mode'])
        ms = np.array([O.min_score(len(s), n.dbsize, n.max_evalue, n.ka_lambda, n.ka_k) for s in q], dtype=np.int32)
        return O.search(q, t, O.params_from(n), min_scores=ms)
    p = O.default_params(par['min_id'] if filters else 0., par['min_qcov'] if filters else 0., par['top_k'] if top_k is None else top_k, par['n_splits'])
    return O.search(q, t, p, max_evalue=par.get('max_evalue', 1.))


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(hits, cigar, stats, trace counters) of the oracle on a case: computed once, shared, never changed"""
    from oracle import oracle as O
    case = CASES[name]()
    O.trace_counts(True)
    h, cg, st = _oracle_search(case['q'], case['t'], case['par'])
    tc = O.trace_counts(True)
    for a in (h, cg):
        a.setflags(write=False)
    return h, cg, st, tc


@functools.lru_cache(maxsize=None)
def oracle_selected(name):
    """the selected pairs of a case in the order the kernels hold them - (q, t, band) -, which are the oracle's hits once nothing filters and
    nothing cuts: the identity and cover filters at 0, top_k beyond every count"""
    case = CASES[name]()
    h, _, st = _oracle_search(case['q'], case['t'], case['par'], top_k=10 ** 6, filters=False)
    assert len(h) == st['tracebacks'], (name, len(h), st)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def oracle_passing(name):
    """the pairs of a case that pass its filters, before top-k: the oracle's hits with top_k beyond every count"""
    case = CASES[name]()
    h, _, _ = _oracle_search(case['q'], case['t'], case['par'], top_k=10 ** 6)
    h.setflags(write=False)
    return h


# ---------------------------------------------------------------------------------------------------------------- building blocks
def _families(name, n, length=(50, 120), family=4, sub=0.25, indel=0.7):
    from peppan_amd import synth
    return synth.make_proteins(n, length=length, seed=zlib.crc32(name.encode()) & 0xFFFF, family=family, sub=sub, indel=indel)


def _random(rng, n, length, alphabet=AA):
    return [np.ascontiguousarray(alphabet[rng.integers(0, len(alphabet), int(rng.integers(length[0], length[1] + 1)))], dtype=np.uint8) for _ in range(n)]


def trim(pool, targets, singles, par, n_sel):
    """queries for exactly n_sel selected pairs: the longest prefix of `pool` whose search selects at most n_sel pairs (queries are independent of
    each other, so the count only grows with the prefix), then as many of `singles` - sequences that select one pair each, themselves among the
    targets - as are missing.  The oracle's tracebacks counter decides."""
    count = lambda qs: _oracle_search(qs, targets, par)[2]['tracebacks'] if qs else 0
    lo, hi = 0, len(pool)                                  # count(pool[:lo]) <= n_sel
    assert count(pool) >= n_sel or count(pool) + len(singles) >= n_sel
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if count(pool[:mid]) <= n_sel:
            lo = mid
        else:
            hi = mid - 1
    q = list(pool[:lo])
    q += singles[:n_sel - count(q)]
    assert count(q) == n_sel, (count(q), n_sel)
    return q


def indel_pair(base, period, fill):
    """base against itself with one residue inserted every `period` residues, in the target and in the query in turns: an alignment of
    2 * (insertions) + 1 runs that never leaves the three central diagonals"""
    q, t, n = [], [], 0
    for pos in range(0, len(base), period):
        q.append(base[pos:pos + period]); t.append(base[pos:pos + period])
        if pos + period < len(base):
            (t if n % 2 == 0 else q).append(fill(1))
            n += 1
    return np.concatenate(q).astype(np.uint8), np.concatenate(t).astype(np.uint8), n


def grouping(n_q, n_t, q_base, per_node):
    """pep_set_grouping's arguments: the queries are the nodes q_base .., `per_node` consecutive targets share a node"""
    n_nodes = q_base + max(n_q, (n_t + per_node - 1) // per_node) + 3
    return dict(n_nodes=n_nodes, q_base=q_base, node_of_target=(np.arange(n_t, dtype=np.uint32) // per_node).astype(np.uint32))


def labels_of(n_nodes, q_base, node_of_target, hits):
    """single linkage over the edges (hit.q + q_base, node of hit.t) in plain Python: every node's label is the smallest node of its component"""
    parent = list(range(n_nodes))

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for h in hits:
        a, b = root(int(h['q']) + q_base), root(int(node_of_target[int(h['t'])]))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([root(x) for x in range(n_nodes)], dtype=np.uint32)


PROT = dict(kind='prot', min_id=0., min_qcov=0., top_k=10, n_splits=5)


# ---------------------------------------------------------------------------------------------------------------- the cases
def _sized(n_sel, par=None, group=None):
    """n_sel selected pairs out of a family set (members select each other: a few pairs per query)"""
    def build():
        name = 'sel_%d' % n_sel
        rng = _rng(name)
        p = dict(PROT, **(par or {}))
        fam = _families('sized', 600)
        singles = _random(rng, 8, (70, 90))
        targets = fam + singles
        if n_sel == 0:
            q, p = fam[:40], dict(p, max_evalue=NEVER)      # candidates, and not one of them reaches its threshold
        else:
            q = trim(fam, targets, singles, p, n_sel)
        g = grouping(len(q), len(targets), *group) if group else None
        return dict(name=name, q=q, t=targets, par=p, group=g, n_sel=n_sel)
    return build


def _straddle(n_splits):
    """one query's selected pairs lie on both sides of the boundary between tile 0 and tile 1, more of them pass in every competition class than
    top_k (2) keeps, and three exact copies of every relative tie in score: the cut goes through them and the target index decides.  The relatives sit at the end of the
    target list, copy c of relative v at offset v + 10 c: the copies of a relative share their class whether n_splits is 1 or 5."""
    def build():
        name = 'straddle_%d' % n_splits
        rng = _rng('straddle')
        p = dict(PROT, top_k=2, n_splits=n_splits)
        fam = _families('straddle', 400)
        root = _random(rng, 1, (110, 110))[0]
        variants = []
        for v in range(10):
            m = root.copy()
            pos = rng.choice(len(m), 3 + v, replace=False)
            m[pos] = AA[rng.integers(0, 20, len(pos))]
            variants.append(m)
        singles = _random(rng, 8, (70, 90))
        targets = fam + singles
        targets += _random(rng, -len(targets) % 5, (70, 90))                      # the relatives start at a multiple of 5 (a random target nobody asks for)
        first = len(targets)
        targets = targets + [variants[x % 10] for x in range(30)]
        prefix = trim(fam, targets, singles, p, TILE - 12)                          # 244 pairs in front of the query: its 30 pairs are the slots 244 .. 273
        return dict(name=name, q=prefix + [root], t=targets, par=p, group=grouping(len(prefix) + 1, len(targets), 5, 4), star=len(prefix), first=first)
    return build


def _keep_none():
    """257 selected pairs and an identity filter nobody passes: both tiles keep nothing"""
    c = _sized(257)()
    return dict(c, name='keep_none', par=dict(c['par'], min_id=101.), group=grouping(len(c['q']), len(c['t']), 2, 3))


def _keep_all():
    """513 selected pairs, no filter, no cut: the first two tiles keep all of their 256 pairs"""
    c = _sized(513)()
    return dict(c, name='keep_all', par=dict(c['par'], top_k=10 ** 6, n_splits=1))


def _long_cigar():
    """one tile that holds a hit of more CIGAR runs than the tile has threads (an insertion every 8 residues, query and target in turns), exact copies
    (one run, settled by rule 5a without a traceback) and family members with indels (traced): the arena is filled from both paths"""
    rng = _rng('long_cigar')
    fam = _families('long_cigar', 60, length=(80, 200))
    base = _random(rng, 1, (1400, 1400))[0]
    lq, lt, n_ins = indel_pair(base, 8, lambda n: AA[rng.integers(0, 20, n)])
    q = fam[:30] + [lq] + fam[30:40]
    t = fam + [lt]
    return dict(name='long_cigar', q=q, t=t, par=dict(PROT), group=None, long_q=30, long_t=len(fam), n_ins=n_ins)


def _short():
    """sequences shorter than a band is wide (20 .. 120 residues, many shorter than 64): a motif against the motif inside random flanks, so that the
    alignment's diagonal - and with it the band - moves about: bands that leave the matrix at the left / top, beyond the last column, at both ends"""
    rng = _rng('short')
    q, t = [], []
    for i in range(90):
        m = _random(rng, 1, (20, 120))[0]
        flanked = np.concatenate([_random(rng, 1, (0, 100))[0], m, _random(rng, 1, (0, 100))[0]]).astype(np.uint8)
        q.append(m if i % 2 else flanked)
        t.append(flanked if i % 2 else m)
    return dict(name='short', q=q, t=t, par=dict(PROT), group=None)


def _nucl_pool(name, n):
    from peppan_amd import synth
    from oracle import oracle as O
    _, seqs = synth.make_genes(n, 0, seed=zlib.crc32(name.encode()) & 0xFFFF)
    return [O.nt_codes(s.decode()) for s in seqs]


def _hsp(mode):
    """the nucleotide tool's configuration (every band that reaches the threshold is traced; mode 2: BLAST's culling, top_k counts subjects) at 257
    selected bands, top_k 1.  The last query meets a target that holds it twice, 400 diagonals apart: two bands of one (q, t) with one score - the
    band order decides which of them mode 1 keeps"""
    def build():
        name = 'hsp_%d' % mode
        rng = _rng(name)
        par = dict(kind='nucl', min_id=60., min_qcov=10., top_k=1, hsp_mode=mode)
        nt = np.arange(4, dtype=np.uint8)
        pool = _nucl_pool('hsp', 200)
        singles = _random(rng, 8, (150, 200), nt)
        twice = _random(rng, 1, (200, 200), nt)[0]
        comp = lambda c: (3 - c[::-1]).astype(np.uint8)
        fwd = pool + singles + [np.concatenate([twice, _random(rng, 1, (200, 200), nt)[0], twice]).astype(np.uint8)]
        targets = fwd + [comp(c) for c in fwd]
        head = trim(pool, targets, singles, par, TILE + 1 - 2)
        return dict(name=name, q=head + [twice], t=targets, par=par, group=None, n_sel=TILE + 1, twice=(len(head), len(fwd) - 1))
    return build


def _batch():
    """two reference sets in one search (pep_set_target_groups): every family has two members in either set, a competition class belongs to one
    set, top_k 1 - at 257 selected pairs"""
    rng = _rng('batch')
    fam = _families('sized', 600)
    singles = _random(rng, 8, (70, 90))
    targets = fam[0::2] + fam[1::2] + singles
    p = dict(PROT, top_k=1, groups=[len(fam[0::2]), len(fam[1::2]) + len(singles)])
    return dict(name='batch', q=trim(fam, targets, singles, p, TILE + 1), t=targets, par=p, group=None, n_sel=TILE + 1)


CASES = {'sel_0': _sized(0, group=(3, 2)), 'sel_1': _sized(1, group=(0, 1)), 'sel_255': _sized(255), 'sel_256': _sized(256, group=(7, 3)),
         'sel_257': _sized(257, par=dict(top_k=1, n_splits=1)), 'sel_513': _sized(513, par=dict(min_id=45., min_qcov=25.), group=(11, 5)),
         'straddle_1': _straddle(1), 'straddle_5': _straddle(5), 'keep_none': _keep_none, 'keep_all': _keep_all, 'long_cigar': _long_cigar,
         'short': _short, 'hsp_1': _hsp(1), 'hsp_2': _hsp(2), 'batch': _batch}
CASES = {k: functools.lru_cache(maxsize=None)(v) for k, v in CASES.items()}
