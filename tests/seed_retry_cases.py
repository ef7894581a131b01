"""Inputs that make the seed stage (peppan_amd/csrc/seeds.hip, pep_find_candidates) run again - the loop `for (int attempt = 0; attempt < 8; ++attempt)` - and an
independent count of the seed statistics.  tests/test_seed_retry_cases_host.py proves from counts alone which retries every case must take,
tests/test_gpu_seed_retry.py compares the GPU with the oracle and with these counts on each.

The three retries and what forces them (the caps are constants of this module; the host test pins their text in seeds.hip):

    slab   a coarse index bucket holds more than PART_CAP = 5 632 entries -> the index is built again by count -> scan -> fill.  Only with the partition
           build, i.e. bucket_bits = ceil(log2(2 * packed query bytes)) >= 16.
    hits   one shape appends more raw seed hits than hit_cap = max(2^22, 2 * packed target bytes) -> hit_cap *= 4
    set    more candidates than list_cap = 2^(table_bits - 1), table_bits = max(20, ceil(log2(64 * queries))) -> table_bits += 2

Why the predictions are sound.  A key that occurs more than PART_CAP times among the query's seeds of one shape lies in ONE coarse bucket whatever the
hash is, so idx_slab must raise its flag or write outside its slab.  More appended hits than hit_cap means some append position g >= hit_cap, so the
matcher must raise its flag.  More candidates than list_cap means counters[0] > list_cap.  These are SUFFICIENT conditions: what a case must take is
proved; the conditions a case must NOT meet are clear by a factor MARGIN = 1.5 at least (for the slab that says: no single key comes near the slab's
capacity - that a coarse bucket collects several keys is the hash's business and not predicted here; nothing on the GPU side asserts that a slab did
NOT overflow).

seed_counts() is the definition in the header comment of seeds.hip and in pep_search_params, nothing of the device's hash, buckets or filter: for every
shape, every window that lies wholly inside one sequence and meets no letter with reduce == 0xFF has the key sum reduce[r[p + offs[i]]] * base**i;
query_seeds / target_seeds count the windows of either side, raw_hits = sum over keys of (count in q) * (count in t).  The library's seed_hits includes
the hits of a gene against itself that a self-search counts and drops, so raw_hits is compared as it is.  For the nucleotide tool the seeds are the
exact 17-mers: seed_match_stride looks 14-mers up at a stride of four, but its seed_hits are the 17-mer hits and its target_seeds the target positions
that start a 17-mer of the four bases - both defined without the look-up word, both asserted.  Its query_seeds is the number of entries of the index,
which holds the 14-mer look-up words: an implementation detail, NOT asserted for that tool.

motif_family(): proteins of about 40 residues, 12 to 15 residues either side of a motif whose positions are drawn independently per sequence from
KREDQN - one letter (0) of the reduced alphabet, so every window inside the motif has the same key in every sequence, while the residues differ and the
ungapped score of a chance pair stays far below ungapped_min = 55.  The flanks are drawn from the fourteen letters of the other classes, so a motif of
15 holds exactly 4 windows of shape 111101110111 and 1 of 111011010010111 with the all-zero key and the counts below follow from the set sizes.
A handful of targets are mutated copies of queries (true homologues), so the hit table is not empty.

Final sizes, counted on the CPU (sets = sequences of q x t; raw hits per shape, in millions; oracle seconds on a 16-thread host):

    case            sets           raw hits                       candidates     hits   oracle s   must take
    quiet           16 x 16        0.002 / 0.002                          73       62      0.1     nothing
    hits_x1         700 x 700      7.99 / 0.65                         4 106    1 799      0.9     hits once
    hits_x2         800 x 2000     26.10 / 2.12                       12 842    5 348      0.6     hits twice
    slab            1500 x 100     2.45 / 0.20                         1 240      510      0.2     slab (one key 6 000 times in q)
    slab_sensitive  1500 x 100     2.45 / 0.20 / 0.23 / 0.72           1 250      513      0.3     slab, all four fused indices built again
    slab_hits       1500 x 350     8.57 / 0.70                         4 245    1 817      0.3     slab, then hits once (the 5 700 x 800 of the proposal
                                                                                                   cut down to land in (2^22, 2^24]: 0.17 GB of hits, not 2.7)
    set_x1          750 x 750      2.43 / 0.04                       808 574      352      2.2     set once (a motif of 13 identical residues, ungapped_min = 0)
    self_hits       700 genes      8.02 / 0.68 (700 x 4200)            4 684    2 318      0.2     hits once with the self map on
    nt_hits         1800 x 3600    6.50                               61 340   61 340      1.7     hits once in seed_match_stride

The controls (a quarter of the sequences on either side) stay below 1.64 M raw hits per shape and 50 727 candidates, with no key more than 1 500 times.

nt_hits shares an 18-mer, not a 20-mer: twenty exact bases score 40 = the nucleotide tool's ungapped_min, so every one of the millions of pairs would be a
candidate and the case would be a test of the alignment stage.  Eighteen bases (two 17-mers, 36 points) with the base on either side of the word taken
from AC in the queries and from GT in the targets stay below it unless more bases match by chance behind the mismatch (one pair in thirty).  The two
17-mers of the word are two keys, so n x n sequences give 2 n^2 raw hits, not the 16 n^2 of the protein motif: 1 800 sequences a side, not 1 100."""
import functools
import time

import numpy as np

from oracle import oracle as O

PART_CAP = 5632                       # entries of one coarse bucket's slab
HIT_CAP_MIN = 1 << 22                 # hit_cap = max(HIT_CAP_MIN, 2 * packed target bytes)
TABLE_BITS_MIN = 20                   # table_bits = max(TABLE_BITS_MIN, ceil(log2(64 * queries))); list_cap = 2^(table_bits - 1)
PARTITION_MIN_BUCKET_BITS = 16        # the partition build (and with it the slab) exists from this bucket_bits on
SEQ_GAP, END_PAD = 16, 64             # packed sets: 16-aligned starts, >= SEQ_GAP bytes between sequences, END_PAD at both ends
MARGIN = 1.5

SOURCE_PINS = {
    'peppan_amd/csrc/seeds.hip': (
        'constexpr int PART_CAP = 5632;',
        'if (hit_cap == 0) hit_cap = std::max<uint64_t>(1ull << 22, 2 * T.total);',
        'int table_bits = std::max(20, std::min(28, ilog2_ceil(64ull * Q.n)));',
        'const uint32_t list_cap = (uint32_t)(cap >> 1);',
        'int bucket_bits = std::max(10, std::min(28, ilog2_ceil(2 * Q.total)));',
        'bool use_partition = P.reserved[2] == 0 && bucket_bits >= 16 && bucket_bits - fine_bits <= 13;',
        'if (h_counters[3]) { use_partition = false; continue; }',
        'if (h_counters[2]) { hit_cap *= 4; continue; }',
        'if (h_counters[1] || h_counters[0] > list_cap) { table_bits += 2; continue; }',
        'for (int attempt = 0; attempt < 8; ++attempt) {',
    ),
    'peppan_amd/csrc/common.h': ('#define PEP_SEQ_GAP 16', '#define PEP_END_PAD 64'),
}

LETTERS = 'ACDEFGHIKLMNPQRSTVWY'
MOTIF_LETTERS = 'KREDQN'
STATS = ('candidates', 'pairs', 'tracebacks', 'hits', 'cells', 'query_seeds', 'target_seeds', 'seed_hits')


# ---- the independent count

def shapes_of(p):
    return [[int(p.offs[s][i]) for i in range(int(p.weight[s]))] for s in range(int(p.n_shapes))]


def seed_keys(seqs, p, s):
    """the key of every seed window of shape s of a set of residue-code arrays, as uint64, in the set's order"""
    offs = shapes_of(p)[s]
    span = offs[-1] + 1
    red = np.array([int(p.reduce[i]) for i in range(32)], dtype=np.uint8)
    gap = np.full(span, 0xFF, dtype=np.uint8)           # a window that leaves its sequence meets a letter of the gap
    parts = []
    for x in seqs:
        parts += [red[np.asarray(x, dtype=np.uint8) & 31], gap]
    r = np.concatenate(parts) if parts else gap
    n = len(r) - span + 1
    key, valid = np.zeros(n, dtype=np.uint64), np.ones(n, dtype=bool)
    for i, o in enumerate(offs):
        g = r[o:o + n]
        valid &= g != 0xFF
        key += g.astype(np.uint64) * np.uint64(int(p.base) ** i)
    return key[valid]


def seed_counts(q, t, p):
    """-> [(query_seeds, target_seeds, raw_hits) per shape]"""
    out = []
    for s in range(int(p.n_shapes)):
        kq, cq = np.unique(seed_keys(q, p, s), return_counts=True)
        kt, ct = np.unique(seed_keys(t, p, s), return_counts=True)
        _, iq, it = np.intersect1d(kq, kt, assume_unique=True, return_indices=True)
        out.append((int(cq.sum()), int(ct.sum()), int((cq[iq].astype(np.int64) * ct[it].astype(np.int64)).sum())))
    return out


def max_key_count(seqs, p, s):
    k = seed_keys(seqs, p, s)
    return int(np.unique(k, return_counts=True)[1].max()) if len(k) else 0


def packed_bounds(seqs):
    """(lower, upper) bound of the bytes of the packed set: the residues alone; every sequence with its gap and its alignment, and both ends"""
    n = sum(len(x) for x in seqs)
    return n, n + len(seqs) * (SEQ_GAP + 15) + 2 * END_PAD + 32


# ---- the inputs

def _codes(s):
    return np.frombuffer(s.encode('ascii'), dtype=np.uint8) - 65


def motif_family(n, seed, motif_len=15, exact=False, flank=(12, 15)):
    """n proteins (uint8 residue codes): flank[0] .. flank[1] residues of the classes other than the motif's, the motif, a flank again.
    exact: every member carries the same motif residues (then the motif alone scores above ungapped_min between any two)"""
    rng = np.random.default_rng(seed)
    motif, other = _codes(MOTIF_LETTERS), _codes(''.join(c for c in LETTERS if c not in MOTIF_LETTERS))
    fixed = motif[rng.integers(0, len(motif), motif_len)]
    out = []
    for _ in range(n):
        a, b = (int(v) for v in rng.integers(flank[0], flank[1] + 1, 2))
        m = fixed if exact else motif[rng.integers(0, len(motif), motif_len)]
        out.append(np.ascontiguousarray(np.concatenate([other[rng.integers(0, len(other), a)], m, other[rng.integers(0, len(other), b)]])))
    return out


def _mutated(x, rng, pools, rate=0.12):
    """a copy with `rate` of its positions redrawn from the pool its residue belongs to (a motif residue stays a motif residue)"""
    y = x.copy()
    for i in np.nonzero(rng.random(len(x)) < rate)[0]:
        pool = next(pl for pl in pools if x[i] in pl)
        y[i] = pool[rng.integers(0, len(pool))]
    return y


def _protein_sets(nq, nt, seed, homologues=8, **kw):
    q, t = motif_family(nq, seed, **kw), motif_family(nt, seed + 1000, **kw)
    rng = np.random.default_rng(seed + 2000)
    pools = (_codes(MOTIF_LETTERS), _codes(''.join(c for c in LETTERS if c not in MOTIF_LETTERS)))
    for i in range(min(homologues, nq, nt)):
        t[i] = _mutated(q[i], rng, pools)
    return q, t


CODONS = {'A': ('GCT', 'GCA'), 'C': ('TGT', 'TGC'), 'D': ('GAT', 'GAC'), 'E': ('GAA', 'GAG'), 'F': ('TTT', 'TTC'), 'G': ('GGT', 'GGC'), 'H': ('CAT', 'CAC'),
          'I': ('ATT', 'ATC'), 'K': ('AAA', 'AAG'), 'L': ('CTG', 'TTA'), 'M': ('ATG',), 'N': ('AAT', 'AAC'), 'P': ('CCG', 'CCA'), 'Q': ('CAA', 'CAG'),
          'R': ('CGT', 'CGC'), 'S': ('TCT', 'AGC'), 'T': ('ACC', 'ACT'), 'V': ('GTT', 'GTG'), 'W': ('TGG',), 'Y': ('TAT', 'TAC')}


def _genes(n, seed):
    """motif proteins back-translated (a codon of two drawn per residue) between ATG and a stop"""
    rng = np.random.default_rng(seed + 3000)
    out = []
    for x in motif_family(n, seed):
        cod = [CODONS[chr(int(c) + 65)] for c in x]
        out.append(('ATG' + ''.join(c[int(rng.integers(0, len(c)))] for c in cod) + 'TAA').encode())
    return out


def _gene_sets(genes):
    """what K1 makes of a gene list on both sides (set_query_nt(g, 11) / set_ref_nt(g, 6, 11)), from the oracle's translation"""
    q = [O.aa_codes(O.query_frame(g.decode(), 11)[1]) for g in genes]
    t = []
    for g in genes:
        for aa in O.translate_frames(g.decode(), range(1, 7), 11):
            t += [O.aa_codes(c) for _, c in O.ref_chunks(aa)]
    return q, t


def _nt_sets(n, seed, homologues=8):
    """base codes: n queries and n targets of about 58 bases around one shared 18-mer (see the module's docstring), targets = forward strands + reverse complements"""
    rng = np.random.default_rng(seed)
    word = rng.integers(0, 4, 18).astype(np.uint8)

    def member(next_to):
        a, b = (int(v) for v in rng.integers(18, 23, 2))
        return np.ascontiguousarray(np.concatenate([rng.integers(0, 4, a - 1), [next_to[rng.integers(0, 2)]], word, [next_to[rng.integers(0, 2)]],
                                                    rng.integers(0, 4, b - 1)]).astype(np.uint8))
    q = [member((0, 1)) for _ in range(n)]
    fwd = [member((2, 3)) for _ in range(n)]
    for i in range(min(homologues, n)):
        y = q[i].copy()
        y[[2, 9, len(y) - 4]] ^= 1
        fwd[i] = y
    return q, fwd + [np.ascontiguousarray((3 - c[::-1]).astype(np.uint8)) for c in fwd]


def _quiet_sets():
    from peppan_amd import synth
    prots = synth.make_proteins(16, length=(60, 200), seed=5, family=4, sub=0.2)
    return prots, prots


NOTHING = dict(slab=False, hit_growths=0, set_growths=0)


def _case(name, tool, q, t, takes, genes=None, overrides=None):
    return dict(name=name, tool=tool, q=q, t=t, genes=genes, overrides=overrides or {}, takes=dict(NOTHING, **takes), self_on=genes is not None)


def _build(name, control):
    """the case, or (control) the same family cut down until no condition holds"""
    k = 4 if control else 1
    label = name + ('/control' if control else '')
    takes = {} if control else None
    if name == 'quiet':
        return _case(label, 'protein', *_quiet_sets(), takes={})
    if name == 'hits_x1':
        return _case(label, 'protein', *_protein_sets(700 // k, 700 // k, 11), takes=takes if control else dict(hit_growths=1))
    if name == 'hits_x2':
        return _case(label, 'protein', *_protein_sets(800 // k, 2000 // k, 12), takes=takes if control else dict(hit_growths=2))
    if name in ('slab', 'slab_sensitive'):
        return _case(label, 'sensitive' if name == 'slab_sensitive' else 'protein', *_protein_sets(1500 // k, 100 // k, 13), takes=takes if control else dict(slab=True))
    if name == 'slab_hits':
        return _case(label, 'protein', *_protein_sets(1500 // k, 350 // k, 14), takes=takes if control else dict(slab=True, hit_growths=1))
    if name == 'set_x1':
        return _case(label, 'protein', *_protein_sets(750 // k, 750 // k, 15, homologues=0, motif_len=13, exact=True), takes=takes if control else dict(set_growths=1),
                     overrides=dict(ungapped_min=0))
    if name == 'self_hits':
        genes = _genes(700 // k, 16)
        return _case(label, 'protein', *_gene_sets(genes), takes=takes if control else dict(hit_growths=1), genes=genes)
    if name == 'nt_hits':
        return _case(label, 'nucleotide', *_nt_sets(1800 // k, 17), takes=takes if control else dict(hit_growths=1))
    raise KeyError(name)


NAMES = ('quiet', 'hits_x1', 'hits_x2', 'slab', 'slab_sensitive', 'slab_hits', 'set_x1', 'self_hits', 'nt_hits')


@functools.lru_cache(maxsize=None)
def case(name, control=False):
    """dict: name, tool (protein / sensitive / nucleotide), q / t (residue-code arrays: what the oracle searches and the count counts), genes (None, or the
    gene list that goes to set_query_nt / set_ref_nt and of which q / t are the translation), overrides (parameters off the tool's defaults),
    takes (slab, hit_growths, set_growths: what the case must take), self_on (the self map applies)"""
    return _build(name, control)


def native_params(c):
    """the library's parameter block of a case (the library loads without a GPU)"""
    from peppan_amd import _native as N
    p = N.nucleotide_params(0., 0.) if c['tool'] == 'nucleotide' else N.default_params(0., 0., 10, 5, sensitive=c['tool'] == 'sensitive')
    for k, v in c['overrides'].items():
        setattr(p, k, v)
    return p


@functools.lru_cache(maxsize=None)
def counts(name, control=False):
    c = case(name, control)
    return tuple(seed_counts(c['q'], c['t'], native_params(c)))


@functools.lru_cache(maxsize=None)
def oracle_result(name, control=False):
    """(hits, cigar, stats, seconds) of the oracle on a case: computed once per process, shared by every test, never changed"""
    c = case(name, control)
    p = native_params(c)
    ms = np.array([O.min_score(len(s), p.dbsize, p.max_evalue, p.ka_lambda, p.ka_k) for s in c['q']], dtype=np.int32)
    t0 = time.perf_counter()
    h, cg, st = O.search(c['q'], c['t'], O.params_from(p), min_scores=ms)
    dt = time.perf_counter() - t0
    h.setflags(write=False)
    cg.setflags(write=False)
    return h, cg, st, dt
