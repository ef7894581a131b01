"""The step of ortho() behind the paralog filter: `synteny_resolver` (PEPPAN.py:1153-1191, called at :1928 with nNeighbor = 2), which splits a
paralogous name by the neighbourhoods of its members.

    ite_synteny_resolver    PEPPAN.py:1097-1151   drop-in for one group
    resolve_groups          the same for many groups, in GPU batches
    split_names             PEPPAN.py:1155-1186   the array-level core of synteny_resolver: columns in, new names out (no pandas)
    synteny_resolver        PEPPAN.py:1153-1191   the file-level drop-in: <prefix>.synteny.Prediction

ite_synteny_resolver computes a distance for every pair of the members of a name in a Python double loop - a set intersection and three
np.min / np.max calls per pair -, sorts all pairs and walks them until the first conflict pair (two members of one genome with d > 0) whose
ends carry different tags.  Two ends of a conflict pair never share a tag, so the walk reads exactly the pairs with d below the smallest d of
a conflict pair, in the order (d, flag, m, k).  K18 (csrc/synteny.hip, Context.synteny_pairs) makes those pairs and the conflict pairs for all
groups of a batch, in that order, with integer arithmetic only; the merge walk itself is sequential and runs on the host (synteny_walk, C++,
about linear in the pairs).  There is no CPU fallback: a missing library or GPU raises PepError.  The context is orthofilter's cached one
(one per process and device; close() releases it).
"""
import numpy as np

from . import _native as N
from .orthofilter import _context, close

__all__ = ['ite_synteny_resolver', 'resolve_groups', 'split_names', 'synteny_resolver', 'close']

PAIR_CAP = 1 << 24                      # pairs of one library call, unless one group alone holds more (the library's own cap: N.SYNTENY_MAX_PAIRS)
WINDOW = 3                              # rows on either side of a row that count as its neighbourhood (:1165)


def _as_list(codes, k):
    """one neighbour set (or any iterable of codes) as a strictly ascending uint32 array"""
    a = np.fromiter(codes, dtype=np.int64, count=len(codes)) if not isinstance(codes, np.ndarray) else codes.astype(np.int64).reshape(-1)
    if len(a) and (a.min() < 0 or a.max() >= 1 << 32):
        raise ValueError('the neighbour codes of member %d do not fit 32 bits' % k)
    return np.unique(a).astype(np.uint32)


def _plan(pairs, counters, pair_cap):
    """greedy cuts of a batch: [(lo, hi)] with the pairs of groups[lo:hi] within pair_cap and their rank counters within N.SYNTENY_MAX_COUNTERS; a group
    that alone exceeds one of them makes a call of its own, which the library accepts up to its own caps and refuses beyond"""
    plan, lo = [], 0
    while lo < len(pairs):
        hi, p, c = lo + 1, pairs[lo], counters[lo]
        while hi < len(pairs) and p + pairs[hi] <= pair_cap and c + counters[hi] <= N.SYNTENY_MAX_COUNTERS:
            p += pairs[hi]
            c += counters[hi]
            hi += 1
        plan.append((lo, hi))
        lo = hi
    return plan


def resolve_groups(groups, nNeighbor, device=None, pair_cap=PAIR_CAP):
    """ite_synteny_resolver (PEPPAN.py:1097-1151) for a list of groups (grp_tag, ids, co_genomes, neighbors): ids ascending prediction ids,
    co_genomes one genome code per member, neighbors one set of ortholog codes per member.  -> per group exactly what the reference returns:
    [None, None] without a conflict pair, [grp_tag, None] when a surviving component holds no member in conflict, else
    [grp_tag, {ids[root]: [ids of the component, in the reference's order]}].  One library call per pair_cap pairs."""
    if not 1 <= int(nNeighbor) <= 1 << 20 or int(nNeighbor) != nNeighbor:
        raise ValueError('nNeighbor must be an integer in [1, 2^20], not %r' % (nNeighbor,))
    prepared = []
    for grp_tag, ids, co_genomes, neighbors in groups:
        ids = np.asarray(ids)
        genome = np.asarray(co_genomes)
        if not (len(ids) == len(genome) == len(neighbors)):
            raise ValueError('group %r: one genome code and one neighbour set per id' % (grp_tag,))
        _, genome = np.unique(genome, return_inverse=True)              # (compared for equality only)
        lists = [_as_list(nb, k) for k, nb in enumerate(neighbors)]
        prepared.append((grp_tag, ids, genome.astype(np.uint32).reshape(-1), lists))
    n = np.array([len(p[1]) for p in prepared], dtype=np.int64)
    longest = np.array([max([len(a) for a in p[3]], default=0) for p in prepared], dtype=np.int64)
    plan = _plan((n * (n - 1) // 2).tolist(), np.where(n >= 2, n * (6 * longest + 14), 0).tolist(), min(int(pair_cap), N.SYNTENY_MAX_PAIRS))
    out = []
    ctx = _context(device) if len(prepared) else None
    for lo, hi in plan:
        part = prepared[lo:hi]
        member_off = np.concatenate([[0], np.cumsum(n[lo:hi])]).astype(np.uint64)
        lists = [a for p in part for a in p[3]]
        nb_off = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.uint64)
        nb = np.concatenate(lists) if len(lists) and nb_off[-1] else np.zeros(0, np.uint32)
        genome = np.concatenate([p[2] for p in part]) if len(part) else np.zeros(0, np.uint32)
        _, _, conf_off, conf, walk_off, walk = ctx.synteny_pairs(member_off, genome, nb_off, nb, int(nNeighbor))
        verdict, comps = N.synteny_walk(member_off, conf_off, conf, walk_off, walk)
        for (grp_tag, ids, _, _), v, cc in zip(part, verdict.tolist(), comps):
            if v == 0:
                out.append([None, None])
            elif v == 1:
                out.append([grp_tag, None])
            else:
                out.append([grp_tag, {ids[root]: [ids[m] for m in c] for root, c in cc}])
    return out


def ite_synteny_resolver(data, device=None):
    """PEPPAN.py:1097-1151 on the GPU.  data: (grp_tag, ids, co_genomes, neighbors, nNeighbor) as synteny_resolver hands them over"""
    grp_tag, ids, co_genomes, neighbors, nNeighbor = data
    return resolve_groups([(grp_tag, ids, co_genomes, neighbors)], nNeighbor, device)[0]


def split_names(name, gid, genome, contig, start, nNeighbor=2, device=None, pair_cap=PAIR_CAP):
    """PEPPAN.py:1155-1186 on the columns of a Prediction table, one entry per row: name (column 0), gid (column 2, the prediction id - one id
    may span several rows), genome (column 3), contig (column 5), start (min of columns 9 and 10).  -> (new name per row, in the order the rows
    came in; the stable row order by (contig, start) the reference works in).

    As the reference does it: the rows are sorted by contig name and start.  A table indexed by id holds (name, genome): it starts as
    ('', '') followed by the sorted rows, shifted by one, and every row then writes its own id's entry - so an id that no row carries keeps what
    the shifted rows left there, id 0 is ('', ''), and an id beyond the number of rows is an IndexError.  The neighbourhood of an id is the set
    of names within three rows of any of its rows on the same contig, minus its own name.  A name is paralogous when two ids of one genome carry
    it; its group is every id of the table with that name, groups run in the order of their member count, and a group of one genome is left
    alone.  The components of a partition are ordered by (-size, ids); component k >= 1 is renamed name + '/0.k'.

    One quirk is kept: :1183 applies a bytes pattern to an object array, which on CPython and x86-64 never matches, so the '.k' branch for names
    that already end in '/digits' is dead - 'P/2' becomes 'P/2/0.1'."""
    name, genome, contig = (np.asarray(a, dtype=object).reshape(-1) for a in (name, genome, contig))
    gid = np.asarray(gid).astype(np.int64).reshape(-1)
    start = np.asarray(start).reshape(-1)
    rows = len(name)
    if not (len(gid) == len(genome) == len(contig) == len(start) == rows):
        raise ValueError('split_names: one entry per row in every column')
    if rows == 0:
        return np.zeros(0, dtype=object), np.zeros(0, dtype=np.int64)
    if gid.min() < 0:
        raise ValueError('split_names: prediction ids must not be negative')
    contig_code = np.unique(contig, return_inverse=True)[1].reshape(-1)
    order = np.lexsort((start, contig_code))
    name_s, genome_s, gid_s, contig_s = name[order], genome[order], gid[order], contig_code[order]
    n_ids = int(gid_s.max()) + 1
    if n_ids > rows + 1:
        raise IndexError('index %d is out of bounds for axis 0 with size %d' % (n_ids - 1, rows + 1))
    table = np.empty((rows + 1, 2), dtype=object)
    table[0] = ''
    table[1:, 0], table[1:, 1] = name_s, genome_s
    table[gid_s, 0], table[gid_s, 1] = name_s, genome_s
    table = table[:n_ids]
    codes = np.unique(table, return_inverse=True)[1].reshape(-1, 2)
    name_code, genome_code = codes[:, 0], codes[:, 1]
    # neighbourhoods: (owner id, name code) over the six shifts, own name dropped, unique, by owner
    owner, seen = [], []
    for shift in range(1, WINDOW + 1):
        same = contig_s[shift:] == contig_s[:-shift]
        a, b = gid_s[shift:][same], gid_s[:-shift][same]
        owner += [a, b]
        seen += [name_code[b], name_code[a]]
    owner, seen = np.concatenate(owner), np.concatenate(seen)
    keep = seen != name_code[owner]
    pairs = np.unique(np.stack([owner[keep], seen[keep]], axis=1), axis=0) if keep.any() else np.zeros((0, 2), dtype=np.int64)
    nb_off = np.searchsorted(pairs[:, 0], np.arange(n_ids + 1))
    # paralogous names: a (name, genome) entry that two ids share
    both, count = np.unique(codes, axis=0, return_counts=True)
    paralogs = np.unique(both[count > 1, 0])
    members = np.bincount(name_code, minlength=int(codes.max()) + 1)
    by_name = np.argsort(name_code, kind='stable')                     # the ids of a name, ascending, lie side by side
    first = np.concatenate([[0], np.cumsum(members)])
    groups = []
    for tag in sorted(paralogs.tolist(), key=lambda p: int(members[p])):
        ids = by_name[first[tag]:first[tag + 1]]
        if len(np.unique(genome_code[ids])) > 1:
            groups.append((tag, ids, genome_code[ids], [pairs[nb_off[i]:nb_off[i + 1], 1] for i in ids]))
    new_name = table[:, 0].copy()
    for (tag, ids, _, _), (_, parts) in zip(groups, resolve_groups(groups, nNeighbor, device, pair_cap)):
        if parts is None:
            continue
        for k, part in enumerate(sorted(parts.values(), key=lambda v: [-len(v), v])):
            if k > 0:
                new_name[part] = new_name[part[0]] + '/0.{0}'.format(k)
    out = np.empty(rows, dtype=object)
    out[order] = new_name[gid_s]
    return out, order


def synteny_resolver(prefix, prediction, nNeighbor=2, device=None):
    """PEPPAN.py:1153-1191: reads the Prediction table, renames the split-off copies of every paralogous name (split_names) and writes
    <prefix>.synteny.Prediction, sorted by columns 0, 2 and 7, byte for byte as the reference does; returns its name.  pandas reads the file,
    does the final sort and writes; the order by (contig, start) is split_names' own, and the rows enter the final, stable sort in that order."""
    import pandas as pd
    rows = pd.read_csv(prediction, sep='\t', header=None).values
    names, order = split_names(rows[:, 0], rows[:, 2], rows[:, 3], rows[:, 5], np.minimum(rows[:, 9], rows[:, 10]), nNeighbor, device)
    rows[:, 0] = names
    out = prefix + '.synteny.Prediction'
    pd.DataFrame(rows[order]).sort_values(by=[0, 2, 7]).to_csv(out, sep='\t', index=False, header=False)
    return out
