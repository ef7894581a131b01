"""filt_genes (PEPPAN.py:525-734) on the library: what turns the gene scores of `initializing` into the pan-gene matrices of `mat_out`.

    prepare_batch       :546-624 (nj / ml) and :641-656 (sbh) for one round of up to 500 genes: K26 (csrc/batchprep.hip, include/peppan_hip.h).
                        Stage A (the screen against `used`) and stage C (the pruning of every group, the decision final / to_run) are one GPU launch each
                        over the whole round; stage B (the unsure walk, sequential over the round's genes) is one call of host C++.  The tables and the
                        members of the .conflicts store are read and laid out with numpy over whole members: no Python statement runs per row.
    exclude_genes       :736-743, exclude_gene for a list of genes: the bookkeeping between stage A and stage B that is the caller's
    get_gene            :486-509
    filt_genes          the drop-in for :525-734: get_gene, prepare_batch, orthofilter.filt_per_groups (or the caller's stand-in) and the selection loop
                        (:663-732), which is sequential dictionary work and plain Python here (DESIGN.md section 9 lists it as the next step).

Deliberate differences, both stated in the header: where two rows tie in column 2 at :603 the reference's order is numpy's unstable sort's and this
project's rule decides (equal keys keep their order; counted in n_ties); a member that the .conflicts store does not hold means "no conflicts" here,
where the reference raises inside a pool worker.  `params` is passed in: the reference reads a module global.  There is no CPU fallback."""
import collections

import numpy as np

from . import _native as N
from .mapbsn import MapBsn

__all__ = ['prepare_batch', 'exclude_genes', 'get_gene', 'filt_genes', 'BatchResult', 'close']

CFL_MEMBER = 30000                       # loci per member of the .conflicts store (PEPPAN.py:516)

BatchResult = collections.namedtuple('BatchResult', 'status mats inparalog conflicts n_ties abandoned')


def _context(device=None):
    from .orthofilter import _context as shared
    return shared(device)


def close():
    from .orthofilter import close as shared
    shared()


def _opened(store):
    own = not isinstance(store, MapBsn)
    return (MapBsn(store) if own else store), own


def _conflict_rows(cfl_store, loci):
    """load_conflict (:511-523) for the loci of a batch, member by member: -> (values int64, start int64[n], length int64[n]) - row r owns
    values[start[r] : start[r] + length[r]].  A member the store does not hold gives empty lists."""
    loci = np.asarray(loci, dtype=np.int64)
    start, length = np.zeros(len(loci), np.int64), np.zeros(len(loci), np.int64)
    parts, base = [], 0
    member = loci // CFL_MEMBER
    store, own = _opened(cfl_store)
    try:
        for m in np.unique(member).tolist():
            if not store.exists(m):
                continue
            d = np.asarray(store.get(m), dtype=np.int64)
            sel = np.flatnonzero(member == m)
            idx = loci[sel] - m * CFL_MEMBER
            a, b = d[idx], d[idx + 1]
            start[sel], length[sel] = a + base, np.maximum(b - a, 0)
            parts.append(d)
            base += len(d)
    finally:
        if own:
            store.close()
    return (np.concatenate(parts) if parts else np.zeros(0, np.int64)), start, length


def _csr(values, start, length):
    """the lists (start, length) gathered one behind the other -> (cfl_off uint64[n + 1], cfl int64)"""
    off = np.zeros(len(start) + 1, np.int64)
    np.cumsum(length, out=off[1:])
    src = np.repeat(start - off[:-1], length) + np.arange(int(off[-1]), dtype=np.int64)
    return off.astype(np.uint64), values[src] if len(src) else np.zeros(0, np.int64)


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.uint64)
    np.cumsum(counts, out=off[1:])
    return off


def _used_state(used, n_loci):
    """`used` as the dense table of pep_batch_screen: 0 absent, 1 present with a value <= 0, 2 present with a value > 0"""
    state = np.zeros(n_loci, np.uint8)
    if used:
        keys = np.fromiter(used.keys(), dtype=np.int64, count=len(used))
        vals = np.fromiter(used.values(), dtype=np.int64, count=len(used))
        ok = (keys >= 0) & (keys < n_loci)
        state[keys[ok]] = np.where(vals[ok] > 0, 2, 1)
    return state


def exclude_genes(excluded, scores, genes, conflicts, conflicting):
    """exclude_gene (:736-743) for every gene of `excluded`: the gene and every gene `conflicting` pairs it with leave scores, genes and conflicts.
    conflicting: int array [k, 2] of gene keys (x 1000), both directions, as :526-527 make it.  -> the genes that left with them"""
    gone = []
    conflicting = np.asarray(conflicting).reshape(-1, 2)
    for gene in excluded:
        for g in [gene] + conflicting[conflicting[:, 0] == gene, 1].tolist():
            for d in (scores, genes, conflicts):
                d.pop(g, None)
            if g != gene:
                gone.append(g)
    return gone


def prepare_batch(tab_store, cfl_store, genes, used, new_groups, params, device=None, conflicting=None, path=N.PREP_AUTO):
    """PEPPAN.py:546-624 / :641-656 for one round.

    tab_store, cfl_store: the .tab and .conflicts stores (MapBsn or path); genes: gene key (x 1000) -> score in the order get_gene left them (a dict or
    a list of pairs); used: locus -> 0, +(gene + 1000) or -(gene + 1000); new_groups: the genes that are groups already (they pass through as 'final' with
    their matrix); params: clust_identity and orthology; conflicting: as for exclude_genes - given, the partners of an excluded gene are 'withdrawn'
    before stage B and the round is abandoned at :563-564 when fewer than half of its genes are left (stages B and C are then not run).
    -> BatchResult: status[gene] in 'excluded', 'withdrawn', 'popped', 'final', 'to_run'; mats[gene] the int64[n, 7] matrix of a final or to_run gene
    (:622, :624, :656); inparalog[gene]; conflicts[gene][locus] -> int64 array, the entries the selection loop reads (:567-577); n_ties: the genes in
    which two rows tied in column 2 at :603; abandoned."""
    genes = list(genes.items()) if isinstance(genes, dict) else [(g, s) for g, s in genes]
    orthology = params.get('orthology', 'nj')
    if orthology not in ('nj', 'ml', 'sbh'):
        raise ValueError('prepare_batch: orthology is nj, ml or sbh, not %r' % (orthology,))
    ci = float(params['clust_identity'])
    status, mats, inparalog, conflicts = {}, {}, {}, {}
    for g, _ in genes:
        if g in new_groups:
            status[g], mats[g], inparalog[g] = 'final', new_groups[g], None
    todo = [g for g, _ in genes if g not in new_groups]
    if not todo:
        return BatchResult(status, mats, inparalog, conflicts, 0, False)
    ctx = _context(device)
    store, own = _opened(tab_store)
    try:
        tables = [np.array(store.get(g // 1000), dtype=np.int64).reshape(-1, 7) for g in todo]
    finally:
        if own:
            store.close()
    # ---- stage A
    M = np.concatenate(tables)
    counts = np.array([len(t) for t in tables], dtype=np.int64)
    n_loci = int(M[:, 5].max()) + 1 if len(M) else 0
    M[:, 3], M[:, 4], _, excluded = ctx.batch_screen(_offsets(counts), M[:, 3], M[:, 5], _used_state(used, n_loci), (ci - 0.02) * 10000)
    owner = np.repeat(np.arange(len(todo)), counts)
    keep = (M[:, 3] != 0) & (excluded[owner] == 0)
    M, owner = M[keep], owner[keep]
    gone = [g for g, x in zip(todo, excluded.tolist()) if x]
    for g in gone:
        status[g] = 'excluded'
    withdrawn = set()
    if conflicting is not None and gone:
        pairs = np.asarray(conflicting).reshape(-1, 2)
        withdrawn = set(pairs[np.isin(pairs[:, 0], gone), 1].tolist()) - set(gone)
        for g, _ in genes:
            if g in withdrawn:
                status[g] = 'withdrawn'
                mats.pop(g, None)
    left = [g for g, _ in genes if status.get(g) in (None, 'final')]
    if conflicting is not None and len(left) < len(genes) * 0.5:
        return BatchResult(status, {}, {}, conflicts, 0, True)
    # ---- the conflict lists of the rows that are left (:567-577)
    alive = np.array([status.get(g) is None for g in todo])
    sel = alive[owner]
    M, owner = M[sel], owner[sel]
    values, start, length = _conflict_rows(cfl_store, M[:, 5])
    for g in todo:
        if status.get(g) is None:
            conflicts[g] = {}
    for r in np.flatnonzero(length).tolist():
        conflicts[todo[owner[r]]][int(M[r, 5])] = values[start[r]:start[r] + length[r]]
    if len(values):
        n_loci = max(n_loci, int(values.max()) // 10 + 1)
    # ---- stage B, the genes by falling score (stable)
    score = dict(genes)
    order = sorted((k for k, g in enumerate(todo) if status.get(g) is None), key=lambda k: -score[todo[k]])
    lo = np.searchsorted(owner, np.arange(len(todo)))
    hi = np.searchsorted(owner, np.arange(len(todo)), side='right')
    take = np.concatenate([np.arange(lo[k], hi[k]) for k in order]) if order else np.zeros(0, np.int64)
    B, b_owner = M[take], owner[take]
    cfl_off, cfl = _csr(values, start[take], length[take])
    B[:, 3], popped = N.batch_unsure_walk(_offsets([hi[k] - lo[k] for k in order]), B[:, 3], B[:, 5], cfl_off, cfl, n_loci)
    for k, p in zip(order, popped.tolist()):
        if p:
            status[todo[k]] = 'popped'
            conflicts.pop(todo[k], None)
    # ---- stage C, the genes in the order of `genes`
    keep = (B[:, 3] > 0) & np.array([status.get(g) is None for g in todo])[b_owner]
    back = np.argsort(b_owner[keep], kind='stable')
    C, c_owner = B[keep][back], b_owner[keep][back]
    c_start, c_length = start[take][keep][back], length[take][keep][back]
    ids, c_counts = np.unique(c_owner, return_counts=True)
    n_ties = 0
    if len(ids):
        cfl_off, cfl = _csr(values, c_start, c_length)
        gene_off = _offsets(c_counts)
        out_off, rows, inpar, final, n_ties = ctx.batch_prune(N.PREP_SBH if orthology == 'sbh' else N.PREP_NJ, gene_off, C[:, 1], C[:, 2], C[:, 3], C[:, 4], C[:, 5],
                                                              cfl_off, cfl, n_loci, ci, 10000 * ci, path)
        for j, k in enumerate(ids.tolist()):
            g = todo[k]
            mats[g] = C[int(gene_off[j]) + rows[int(out_off[j]):int(out_off[j + 1])]]
            status[g], inparalog[g] = ('final' if final[j] else 'to_run'), bool(inpar[j])
    return BatchResult(status, mats, inparalog, conflicts, n_ties, False)


def get_gene(all_scores, priorities, ortho_groups, cnt=1):
    """PEPPAN.py:486-509: up to cnt genes of the best rank present, by falling score, none that an earlier pick's ortho_groups rows name (unless
    fewer than 2 cnt genes have that rank) -> [[gene, score, rank]]; with nothing to pick the genes of that rank leave all_scores and [] comes back"""
    rank = {g: priorities[g][0] for g in all_scores if g in priorities}
    best = min(rank.values()) if rank else -1
    scores = {g: all_scores[g] for g, r in rank.items() if r == best}
    picked, taken = [], set()
    for gene, score in sorted(scores.items(), key=lambda x: x[1], reverse=True):
        if score <= 0:
            break
        if gene not in taken or len(scores) < 2 * cnt:
            picked.append([gene, score, best])
            if len(picked) >= cnt:
                break
            taken.update(ortho_groups[ortho_groups[:, 0] == int(gene), 1].tolist())
    if not picked:
        for gene in scores:
            all_scores.pop(gene)
    return picked


def _group_score(mat):
    """:637 / :661: the sum of |column 2| over the first row of every genome"""
    return np.sum(np.abs(mat[np.unique(mat[:, 1], return_index=True)[1], 2]))


def _name(encodes, key):
    return encodes[key // 1000] + ('/' + str(key % 1000) if key % 1000 > 0 else '')


def filt_genes(groups, ortho_groups, global_file, cfl_file, priorities, scores, encodes, params, mat_out, per_groups=None, device=None, logger=None):
    """The drop-in for filt_genes (PEPPAN.py:525-734).  groups: the .tab store (MapBsn or path); ortho_groups int64[k, 3]; global_file: the saved
    global_differences; cfl_file: the .conflicts store; priorities: gene -> [rank, ...]; scores: gene -> score; encodes: name -> number; params:
    clust, clust_identity, orthology, map_bsn, self_id, allowed_sigma (the reference's module global); mat_out: the list (or queue-like object with
    append) that receives [pan gene name, gene name, rank, matrix] and the closing [0, 0, 0, []].  per_groups(to_run) -> per entry the list of
    matrices filt_per_group returns; default orthofilter.filt_per_groups over params['map_bsn'] + '.seq.npz' and global_file.  -> n_ties, the ties
    of both halves summed (the header's tie paragraphs)."""
    from .configure import readFasta
    ortho_groups = np.asarray(ortho_groups)
    conflicting = ortho_groups[ortho_groups[:, 2] < 0]
    conflicting = np.vstack([conflicting[:, :2], conflicting[:, [1, 0]]]) * 1000
    ortho_groups = np.vstack([ortho_groups[:, :2], ortho_groups[:, [1, 0]]]) * 1000
    priorities = {k * 1000: v for k, v in priorities.items()}
    scores = {k * 1000: v for k, v in scores.items()}
    names = [n for _, n in sorted((i, n) for n, i in encodes.items())]
    ref_len = {int(n) * 1000: len(s) for n, s in readFasta(params['clust']).items()}
    seq_file = params['map_bsn'] + '.seq.npz'
    ties = [0]
    if per_groups is None:
        from .orthofilter import filt_per_groups
        gd = np.load(global_file, allow_pickle=True)

        def per_groups(to_run):
            out, n = filt_per_groups(seq_file, to_run, gd, params, device=device)
            ties[0] += n
            return out
    conflicts, new_groups, used, pangenome, pan_list = {}, {}, {}, {}, {}
    lowest_p = max(v[0] for v in priorities.values())
    tab, own = _opened(groups)
    try:
        while scores:
            ortho_groups = ortho_groups[np.isin(ortho_groups, list(scores.keys())).all(1)]
            picked = get_gene(scores, priorities, ortho_groups, cnt=500)
            if not picked:
                continue
            min_score, min_rank = picked[-1][1:]
            genes = {g: s for g, s, _ in picked}
            res = prepare_batch(tab, cfl_file, genes, used, new_groups, params, device=device, conflicting=conflicting)
            ties[0] += res.n_ties
            exclude_genes([g for g, s in res.status.items() if s == 'excluded'], scores, genes, conflicts, conflicting)
            if res.abandoned:
                continue
            conflicts.update(res.conflicts)
            for g, s in res.status.items():
                if s == 'popped':
                    genes.pop(g, None)
            to_run = []
            for g in genes:
                if g in new_groups:
                    continue
                if res.status[g] == 'final':
                    new_groups[g] = res.mats[g]
                else:
                    to_run.append([res.mats[g], res.inparalog[g], ref_len[int(res.mats[g][0, 0]) * 1000], seq_file, global_file])
            to_run.sort(key=lambda r: (r[1], r[0].shape[0] * r[0].shape[0] * r[2]), reverse=True)
            for parts in (per_groups(to_run) if to_run else []):
                gene = int(parts[0][0][0]) * 1000
                new_groups[gene] = parts[0]
                cfl = conflicts.get(gene, {})
                for k, matches in enumerate(parts[1:]):
                    ng = gene + k + 2
                    new_groups[ng] = matches
                    conflicts[ng] = {int(l): cfl.pop(int(l), {}) for l in matches[:, 5]}
                    scores[ng] = _group_score(matches)
                    priorities[ng] = priorities[gene][:]
                    priorities[ng][0] = lowest_p
            for g in genes:
                scores[g] = _group_score(new_groups[g])
            # ---- the selection loop (:663-732)
            while genes:
                score, gene = max([scores[g], g] for g in genes)
                if score < min_score:
                    break
                mat = new_groups.pop(gene)
                paralog, supergroup, used2, idens = False, {}, {}, 0.
                own_cfl = conflicts.get(gene, {})
                for m in mat:
                    locus = int(m[5])
                    seen = used[locus] if locus in used else used2.get(locus)
                    if seen is not None:
                        if seen < 0:
                            sup = pangenome[-(seen + 1000)]
                            supergroup[sup] = supergroup.get(sup, 0) + (2 if m[4] >= ci_x(params) else 1)
                        elif seen > 0:
                            paralog = True
                        m[3] = -1
                        continue
                    idens = max(idens, m[4])
                    used2[locus] = 0
                    for v in own_cfl.get(locus, []):
                        other, kind = int(v) // 10, int(v) % 10
                        if kind == 1:
                            if other not in used:
                                used2[other] = -(gene + 1000)
                        else:
                            used2[other] = gene + 1000 if kind == 2 else 0
                if idens < (params['clust_identity'] - 0.02) * 10000:
                    exclude_genes([gene], scores, genes, conflicts, conflicting)
                    continue
                mat = mat[mat[:, 3] > 0]
                top = [None, -999, 0]
                for sup, cnt in sorted(supergroup.items(), key=lambda d: d[1], reverse=True):
                    if cnt >= mat.shape[0] or cnt >= len(pan_list[sup]):
                        mine = set(mat[:, 1].tolist())
                        s = len(mine - pan_list[sup]) - 2 * len(pan_list[sup] & mine)
                        s = -1 if s < 0 else s
                        if [s, cnt] > top[1:]:
                            top = [sup, s, cnt]
                if top[1] > 0 or top[2] > 0:
                    pangene = top[0]
                elif paralog:
                    new_groups[gene] = mat
                    continue
                else:
                    pangene = gene
                exclude_genes([gene], scores, genes, conflicts, conflicting)
                pangenome[gene] = pangene
                used.update(used2)
                pan_list[pangene] = pan_list.get(pangene, set()) | set(mat[:, 1].tolist())
                if logger is not None and len(pangenome) % 100 == 0:
                    logger('{0} / {1}: pan gene "{2}" : "{3}" picked from rank {4} and score {5}'.format(
                        len(pangenome), len(scores) + len(pangenome), _name(names, pangene), _name(names, gene), min_rank, score / 10000.))
                mat_out.append([_name(names, pangene), _name(names, gene), min_rank, mat])
    finally:
        if own:
            tab.close()
    mat_out.append([0, 0, 0, []])
    return ties[0]


def ci_x(params):
    """clust_identity x 10^4, the float64 product the reference compares column 4 with (:681)"""
    return params['clust_identity'] * 10000
