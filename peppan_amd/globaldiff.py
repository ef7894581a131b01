"""The genome-pair identity statistics of the reference's get_global_difference (PEPPAN.py:1611-1666): the (mean, sigma) table that K16
(orthofilter.gd_table) and K17 (ingroups.initializing) read.

    get_global_difference   the drop-in for PEPPAN.py:1611-1666 (called at :1897): the same arguments, the same object array
    pair_statistics         the device call on its own, for callers that bring their own events
    log_table               the logarithm of every value code, made by numpy as the reference makes it

The function is cut as include/peppan_hip.h describes.  The group selection (:1612-1629) stays Python as the reference writes it - a few thousand
groups, and sha1(bytes(g)) of a numpy integer is what it is.  The dictionary walk over the selected rows (:1632-1659 without its inner loops) is host
C++ (N.global_diff_walk): it only decides which two member lists meet at each row.  The cross product of those lists, grouped by genome pair, and numpy's
two means per pair are K22 (csrc/globaldiff.hip, Context.global_diff), bit for bit.  The tail (:1663-1665) is numpy exactly as written.  There is no CPU
fallback.  The context is orthofilter's cached one."""
import hashlib

import numpy as np

from . import _native as N
from .orthofilter import _context

__all__ = ['get_global_difference', 'pair_statistics', 'log_table']


def log_table():
    """np.log(1.005 - np.array(data) / 10000.) (:1661) depends on the integer alone: element i of this table is bit for bit the reference's element
    for a value i, for lists of any length"""
    return np.log(1.005 - np.arange(N.GDIFF_TABLE) / 10000.)


def pair_statistics(events, arena, table=None, n_genomes=None, chunk_items=0, device=None):
    """K22 alone.  events: integer [n, 6] = (a_off, a_len, b_off, b_len, value, drop_same), two prefixes of lists in `arena` (genome ranks 0 .. G - 1);
    table: float64[10050], by default log_table().  -> (g1, g2, n, mean, var) per genome pair in the order the pairs are first met: the ranks g1 <= g2,
    the number of values, numpy's mean of table[value] over them in event order and numpy's mean of the squared deviations from it."""
    arena = np.asarray(arena)
    if n_genomes is None:
        n_genomes = int(arena.max()) + 1 if arena.size else 0
    return _context(device).global_diff(events, arena, n_genomes, log_table() if table is None else table, chunk_items)


def get_global_difference(geneGroups, cluFile, bsnFile, geneInGenomes, nGene=1000, device=None):
    """PEPPAN.py:1611-1666: -> the object array [k, 2] of ((g1, g2), (mean, sigma)) in the reference's row order; shape (0, 0) when nothing is selected."""
    groupPresences = {}
    for grp, genes in geneGroups.items():
        gg = np.array([geneInGenomes[g] for g in genes])
        presence = np.unique(gg[gg >= 0], return_counts=True)
        groupPresences[grp] = [np.sum(presence[1] == 1), gg.size]
    groupScore = sorted([[-p[0], p[1] - p[0], int(hashlib.sha1(bytes(g)).hexdigest(), 16), g] for g, p in groupPresences.items() if p[0] > 1])
    selectedGenes = []
    for g in groupScore[:nGene]:
        selectedGenes.extend(geneGroups[g[3]])
    selectedGenes = np.array(selectedGenes, dtype=np.int64)

    clu = np.load(cluFile.rsplit('.', 1)[0] + '.npy', allow_pickle=True)
    bsn = np.load(bsnFile, allow_pickle=True)
    clu, bsn = (np.asarray(t).astype(np.int64).reshape(-1, 3) for t in (clu, bsn))
    bsn = bsn[bsn.T[2] > 0]
    selectedClu = clu[np.isin(clu.T[0], selectedGenes)]
    selectedBsn = bsn[np.isin(bsn.T[0], selectedGenes)]

    # the genes of the selected rows with their genomes; one the map lacks is left out, and the walk names it
    genes, genome_of, as_given = [], [], {}
    for g in np.unique(np.concatenate([selectedClu[:, :2].reshape(-1), selectedBsn[:, :2].reshape(-1)])).tolist():
        try:
            genome = geneInGenomes[g]
        except (KeyError, IndexError):
            continue
        genes.append(g)
        genome_of.append(int(genome))
        as_given.setdefault(int(genome), genome)
    events, arena, genomes = N.global_diff_walk(selectedClu, selectedBsn, genes, genome_of)
    g1, g2, n, mean, var = _context(device).global_diff(events, arena, len(genomes), log_table())
    if len(n) == 0:
        return np.empty((0, 0), dtype=object)
    global_differences = np.empty((len(n), 2), dtype=object)
    for k in range(len(n)):
        mean_diff2 = mean[k]
        mean_diff = min(max(mean_diff2, np.log(0.02)), np.log(0.5))
        sigma = min(max(np.sqrt(var[k]), np.log(1.6)), np.log(2.4))
        global_differences[k, 0] = (as_given[int(genomes[g1[k]])], as_given[int(genomes[g2[k]])])
        global_differences[k, 1] = (np.exp(mean_diff), sigma)
    return global_differences
