"""The two counting steps of PEPPAN_parser, the tool a user runs on the GFF that write_output produced (PEPPAN_parser.py, installed as a console script
beside PEPPAN): the rarefaction curves of option -c and the core gene allelic distances of option -a.

    getOrtho               PEPPAN_parser.py:37-61     the GFF -> {genome: {ortholog group: {gene ID: allele}}} (host)
    writeCurve             PEPPAN_parser.py:63-115    <prefix>_content.curve, byte for byte
    rarefaction_curves     its loop, :74-80           the `curves` array alone
    getDistance            PEPPAN_parser.py:172-179   drop-in, float64 [n, n]
    writeCGAV              PEPPAN_parser.py:145-170   <prefix>_CGAV.profile and <prefix>_CGAV.dist, byte for byte; <prefix>_CGAV.nwk by K21 (njtree.py) without rapidnj

The reference walks 1 000 random genome orders and sums a counter per gene twice per step, and compares every pair of profiles with three numpy passes -
minutes of Python at 2 000 genomes.  K20 (csrc/parser.hip) does both as integer kernels: Context.rarefaction_curves walks every order over bit rows
(pan = popcount of the running OR, core = popcount of the running AND), Context.profile_pairs counts per pair the genes both carry and those with the same
allele.  Both results are exact integers; every float - the curve fits, the means, -log((shared + .5) / (presence + 1)) - is made here from them with the
reference's own expressions, so the files come out as the reference writes them.  There is no CPU fallback: a missing library or GPU raises PepError.  The
context is orthofilter's cached one (one per process and device; close() releases it).

Not here: writeMatrix and splitGFF (text only), writeTree (FastTree and ete3) and the command line.
"""
import re
import shutil
import subprocess
from collections import defaultdict

import numpy as np

from . import _native as N
from . import njtree
from .configure import logger, uopen
from .orthofilter import _context, close

__all__ = ['getOrtho', 'rarefaction_curves', 'writeCurve', 'getDistance', 'writeCGAV', 'close']


def getOrtho(fname, noPseudogene=False):
    """PEPPAN_parser.py:37-61: {genome: {group: {ID: allele}}} of the CDS (and, unless noPseudogene, pseudogene) lines of a PEPPAN GFF.  The genome is the
    contig's name up to its first ':', an allele that is no number is -1, a gene ID counts once."""
    seen = set()
    groups = defaultdict(dict)
    with uopen(fname) as fin:
        for line in fin:
            if line.startswith('#'):
                continue
            part = line.strip().split('\t')
            if part[1] != 'CDS' and (part[1] != 'pseudogene' or noPseudogene):
                continue
            gene = re.findall(r'ID=([^;]+);', part[8])[0]
            if gene in seen:
                continue
            seen.add(gene)
            of_genome = groups[part[0].split(':', 1)[0]]
            inference = re.findall(r'inference=ortholog_group:([^;]+)', part[8])[0]
            for entry in inference.split(','):
                group, allele = entry.split(':')[1:3]
                of_genome.setdefault(group, {})[gene] = int(allele) if allele.isdigit() else -1
    return groups


def presence_matrix(groups):
    """genes numbered in the order they are first seen over groups.values() (:65-69) -> bool[n_genomes, n_genes], genomes in the order of groups"""
    code = {}
    for of_genome in groups.values():
        for g in of_genome:
            code.setdefault(g, len(code))
    presence = np.zeros((len(groups), len(code)), dtype=bool)
    for k, of_genome in enumerate(groups.values()):
        presence[k, [code[g] for g in of_genome]] = True
    return presence


def shuffled_orders(n_genomes, n_iter):
    """the genome orders the reference walks: it shuffles its list of genomes in place once per iteration (:76), each shuffle starting from the last one's
    result; numpy's global legacy generator permutes an index array exactly as it permutes that list, so np.random.seed reproduces the reference's run"""
    index = np.arange(n_genomes, dtype=np.uint32)
    orders = np.zeros((n_iter, n_genomes), dtype=np.uint32)
    for t in range(n_iter):
        np.random.shuffle(index)
        orders[t] = index
    return orders


def _curves_of(presence, n_iter, orders, device):
    if orders is None:
        orders = shuffled_orders(presence.shape[0], n_iter)
    return _context(device).rarefaction_curves(N.pack_presence(presence), presence.shape[1], orders)


def rarefaction_curves(groups, n_iter=1000, orders=None, device=None):
    """the `curves` of writeCurve (:74-80) -> int64[n_genomes, n_iter, 2]: at [k, t] the genes present in at least one and in all of the first k + 1 genomes
    of order t.  orders (int [n_iter, n_genomes], rows permutations of the genomes' indices in groups) default to shuffled_orders(n_genomes, n_iter)."""
    return _curves_of(presence_matrix(groups), n_iter, orders, device)


def func_powerlaw(x, m, c):
    return x ** m * c


def curve_text(curves, n_genomes, mean_size, n_pan, pseudogene=True):
    """the text of <prefix>_content.curve (:81-113) from the curves and the three header counts: the fits of the mean curves by scipy on the host, the
    median / 2.5 % / 97.5 % table by the reference's index expressions"""
    from scipy.optimize import curve_fit
    from scipy.stats.distributions import t
    gtype = ['CDSs', 'genes'][int(pseudogene)]
    x = np.arange(len(curves)) + 1
    y = np.mean(curves, 1)
    fits = []
    for xs, ys in ((x, y[:, 0]), (x[1:], y[1:, 0] - y[:-1, 0]), (x, y[:, 1])):
        opt, cov = curve_fit(func_powerlaw, xs, ys, maxfev=3000)
        tval = t.ppf(1.0 - .05 / 2.0, max(0, len(xs) - 2))
        fits.append((opt, np.diag(cov) ** 0.5 * tval))
    (o1, c1), (o2, c2), (o3, c3) = fits
    last = x[-1]
    out = ['#! No. genomes: {0}\n'.format(n_genomes),
           '#! Ave. {1} per genome: {0:.03f}\n'.format(mean_size, gtype),
           '#! No. pan {1}: {0}\n'.format(n_pan, gtype),
           '#! No. core {1}: {0}\n'.format(curves[-1, 0, 1], gtype),
           '#! Heaps\' law model in DOI: 10.1016/j.mib.2008.09.006:\tGamma={0:.03f} +/- {1:.03f}, Kappa={2:.03f} +/- {3:.03f}, ~{4:.03f} new genes per new genome.\n'.format(
               o1[0], c1[0], o1[1], c1[1], (last + 1) ** o1[0] * o1[1] - last ** o1[0] * o1[1]),
           '#! Power law model in DOI: 10.1016/j.mib.2008.09.006:\tAlpha={0:.03f} +/- {1:.03f}, Kappa={2:.03f} +/- {3:.03f}, ~{4:.03f} new genes per new genome.\n'.format(
               -o2[0], c2[0], o2[1], c2[1], (last + 1) ** o2[0] * o2[1]),
           '#! Power law model for the core genome:              \tAlpha={0:.03f} +/- {1:.03f}, Kappa={2:.03f} +/- {3:.03f}, ~{4:.03f} fewer core genes per new genome.\n'.format(
               -o3[0], c3[0], o3[1], c3[1], -(last + 1) ** o3[0] * o3[1] + last ** o3[0] * o3[1]),
           '#No. genome\t(Pan-genome)Median\t2.5%\t97.5%\t|\t(Core-genome)Median\t2.5%\t97.5%\n']
    ranked = np.sort(curves, axis=1)                                        # every genome count's pan and core values over the orders, ascending
    size = curves.shape[1]
    low, mid, high = int(size * 0.025), int(size * 0.5), int(size * 0.975)
    for k, r in enumerate(ranked):
        out.append('{0}\t{1}\t{2}\t{3}\t|\t{4}\t{5}\t{6}\n'.format(k + 1, r[mid, 0], r[low, 0], r[high, 0], r[mid, 1], r[low, 1], r[high, 1]))
    return ''.join(out)


def writeCurve(prefix, groups, pseudogene=True, n_iter=1000, device=None):
    """PEPPAN_parser.py:63-115: writes <prefix>_content.curve and returns what the reference returns, its all-zero summary"""
    presence = presence_matrix(groups)
    curves = _curves_of(presence, n_iter, None, device)
    text = curve_text(curves, len(groups), np.mean(presence.sum(1)), presence.shape[1], pseudogene)
    with open('{0}_content.curve'.format(prefix), 'w') as fout:
        fout.write(text)
    logger('Curves for {1} are saved in {0}_content.curve'.format(prefix, ['CDS', 'all genes'][int(pseudogene)]))
    return np.zeros([len(groups), 2, 5], dtype=int)


def _as_int32(profiles):
    """profiles as int32 with `> 0` and equality kept: values that int32 cannot hold (or that are no integers) are replaced by their rank among the matrix's
    distinct values, shifted so that the positive ones get 1, 2, .. and the others 0, -1, .. - injective, positives to positives"""
    if profiles.dtype.kind in 'iub' and (profiles.size == 0 or (int(profiles.min()) >= -2 ** 31 and int(profiles.max()) < 2 ** 31)):
        return profiles.astype(np.int32)
    values, rank = np.unique(profiles, return_inverse=True)
    n_rest = int(np.sum(~(values > 0)))
    return (rank.reshape(profiles.shape).astype(np.int64) - n_rest + 1).astype(np.int32)


def pair_counts(profiles, device=None):
    """(shared, presence) int32[n, n] of getDistance's pair loop: the genes two profiles both carry with the same allele / both carry"""
    profiles = np.asarray(profiles)
    n = profiles.shape[0]
    if n == 0 or profiles.ndim != 2 or profiles.shape[1] == 0:               # no pair or no gene: nothing to count
        return np.zeros((n, n), np.int32), np.zeros((n, n), np.int32)
    return _context(device).profile_pairs(_as_int32(profiles))


def distances_of(shared, presence):
    """:177-178 on exact counts: -log((shared + 0.5) / (presence + 1.)), diagonal 0"""
    distances = -np.log((shared + 0.5) / (presence + 1.))
    np.fill_diagonal(distances, 0.)
    return distances


def getDistance(profiles, device=None):
    """PEPPAN_parser.py:172-179: float64 [n, n] distances of allelic profiles (rows; a value > 0 is an allele)"""
    return distances_of(*pair_counts(profiles, device))


def cgav_profiles(ortho, pCore):
    """:146-159: (genomes sorted, the genes carried as one copy with an allele in at least pCore % of the genomes, sorted; the profile rows)"""
    genomes = sorted(ortho.keys())
    min_presence = len(ortho) * pCore / 100.
    count = defaultdict(int)
    for of_genome in ortho.values():
        for g, copies in of_genome.items():
            if len(copies) == 1 and list(copies.values())[0] > 0:
                count[g] += 1
    genes = sorted(g for g, c in count.items() if c >= min_presence)
    profiles = []
    for genome in genomes:
        of_genome = ortho[genome]
        profiles.append([max(list(of_genome[g].values())[0], 0) if len(of_genome.get(g, {})) == 1 else 0 for g in genes])
    return genomes, genes, profiles


def profile_text(genomes, genes, profiles):
    return '\t'.join(['#Genome'] + genes) + '\n' + ''.join('{0}\t{1}\n'.format(genome, '\t'.join(str(a) for a in row)) for genome, row in zip(genomes, profiles))


def dist_text(genomes, distances):
    return '    {0}\n'.format(len(genomes)) + ''.join('{0} {1}\n'.format(genome, ' '.join(d.astype(str))) for genome, d in zip(genomes, distances))


def writeCGAV(prefix, ortho, pCore, device=None):
    """PEPPAN_parser.py:145-170: writes <prefix>_CGAV.profile, <prefix>_CGAV.dist and <prefix>_CGAV.nwk - the tree by rapidnj when it is installed (:168), as the
    reference makes it; else by K21 from the distances in memory (njtree.py: float64 where rapidnj computes in float32, the same five printed digits)"""
    genomes, genes, profiles = cgav_profiles(ortho, pCore)
    with open('{0}_CGAV.profile'.format(prefix), 'w') as fout:
        fout.write(profile_text(genomes, genes, profiles))
    distances = getDistance(np.array(profiles), device)
    with open('{0}_CGAV.dist'.format(prefix), 'w') as fout:
        fout.write(dist_text(genomes, distances))
    logger('Core gene allelic variation profile is saved in {0}_CGAV.profile'.format(prefix))
    rapidnj = shutil.which('rapidnj')
    if rapidnj is None:
        if len(genomes) < 2:
            logger('fewer than two genomes: {0}_CGAV.nwk is skipped'.format(prefix))
            return
        tree = njtree.newick(njtree.nj_trees([distances], device)[0], genomes) + '\n'
    else:
        tree = subprocess.run([rapidnj, '-i', 'pd', '{0}_CGAV.dist'.format(prefix)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True).stdout
    with open('{0}_CGAV.nwk'.format(prefix), 'w') as fout:
        fout.write(tree.replace("'", ''))
    logger('Core gene allelic variation tree is saved in {0}_CGAV.nwk'.format(prefix))
