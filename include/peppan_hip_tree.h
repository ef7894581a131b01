/* K21 of libpeppan_hip.so: neighbour-joining trees, the two rapidnj calls of the reference (PEPPAN.py:19, 409-417: `rapidnj -i fa -t d` per paralogous
 * group of filt_per_group; PEPPAN_parser.py:168: `rapidnj -i pd` behind writeCGAV).
 *
 * A header of its own only because tests/test_abi.py pins include/peppan_hip.h to the prototypes of ABI 19: these functions are additive, PEP_ABI_VERSION
 * stays 19 and PEP_CALL_COUNT stays 6.  The pull request that may next touch tests/test_abi.py folds this file into include/peppan_hip.h (as ABI 19 did
 * with the headers of K18 - K20) and gives K21 a pep_call_times selector in place of the `ms` parameters below.
 *
 * Conventions as in peppan_hip.h: int status, the message behind pep_last_error, a null context is PEP_ERR_ARG before anything else, caller-owned inputs
 * are only read, everything is checked on the host before a launch. */
#ifndef PEPPAN_HIP_TREE_H
#define PEPPAN_HIP_TREE_H

#include "peppan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* trees of up to this many leaves are joined by one workgroup each (all of them in one launch per size class); larger ones by a chain of launches, two per join */
#define PEP_NJ_BLOCK_LEAVES 256
/* leaves of one tree */
#define PEP_NJ_MAX_LEAVES 8192
/* bytes of distance matrices of one pep_nj_trees call (8 * dist_off[n_trees]); bytes of pair counts of one pep_kimura_pairs call */
#define PEP_NJ_MAX_BYTES (1ull << 30)

/* K21a: the three pair counts of Kimura's distance, which `rapidnj -i fa` computes from the FASTA the reference writes (PEPPAN.py:19, 409-417).  Rows and
 * groups exactly as for pep_allele_diff: base-5 packed rows, row_off[n_rows + 1], row_len[n_rows], grp_off[n_groups + 1], grp_rows = row indices, the rows
 * of a group of one row_len.  For every pair a < b of group g, in the row-major order of pep_allele_diff's packed triangle, three int32 at
 * out[out_off[g] + 3 * pair]: the columns where both codes are 1..4 (comparable), among those the columns A <-> G or C <-> T (transitions: codes 1 <-> 3,
 * 2 <-> 4), and the other mismatching comparable columns (transversions).  Raw counts, without pep_allele_diff's + 1 / + 2; the logarithm is host work
 * (peppan_amd/njtree.py: kimura_distances).  out_off[g] and out_cap count int32 values.  Empty batches, empty groups and groups of one row are legal.
 * PEP_ERR_ARG: what pep_allele_diff names for rows and groups, an output that runs past out_cap or overlaps another group's.  PEP_ERR_LIMIT: more than
 * PEP_NJ_MAX_BYTES of counts, or what pep_allele_diff names for the bit planes; the message says how much was asked for.
 * ms (optional, double[4]): ms[0], ms[1] the kernel times - bit planes, pairs - when pep_set_timing is 2, zeros otherwise. */
int pep_kimura_pairs(pep_ctx *ctx, const uint8_t *packed, const uint64_t *row_off, const uint32_t *row_len, uint64_t n_rows, uint32_t n_groups,
                     const uint64_t *grp_off, const uint32_t *grp_rows, int32_t *out, const uint64_t *out_off, uint64_t out_cap, double *ms);

/* K21b: neighbour joining over a batch of distance matrices (what rapidnj does for PEPPAN.py:416 and PEPPAN_parser.py:168).  Matrix t is row-major
 * double[n][n], n = n_leaves[t], at dist + dist_off[t]; only entries with row < column are read.  dist_off and out_off have n_trees + 1 entries, the last
 * one the length of the array (of dist in doubles; of node and length in entries): dist_off[t] + n * n <= dist_off[t + 1] and out_off[t] + 2 n - 3 <=
 * out_off[t + 1] (n = 2: + 2), so no two trees overlap and none runs past its array.  Entries of node / length between two trees are zeroed.
 *
 * The arithmetic, every operation one correctly rounded double operation (nothing is contracted into a fused multiply-add): slots 0 .. n - 1 hold the
 * leaves, node[slot] the node id (leaves 0 .. n - 1, join s creates node n + s).  r[k] = D[k,0] + D[k,1] + .. from 0.0, left to right, the diagonal as 0.
 * With m live slots, m > 3: over live a < b, Q = ((m - 2) * D[a,b] - r[a]) - r[b]; the smallest Q below +infinity wins (a NaN never), ties go to the smaller
 * a, then the smaller b; when no Q is below +infinity, the first two live slots.  la = 0.5 * D[a,b] + (r[a] - r[b]) / (2 * (m - 2)), lb = D[a,b] - la.  For every other
 * live k: du = ((D[a,k] + D[b,k]) - D[a,b]) * 0.5, r[k] = ((r[k] - D[a,k]) - D[b,k]) + du, D[a,k] = D[k,a] = du.  Then r[a] = 0.5 * ((r[a] + r[b]) - m * D[a,b]),
 * slot a becomes node n + s, slot b is retired.  At m = 3, live a < b < c: la = 0.5 * ((D[a,b] + D[a,c]) - D[b,c]), lb = D[a,b] - la, lc = D[a,c] - la.
 * n = 2: both leaves get D[0,1].
 * Output of tree t at out_off[t], 2 n - 3 entries of node[] and length[]: for s = 0 .. n - 4 the two joined node ids (slot a's first) and la, lb; then the
 * last three node ids in slot order with la, lb, lc; n = 2: two entries.  One exception, so that the text of a three-leaf tree is rapidnj's character for
 * character: n = 3 gives leaves 1, 0, 2 with lb, la, lc, the order rapidnj prints them in (('B':..,'A':..,'C':..);).
 * PEP_ERR_ARG: a null table, n < 2, offsets that overlap or run past their arrays, a distance of the read triangle that is not finite (the message names
 * tree, row and column).  PEP_ERR_LIMIT: n > PEP_NJ_MAX_LEAVES, more than PEP_NJ_MAX_BYTES of matrices; the message says how much was asked for.
 * n_trees == 0 is legal.
 * ms (optional, double[4]): ms[0] the time of the one-workgroup-per-tree kernels, ms[1] of the launch chains, when pep_set_timing is 2, zeros otherwise. */
int pep_nj_trees(pep_ctx *ctx, const double *dist, const uint64_t *dist_off, const uint32_t *n_leaves, uint32_t n_trees, uint32_t *node, double *length,
                 const uint64_t *out_off, double *ms);
/* every check of pep_nj_trees that does not read a distance, without a context or a device: its code, its text in msg[msg_cap] (cut to fit) */
int pep_nj_trees_check(const uint32_t *n_leaves, uint32_t n_trees, const uint64_t *dist_off, const uint64_t *out_off, char *msg, uint64_t msg_cap);

#ifdef __cplusplus
}
#endif

#endif
