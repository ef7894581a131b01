/* K25 of libpeppan_hip.so: the tree cutting of filt_per_group (PEPPAN.py:424-482), which the reference does with ete3, for a batch of trees.
 *
 * A header of its own for the reason include/peppan_hip_tree.h gives: tests/test_abi.py pins include/peppan_hip.h to the prototypes of ABI 19; these
 * functions are additive, PEP_ABI_VERSION stays 19 and PEP_CALL_COUNT stays 6.  Conventions as in peppan_hip.h.
 *
 * What is restated.  :424-482 are a computation on the UNROOTED tree: a node's score is a sum over (leaves below) x (the component's other leaves) of a
 * symmetric matrix, so it belongs to the branch's bipartition, whichever side is "below"; the two children of the root are one bipartition with one length
 * (:440-442); the smallest leaf name, not the direction of the cut, decides which part stays in place (:466-467); pruning a subtree and suppressing the node
 * of degree two (:462-465) leaves the tree induced on the remaining leaves, whose branches are the distinct non-trivial restrictions of the original
 * bipartitions.  So the device works on bit sets of leaves and never roots a tree.  The rooting shows in exactly one place: an exact tie of the first two
 * sort keys of :458 between two DIFFERENT bipartitions, where the reference reads n.dist, which its doubling of the root branch (:440-442) makes depend on
 * ete3's midpoint rooting.  AT THESE TIES, AND ONLY THERE, THE REFERENCE'S CHOICE IS NOT RESTATED: the rule below decides, and every such tie is counted in
 * n_ties for the caller to see.  ete3 itself cannot be run where this project is built; the contract therefore stands on two legs: PEPPAN.py:326-484
 * themselves, run over a small stand-in for the ete3 calls they make, rooted two ways (tests/golden/make_golden_treecut.py), and a numpy restatement of the
 * definition below, operation for operation (tests/treecut_helpers.py), which the device equals bit for bit.
 *
 * Input of tree t (n = n_leaves[t] leaves, 2 <= n <= PEP_NJ_MAX_LEAVES; words = (n + 63) / 64):
 *   leaves         0 .. n - 1, in the order of the reference's leaf names read as integers (the leader rows g[0], ascending)
 *   branches       B = branch_off[t + 1] - branch_off[t] of them, 1 <= B <= 2 n (2 n - 3 from a text of njtree.newick; 2 for n = 2).  Branch e: the bit
 *                  set of the leaves on one of its sides, `words` 64-bit words at sets + set_off[t] + e * words (leaf l is bit l % 64 of word l / 64),
 *                  and length[branch_off[t] + e], the printed %.5g value, since the reference parses the text
 *   W0, W1         incompatible[:, :, 0] and [:, :, 1] (:400-404) compacted to the leaves, row-major double[n][n] at w0 / w1 + mat_off[t]; symmetric,
 *                  every entry finite and >= 0
 *   strong[leaf]   at strong + leaf_off[t]: non-zero when mat[leader, 4] >= (clust_identity - 0.02) * 10000, which the host evaluates in float64 (:469)
 *   cap[t]         the iterations of one component (:435; the reference's 3000)
 * Every offsets table has n_trees + 1 entries, the last one the length of its arrays: leaf_off[t] + n <= leaf_off[t + 1], mat_off[t] + n * n <=
 * mat_off[t + 1], set_off[t] + B * words <= set_off[t + 1]; branch_off is dense.
 *
 * The definition.  M[a][b] = W1[a][b] where W0[a][b] > W1[a][b], else 0.0.  The queue of components (gene_phys, :431-473) starts as [all leaves]; component
 * q is taken when its turn comes, T its leaves, t0 the smallest of them.  At most cap[t] times:
 *   1. if W0[a][b] <= W1[a][b] for all a, b of T (the diagonal included, :438) the component is finished.
 *   2. every branch e whose far side F = (side_e or its complement, whichever does not hold t0) restricted to T is not empty is a candidate; C = T \ F.
 *      For each of the three matrices X = W0, W1, M the sum over a in F, b in C in this order: for a row a, lane l = 0 .. 63 holds p[l] = 0.0 + X[a][l] +
 *      X[a][l + 64] + .. over the b = l, l + 64, .. that are in C, ascending; then for off = 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l ^ off] for all l at once;
 *      rowsum(a) = p[0].  s = 0.0, then s = s + rowsum(a) over the rows a of F, ascending.  This gives s0, s1, m.
 *      ic0 = s0 / (s1 > 1.0 ? s1 : 1.0); key = ic0 * sqrt(m) (:451-456).  Every operation is one correctly rounded double operation, nothing is contracted;
 *      the order depends on T and the branch alone, not on the batch, the launch geometry or the path.
 *   3. among the candidates with ic0 > 1 whose key is no NaN the largest (key, ic0) wins (:456-458); branches with the same F are ONE candidate.  None: the
 *      component is finished (:471-472).  Several different F with the winner's (key, ic0): the larger sum of the lengths of its inducing branches (0.0 +
 *      length, ascending branch index) wins, then the smaller smallest leaf of F, then the lower branch index; n_ties grows by the number of the OTHER F.
 *   4. the cut: T \ F keeps the component's place in the queue (:466-468); F is appended to the queue when one of its leaves is strong (:469-470) and is
 *      dropped otherwise, its leaves belonging to no output.
 * Output of tree t: part[leaf_off[t] + leaf] the index of the leaf's component in the queue - the order of the reference's returned list -, -1 for a dropped
 * leaf; counts[4 t ..] = n_parts, n_cuts, n_ties, 0; and for cut c = 0 .. n_cuts - 1 (at most n - 1) the record i = leaf_off[t] + c: log_where[2 i] the
 * component's index, log_where[2 i + 1] the lowest inducing branch index; log_val[4 i ..] = s0, s1, m, key.  Entries of part between two trees are -1, log entries
 * behind a tree's records zero.
 *
 * Two paths that give identical bits: trees of up to PEP_NJ_BLOCK_LEAVES leaves are cut by one workgroup each, all of them in one launch, the bit sets in
 * LDS; larger ones by a chain of launches, two per iteration (score, select-and-apply), enqueued PEP_CUT_ROUND iterations at a time with one read of the
 * tree's `done` flag between rounds.  path: PEP_CUT_AUTO, PEP_CUT_BLOCK (PEP_ERR_LIMIT for a larger tree), PEP_CUT_CHAIN (any tree).
 *
 * PEP_ERR_ARG: a null table; n < 2; offsets that overlap or run past their arrays; B < 1 or B > 2 n; a branch that is no bipartition of the tree's leaves
 * (a bit beyond leaf n - 1, an empty side, a side with every leaf); branches that are not pairwise compatible; an unknown path - all of these by
 * pep_tree_cut_check as well -; and by pep_tree_cut alone, which reads them: a W entry or a length that is not finite, a negative W entry, W not symmetric.
 * PEP_ERR_LIMIT: n > PEP_NJ_MAX_LEAVES, PEP_CUT_BLOCK for n > PEP_NJ_BLOCK_LEAVES, more than PEP_NJ_MAX_BYTES of one matrix (8 * mat_off[n_trees]) or of
 * bit sets; the message says how much was asked for.  n_trees == 0 is legal.
 * ms (optional, double[4]): ms[0] the time of the preparation and the one-workgroup kernel, ms[1] of the launch chains, when pep_set_timing is 2, else zeros. */
#ifndef PEPPAN_HIP_TREECUT_H
#define PEPPAN_HIP_TREECUT_H

#include "peppan_hip_tree.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PEP_CUT_AUTO 0
#define PEP_CUT_BLOCK 1
#define PEP_CUT_CHAIN 2
/* iterations of a launch chain that are enqueued between two reads of the `done` flag */
#define PEP_CUT_ROUND 8
/* the reference's iterations per component (PEPPAN.py:435) */
#define PEP_CUT_DEFAULT_CAP 3000

int pep_tree_cut(pep_ctx *ctx, const uint32_t *n_leaves, uint32_t n_trees, const uint64_t *leaf_off, const uint64_t *mat_off, const uint64_t *branch_off,
                 const uint64_t *set_off, const uint64_t *sets, const double *length, const double *w0, const double *w1, const uint8_t *strong,
                 const uint32_t *cap, uint32_t path, int32_t *part, int32_t *counts, int32_t *log_where, double *log_val, double *ms);
/* every check of pep_tree_cut that reads no matrix and no length, without a context or a device: its code, its text in msg[msg_cap] (cut to fit) */
int pep_tree_cut_check(const uint32_t *n_leaves, uint32_t n_trees, const uint64_t *leaf_off, const uint64_t *mat_off, const uint64_t *branch_off,
                       const uint64_t *set_off, const uint64_t *sets, uint32_t path, char *msg, uint64_t msg_cap);

#ifdef __cplusplus
}
#endif

#endif
