/* K26 of libpeppan_hip.so: the front half of every round of filt_genes (PEPPAN.py:546-624, and :641-656 for `--orthology sbh`) for one batch of genes:
 * what stands between the gene scores and the `to_run` list of filt_per_group.
 *
 * A header of its own for the reason include/peppan_hip_tree.h gives: tests/test_abi.py pins include/peppan_hip.h to the prototypes of ABI 19; these
 * functions are additive, PEP_ABI_VERSION stays 19 and PEP_CALL_COUNT stays 6.  Conventions as in peppan_hip.h.
 *
 * Tables.  A gene's table is int64[n, 7] rows of the .tab store: 0 exemplar, 1 genome, 2 score x 10^4, 3 identity x 10^4, 4 a copy of column 3, 5 locus id,
 * 6 hit count.  A batch is the tables of its genes one behind the other, handed over column by column: gene g owns the rows gene_off[g] .. gene_off[g + 1] - 1;
 * gene_off has n_genes + 1 entries, starts at 0 and never falls.  The conflict lists (load_conflict, :511-523) are one CSR table over the batch's rows: row r
 * owns cfl[cfl_off[r] .. cfl_off[r + 1] - 1], every value other_locus * 10 + kind (>= 0), in the order of the .conflicts store; cfl_off has gene_off[n_genes]
 * + 1 entries, starts at 0 and never falls.  Locus ids lie in [0, n_loci), n_loci <= PEP_PREP_MAX_LOCI, and no locus comes twice in one gene's table.
 *
 * Stage A, pep_batch_screen (:548-562; device, order-free per gene because `used` is not written in that loop).  used_state[locus] says what `used` holds for
 * the locus: 0 absent, 1 present with a value <= 0, anything else present with a value > 0.  For gene g with m = max(col3) over its rows (m > 0):
 *   out4[r] = trunc((double)(10000 * col3[r]) / (double)m) - the product is an integer one, the quotient ONE float64 division, the cast cuts toward zero (:552);
 *   state 0: out3[r] = col3[r] and the row counts for present[g] = max(0, out4 over these rows); state 1: out3[r] = -col3[r]; else: out3[r] = 0 (:553-558);
 *   excluded[g] = (double)present[g] < threshold, where threshold is (clust_identity - 0.02) * 10000 as the host evaluated it in float64 (:559).
 * The rows that go on are those with out3 != 0 (:562): the caller's gather.
 *
 * Stage B, pep_batch_unsure_walk (:579-593; host C++, no context, because one set `used2` of locus ids is shared by the whole round: a bitmap over
 * [0, n_loci) here).  The genes come in the caller's order - falling score, stable (:580).  Per gene, with pos = the number of its rows with col3 > 0:
 *   unsure = the number of rows with col3 > 0 whose locus is in used2; when (double)unsure >= (double)pos * 0.6 the gene is popped (popped[g] = 1) and nothing
 *   else happens to it (:583-585; pos = 0 pops).  Otherwise, row by row in table order, negative rows included: when the row's locus is not in used2 every
 *   value / 10 of its list enters used2 - at once, so a list can close the door on a later row of the same table; the row's own locus does not enter
 *   (:588-590).  Then every third row with col3 < 0 is negated back, counting from the first one (:591-592).  The rows with col3 > 0 go on (:593).
 * col3 is rewritten in place.
 *
 * Stage C, pep_batch_prune (device, order-free per gene: `used2` is a new set for every gene, :604 / :648).  Rows are named by their index within the gene's
 * table (source rows); `order` is the current sequence of source rows, at first 0 .. n - 1.  Conflict values that name a locus outside the gene's own table
 * have no effect in this stage.  Of an order: G = the number of distinct genomes, best(k) = the first row of the order with the genome of row k (:600),
 * rs(k) = (double)col4[k] / (double)col4[best(k)], one float64 division (:601).  walk(order): used2 empty; row by row, a row whose locus is in used2 is dropped,
 * of any other row every value / 10 of its list enters used2 (:604-610).
 *  mode PEP_PREP_NJ (nj and ml, :596-624):
 *   1. when n >= 2 G: the order sorted by falling column 2; walk; the survivors sorted by falling column 3; G, best, rs anew (:602-613).
 *   2. when n > 3 G and n > 1000 (n now the rows left): cut = the (3 G)-th largest rs; when cut >= clust_identity, cut = the (6 G + 1)-th largest rs when
 *      n > 6 G, else clust_identity; the rows with rs >= cut stay (:614-619).  The k-th largest is taken on the bit patterns of the doubles, a NaN (0 / 0)
 *      above every number; NaN >= x and x >= NaN are false.  (The reference's sorted() gives no defined order to a list that holds a NaN.)
 *   3. inparalog = some genome has more than one of the rows left (:620).  final = (not inparalog and (double)min(col3) >= final_threshold) or at most one row
 *      left (:621), final_threshold being 10000 * clust_identity as the host evaluated it; every other gene is a `to_run` entry (:624).
 *  mode PEP_PREP_SBH (:641-656): rs(k) = min((double)col2[k] / (double)col2[best(k)], (double)col4[k] / (double)col4[best(k)]), a NaN quotient making rs NaN; the
 *   rows with rs >= clust_identity stay, a NaN dropping the row; walk in table order, WITH WHAT :653 COMPUTES: it adds the one-element list [locus * 10] to
 *   the row's list, which is an array of the store wherever it is not empty, and numpy sums the two element by element - so of a kept row with a list
 *   every (value + locus * 10) / 10 = value / 10 + locus enters used2, and of a kept row without one its own locus, which no other row carries; final
 *   always; inparalog as above.
 * TIES.  The reference sorts with numpy's default, unstable sort, whose order of equal keys depends on the machine's SIMD path.  THE REFERENCE'S ORDER OF
 * EQUAL KEYS IS NOT RESTATED: here equal keys keep their current order in both sorts (the position is the low key).  Two rows that tie in column 2 at :603
 * can change which row the walk keeps: n_ties counts, per call, the genes in which that sort met two equal keys.  Ties in column 3 at :611 change the
 * order of the rows alone, never a value: equal |column 3| within one table means equal column 4.
 * Output of gene g: rows[out_off[g] .. out_off[g + 1] - 1] the source rows left, in final order (the host gathers mat[rows]); inparalog[g]; is_final[g].
 *
 * Two paths of pep_batch_prune that give identical bits: a gene of up to PEP_PREP_LDS_ROWS rows has its working arrays (the order, a sort buffer, best) in
 * LDS, a larger one in a slot of the context's workspace; one workgroup per gene either way, both in one call.  path: PEP_PREP_AUTO, PEP_PREP_LDS
 * (PEP_ERR_LIMIT for a larger gene), PEP_PREP_WS (any gene).
 *
 * A DELIBERATE DIFFERENCE lies in front of these functions: for a member of the .conflicts store that does not exist the reference raises inside a pool
 * worker; peppan_amd.paralogfilter reads it as "no conflicts" (empty lists).
 *
 * PEP_ERR_ARG (the message names the gene): a null table; gene_off or cfl_off that does not start at 0, falls (two genes or lists would overlap) or, for
 * cfl_off, runs past the budget below; an empty gene in C; max(col3) <= 0 in A; a locus id outside [0, n_loci); a locus twice in one gene's table; a conflict
 * value below 0 or (B) naming a locus outside [0, n_loci); a genome id outside [0, 2^32); column 3 or 4 (C: column 2 as well, to 2^62) of 2^31 or more in
 * magnitude; an unknown mode or path; n_loci > PEP_PREP_MAX_LOCI.  PEP_ERR_LIMIT, with the amount asked for: a gene of more than PEP_PREP_MAX_ROWS rows;
 * PEP_PREP_LDS for a gene of more than PEP_PREP_LDS_ROWS rows; more than PEP_PREP_MAX_CFL_BYTES of conflict values (8 bytes each) in one call.  n_genes == 0
 * is legal.  Every check is made by the ..._check twin as well, without a context or a device; the context stays usable after a refusal.
 * ms (optional, double[2]): the kernel time of the call when pep_set_timing is 2, else zeros. */
#ifndef PEPPAN_HIP_BATCHPREP_H
#define PEPPAN_HIP_BATCHPREP_H

#include "peppan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PEP_PREP_NJ 0
#define PEP_PREP_SBH 1
#define PEP_PREP_AUTO 0
#define PEP_PREP_LDS 1
#define PEP_PREP_WS 2
/* rows of one gene whose working arrays stay in LDS (a power of two) */
#define PEP_PREP_LDS_ROWS 4096
/* rows of one gene: 2 000 genomes x 32 copies */
#define PEP_PREP_MAX_ROWS 65536
/* conflict values of one call, in bytes */
#define PEP_PREP_MAX_CFL_BYTES (1ull << 31)
#define PEP_PREP_MAX_LOCI (1ull << 40)

int pep_batch_screen(pep_ctx *ctx, uint32_t n_genes, const uint64_t *gene_off, const int64_t *col3, const int64_t *locus, const uint8_t *used_state,
                     uint64_t n_loci, double threshold, int64_t *out3, int64_t *out4, int64_t *present, uint8_t *excluded, double *ms);
int pep_batch_screen_check(uint32_t n_genes, const uint64_t *gene_off, const int64_t *col3, const int64_t *locus, uint64_t n_loci, char *msg, uint64_t msg_cap);
int pep_batch_unsure_walk(uint32_t n_genes, const uint64_t *gene_off, int64_t *col3, const int64_t *locus, const uint64_t *cfl_off, const int64_t *cfl,
                          uint64_t n_loci, uint8_t *popped, char *msg, uint64_t msg_cap);
int pep_batch_unsure_walk_check(uint32_t n_genes, const uint64_t *gene_off, const int64_t *col3, const int64_t *locus, const uint64_t *cfl_off,
                                const int64_t *cfl, uint64_t n_loci, char *msg, uint64_t msg_cap);
int pep_batch_prune(pep_ctx *ctx, uint32_t mode, uint32_t n_genes, const uint64_t *gene_off, const int64_t *genome, const int64_t *col2, const int64_t *col3,
                    const int64_t *col4, const int64_t *locus, const uint64_t *cfl_off, const int64_t *cfl, uint64_t n_loci, double clust_identity,
                    double final_threshold, uint32_t path, uint64_t *out_off, int32_t *rows, uint8_t *inparalog, uint8_t *is_final, uint64_t *n_ties, double *ms);
int pep_batch_prune_check(uint32_t mode, uint32_t n_genes, const uint64_t *gene_off, const int64_t *genome, const int64_t *col2, const int64_t *col3,
                          const int64_t *col4, const int64_t *locus, const uint64_t *cfl_off, const int64_t *cfl, uint64_t n_loci, uint32_t path, char *msg,
                          uint64_t msg_cap);

#ifdef __cplusplus
}
#endif

#endif
