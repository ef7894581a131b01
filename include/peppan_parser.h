/* peppan_parser.h - K20 of libpeppan_hip.so: the two counting loops of PEPPAN_parser.
 *
 * A header of its own beside peppan_hip.h, with a version of its own, as peppan_synteny.h and peppan_genestruct.h are: the entry points
 * below were added without touching the main interface.  Same conventions: C ABI, functions returning int return PEP_OK (0) or a negative
 * PEP_ERR_* code, nothing is ever silently dropped, and a context function leaves its message in pep_last_error().
 *
 * Reference interface each entry point replaces (file:line in zheminzhou/PEPPAN):
 *   pep_rarefaction_curves (+ _check)   the n_iter x n_genomes loop of writeCurve: genes seen in at least one / in all of the first
 *                                       k + 1 genomes of every random genome order                      PEPPAN_parser.py:74-80
 *   pep_profile_pairs (+ _check)        the pair loop of getDistance: per pair of allelic profiles the genes both carry and the
 *                                       genes where both carry the same allele                          PEPPAN_parser.py:172-179
 */
#ifndef PEPPAN_PARSER_H
#define PEPPAN_PARSER_H
#include "peppan_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PEP_PARSER_ABI_VERSION 1

/* a presence matrix holds fewer genes than this (the counts travel as int32) */
#define PEP_PARSER_MAX_GENES (1ull << 31)
/* n_genomes * n_iter of one pep_rarefaction_curves call stays below this (2 GiB of int32 pairs) */
#define PEP_PARSER_MAX_CURVE_POINTS (1ull << 28)
/* profiles of one pep_profile_pairs call (two n x n int32 matrices of 1 GiB each at the limit) */
#define PEP_PARSER_MAX_PROFILES 16384

int pep_parser_version(void);

/* K20a: the loop of writeCurve (PEPPAN_parser.py:74-80).  bits: the presence matrix as bit rows, uint64[n_genomes][W] with
 * W = (n_genes + 63) / 64, gene e of genome g at bit e % 64 of bits[g * W + e / 64]; the bits of the last word at and above n_genes (the
 * padding) are zero.  orders: uint32[n_iter][n_genomes], every row a permutation of 0 .. n_genomes - 1.
 *     curves[(k * n_iter + t) * 2 + 0]   genes present in at least one of the genomes orders[t][0 .. k]   (np.sum(genes >= 1))
 *     curves[(k * n_iter + t) * 2 + 1]   genes present in all of them                                     (np.sum(genes >= k + 1))
 * - the reference's array curves[n_genomes][n_iter][2], as int32.  Integer arithmetic only; no size of n_genomes, n_genes or n_iter below
 * the limits is special.  curves is written only when the call succeeds; on any error the context stays usable.  Everything is checked on
 * the host before anything is launched:
 * PEP_ERR_ARG: a null table, n_genomes, n_genes or n_iter of 0, an order row that is no permutation (the message names the row and the
 * entry), a padding bit that is set (the message names the genome).  PEP_ERR_LIMIT: n_genes >= PEP_PARSER_MAX_GENES, n_genomes * n_iter >=
 * PEP_PARSER_MAX_CURVE_POINTS.
 * pep_rarefaction_curves_check runs exactly these checks: no context, no device; the message goes to msg (msg_cap bytes, 0-terminated). */
int pep_rarefaction_curves(pep_ctx *ctx, const uint64_t *bits, uint32_t n_genomes, uint64_t n_genes, const uint32_t *orders, uint32_t n_iter, int32_t *curves);
int pep_rarefaction_curves_check(const uint64_t *bits, uint32_t n_genomes, uint64_t n_genes, const uint32_t *orders, uint32_t n_iter, char *msg, uint64_t msg_cap);

/* K20b: the pair loop of getDistance (PEPPAN_parser.py:172-179).  profiles: int32[n][n_genes], a value > 0 is an allele, anything else
 * "no allele".  For i < j
 *     presence[i * n + j]   genes with profiles[i][e] > 0 and profiles[j][e] > 0
 *     shared[i * n + j]     those of them with profiles[i][e] == profiles[j][e]
 * Every other entry of the two int32[n][n] matrices is 0.  Written only when the call succeeds.
 * PEP_ERR_ARG: a null table, n or n_genes of 0.  PEP_ERR_LIMIT: n > PEP_PARSER_MAX_PROFILES, n_genes >= PEP_PARSER_MAX_GENES.
 * pep_profile_pairs_check runs exactly the checks of the sizes: no context, no device. */
int pep_profile_pairs(pep_ctx *ctx, const int32_t *profiles, uint32_t n, uint64_t n_genes, int32_t *shared, int32_t *presence);
int pep_profile_pairs_check(uint32_t n, uint64_t n_genes, char *msg, uint64_t msg_cap);

/* of the newest pep_rarefaction_curves and the newest pep_profile_pairs of the context: their kernel times in ms when pep_set_timing is 2
 * (else 0), and the bytes the newer of the two calls sent to the device and to the host */
int pep_parser_times(const pep_ctx *ctx, double *ms_curves, double *ms_pairs, uint64_t *bytes_to_device, uint64_t *bytes_to_host);

#ifdef __cplusplus
}
#endif
#endif
