/* K24 of libpeppan_hip.so: the allele pass of the reference's write_output (PEPPAN.py:1391-1472) for a whole prediction table - which window
 * determineGeneStructure is to look at for every prediction, which bytes are its allele, and which number that allele gets in its gene.
 *
 * A header of its own for the reason include/peppan_hip_tree.h gives: tests/test_abi.py pins include/peppan_hip.h to the prototypes of ABI 19.  These
 * functions are additive, PEP_ABI_VERSION stays 19 and PEP_CALL_COUNT stays 6; the pull request that may next touch tests/test_abi.py folds this file into
 * include/peppan_hip.h and gives K24 a pep_call_times selector in place of the `ms` parameter below.
 *
 * Conventions as in peppan_hip.h: int status, the message behind pep_last_error (or in msg[msg_cap] for the function without a context), a null context
 * is PEP_ERR_ARG before anything else, caller-owned inputs are only read, everything is checked on the host before a launch.
 *
 * The host (peppan_amd/outalleles.py) resolves names to indices, evaluates the reference's float expressions in float64 and formats the texts; the
 * device sees integers and bytes only.
 *
 * ---- the inputs.  nt: contigs one after another, contig c at nt[contig_off[c] .. contig_off[c + 1]), ASCII as the reference holds them.  The
 * representative of a gene that has one (clust_ref) is appended as a contig of its own: seed_contig[g] names it, -1 = gene g has no seed.  Row i of the
 * prediction table, in the table's order, is the PEP_OUTA_COLS int32 values rows[PEP_OUTA_COLS i ..]:
 *   PEP_OUTA_GENE    index of column 0 among the distinct names (0 .. n_genes - 1; not read for a skipped row)
 *   PEP_OUTA_CONTIG  index of column 5 (rows of one contig name carry one index: the neighbour search compares it)
 *   PEP_OUTA_FLAGS   PEP_OUTA_MISC: column 15 is misc_feature; PEP_OUTA_NONAME: column 0 is empty; PEP_OUTA_SECONDARY: column 4 is not empty;
 *                    PEP_OUTA_MINUS: column 11 is not '+'
 *   PEP_OUTA_S, _E   columns 9 and 10, 1-based, inclusive: s, e
 *   PEP_OUTA_PART    column 1        PEP_OUTA_QS, _QE  columns 7 and 8        PEP_OUTA_REFLEN  column 12        PEP_OUTA_CLEN  column 13 as it stands at :1390
 *   PEP_OUTA_VARY    allowed_vary = int(col12 * (1 - pseudogene) + 0.01)  (:1408)
 *   PEP_OUTA_SVMIN   0: no structural-variation test; else the smallest allele length that passes it, ceil(pseudogene * len(representative))  (:1461)
 * look9 (optional, int32[n_rows]): column 9 as a row of an EARLIER batch of PEP_OUTA_BATCH rows shows it to a '-' row i with i % PEP_OUTA_BATCH < 5 -
 * the reference writes determineGeneStructure's results back after every batch (:1468-1472), so those rows alone see updated neighbours.  NULL: s.
 *
 * ---- the plan of row i, plan[PEP_OUTA_PLAN_COLS i ..]: class, s2, e2, lp, a, len.
 *   PEP_OUTA_SKIPPED   PEP_OUTA_MISC or PEP_OUTA_NONAME (:1405).  Nothing else of the row is read or checked; it is in no class, its other outputs are zero.
 *   PEP_OUTA_FRAGMENT  column 1 > 1 or e - s + 1 < col12 - allowed_vary (:1415).  s2 = s, e2 = e, lp = 0; the allele is [s - 1, e) of the contig.
 *   PEP_OUTA_INTACT    otherwise (:1422-1458), with 3 int(x / 3) truncating toward zero.  pred2 is, for '+', the LAST row that is not PEP_OUTA_MISC among rows
 *                      i + 1 .. i + 4, for '-' the FARTHEST such row among i - 1 .. i - 5, the walk ending at the table's end or at the first row of another contig.
 *                        '+'  e2 = e + min(3 int((clen - e) / 3), pred2 ? 3 int((e(pred2) + 300 - e) / 3) : 600 + col12 - col8)
 *                             s2 = s - min(3 int((s - 1) / 3), 60 + col7 - 1);  lp = s - s2, rp = e2 - e
 *                        '-'  s2 = s - min(3 int((s - 1) / 3), pred2 ? 3 int((s - s9(pred2) + 300) / 3) : 600 + col12 - col8)
 *                             e2 = e + min(3 int((clen - e) / 3), 60 + col7 - 1);  lp = e2 - e, rp = s - s2
 *                      The window of determineGeneStructure is [s2 - 1, e2).  The allele is window[lp : len - rp] with Python's slice semantics: [s - 1, e) when
 *                      rp >= 0, and the shorter [s - 1, e2) on '+' / [s2 - 1, e) on '-' when rp < 0 (a nested neighbour) - empty when that is no span.
 *   PEP_OUTA_STRUCTVAR intact, and len < PEP_OUTA_SVMIN: the row does not go to determineGeneStructure (:1461-1462).
 * a: the 0-based position of the allele's first byte in its contig, len: its bytes.  On '-' the allele is those bytes upper-cased, complemented and reversed,
 * everything outside ACGTN becoming N (modules/configure.py:152-154); on '+' the bytes as they stand.
 *
 * ---- the numbering.  Two rows that are not skipped are in one class when their genes and their allele bytes are equal; the seed of a gene is in front of all
 * its rows.  first[i]: the smallest row index of the class of row i, -1 when that is the seed, -2 for a skipped row.  rank[i]: 1 + the number of classes of
 * the gene whose first member comes before this one's - the number the reference's dictionary gives (:1420, :1455-1457), the seed being 1.  tflag[i]: 1 when
 * the allele's id carries the 't' prefix, a property of the class's first member: never for the seed, always for a fragment, for an intact row unless
 * PEP_OUTA_SECONDARY is clear, col7 = 1 and col8 = col12 (:1454).  None of it depends on the order in which the device worked.
 *
 * ---- what is refused, PEP_ERR_ARG with the row in the message, for a row that is not skipped: s < 1; e < s - 1; e beyond the actual contig; col7 < 1;
 * lp < 0 (the reference's slice would wrap); e2 < s2 - 1 (no window); e2 beyond the actual contig.  (s2 >= 1 follows from s >= 1.)  Also PEP_ERR_ARG: a
 * null table; contig_off that does not start at 0 or decreases; a gene, contig or seed index out of range; flag bits beyond the four; key_bits > 31.
 * PEP_ERR_LIMIT: a contig of PEP_OUTA_MAX_CONTIG bytes or more (positions are int32); n_rows + n_genes of PEP_OUTA_MAX_ITEMS or more. */
#ifndef PEPPAN_HIP_OUTALLELES_H
#define PEPPAN_HIP_OUTALLELES_H

#include "peppan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PEP_OUTA_COLS 12
#define PEP_OUTA_GENE 0
#define PEP_OUTA_CONTIG 1
#define PEP_OUTA_FLAGS 2
#define PEP_OUTA_S 3
#define PEP_OUTA_E 4
#define PEP_OUTA_PART 5
#define PEP_OUTA_QS 6
#define PEP_OUTA_QE 7
#define PEP_OUTA_REFLEN 8
#define PEP_OUTA_CLEN 9
#define PEP_OUTA_VARY 10
#define PEP_OUTA_SVMIN 11
/* the bits of PEP_OUTA_FLAGS */
#define PEP_OUTA_MISC 1
#define PEP_OUTA_NONAME 2
#define PEP_OUTA_SECONDARY 4
#define PEP_OUTA_MINUS 8
/* the columns of a plan record and the classes */
#define PEP_OUTA_PLAN_COLS 6
#define PEP_OUTA_SKIPPED 0
#define PEP_OUTA_FRAGMENT 1
#define PEP_OUTA_INTACT 2
#define PEP_OUTA_STRUCTVAR 3
/* rows between two write-backs of the reference (:1401) */
#define PEP_OUTA_BATCH 10000
#define PEP_OUTA_MAX_CONTIG (1u << 31)
#define PEP_OUTA_MAX_ITEMS (1u << 30)
/* two rows that the digest put into one class hold different bytes: nothing was merged, nothing was written */
#define PEP_ERR_ALLELE_CLASS (-24)

/* every check of pep_out_alleles, without a context or a device (nt is not read): its code, its text in msg[msg_cap] (cut to fit).  n_rows = 0 is legal. */
int pep_out_alleles_check(const uint64_t *contig_off, uint32_t n_contigs, uint32_t n_genes, const int32_t *seed_contig, uint32_t n_rows,
                          const int32_t *rows, const int32_t *look9, uint32_t key_bits, char *msg, uint64_t msg_cap);

/* K24: plan[PEP_OUTA_PLAN_COLS n_rows], first[n_rows], rank[n_rows], tflag[n_rows] as stated above; on an error nothing is written.
 * plan_only != 0: the plan alone (one launch; nt may be NULL and is not uploaded; first, rank and tflag may be NULL and are not written) - what the first of the
 * reference's two rounds needs before column 9 of the earlier batches is known.
 * Otherwise, on the context's stream: the plan; SHA-1 of every allele read in place, strand-corrected, one thread per allele; a table that gives every
 * (gene, length, digest) its smallest member; a comparison of every member's bytes with that one's - a difference ends the call with PEP_ERR_ALLELE_CLASS and
 * the two rows in the message; the library's radix sort over the first members by (gene, index), from which the ranks follow.
 * key_bits (testing only, 0 in every other use): when 1 .. 31, a class is (gene, the low key_bits bits of the digest's first word) - distinct alleles then
 * share classes, which is the one way to see the comparison refuse them.
 * ms (optional, double[6]): plan, digest, classes, comparison, sort, ranks - kernel times when pep_set_timing is 2, zeros otherwise. */
int pep_out_alleles(pep_ctx *ctx, const uint8_t *nt, const uint64_t *contig_off, uint32_t n_contigs, uint32_t n_genes, const int32_t *seed_contig,
                    uint32_t n_rows, const int32_t *rows, const int32_t *look9, int plan_only, uint32_t key_bits, int32_t *plan, int32_t *first,
                    uint32_t *rank, uint8_t *tflag, double *ms);

#ifdef __cplusplus
}
#endif

#endif
