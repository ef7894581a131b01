/* K23 of libpeppan_hip.so: the verdict and the digest of every annotated CDS, the per-gene work of the reference's GFF front end - iter_readGFF
 * (PEPPAN.py:117-182), checkPseu (:992-1010) and addGenes (:1013-1021) - which builds the gene dictionary that writeGenes and every later stage start from.
 *
 * A header of its own for the reason include/peppan_hip_tree.h gives: tests/test_abi.py pins include/peppan_hip.h to the prototypes of ABI 19.  These
 * functions are additive, PEP_ABI_VERSION stays 19 and PEP_CALL_COUNT stays 6; the pull request that may next touch tests/test_abi.py folds this file into
 * include/peppan_hip.h and gives K23 a pep_call_times selector in place of the `ms` parameter below.
 *
 * Conventions as in peppan_hip.h: int status, the message behind pep_last_error (or in msg[msg_cap] for the function without a context), a null context
 * is PEP_ERR_ARG before anything else, caller-owned inputs are only read, everything is checked on the host before a launch.
 *
 * The host (peppan_amd/gffgenes.py) reads the files, resolves names and makes the gene texts; the device judges and digests.
 *
 * ---- the inputs.  nt: the contigs of a batch of files, one after another, contig c at nt[contig_off[c] .. contig_off[c + 1]): ASCII, ALREADY UPPER-CASED by
 * the caller (:167).  CDS i is ONE window of ONE contig: win_len[i] bytes from the 0-based win_off[i] of contig contig[i] - the reference keeps the first
 * line of a gene name and ignores every later one (the elif of :158 compares a bare sequence id with a prefixed one and is never true), so :170-172 cut
 * exactly one slice.  strand[i] = 1: the window is read backward and complemented as rc() does (modules/configure.py:152-154): A <-> T, C <-> G, every
 * other byte - N and '-' included - becomes N.  strand[i] = 0: the bytes as they stand.  Call the text so read s, L = win_len[i].
 *
 * ---- the verdict, checkPseu (:992-1010).  The rules in this order, each but the first waived by its bit of `mask`:
 *   1  L < min_cds                                                             (:993)
 *   2  L % 3 != 0, unless PEP_CDS_ALLOW_FRAMESHIFT                             (:997)
 *   The translation is frame 1 with marked starts (:1000; transeq, modules/configure.py:160-194), n = ceil(L / 3) codons, the last one padded with
 *   characters outside the alphabet when L % 3 != 0 (:186-187).  A codon holding a '-' is '-' (:190) - also beside another odd character, also when the
 *   '-' sits in a padded last codon; else a codon with a character outside ACGT is X (:191); else M for ATG GTG TTG (:172, and table[14]), X for TAA TAG
 *   and - unless table4 - TGA (:168-170), anything else otherwise.
 *   3  codon 0 is not M, unless PEP_CDS_ALLOW_NO_START                         (:1001)
 *   4  codon n - 1 is not X, unless PEP_CDS_ALLOW_NO_STOP                      (:1004)
 *   5  an X among codons 0 .. n - 2, unless PEP_CDS_ALLOW_INNER_STOP           (:1007)
 *   0  otherwise.
 * With one codon, codon 0 is codon n - 1.  L = 0 with min_cds = 0 has no codon: the reference raises there (iter_readGFF turns that into its code 6, addGenes
 * lets it escape); the library answers as if no codon were M or X, and its Python callers never send such a window.  Codes 1 and 2 are decided before a
 * byte is read.  Nothing outside the window is read.
 *
 * ---- the digest (:178, :1020).  digest[20 i ..]: SHA-1 of s, the 20 bytes of hashlib.sha1(s).digest(), for every CDS of code 0; twenty zero bytes for the
 * others.  It is computed straight from nt: no copy of s is made anywhere. */
#ifndef PEPPAN_HIP_CDS_H
#define PEPPAN_HIP_CDS_H

#include "peppan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a window holds fewer bytes than this */
#define PEP_CDS_MAX_WINDOW (1u << 31)
/* CDS of one call: fewer than this (n_cds is 32 bits wide; the Python binding refuses more) */
#define PEP_CDS_MAX_ITEMS (1ull << 32)
/* the bits of `mask`, one per letter of the reference's incompleteCDS parameter: s, i, f, e */
#define PEP_CDS_ALLOW_NO_START 1
#define PEP_CDS_ALLOW_INNER_STOP 2
#define PEP_CDS_ALLOW_FRAMESHIFT 4
#define PEP_CDS_ALLOW_NO_STOP 8

/* every check of pep_cds_genes, without a context or a device (nt is not read): its code, its text in msg[msg_cap] (cut to fit).
 * PEP_ERR_ARG: a null table; contig_off that does not start at 0 or decreases (offsets are 64 bits wide); a contig index outside 0 .. n_contigs - 1; a
 * window that leaves its contig; a strand byte that is not 0 or 1; a mask with bits beyond the four.  PEP_ERR_LIMIT: a window of PEP_CDS_MAX_WINDOW bytes
 * or more.  The message names the CDS.  n_cds = 0 is legal. */
int pep_cds_genes_check(const uint64_t *contig_off, uint32_t n_contigs, uint32_t n_cds, const uint32_t *contig, const uint64_t *win_off,
                        const uint32_t *win_len, const uint8_t *strand, uint32_t mask, char *msg, uint64_t msg_cap);

/* K23: code[n_cds] (0 .. 5) and digest[20 n_cds] as stated above.  Two launches on the context's stream - the verdicts, one wavefront per CDS; the digests of
 * the CDS of code 0, one thread per CDS - with nothing in between; on an error nothing is written.
 * ms (optional, double[2]): the kernel time of each launch when pep_set_timing is 2, zeros otherwise. */
int pep_cds_genes(pep_ctx *ctx, const uint8_t *nt, const uint64_t *contig_off, uint32_t n_contigs, uint32_t n_cds, const uint32_t *contig,
                  const uint64_t *win_off, const uint32_t *win_len, const uint8_t *strand, uint32_t min_cds, uint32_t mask, int table4,
                  uint8_t *code, uint8_t *digest, double *ms);

#ifdef __cplusplus
}
#endif

#endif
