/* peppan_genestruct.h - K19 of libpeppan_hip.so: the gene structure of predictions.
 *
 * A header of its own beside peppan_hip.h, with a version of its own, as peppan_synteny.h is: the entry points below were added without
 * touching the main interface.  Same conventions: C ABI, functions returning int return PEP_OK (0) or a negative PEP_ERR_* code, nothing is
 * ever silently dropped, and a context function leaves its message in pep_last_error().
 *
 * Reference interface each entry point replaces (file:line in zheminzhou/PEPPAN):
 *   pep_gene_structure (+ _check, _times)   determineGeneStructure for every intact prediction of write_output: the marked-start translation
 *                                           of the window in the tried frames and the search for start and stop   PEPPAN.py:1193-1229
 */
#ifndef PEPPAN_GENESTRUCT_H
#define PEPPAN_GENESTRUCT_H
#include "peppan_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PEP_GENESTRUCT_ABI_VERSION 1

/* a window holds fewer nucleotides than this */
#define PEP_GENESTRUCT_MAX_WINDOW (1ull << 31)
/* stop_aa of a frame without a stop codon */
#define PEP_GENESTRUCT_NO_STOP 0xFFFFFFFFu
/* kind[]: the outcome of a frame */
#define PEP_GENESTRUCT_CDS 0
#define PEP_GENESTRUCT_NOSTART 1
#define PEP_GENESTRUCT_NOSTOP 2
#define PEP_GENESTRUCT_PREMATURE 3

int pep_genestruct_version(void);

/* K19: determineGeneStructure (PEPPAN.py:1193-1229) for a batch of predictions.  The nucleotide set is ASCII bytes, sequence i at
 * nt[seq_off[i] .. seq_off[i+1]) (n_seq + 1 offsets).  Prediction p reads the window of win_len[p] nucleotides that starts at the 0-based
 * win_off[p] of sequence seq[p] - forward, or, when bit 0 of flags[p] is set, backward and complemented as the reference's rc() does it
 * (upper-cased, A<->T, C<->G, everything else N: a '-' read backward is an N).  Bits 1-3 of flags[p] are the tried frames 0, 1, 2.
 * Frame f of a window of L nucleotides has n = max(0, (L - f) / 3) codons, codon k = window[f + 3k .. f + 3k + 3) (a partial last codon is
 * dropped, :1197).  A codon with a '-' is neither start nor stop; otherwise a codon with a character outside ACGT (either case) is a stop 'X';
 * otherwise TAA and TAG are stops, TGA too unless table4, and ATG, GTG, TTG are starts 'M' (modules/configure.py:167-172).
 * With a = lp / 3, b = (lp + allowed_vary) / 3, and "first / last in [u, v)" clipped to n as str.find / str.rfind clip:
 *     start = first M in [a, b), else last M in [0, a), else a with the outcome NOSTART
 *     stop  = first X in [start, n)
 *     while 0 <= stop < b and there is a first M in [stop, b): start = that M, stop = first X in [start, n)
 *     no stop: NOSTOP, else (stop - start + 1) * 3 < ref_len - allowed_vary: PREMATURE (both override NOSTART); else NOSTART or CDS.
 * The tried frames are judged in ascending order:
 *     frame[p]      the lowest tried frame whose outcome is CDS, or -1
 *     start_aa[p], stop_aa[p]   start and stop (codon numbers) of that frame; of the FIRST tried frame when frame[p] is -1, with
 *                   PEP_GENESTRUCT_NO_STOP for a frame without a stop
 *     kind[p]       the outcome of the first tried frame (PEP_GENESTRUCT_*)
 * Integer arithmetic only.  The four outputs are written only when the call succeeds; on any error nothing is written and the context
 * stays usable.  All tables are checked on the host before anything is launched:
 * PEP_ERR_ARG: seq_off does not ascend from 0, seq[p] >= n_seq, a window that leaves its sequence, no tried frame or flag bits above bit 3,
 * ref_len[p] == 0.  PEP_ERR_LIMIT: a window of PEP_GENESTRUCT_MAX_WINDOW nucleotides or more; the message names the prediction.
 * pep_gene_structure_check runs exactly these checks: no context, no device, the nucleotides themselves are not read; the message goes to
 * msg (msg_cap bytes, 0-terminated).
 * pep_gene_structure_times: of the newest call, the kernel time in ms when pep_set_timing is 2 (else 0), and the bytes it sent to the device
 * and to the host. */
int pep_gene_structure(pep_ctx *ctx, const uint8_t *nt, const uint64_t *seq_off, uint32_t n_seq, uint32_t n_pred, const uint32_t *seq, const uint64_t *win_off,
                       const uint32_t *win_len, const uint8_t *flags, const uint32_t *lp, const uint32_t *allowed_vary, const uint32_t *ref_len, int table4,
                       int32_t *frame, uint32_t *start_aa, uint32_t *stop_aa, uint8_t *kind);
int pep_gene_structure_check(const uint64_t *seq_off, uint32_t n_seq, uint32_t n_pred, const uint32_t *seq, const uint64_t *win_off, const uint32_t *win_len,
                             const uint8_t *flags, const uint32_t *lp, const uint32_t *allowed_vary, const uint32_t *ref_len, char *msg, uint64_t msg_cap);
int pep_gene_structure_times(const pep_ctx *ctx, double *kernel_ms, uint64_t *bytes_to_device, uint64_t *bytes_to_host);

#ifdef __cplusplus
}
#endif
#endif
