/* K22 of libpeppan_hip.so: the genome-pair identity statistics of the reference's get_global_difference (PEPPAN.py:1611-1666), the (mean, sigma) table
 * that K16 (orthofilter.gd_table) and K17 (ingroups.initializing) read.
 *
 * A header of its own for the reason include/peppan_hip_tree.h gives: tests/test_abi.py pins include/peppan_hip.h to the prototypes of ABI 19.  These
 * functions are additive, PEP_ABI_VERSION stays 19 and PEP_CALL_COUNT stays 6; the pull request that may next touch tests/test_abi.py folds this file into
 * include/peppan_hip.h and gives K22 a pep_call_times selector in place of the `ms` parameter below.
 *
 * Conventions as in peppan_hip.h: int status, the message behind pep_last_error (or in msg[msg_cap] for the functions without a context), a null context
 * is PEP_ERR_ARG before anything else, caller-owned inputs are only read, everything is checked on the host before a launch.
 *
 * The function is cut in two.  The ORDER-DEPENDENT part (:1632-1659 without its two inner loops) is a dictionary walk over the selected rows that only
 * decides which two member lists meet at each row; it costs the sum of the list lengths and is host C++ (pep_global_diff_walk), like pep_similar_scan.
 * The QUADRATIC part - the cross product of the two lists of every row, grouped by genome pair, and the two means per pair - is the device's
 * (pep_global_diff).  The host tail (:1663-1665: two clamps, np.sqrt, np.exp) stays numpy (peppan_amd/globaldiff.py). */
#ifndef PEPPAN_HIP_GDIFF_H
#define PEPPAN_HIP_GDIFF_H

#include "peppan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* distinct genomes of one call: the keys live in a dense triangular table of G (G + 1) / 2 entries */
#define PEP_GDIFF_MAX_GENOMES 16384
/* items (list-pair members, the sum of a_len * b_len over the events) of one call: at most this many */
#define PEP_GDIFF_MAX_ITEMS (1ull << 32)
/* entries of the logarithm table: a value code is 0 .. PEP_GDIFF_TABLE - 1 (1.005 - code / 10000 stays positive) */
#define PEP_GDIFF_TABLE 10050
/* items of one chunk when chunk_items is 0, and the most a caller may ask for (the chunk's keys are sorted by pep_sort_u64) */
#define PEP_GDIFF_CHUNK_ITEMS (1u << 24)
#define PEP_GDIFF_MAX_CHUNK_ITEMS (1u << 26)
/* bytes of device workspace of one call, as computed from its sizes before anything is reserved */
#define PEP_GDIFF_MAX_BYTES (1ull << 34)

/* ---- the host walk (no context, no device).
 * clu / bsn: the selected rows (r, q, value) of the .clu.npy and the .bsn.npy table as int64[n][3], in file order, bsn already without its rows of
 * value <= 0 (:1626).  genes / genome_of: the gene -> genome map, gene ids strictly ascending, the int32 genome of each.  Genome ids are signed (-1 is
 * a legal genome and a legal key member); they are replaced by their ranks 0 .. G - 1 in ascending order over genome_of, which keeps the order of
 * tuple(sorted(...)).
 *
 * The dictionary semantics of :1632-1659, literally.  A dictionary gene -> list, empty at the start.  A list is a span (off, len, cap) of the arena, an
 * append-only array of genome ranks; `the list [g]` below is a new span of one entry at the arena's end.
 *   clu row (r, q, i):  rr = the list of key r if the dictionary has one, else the list [r] (the key r itself, not a root).  qq = the list of key q,
 *       which is REMOVED from the dictionary, else the list [q].  (r == q: rr and qq are the same list when it has one; else two lists [r].)  The event
 *       (rr.off, rr.len, qq.off, qq.len, i, 0).  Then the dictionary's entry of r becomes rr + qq: with need = rr.len + qq.len, if need > rr.cap: when rr ends where
 *       the arena ends the arena grows to make rr.cap = need, else rr moves - cap = 2 * need new entries (zeros) at the arena's end, its len
 *       entries copied; then qq's len entries are copied behind rr's and rr.len = need.  Nothing that an earlier event names is ever overwritten.
 *   bsn row (r, q, i):  rr and qq as above (q's entry removed); the event (.., i, 1); nothing is written back.
 * An event names two prefixes of lists; drop_same = 0 for clu rows (same-genome pairs count), 1 for bsn rows (:1654).
 * PEP_ERR_ARG: a null table; gene ids not strictly ascending; a gene of a row that is not in the map (the message names the gene); a value outside
 * 0 .. PEP_GDIFF_TABLE - 1 (the message names the row: the reference would take the logarithm of a number that is not positive); an arena beyond 2^32 - 1.
 * *out: a handle to the result, to be freed by pep_global_diff_walk_free on every path that got one. */
typedef struct pep_gdiff_walk pep_gdiff_walk;
int pep_global_diff_walk(const int64_t *clu, uint64_t n_clu, const int64_t *bsn, uint64_t n_bsn, const int64_t *genes, const int32_t *genome_of,
                         uint64_t n_genes, pep_gdiff_walk **out, char *msg, uint64_t msg_cap);
/* events (one per row: n_clu + n_bsn), entries of the arena, distinct genomes G */
int pep_global_diff_walk_size(const pep_gdiff_walk *walk, uint64_t *n_events, uint64_t *arena_len, uint32_t *n_genomes);
/* events: int64[n_events][6] = (a_off, a_len, b_off, b_len, value, drop_same); arena: int32[arena_len] genome ranks; genomes: int32[G], the genome id of every rank */
int pep_global_diff_walk_copy(const pep_gdiff_walk *walk, int64_t *events, int32_t *arena, int32_t *genomes);
void pep_global_diff_walk_free(pep_gdiff_walk *walk);

/* ---- K22.  events and arena as the walk leaves them (a caller may bring its own), n_genomes = G, table = double[PEP_GDIFF_TABLE], for the reference
 * np.log(1.005 - np.arange(10050) / 10000.) made by numpy on the host: element i is bit for bit the reference's logarithm of a value i.
 *
 * Item (a, b) of event e, 0 <= a < a_len, 0 <= b < b_len: key = (min, max) of arena[a_off + a] and arena[b_off + b]; value code = the event's value;
 * sequence number = base(e) + a * b_len + b, base the exclusive sum of a_len * b_len over the events.  An item of two equal ranks in a drop_same event
 * does not exist (its sequence number stays unused).  For every key with at least one item, with x_0 .. x_(n-1) = table[code] of its items in the order
 * of their events (all items of one event have one code, so their order inside the event does not matter):
 *   S(x) = numpy's sum of a float64 array as np.mean computes it: s = 0.0; for every buffer of 8192 elements (the last one shorter), left to right,
 *          s = s + P(buffer).  P(v, n) is numpy's pairwise sum: n < 8: r = 0.0, r = r + v[i] left to right.  n <= 128: eight accumulators r[j] = v[j],
 *          r[j] = r[j] + v[i + j] for i = 8, 16, .. while i + 8 <= n; r = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); then r = r + v[i] for the
 *          rest.  n > 128: P(v, h) + P(v + h, n - h) with h = n / 2 - (n / 2) % 8.
 *   m = S(x) / n,   v = S((x - m) * (x - m)) / n.
 * Every operation is one correctly rounded IEEE double operation; nothing is contracted into a fused multiply-add.
 * The call leaves the keys on the device: *n_keys is their number; pep_global_diff_copy fetches them, ordered by the smallest sequence number of each
 * key - the insertion order of the reference's dictionary, also where two keys first appear inside one event.
 *
 * chunk_items: the lists are filled chunk by chunk - chunks of this many sequence numbers, cut in event order, an event larger than a chunk split by
 * item range; 0 = PEP_GDIFF_CHUNK_ITEMS.  The result does not depend on it.
 * PEP_ERR_ARG: a null table, an event that runs past the arena or has an empty list, a value code outside the table, a drop_same other than 0 / 1, a
 * rank outside 0 .. G - 1 (the message names event or entry), chunk_items above PEP_GDIFF_MAX_CHUNK_ITEMS.  PEP_ERR_LIMIT, with the amount asked for in
 * the message: G > PEP_GDIFF_MAX_GENOMES, more than PEP_GDIFF_MAX_ITEMS items, more than PEP_GDIFF_MAX_BYTES of workspace (keys counted as
 * min(G (G + 1) / 2, items)).  No events, or no genomes, is legal and gives no keys.
 * ms (optional, double[4]): ms[0] counting and offsets, ms[1] the chunks (emit, sort, copy), ms[2] the sums, when pep_set_timing is 2, zeros otherwise. */
int pep_global_diff(pep_ctx *ctx, const int64_t *events, uint64_t n_events, const int32_t *arena, uint64_t arena_len, uint32_t n_genomes,
                    const double *table, uint64_t chunk_items, uint64_t *n_keys, double *ms);
/* the keys of the newest pep_global_diff of this context, n_keys of them: the two ranks (g1 <= g2), the number of items, m and v.  PEP_ERR_ARG: n_keys is
 * not what that call reported. */
int pep_global_diff_copy(pep_ctx *ctx, uint64_t n_keys, int32_t *g1, int32_t *g2, uint64_t *n, double *mean, double *var);
/* every check of pep_global_diff, without a context or a device: its code, its text in msg[msg_cap] (cut to fit) */
int pep_global_diff_check(const int64_t *events, uint64_t n_events, const int32_t *arena, uint64_t arena_len, uint32_t n_genomes, uint64_t chunk_items,
                          char *msg, uint64_t msg_cap);

#ifdef __cplusplus
}
#endif

#endif
