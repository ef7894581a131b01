/* peppan_synteny.h - K18 of libpeppan_hip.so: neighbourhood paralog splitting.
 *
 * A header of its own beside peppan_hip.h, with a version of its own: the entry points below were added without touching the main
 * interface.  Same conventions: C ABI, functions returning int return PEP_OK (0) or a negative PEP_ERR_* code, nothing is ever silently
 * dropped, and a context function leaves its message in pep_last_error().
 *
 * Reference interface each entry point replaces (file:line in zheminzhou/PEPPAN):
 *   pep_synteny_pairs (+ _copy, _check, _times)   the pair loop of ite_synteny_resolver: distance, conflict pairs, the sort of the pairs   PEPPAN.py:1101-1117
 *   pep_synteny_walk                              its merge walk and verdict (host C++, no context)                                     PEPPAN.py:1118-1151
 */
#ifndef PEPPAN_SYNTENY_H
#define PEPPAN_SYNTENY_H
#include "peppan_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PEP_SYNTENY_ABI_VERSION 1

/* most pairs (sum over the groups of n * (n - 1) / 2) of one pep_synteny_pairs call: a single group may hold 16 384 members */
#define PEP_SYNTENY_MAX_PAIRS (1ull << 27)
/* most rank counters of one call: sum over the groups of n * (6 * longest list of the group + 14) */
#define PEP_SYNTENY_MAX_COUNTERS (1ull << 26)
/* longest neighbour list of one member */
#define PEP_SYNTENY_MAX_LIST (1u << 20)

int pep_synteny_version(void);

/* K18: the pair loop of ite_synteny_resolver (PEPPAN.py:1097-1151) for a batch of paralogous names.  Group g is members
 * [member_off[g], member_off[g+1]) of genome[] (compared for equality only) and of the neighbour lists in CSR form: member i owns
 * nb[nb_off[i] .. nb_off[i+1]), strictly ascending ortholog codes.  Members are numbered 0 .. n-1 inside their group.  For m < k with
 * c = |N_m & N_k| (:1108-1110):
 *   s = 3 c + max(6 - min(6, |N_m|), 6 - min(6, |N_k|), 0) + 1,   d = 3 n_neighbor - s,   flag = (genome[m] != genome[k]).
 * A pair is a conflict iff flag is false and d > 0 (:1112).  dc[g] is the smallest d of a conflict pair (0 and has_conflict[g] = 0 when there
 * is none).  The call leaves two lists of (m, k) pairs, two uint32 each, in the context:
 *   conf   the conflict pairs, ascending by (m, k);
 *   walk   every pair with d < dc, in the order (d, flag, m, k) - the part of the sorted list (:1117) the walk of :1119-1141 reads before it
 *          stops at the first conflict pair.  Empty for a group without a conflict.
 * Group g owns conf pairs [conf_off[g], conf_off[g+1]) and walk pairs [walk_off[g], walk_off[g+1]) (G + 1 offsets each, counted in pairs).
 * The lists are counted first and the context's buffers sized from the count: nothing is truncated.  pep_synteny_pairs_copy downloads the
 * lists of the newest call: n_conf / n_walk must be conf_off[G] / walk_off[G].
 * PEP_ERR_ARG: n_neighbor outside [1, 2^20], offsets that do not ascend from 0 to their end, a list that is not strictly ascending.
 * PEP_ERR_LIMIT: more pairs than PEP_SYNTENY_MAX_PAIRS (the message names the group at which the sum passes it), more counters than
 * PEP_SYNTENY_MAX_COUNTERS, a list longer than PEP_SYNTENY_MAX_LIST.  All tables are checked on the host before anything is launched.  The
 * kernels keep a fault word for what those checks exclude - a distance beyond the group's bound, a pair beyond the counted lists: it is read
 * after each pass, and the call then fails with PEP_ERR_HIP instead of returning a list.  The four outputs are written only when the call
 * succeeds; on any error nothing is written and the context stays usable.  Integer arithmetic only.
 * pep_synteny_pairs_check runs the checks alone: no context, no device; the message goes to msg (msg_cap bytes, 0-terminated).
 * pep_synteny_pairs_times: of the newest call, the kernel times in ms - count, scans, emit - when pep_set_timing is 2 (else zeros), and the
 * bytes the call and its copy sent to the host. */
int pep_synteny_pairs(pep_ctx *ctx, uint32_t n_groups, const uint64_t *member_off, const uint32_t *genome, uint64_t n_members, const uint64_t *nb_off, const uint32_t *nb,
                      uint64_t n_nb, int32_t n_neighbor, uint8_t *has_conflict, int32_t *dc, uint64_t *conf_off, uint64_t *walk_off);
int pep_synteny_pairs_copy(pep_ctx *ctx, uint32_t *conf, uint64_t n_conf, uint32_t *walk, uint64_t n_walk);
int pep_synteny_pairs_check(uint32_t n_groups, const uint64_t *member_off, const uint32_t *genome, uint64_t n_members, const uint64_t *nb_off, const uint32_t *nb,
                            uint64_t n_nb, int32_t n_neighbor, char *msg, uint64_t msg_cap);
int pep_synteny_pairs_times(const pep_ctx *ctx, double ms[3], uint64_t *bytes_to_host);

/* The walk of ite_synteny_resolver over the two lists of pep_synteny_pairs (PEPPAN.py:1118-1151), on the host, without a context.  Every
 * member starts as a component of its own, with list A = [member] when it is an end of a conflict pair and B = [member] otherwise.  For each
 * walk pair (m, k) whose ends lie in different components ti, tj: the merge is skipped iff a conflict pair joins A[ti] and A[tj]; otherwise
 * A[ti] += A[tj], B[ti] += B[tj] (:1124-1141).  verdict[g]: 0 no conflict pair (the reference returns [None, None]), 1 a surviving component
 * has an empty A ([tag, None], :1147-1150), 2 a partition.  For verdict 2, n_comp[g] components in the order of their roots (the dictionary
 * order of :1148): component c of group g has the root comp_root[member_off[g] + c] - the member whose id is its key in the reference's
 * dictionary, not always its smallest - and comp_len[member_off[g] + c] members, and members[member_off[g] ..] holds the lists A + B of the
 * components one after the other (n entries in all).  For the other verdicts n_comp[g] = 0.  The skip test reads per-member conflict
 * adjacency, and components are joined by union-find over linked lists: the walk stays about linear in the pairs.
 * PEP_ERR_ARG: offsets that do not ascend from 0, a pair that is not m < k < n. */
int pep_synteny_walk(uint32_t n_groups, const uint64_t *member_off, const uint64_t *conf_off, const uint32_t *conf, const uint64_t *walk_off, const uint32_t *walk,
                     uint8_t *verdict, uint32_t *n_comp, uint32_t *comp_root, uint32_t *comp_len, uint32_t *members, char *msg, uint64_t msg_cap);

#ifdef __cplusplus
}
#endif
#endif
