// K18: neighbourhood paralog splitting - ite_synteny_resolver (PEPPAN.py:1097-1151) as synteny_resolver (:1153-1191) runs it for every paralogous name.
// The reference computes, in a Python double loop over the members of a name, a distance for every pair from the intersection of two neighbour
// sets, sorts all pairs and walks them.  Restated without an order (include/peppan_hip.h, K18): with dc the smallest distance of a conflict pair
// (same genome, d > 0), the walk reads exactly the pairs with d < dc in the order (d, flag, m, k) and stops.  The device makes the two sparse lists -
// the conflict pairs and the walked pairs, ranked - and the host walks them (pep_synteny_walk below, no context).
//   synteny_count    one wavefront per member m (row): lanes take the members k > m, 64 at a time.  The row's list sits in eight uniform registers
//                    when it has at most 8 ids (six is the usual size); a lane then tests every id of its own list against them.  Longer rows take a
//                    two-pointer merge of the two ascending lists.  Per row: the count of conflict pairs, atomicMin of their d into dc[group], and a
//                    count per bin = (d, flag) - equal bins of a chunk are added once, by the first lane that holds them.
//   synteny_mask     clears the bins with d >= dc (all of a group without a conflict).  The counters lie bin-major, row-minor inside a group, so ONE
//                    exclusive scan over them (scan.hip) gives every (row, bin) its place in the walked list of the whole batch, in the order
//                    (group, d, flag, m); a second scan places the conflict pairs of every row.
//   synteny_offsets  the places where the groups start, for the host.
//   synteny_emit     the count pass again, now storing: a conflict pair at its row's place + its rank inside the row, a walked pair at its (row, bin)
//                    place, which the row's wavefront moves on chunk by chunk - so k ascends inside a bin of a row.
// Integers only, plain vector stores, no LDS: the lists of a group of 4 000 members are 100 KB and stay in L2.  What bounds it: a row is one
// wavefront's, so a group's longest row (n - 1 pairs) is serial in chunks of 64, and a tiny group fills one lane per pair.
#include "common.h"
#include <algorithm>
#include <cstring>

namespace {

constexpr uint32_t K18_NONE = 0xFFFFFFFFu;

// the slots of pep_ctx::k18
enum { K18_MEMBER_OFF = 0, K18_GRP_OF, K18_GENOME, K18_NB_OFF, K18_NB, K18_CNT_BASE, K18_SMAX, K18_DC, K18_CNT, K18_POS, K18_CONF_CNT, K18_CONF_POS, K18_WALK_OFF,
       K18_CONF_OFF, K18_CONF_OUT, K18_WALK_OUT, K18_SCAN_TMP, K18_FAULT, K18_SLOTS };
static_assert(K18_SLOTS == sizeof(pep_ctx::k18) / sizeof(DevBuf), "one member of pep_ctx::k18 per slot");

struct SynTab {
    const uint64_t *member_off;      // [G + 1]
    const uint32_t *grp_of;          // [M]: the group of every member
    const uint32_t *genome;          // [M]
    const uint64_t *nb_off;          // [M + 1]
    const uint32_t *nb;
    const uint64_t *cnt_base;        // [G + 1]: where the group's n * 2 * smax counters start
    const uint32_t *smax;            // [G]: 3 * longest list + 7, no s of the group is larger
    uint32_t *fault;                 // one word, set when a kernel meets what the host checks exclude: the call then fails instead of returning a list
    uint64_t n_members;
    int32_t n3;                      // 3 * nNeighbor
};

// the row of a wavefront: member i = row m of group g, its list and genome (all uniform over the wavefront)
struct SynRow {
    uint64_t base, cnt_at, am;
    uint32_t g, n, m, lm, gm, smax;
    uint32_t a[8];
    bool fast;
};

__device__ __forceinline__ bool syn_row(const SynTab &T, uint64_t i, SynRow &R)
{
    if (i >= T.n_members) return false;
    R.g = T.grp_of[i];
    R.base = T.member_off[R.g];
    R.n = (uint32_t)(T.member_off[R.g + 1] - R.base);
    R.m = (uint32_t)(i - R.base);
    if (R.m + 1 >= R.n) return false;                                  // the last member of a group has no pair of its own
    R.am = T.nb_off[i];
    R.lm = (uint32_t)(T.nb_off[i + 1] - R.am);
    R.gm = T.genome[i];
    R.smax = T.smax[R.g];
    R.cnt_at = T.cnt_base[R.g] + R.m;
    R.fast = R.lm <= 8;
    if (R.fast && R.lm)
#pragma unroll
        for (uint32_t t = 0; t < 8; ++t) R.a[t] = T.nb[R.am + (t < R.lm ? t : R.lm - 1)];      // (a slot past the end repeats the last id: the test below is an OR)
    return true;
}

// s of :1109 for the row and member k of its group, and whether the genomes differ
__device__ __forceinline__ uint32_t syn_pair(const SynTab &T, const SynRow &R, uint32_t k, bool &differ)
{
    const uint64_t ak = T.nb_off[R.base + k];
    const uint32_t lk = (uint32_t)(T.nb_off[R.base + k + 1] - ak);
    differ = T.genome[R.base + k] != R.gm;
    uint32_t c = 0;
    if (R.fast) {
        if (R.lm)
            for (uint32_t t = 0; t < lk; ++t) {
                const uint32_t x = T.nb[ak + t];
                c += (x == R.a[0]) | (x == R.a[1]) | (x == R.a[2]) | (x == R.a[3]) | (x == R.a[4]) | (x == R.a[5]) | (x == R.a[6]) | (x == R.a[7]);
            }
    } else {
        uint64_t i = R.am, j = ak;
        const uint64_t ie = R.am + R.lm, je = ak + lk;
        while (i < ie && j < je) {
            const uint32_t x = T.nb[i], y = T.nb[j];
            c += x == y;
            i += x <= y;
            j += y <= x;
        }
    }
    const uint32_t pm = 6u - min(6u, R.lm), pk = 6u - min(6u, lk);
    const uint32_t s = 3u * c + max(pm, pk) + 1u;
    if (s > R.smax) *T.fault = 1u;                                      // (no s passes smax for ascending lists; the min keeps the counter index in its group all the same)
    return min(s, R.smax);
}

// among the lanes with `on`: rank = how many lower lanes hold the same key, cnt = how many lanes hold it, lead = the lowest of them
__device__ __forceinline__ void wave_rank(bool on, uint32_t key, uint32_t lane, uint32_t &rank, uint32_t &cnt, uint32_t &lead)
{
    unsigned long long todo = __ballot(on);
    const unsigned long long below = (1ull << lane) - 1ull;
    rank = cnt = 0;
    lead = lane;
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const uint32_t k0 = __shfl(key, first, 64);
        const bool mine = on && key == k0;
        const unsigned long long same = __ballot(mine);
        if (mine) {
            rank = (uint32_t)__popcll(same & below);
            cnt = (uint32_t)__popcll(same);
            lead = (uint32_t)first;
        }
        todo &= ~same;
    }
}

__global__ __launch_bounds__(256) void synteny_count(const SynTab T, uint32_t *__restrict__ cnt, uint32_t *__restrict__ conf_cnt, uint32_t *__restrict__ dc)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    SynRow R;
    if (!syn_row(T, i, R)) return;                                      // (uniform over the wavefront; conf_cnt was cleared)
    uint32_t n_conf = 0, d_min = K18_NONE;
    for (uint32_t k0 = R.m + 1; k0 < R.n; k0 += 64) {
        const uint32_t k = k0 + lane;
        const bool on = k < R.n;
        bool differ = false;
        const uint32_t s = on ? syn_pair(T, R, k, differ) : 1u;
        const int32_t d = T.n3 - (int32_t)s;
        if (on && !differ && d > 0) {
            ++n_conf;
            d_min = min(d_min, (uint32_t)d);
        }
        const uint32_t bin = 2 * (R.smax - s) + (differ ? 1u : 0u);
        uint32_t rank, same, lead;
        wave_rank(on, bin, lane, rank, same, lead);
        if (on && rank == 0) atomicAdd(&cnt[R.cnt_at + (uint64_t)bin * R.n], same);
    }
    for (int w = 32; w > 0; w >>= 1) {
        n_conf += __shfl_xor(n_conf, w, 64);
        d_min = min(d_min, (uint32_t)__shfl_xor(d_min, w, 64));
    }
    if (lane == 0) {
        conf_cnt[i] = n_conf;
        if (d_min != K18_NONE) atomicMin(&dc[R.g], d_min);
    }
}

// one workgroup per group: the counters of the bins the walk does not read become 0
__global__ __launch_bounds__(256) void synteny_mask(const SynTab T, const uint32_t *__restrict__ dc, uint32_t *__restrict__ cnt)
{
    const uint32_t g = blockIdx.x;
    const uint64_t lo = T.cnt_base[g], total = T.cnt_base[g + 1] - lo;
    const uint64_t n = T.member_off[g + 1] - T.member_off[g];
    const uint32_t dcg = dc[g], smax = T.smax[g];
    for (uint64_t e = threadIdx.x; e < total; e += 256) {
        const uint32_t bin = (uint32_t)(e / n);
        const int32_t d = T.n3 - (int32_t)(smax - bin / 2);
        if (dcg == K18_NONE || d >= (int32_t)dcg) cnt[lo + e] = 0;
    }
}

__global__ __launch_bounds__(256) void synteny_offsets(const SynTab T, uint32_t n_groups, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ conf_pos,
                                                       uint32_t *__restrict__ walk_off, uint32_t *__restrict__ conf_off)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g > n_groups) return;
    walk_off[g] = pos[T.cnt_base[g]];
    conf_off[g] = conf_pos[T.member_off[g]];
}

__global__ __launch_bounds__(256) void synteny_emit(const SynTab T, const uint32_t *__restrict__ dc, uint32_t *__restrict__ pos, const uint32_t *__restrict__ conf_pos,
                                                    uint2 *__restrict__ conf_out, uint64_t n_conf, uint2 *__restrict__ walk_out, uint64_t n_walk)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    SynRow R;
    if (!syn_row(T, i, R)) return;
    const uint32_t dcg = dc[R.g];
    if (dcg == K18_NONE) return;                                        // no conflict in the group: neither list has a pair of it
    const unsigned long long below = (1ull << lane) - 1ull;
    uint64_t conf_at = conf_pos[i];
    for (uint32_t k0 = R.m + 1; k0 < R.n; k0 += 64) {
        const uint32_t k = k0 + lane;
        const bool on = k < R.n;
        bool differ = false;
        const uint32_t s = on ? syn_pair(T, R, k, differ) : 1u;
        const int32_t d = T.n3 - (int32_t)s;
        const bool conflict = on && !differ && d > 0;
        const unsigned long long cb = __ballot(conflict);
        if (conflict) {
            const uint64_t at = conf_at + (uint64_t)__popcll(cb & below);
            if (at < n_conf) conf_out[at] = make_uint2(R.m, k); else *T.fault = 1u;
        }
        conf_at += (uint64_t)__popcll(cb);
        const bool walked = on && d < (int32_t)dcg;
        const uint32_t bin = 2 * (R.smax - s) + (differ ? 1u : 0u);
        uint32_t rank, same, lead;
        wave_rank(walked, bin, lane, rank, same, lead);
        uint32_t start = 0;
        if (walked && rank == 0) start = atomicAdd(&pos[R.cnt_at + (uint64_t)bin * R.n], same);
        start = __shfl(start, lead, 64);
        if (walked) {
            const uint64_t at = (uint64_t)start + rank;
            if (at < n_walk) walk_out[at] = make_uint2(R.m, k); else *T.fault = 1u;
        }
    }
}

struct Layout {
    std::vector<uint32_t> grp_of, smax;
    std::vector<uint64_t> cnt_base;
    uint64_t pairs = 0;
};

const char *const K18_ME = "pep_synteny_pairs: ";

// every check of the tables, on the host, before anything is launched; also makes the layout of the counters
int k18_check(uint32_t n_groups, const uint64_t *member_off, const uint32_t *genome, uint64_t n_members, const uint64_t *nb_off, const uint32_t *nb, uint64_t n_nb,
              int32_t n_neighbor, Layout &L, std::string &msg)
{
    const auto bad = [&](int code, const std::string &text) { msg = K18_ME + text; return code; };
    if (!member_off || !nb_off || (n_members && !genome) || (n_nb && !nb)) return bad(PEP_ERR_ARG, "null table");
    if (n_neighbor < 1 || n_neighbor > (1 << 20)) return bad(PEP_ERR_ARG, "n_neighbor must lie in [1, 2^20], not " + std::to_string(n_neighbor));
    const uint64_t pair_cap = PEP_SYNTENY_MAX_PAIRS;
    if (n_members >= 0xFFFFFFFFull) return bad(PEP_ERR_LIMIT, "more than 2^32 - 2 members");
    if (member_off[0] != 0) return bad(PEP_ERR_ARG, "member_off must start at 0");
    for (uint32_t g = 0; g < n_groups; ++g) {
        if (member_off[g + 1] < member_off[g]) return bad(PEP_ERR_ARG, "member_off must be non-decreasing (group " + std::to_string(g) + ")");
        if (member_off[g + 1] > n_members) return bad(PEP_ERR_ARG, "member_off of group " + std::to_string(g) + " runs past n_members");
    }
    if (member_off[n_groups] != n_members) return bad(PEP_ERR_ARG, "member_off must end at n_members");
    if (nb_off[0] != 0) return bad(PEP_ERR_ARG, "nb_off must start at 0");
    for (uint64_t i = 0; i < n_members; ++i) {
        if (nb_off[i + 1] < nb_off[i]) return bad(PEP_ERR_ARG, "nb_off must be non-decreasing (member " + std::to_string(i) + ")");
        if (nb_off[i + 1] > n_nb) return bad(PEP_ERR_ARG, "nb_off of member " + std::to_string(i) + " runs past n_nb");
        if (nb_off[i + 1] - nb_off[i] > PEP_SYNTENY_MAX_LIST) return bad(PEP_ERR_LIMIT, "the list of member " + std::to_string(i) + " holds more than 2^20 ids");
        for (uint64_t t = nb_off[i] + 1; t < nb_off[i + 1]; ++t)
            if (nb[t] <= nb[t - 1]) return bad(PEP_ERR_ARG, "the list of member " + std::to_string(i) + " is not strictly ascending");
    }
    if (nb_off[n_members] != n_nb) return bad(PEP_ERR_ARG, "nb_off must end at n_nb");
    L.grp_of.resize(n_members);
    L.smax.resize(n_groups);
    L.cnt_base.assign((size_t)n_groups + 1, 0);
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint64_t n = member_off[g + 1] - member_off[g];
        uint64_t longest = 0;
        for (uint64_t i = member_off[g]; i < member_off[g + 1]; ++i) {
            L.grp_of[i] = g;
            longest = std::max(longest, nb_off[i + 1] - nb_off[i]);
        }
        const uint64_t pairs = n ? n * (n - 1) / 2 : 0;
        if (pairs > pair_cap || L.pairs + pairs > pair_cap)
            return bad(PEP_ERR_LIMIT, "group " + std::to_string(g) + " (" + std::to_string(n) + " members) takes the call past " + std::to_string(pair_cap) + " pairs (split the batch)");
        L.pairs += pairs;
        L.smax[g] = (uint32_t)(3 * longest + 7);
        L.cnt_base[g + 1] = L.cnt_base[g] + (n >= 2 ? n * 2 * L.smax[g] : 0);
        if (L.cnt_base[g + 1] > PEP_SYNTENY_MAX_COUNTERS)
            return bad(PEP_ERR_LIMIT, "group " + std::to_string(g) + " takes the call past " + std::to_string(PEP_SYNTENY_MAX_COUNTERS) + " rank counters (split the batch)");
    }
    return PEP_OK;
}

int k18_pairs(pep_ctx *ctx, uint32_t n_groups, const uint64_t *member_off, const uint32_t *genome, uint64_t n_members, const uint64_t *nb_off, const uint32_t *nb,
              uint64_t n_nb, int32_t n_neighbor, uint8_t *has_conflict, int32_t *dc, uint64_t *conf_off, uint64_t *walk_off)
{
    CallTimes &times = ctx->calls[PEP_CALL_SYNTENY_PAIRS];
    times = {};
    ctx->k18_n_conf = ctx->k18_n_walk = 0;
    Layout L;
    std::string msg;
    const int rc = k18_check(n_groups, member_off, genome, n_members, nb_off, nb, n_nb, n_neighbor, L, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    if (L.pairs == 0) {                                                 // no group of two members: nothing to launch
        for (uint32_t g = 0; g < n_groups; ++g) has_conflict[g] = 0, dc[g] = 0;
        for (uint32_t g = 0; g <= n_groups; ++g) conf_off[g] = walk_off[g] = 0;
        return PEP_OK;
    }
    DevBuf *W = ctx->k18;
    hipStream_t st = ctx->stream;
    const uint64_t n_cnt = L.cnt_base[n_groups];
    PEP_TRY(pep_tables_to_device(ctx, W, {{K18_MEMBER_OFF, member_off, ((size_t)n_groups + 1) * 8, 0}, {K18_GRP_OF, L.grp_of.data(), n_members * 4, 0},
                                          {K18_GENOME, genome, n_members * 4, 0},                     {K18_NB_OFF, nb_off, (n_members + 1) * 8, 0},
                                          {K18_NB, nb, n_nb * 4, 4},                                  {K18_CNT_BASE, L.cnt_base.data(), ((size_t)n_groups + 1) * 8, 0},
                                          {K18_SMAX, L.smax.data(), (size_t)n_groups * 4, 0},         {K18_DC, nullptr, (size_t)n_groups * 4, 0},
                                          {K18_CNT, nullptr, (n_cnt + 1) * 4, 0},                     {K18_POS, nullptr, (n_cnt + 1) * 4, 0},
                                          {K18_CONF_CNT, nullptr, (n_members + 1) * 4, 0},            {K18_CONF_POS, nullptr, (n_members + 1) * 4, 0},
                                          {K18_WALK_OFF, nullptr, ((size_t)n_groups + 1) * 4, 0},     {K18_CONF_OFF, nullptr, ((size_t)n_groups + 1) * 4, 0},
                                          {K18_FAULT, nullptr, 4, 0}}));
    PEP_HIP(ctx, hipMemsetAsync(W[K18_DC].p, 0xFF, (size_t)n_groups * 4, st));
    PEP_HIP(ctx, hipMemsetAsync(W[K18_CNT].p, 0, (n_cnt + 1) * 4, st));
    PEP_HIP(ctx, hipMemsetAsync(W[K18_CONF_CNT].p, 0, (n_members + 1) * 4, st));
    PEP_HIP(ctx, hipMemsetAsync(W[K18_FAULT].p, 0, 4, st));
    const SynTab T{W[K18_MEMBER_OFF].as<const uint64_t>(), W[K18_GRP_OF].as<const uint32_t>(), W[K18_GENOME].as<const uint32_t>(), W[K18_NB_OFF].as<const uint64_t>(),
                   W[K18_NB].as<const uint32_t>(), W[K18_CNT_BASE].as<const uint64_t>(), W[K18_SMAX].as<const uint32_t>(), W[K18_FAULT].as<uint32_t>(), n_members, 3 * n_neighbor};
    uint32_t *d_dc = W[K18_DC].as<uint32_t>(), *d_cnt = W[K18_CNT].as<uint32_t>(), *d_pos = W[K18_POS].as<uint32_t>();
    uint32_t *d_conf_cnt = W[K18_CONF_CNT].as<uint32_t>(), *d_conf_pos = W[K18_CONF_POS].as<uint32_t>();
    const dim3 rows((unsigned)ceil_div(n_members, 4));
    pep_timed_stage(ctx, times.ms[0], [&] {
        hipLaunchKernelGGL(synteny_count, rows, dim3(256), 0, st, T, d_cnt, d_conf_cnt, d_dc);
        hipLaunchKernelGGL(synteny_mask, dim3(n_groups), dim3(256), 0, st, T, (const uint32_t *)d_dc, d_cnt);
    });
    PEP_HIP(ctx, hipGetLastError());
    int scan_rc = PEP_OK;
    pep_timed_stage(ctx, times.ms[1], [&] {
        scan_rc = pep_scan_u32(ctx, d_cnt, d_pos, n_cnt, W[K18_SCAN_TMP]);
        if (scan_rc == PEP_OK) scan_rc = pep_scan_u32(ctx, d_conf_cnt, d_conf_pos, n_members, W[K18_SCAN_TMP]);
        if (scan_rc == PEP_OK)
            hipLaunchKernelGGL(synteny_offsets, dim3((unsigned)ceil_div((uint64_t)n_groups + 1, 256)), dim3(256), 0, st, T, n_groups, (const uint32_t *)d_pos,
                               (const uint32_t *)d_conf_pos, W[K18_WALK_OFF].as<uint32_t>(), W[K18_CONF_OFF].as<uint32_t>());
    });
    PEP_TRY(scan_rc);
    PEP_HIP(ctx, hipGetLastError());
    std::vector<uint32_t> h_dc(n_groups), h_walk((size_t)n_groups + 1), h_conf((size_t)n_groups + 1);
    PEP_TRY(pep_d2h_queue(ctx, h_dc.data(), W[K18_DC].p, (size_t)n_groups * 4));
    PEP_TRY(pep_d2h_queue(ctx, h_walk.data(), W[K18_WALK_OFF].p, ((size_t)n_groups + 1) * 4));
    PEP_TRY(pep_d2h_queue(ctx, h_conf.data(), W[K18_CONF_OFF].p, ((size_t)n_groups + 1) * 4));
    uint32_t fault = 0;
    const std::string inconsistent = std::string(K18_ME) + "the device met lists or counts that the host checks exclude";
    PEP_TRY(pep_d2h_queue(ctx, &fault, W[K18_FAULT].p, 4));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    if (fault) return pep_fail(ctx, PEP_ERR_HIP, inconsistent);
    const uint64_t n_conf = h_conf[n_groups], n_walk = h_walk[n_groups];
    if (n_conf + n_walk > L.pairs) return pep_fail(ctx, PEP_ERR_HIP, inconsistent);
    // the stream is idle: the two lists grow to what was counted
    PEP_TRY(dev_reserve(ctx, W[K18_CONF_OUT], std::max<uint64_t>(n_conf, 1) * 8));
    PEP_TRY(dev_reserve(ctx, W[K18_WALK_OUT], std::max<uint64_t>(n_walk, 1) * 8));
    if (n_conf) {
        pep_timed_stage(ctx, times.ms[2], [&] {
            hipLaunchKernelGGL(synteny_emit, rows, dim3(256), 0, st, T, (const uint32_t *)d_dc, d_pos, (const uint32_t *)d_conf_pos, W[K18_CONF_OUT].as<uint2>(), n_conf,
                               W[K18_WALK_OUT].as<uint2>(), n_walk);
        });
        PEP_HIP(ctx, hipGetLastError());
        PEP_TRY(pep_d2h_queue(ctx, &fault, W[K18_FAULT].p, 4));
        PEP_HIP(ctx, pep_stream_wait(ctx));
        pep_d2h_finish(ctx);
        if (fault) return pep_fail(ctx, PEP_ERR_HIP, inconsistent);
    }
    for (uint32_t g = 0; g < n_groups; ++g) {
        has_conflict[g] = h_dc[g] != K18_NONE;
        dc[g] = h_dc[g] != K18_NONE ? (int32_t)h_dc[g] : 0;
    }
    for (uint32_t g = 0; g <= n_groups; ++g) conf_off[g] = h_conf[g], walk_off[g] = h_walk[g];
    ctx->k18_n_conf = n_conf;
    ctx->k18_n_walk = n_walk;
    times.bytes_to_host = 12ull * n_groups + 12 + (n_conf ? 4 : 0);     // dc and two offsets per group, the two totals, the fault word after each pass
    return PEP_OK;
}

// union-find over the members of one group; the root carries the component's two linked lists
struct Walker {
    std::vector<uint32_t> parent, next, a_head, a_tail, b_head, b_tail, adj_off, adj, in_conflict;
    std::vector<uint64_t> weight;                                        // conflict ends listed under the root's A: what a skip test over this side costs
    uint32_t find(uint32_t x)
    {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    }
};

}  // namespace

extern "C" {

int pep_synteny_pairs_check(uint32_t n_groups, const uint64_t *member_off, const uint32_t *genome, uint64_t n_members, const uint64_t *nb_off, const uint32_t *nb,
                            uint64_t n_nb, int32_t n_neighbor, char *msg, uint64_t msg_cap)
{
    Layout L;
    std::string text;
    const int rc = k18_check(n_groups, member_off, genome, n_members, nb_off, nb, n_nb, n_neighbor, L, text);
    return pep_message_out(rc, text, msg, msg_cap);
}

int pep_synteny_pairs(pep_ctx *ctx, uint32_t n_groups, const uint64_t *member_off, const uint32_t *genome, uint64_t n_members, const uint64_t *nb_off, const uint32_t *nb,
                      uint64_t n_nb, int32_t n_neighbor, uint8_t *has_conflict, int32_t *dc, uint64_t *conf_off, uint64_t *walk_off)
{
    if (!ctx) return PEP_ERR_ARG;
    if (!conf_off || !walk_off || (n_groups && (!has_conflict || !dc))) return pep_fail(ctx, PEP_ERR_ARG, std::string(K18_ME) + "null table");
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    return k18_pairs(ctx, n_groups, member_off, genome, n_members, nb_off, nb, n_nb, n_neighbor, has_conflict, dc, conf_off, walk_off);
}

int pep_synteny_pairs_copy(pep_ctx *ctx, uint32_t *conf, uint64_t n_conf, uint32_t *walk, uint64_t n_walk)
{
    if (!ctx) return PEP_ERR_ARG;
    if (n_conf != ctx->k18_n_conf || n_walk != ctx->k18_n_walk)
        return pep_fail(ctx, PEP_ERR_ARG, "pep_synteny_pairs_copy: the newest pep_synteny_pairs of this context left " + std::to_string(ctx->k18_n_conf) + " conflict and " +
                                              std::to_string(ctx->k18_n_walk) + " walk pairs");
    if ((n_conf && !conf) || (n_walk && !walk)) return pep_fail(ctx, PEP_ERR_ARG, "pep_synteny_pairs_copy: null table");
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    // both lists wait in memory of the library until the stream has been waited for: on an error nothing is written
    std::vector<uint32_t> h_conf(2 * n_conf), h_walk(2 * n_walk);
    PEP_TRY(pep_d2h_queue(ctx, h_conf.data(), ctx->k18[K18_CONF_OUT].p, n_conf * 8));
    PEP_TRY(pep_d2h_queue(ctx, h_walk.data(), ctx->k18[K18_WALK_OUT].p, n_walk * 8));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    if (n_conf) memcpy(conf, h_conf.data(), n_conf * 8);
    if (n_walk) memcpy(walk, h_walk.data(), n_walk * 8);
    ctx->calls[PEP_CALL_SYNTENY_PAIRS].bytes_to_host += 8 * (n_conf + n_walk);
    return PEP_OK;
}

int pep_synteny_walk(uint32_t n_groups, const uint64_t *member_off, const uint64_t *conf_off, const uint32_t *conf, const uint64_t *walk_off, const uint32_t *walk,
                     uint8_t *verdict, uint32_t *n_comp, uint32_t *comp_root, uint32_t *comp_len, uint32_t *members, char *msg, uint64_t msg_cap)
{
    const auto bad = [&](const std::string &text) { return pep_message_out(PEP_ERR_ARG, "pep_synteny_walk: " + text, msg, msg_cap); };
    if (!member_off || !conf_off || !walk_off || (n_groups && (!verdict || !n_comp))) return bad("null table");
    if (member_off[0] != 0 || conf_off[0] != 0 || walk_off[0] != 0) return bad("offsets must start at 0");
    for (uint32_t g = 0; g < n_groups; ++g)
        if (member_off[g + 1] < member_off[g] || conf_off[g + 1] < conf_off[g] || walk_off[g + 1] < walk_off[g] || member_off[g + 1] - member_off[g] >= 0xFFFFFFFFull)
            return bad("offsets must be non-decreasing (group " + std::to_string(g) + ")");
    if ((conf_off[n_groups] && !conf) || (walk_off[n_groups] && !walk) || (member_off[n_groups] && (!comp_root || !comp_len || !members))) return bad("null table");
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t n = (uint32_t)(member_off[g + 1] - member_off[g]);
        for (int which = 0; which < 2; ++which) {
            const uint32_t *list = which ? walk : conf;
            const uint64_t *off = which ? walk_off : conf_off;
            for (uint64_t p = off[g]; p < off[g + 1]; ++p)
                if (!(list[2 * p] < list[2 * p + 1] && list[2 * p + 1] < n))
                    return bad(std::string(which ? "walk" : "conflict") + " pair " + std::to_string(p) + " of group " + std::to_string(g) + " is not m < k < n");
        }
    }
    Walker W;
    const uint32_t none = 0xFFFFFFFFu;
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t n = (uint32_t)(member_off[g + 1] - member_off[g]);
        const uint32_t *cf = conf ? conf + 2 * conf_off[g] : nullptr;
        const uint64_t n_cf = conf_off[g + 1] - conf_off[g];
        verdict[g] = 0;
        n_comp[g] = 0;
        if (n_cf == 0) continue;
        // conflict adjacency in CSR form
        W.adj_off.assign((size_t)n + 1, 0);
        for (uint64_t p = 0; p < n_cf; ++p) ++W.adj_off[cf[2 * p] + 1], ++W.adj_off[cf[2 * p + 1] + 1];
        for (uint32_t i = 0; i < n; ++i) W.adj_off[i + 1] += W.adj_off[i];
        W.adj.resize(2 * n_cf);
        W.in_conflict.assign(W.adj_off.begin(), W.adj_off.end() - 1);    // (fill cursors first)
        for (uint64_t p = 0; p < n_cf; ++p) {
            W.adj[W.in_conflict[cf[2 * p]]++] = cf[2 * p + 1];
            W.adj[W.in_conflict[cf[2 * p + 1]]++] = cf[2 * p];
        }
        W.parent.resize(n);
        W.next.assign(n, none);
        W.a_head.assign(n, none), W.a_tail.assign(n, none), W.b_head.assign(n, none), W.b_tail.assign(n, none);
        W.weight.assign(n, 0);
        for (uint32_t i = 0; i < n; ++i) {
            W.parent[i] = i;
            W.in_conflict[i] = W.adj_off[i + 1] > W.adj_off[i];
            if (W.in_conflict[i]) W.a_head[i] = W.a_tail[i] = i, W.weight[i] = W.adj_off[i + 1] - W.adj_off[i];
            else W.b_head[i] = W.b_tail[i] = i;
        }
        const uint32_t *wk = walk ? walk + 2 * walk_off[g] : nullptr;
        for (uint64_t p = walk_off[g]; p < walk_off[g + 1]; ++p, wk += 2) {
            const uint32_t ti = W.find(wk[0]), tj = W.find(wk[1]);
            if (ti == tj) continue;
            // a conflict pair between the two A lists?  over the conflict ends of the cheaper side
            const uint32_t from = W.weight[ti] <= W.weight[tj] ? ti : tj, other = from == ti ? tj : ti;
            bool skip = false;
            for (uint32_t x = W.a_head[from]; x != none && !skip; x = W.next[x])
                for (uint32_t e = W.adj_off[x]; e < W.adj_off[x + 1]; ++e)
                    if (W.find(W.adj[e]) == other) { skip = true; break; }
            if (skip) continue;
            // tj goes into ti: the root of the union is ti, as the reference keeps tags[i]
            W.parent[tj] = ti;
            if (W.a_head[tj] != none) {
                if (W.a_head[ti] == none) W.a_head[ti] = W.a_head[tj]; else W.next[W.a_tail[ti]] = W.a_head[tj];
                W.a_tail[ti] = W.a_tail[tj];
            }
            if (W.b_head[tj] != none) {
                if (W.b_head[ti] == none) W.b_head[ti] = W.b_head[tj]; else W.next[W.b_tail[ti]] = W.b_head[tj];
                W.b_tail[ti] = W.b_tail[tj];
            }
            W.weight[ti] += W.weight[tj];
        }
        bool all_in_conflict = true;
        for (uint32_t i = 0; i < n; ++i)
            if (W.parent[i] == i && W.a_head[i] == none) all_in_conflict = false;
        if (!all_in_conflict) { verdict[g] = 1; continue; }
        verdict[g] = 2;
        uint32_t *out = members + member_off[g], *len = comp_len + member_off[g], *root = comp_root + member_off[g];
        uint32_t at = 0, comps = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (W.parent[i] != i) continue;
            const uint32_t before = at;
            for (uint32_t x = W.a_head[i]; x != none; x = W.next[x]) out[at++] = x;
            for (uint32_t x = W.b_head[i]; x != none; x = W.next[x]) out[at++] = x;
            root[comps] = i;
            len[comps++] = at - before;
        }
        n_comp[g] = comps;
    }
    return pep_message_out(PEP_OK, "", msg, msg_cap);
}

}  // extern "C"
