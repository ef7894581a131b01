// K21: neighbour-joining trees, the two rapidnj calls of the reference - `rapidnj -i fa -t d` per paralogous group of filt_per_group (PEPPAN.py:19,
// 409-417) and `rapidnj -i pd` behind writeCGAV (PEPPAN_parser.py:168).  One process and one temporary file per tree there; one batch here.
//   kimura_pairs     (PEPPAN.py:19, 409-417: the distance `-i fa` computes.)  K15's bit planes (allelediff.hip) and K15's tile body with its SPLIT
//                    parameter (allelediff_tile.h): per pair the comparable columns, the transitions - mismatches whose codes differ in plane B1 alone -
//                    and the other mismatches, three int32 per pair in the order of K15's packed triangle.  The logarithm is host work (njtree.py).
//   nj_block<CAP>    (PEPPAN.py:416, PEPPAN_parser.py:168.)  One workgroup per tree of up to PEP_NJ_BLOCK_LEAVES leaves.  The upper triangle is mirrored
//                    into a full matrix - in LDS with an odd row length for n <= CAP, else in place in the call's device copy -, the row sums r are
//                    added up once and then kept by the rank-one update, and every round is: arg-min of Q over the pairs of live slots (a wavefront
//                    per row a, lanes along b; shuffles within the wavefront, four partial results through LDS), the join, the update of row a and r.
//                    The live slots are an ascending list that is rewritten into its second copy by the update, so a round has two barriers.
//   nj_chain_*       (PEPPAN_parser.py:168 at thousands of genomes.)  Larger trees: the same round as two plain launches on the context's stream,
//                    nj_chain_argmin (up to 256 workgroups leave one partial result each) and nj_chain_update (every workgroup reduces the partial
//                    results for itself, then updates its share of row a).  The end of a launch is the only thing one workgroup ever knows of another:
//                    no grid-wide barrier, no cooperative launch, no ticket, no loop that waits.
// The arithmetic is stated in include/peppan_hip.h (K21) and restated in numpy by tests/njtree_helpers.py; the device equals it bit for bit, so every
// double operation here is one correctly rounded operation: contraction into fused multiply-adds is switched off for the whole file.
// Not tuned: the rates are in profiles/njtree_rate.txt.  Known slack: a workgroup of 256 threads for a tree of 5 leaves; the row sums are one thread per row.
#include "common.h"
#include "allelediff_tile.h"
#include "grouptable.h"
#include <algorithm>
#include <cmath>
#include <numeric>

#pragma clang fp contract(off)

namespace {

// the slots of pep_ctx::k21
enum { K21_DIST = 0, K21_TREES, K21_NODE, K21_LEN, K21_STATE, K21_SLOTS };
static_assert(K21_SLOTS == sizeof(pep_ctx::k21) / sizeof(DevBuf), "one member of pep_ctx::k21 per slot");
static_assert(K15_WS_SLOTS <= PEP_WS_HITS_OUT, "pep_kimura_pairs uses K15's slots of ctx->ws: it leaves the device-resident hit table alone");

constexpr int NJ_BLOCK = 256;
constexpr int NJ_WAVES = NJ_BLOCK / 64;
constexpr uint32_t NJ_NO_PAIR = 0xFFFFFFFFu;
constexpr int NJ_CHAIN_PARTS = 256;                     // most workgroups of nj_chain_argmin
constexpr int NJ_LDS_SMALL = 32, NJ_LDS_MID = 80;       // nj_block's two LDS classes: 8.3 KiB and 50.6 KiB of matrix
static_assert(PEP_NJ_BLOCK_LEAVES <= NJ_BLOCK && PEP_NJ_MAX_LEAVES < 65536, "a live list per thread; a pair key is two 16-bit list positions");

struct NjTree { uint64_t dist_off, out_off; uint32_t n, pad; };

__global__ __launch_bounds__(256) void kimura_pairs(const DiffTile *__restrict__ tiles, const GroupRec *__restrict__ groups, const uint32_t *__restrict__ grp_rows,
                                                    const uint64_t *__restrict__ plane_off, const unsigned long long *__restrict__ planes, int32_t *__restrict__ out)
{
    const DiffTile T = tiles[blockIdx.x];
    const GroupRec G = groups[T.g];
    const uint32_t tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    uint32_t mis[4][4], cmp[4][4], ts[4][4];
    k15_tile_counts_of<true>(grp_rows + G.rows_off, G.n, G.words, T, plane_off, planes, mis, cmp, ts);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t a = (uint64_t)T.ti * K15_TILE + ty * 4 + i, b = (uint64_t)T.tj * K15_TILE + tx + 16 * j, n = G.n;
            if (a < b && b < n) {
                int32_t *o = out + 3 * (G.tri_off + a * (2 * n - a - 1) / 2 + (b - a - 1));
                o[0] = (int32_t)cmp[i][j];
                o[1] = (int32_t)ts[i][j];
                o[2] = (int32_t)(mis[i][j] - ts[i][j]);
            }
        }
}

// ---- the round, shared by both paths

// the better of two candidates: the smaller Q, then the smaller key (a NaN is never the smaller Q; a lane without a pair holds +infinity and NJ_NO_PAIR)
__device__ __forceinline__ void nj_take(double &q, uint32_t &key, double oq, uint32_t okey)
{
    if (oq < q || (oq == q && okey < key)) { q = oq; key = okey; }
}

__device__ __forceinline__ void nj_wave_min(double &q, uint32_t &key)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double oq = __shfl_xor(q, off, 64);
        const uint32_t okey = __shfl_xor(key, off, 64);
        nj_take(q, key, oq, okey);
    }
}

// the best pair of rows row0, row0 + row_step, .. of the live list as this lane sees it (a wavefront per row, its lanes along the columns): list positions
// i < j in key = i << 16 | j, visited in ascending key order
__device__ __forceinline__ void nj_scan_rows(const double *D, uint32_t ld, const double *r, const uint32_t *live, uint32_t m, uint32_t row0, uint32_t row_step,
                                             uint32_t lane, double &q_best, uint32_t &key_best)
{
    const double mm2 = (double)(m - 2);
    for (uint32_t i = row0; i + 1 < m; i += row_step) {
        const uint32_t a = live[i];
        const double ra = r[a];
        const double *row = D + (uint64_t)a * ld;
        for (uint32_t j = i + 1 + lane; j < m; j += 64) {
            const uint32_t b = live[j];
            const double q = (mm2 * row[b] - ra) - r[b];
            if (q < q_best) { q_best = q; key_best = (i << 16) | j; }
        }
    }
}

// the join of list positions i < j at m live slots, join number s of a tree of n leaves, by ONE thread: the two output entries, r[a] and node[a]
__device__ __forceinline__ void nj_join(const double *D, uint32_t ld, double *r, uint32_t *node, uint32_t a, uint32_t b, uint32_t m, uint32_t n, uint32_t s,
                                        uint32_t *node_out, double *len_out)
{
    const double dab = D[(uint64_t)a * ld + b], ra = r[a], rb = r[b];
    const double la = 0.5 * dab + (ra - rb) / (double)(2 * (m - 2));
    node_out[2 * s] = node[a];
    node_out[2 * s + 1] = node[b];
    len_out[2 * s] = la;
    len_out[2 * s + 1] = dab - la;
    r[a] = 0.5 * ((ra + rb) - (double)m * dab);
    node[a] = n + s;
}

// live slot k (neither a nor b) after the join of a and b
__device__ __forceinline__ void nj_update(double *D, uint32_t ld, double *r, uint32_t a, uint32_t b, uint32_t k, double dab)
{
    const double dak = D[(uint64_t)a * ld + k], dbk = D[(uint64_t)b * ld + k];
    const double du = ((dak + dbk) - dab) * 0.5;
    r[k] = ((r[k] - dak) - dbk) + du;
    D[(uint64_t)a * ld + k] = du;
    D[(uint64_t)k * ld + a] = du;
}

// the last three live slots a < b < c (n >= 3), by one thread: entries 2 (n - 3) .. 2 n - 4, in slot order but for a tree of three leaves
__device__ __forceinline__ void nj_last_three(const double *D, uint32_t ld, const uint32_t *node, const uint32_t *live, uint32_t n, uint32_t *node_out, double *len_out)
{
    const uint32_t a = live[0], b = live[1], c = live[2];
    const double dab = D[(uint64_t)a * ld + b], dac = D[(uint64_t)a * ld + c], dbc = D[(uint64_t)b * ld + c];
    const double la = 0.5 * ((dab + dac) - dbc);
    const uint32_t at = 2 * (n - 3), ia = n == 3 ? 1u : 0u;           // (three leaves: rapidnj prints them 1, 0, 2)
    node_out[at + ia] = node[a]; node_out[at + (ia ^ 1u)] = node[b]; node_out[at + 2] = node[c];
    len_out[at + ia] = la; len_out[at + (ia ^ 1u)] = dab - la; len_out[at + 2] = dac - la;
}

// ---- one workgroup per tree.  CAP > 0: trees of at most CAP leaves, the matrix in LDS; CAP == 0: the matrix in place in `dist` (the call's device copy)
template <int CAP>
__global__ __launch_bounds__(NJ_BLOCK) void nj_block(const NjTree *__restrict__ trees, const uint32_t *__restrict__ which, double *dist,
                                                     uint32_t *__restrict__ node_all, double *__restrict__ len_all)
{
    constexpr int LDS_DOUBLES = CAP ? CAP * (CAP | 1) : 1;
    __shared__ double s_mat[LDS_DOUBLES];
    __shared__ double s_r[NJ_BLOCK], s_pq[NJ_WAVES];
    __shared__ uint32_t s_live[2][NJ_BLOCK], s_node[NJ_BLOCK], s_pkey[NJ_WAVES];
    const NjTree T = trees[which[blockIdx.x]];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = T.n;
    const uint32_t ld = CAP ? (n | 1u) : n;                 // (LDS: an odd row length, so the rows of a column spread over the banks)
    double *g = dist + T.dist_off;
    double *D = CAP ? s_mat : g;
    uint32_t *node_out = node_all + T.out_off;
    double *len_out = len_all + T.out_off;
    if (n == 2) {
        if (tid < 2) { node_out[tid] = tid; len_out[tid] = g[1]; }
        return;
    }
    // the full matrix from the upper triangle
    for (uint32_t e = tid; e < n * n; e += NJ_BLOCK) {
        const uint32_t i = e / n, j = e % n;
        if (CAP) D[i * ld + j] = i < j ? g[(uint64_t)i * n + j] : i > j ? g[(uint64_t)j * n + i] : 0.0;
        else if (i > j) g[e] = g[(uint64_t)j * n + i];
        else if (i == j) g[e] = 0.0;
    }
    __syncthreads();
    if (tid < n) {
        double sum = 0.0;
        for (uint32_t j = 0; j < n; ++j) sum = sum + D[(uint64_t)tid * ld + j];
        s_r[tid] = sum;
        s_live[0][tid] = tid;
        s_node[tid] = tid;
    }
    __syncthreads();
    uint32_t p = 0;
    for (uint32_t m = n, s = 0; m > 3; --m, ++s, p ^= 1) {
        const uint32_t *live = s_live[p];
        uint32_t *next = s_live[p ^ 1];
        double q = INFINITY;
        uint32_t key = NJ_NO_PAIR;
        nj_scan_rows(D, ld, s_r, live, m, wave, NJ_WAVES, lane, q, key);
        nj_wave_min(q, key);
        if (lane == 0) { s_pq[wave] = q; s_pkey[wave] = key; }
        __syncthreads();
        q = s_pq[0]; key = s_pkey[0];
#pragma unroll
        for (int w = 1; w < NJ_WAVES; ++w) nj_take(q, key, s_pq[w], s_pkey[w]);
        if (key == NJ_NO_PAIR) key = 1;                     // no Q below +infinity: the first two live slots
        const uint32_t i = key >> 16, j = key & 0xFFFFu, a = live[i], b = live[j];
        const double dab = D[(uint64_t)a * ld + b];
        if (tid < m && tid != j) {
            const uint32_t k = live[tid];
            if (tid != i) nj_update(D, ld, s_r, a, b, k, dab);
            next[tid - (tid > j ? 1u : 0u)] = k;
        }
        if (tid == NJ_BLOCK - 1) nj_join(D, ld, s_r, s_node, a, b, m, n, s, node_out, len_out);       // (r[a], r[b], node[a]: nobody else's this round)
        __syncthreads();
    }
    if (tid == 0) nj_last_three(D, ld, s_node, s_live[p], n, node_out, len_out);
}

// ---- the launch chain of one large tree.  State in device memory: r[n], the partial results, two live lists, node[n]
struct NjChain {
    double *D, *r, *pq;
    uint32_t *pkey, *live0, *live1, *node;
    uint32_t *node_out;
    double *len_out;
    uint32_t n;
};

__global__ __launch_bounds__(NJ_BLOCK) void nj_chain_fill(NjChain C)
{
    const uint64_t n = C.n, e = (uint64_t)blockIdx.x * NJ_BLOCK + threadIdx.x;
    if (e >= n * n) return;
    const uint64_t i = e / n, j = e % n;
    if (i > j) C.D[e] = C.D[j * n + i];
    else if (i == j) C.D[e] = 0.0;
}

__global__ __launch_bounds__(NJ_BLOCK) void nj_chain_rows(NjChain C)
{
    const uint32_t k = blockIdx.x * NJ_BLOCK + threadIdx.x;
    if (k >= C.n) return;
    double sum = 0.0;
    for (uint32_t j = 0; j < C.n; ++j) sum = sum + C.D[(uint64_t)k * C.n + j];
    C.r[k] = sum;
    C.live0[k] = k;
    C.node[k] = k;
}

// workgroup x of gridDim.x <= NJ_CHAIN_PARTS takes rows 4 x + wave, + 4 gridDim.x, .. and leaves its best pair in pq[x], pkey[x]
__global__ __launch_bounds__(NJ_BLOCK) void nj_chain_argmin(NjChain C, uint32_t m, uint32_t parity)
{
    __shared__ double s_pq[NJ_WAVES];
    __shared__ uint32_t s_pkey[NJ_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double q = INFINITY;
    uint32_t key = NJ_NO_PAIR;
    nj_scan_rows(C.D, C.n, C.r, parity ? C.live1 : C.live0, m, blockIdx.x * NJ_WAVES + wave, gridDim.x * NJ_WAVES, lane, q, key);
    nj_wave_min(q, key);
    if (lane == 0) { s_pq[wave] = q; s_pkey[wave] = key; }
    __syncthreads();
    if (tid == 0) {
        q = s_pq[0]; key = s_pkey[0];
#pragma unroll
        for (int w = 1; w < NJ_WAVES; ++w) nj_take(q, key, s_pq[w], s_pkey[w]);
        C.pq[blockIdx.x] = q;
        C.pkey[blockIdx.x] = key;
    }
}

// every workgroup reduces the `parts` partial results of the launch before for itself; thread x of the grid then has list position x
__global__ __launch_bounds__(NJ_BLOCK) void nj_chain_update(NjChain C, uint32_t m, uint32_t s, uint32_t parity, uint32_t parts)
{
    __shared__ double s_pq[NJ_WAVES];
    __shared__ uint32_t s_pkey[NJ_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double q = tid < parts ? C.pq[tid] : INFINITY;
    uint32_t key = tid < parts ? C.pkey[tid] : NJ_NO_PAIR;
    if (!(q < INFINITY)) { q = INFINITY; key = NJ_NO_PAIR; }
    nj_wave_min(q, key);
    if (lane == 0) { s_pq[wave] = q; s_pkey[wave] = key; }
    __syncthreads();
    q = s_pq[0]; key = s_pkey[0];
#pragma unroll
    for (int w = 1; w < NJ_WAVES; ++w) nj_take(q, key, s_pq[w], s_pkey[w]);
    if (key == NJ_NO_PAIR) key = 1;
    const uint32_t *live = parity ? C.live1 : C.live0;
    uint32_t *next = parity ? C.live0 : C.live1;
    const uint32_t i = key >> 16, j = key & 0xFFFFu, a = live[i], b = live[j], x = blockIdx.x * NJ_BLOCK + tid;
    const double dab = C.D[(uint64_t)a * C.n + b];
    if (x < m && x != j) {
        const uint32_t k = live[x];
        if (x != i) nj_update(C.D, C.n, C.r, a, b, k, dab);
        next[x - (x > j ? 1u : 0u)] = k;
    }
    if (x == i) nj_join(C.D, C.n, C.r, C.node, a, b, m, C.n, s, C.node_out, C.len_out);        // (the one thread that touches r[a], r[b], node[a] in this launch)
}

__global__ void nj_chain_last(NjChain C, uint32_t parity)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) nj_last_three(C.D, C.n, C.node, parity ? C.live1 : C.live0, C.n, C.node_out, C.len_out);
}

const char *const K21_PAIRS_ME = "pep_kimura_pairs: ";
const char *const K21_NJ_ME = "pep_nj_trees: ";

uint64_t nj_entries(uint32_t n) { return n == 2 ? 2 : 2 * (uint64_t)n - 3; }

// every check of pep_nj_trees that reads no distance
int nj_check(const uint32_t *n_leaves, uint32_t n_trees, const uint64_t *dist_off, const uint64_t *out_off, std::string &msg)
{
    const auto bad = [&](int code, const std::string &text) { msg = K21_NJ_ME + text; return code; };
    if (n_trees == 0) return PEP_OK;
    if (!n_leaves || !dist_off || !out_off) return bad(PEP_ERR_ARG, "null table");
    for (uint32_t t = 0; t < n_trees; ++t) {
        const uint64_t n = n_leaves[t];
        const std::string tree = "tree " + std::to_string(t);
        if (n < 2) return bad(PEP_ERR_ARG, tree + " has " + std::to_string(n) + " leaves, a tree needs 2");
        if (n > PEP_NJ_MAX_LEAVES) return bad(PEP_ERR_LIMIT, tree + " has " + std::to_string(n) + " leaves, more than " + std::to_string(PEP_NJ_MAX_LEAVES));
        if (dist_off[t + 1] < dist_off[t] || dist_off[t + 1] - dist_off[t] < n * n)
            return bad(PEP_ERR_ARG, "the matrix of " + tree + " (" + std::to_string(n * n) + " distances from " + std::to_string(dist_off[t]) +
                                        ") overlaps the next one or runs past the array (dist_off[" + std::to_string(t + 1) + "] = " + std::to_string(dist_off[t + 1]) + ")");
        if (out_off[t + 1] < out_off[t] || out_off[t + 1] - out_off[t] < nj_entries((uint32_t)n))
            return bad(PEP_ERR_ARG, "the output of " + tree + " (" + std::to_string(nj_entries((uint32_t)n)) + " entries from " + std::to_string(out_off[t]) +
                                        ") overlaps the next one or runs past the arrays (out_off[" + std::to_string(t + 1) + "] = " + std::to_string(out_off[t + 1]) + ")");
    }
    const uint64_t span = dist_off[n_trees] - dist_off[0];
    if (span > PEP_NJ_MAX_BYTES / 8)
        return bad(PEP_ERR_LIMIT, std::to_string(span) + " distances (" + std::to_string(span / 1024 * 8) + " KiB) asked for, the device budget of one call is " +
                                      std::to_string((uint64_t)PEP_NJ_MAX_BYTES) + " bytes (split the batch)");
    if (out_off[n_trees] - out_off[0] > PEP_NJ_MAX_BYTES / 8)
        return bad(PEP_ERR_LIMIT, std::to_string(out_off[n_trees] - out_off[0]) + " output entries asked for, more than " + std::to_string((uint64_t)PEP_NJ_MAX_BYTES / 8));
    return PEP_OK;
}

}  // namespace

extern "C" {

int pep_kimura_pairs(pep_ctx *ctx, const uint8_t *h_packed, const uint64_t *h_row_off, const uint32_t *h_row_len, uint64_t n_rows, uint32_t n_groups,
                     const uint64_t *h_grp_off, const uint32_t *h_grp_rows, int32_t *h_out, const uint64_t *h_out_off, uint64_t out_cap)
{
    if (!ctx) return PEP_ERR_ARG;
    CallTimes &times = ctx->calls[PEP_CALL_KIMURA_PAIRS];
    times = {};
    if (!h_row_off || (n_rows && !h_row_len) || (n_groups && (!h_grp_off || !h_out_off)) || (out_cap && !h_out))
        return pep_fail(ctx, PEP_ERR_ARG, std::string(K21_PAIRS_ME) + "null table");
    if (n_groups && h_grp_off[n_groups] && !h_grp_rows) return pep_fail(ctx, PEP_ERR_ARG, std::string(K21_PAIRS_ME) + "null table");
    if (n_rows && h_row_off[n_rows] && !h_packed) return pep_fail(ctx, PEP_ERR_ARG, std::string(K21_PAIRS_ME) + "null table");
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    if (n_groups == 0) return PEP_OK;
    const GroupTables T{h_packed, h_row_off, h_row_len, n_rows, n_groups, h_grp_off, h_grp_rows};
    const GroupSpec S{K21_PAIRS_ME, "pair counts", "tiles of pairs", 2};
    GroupLayout L;
    std::vector<uint64_t> need(n_groups, 0);            // int32 values of every group's output
    std::string msg;
    const int rc = group_tables_check(T, S, [&](uint32_t, unsigned &want) { want = 1; return std::string(); },
                                      [&](uint32_t g, const GroupRec &, uint64_t added) { need[g] = 3 * added; return 0; }, L, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    if (L.pairs * 12 > PEP_NJ_MAX_BYTES)
        return pep_fail(ctx, PEP_ERR_LIMIT, K21_PAIRS_ME + std::to_string(L.pairs * 12) + " bytes of pair counts asked for, the device budget of one call is " +
                                                std::to_string((uint64_t)PEP_NJ_MAX_BYTES) + " (split the batch)");
    std::vector<uint32_t> order(n_groups);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return h_out_off[a] < h_out_off[b]; });
    uint64_t end_before = 0;
    for (uint32_t g : order) {
        if (!need[g]) continue;
        if (h_out_off[g] > out_cap || need[g] > out_cap - h_out_off[g])
            return pep_fail(ctx, PEP_ERR_ARG, K21_PAIRS_ME + ("output of group " + std::to_string(g)) + " runs past out_cap");
        if (h_out_off[g] < end_before) return pep_fail(ctx, PEP_ERR_ARG, K21_PAIRS_ME + ("output of group " + std::to_string(g)) + " overlaps another group's");
        end_before = h_out_off[g] + need[g];
    }
    if (L.tiles.empty()) {
        // no group of two rows: no kernel runs, so the bytes are looked at here
        for (uint64_t k = 0; k < h_row_off[n_rows]; ++k)
            if (h_packed[k] > 124) return group_tables_bad_byte(ctx, S, (uint64_t)(std::upper_bound(h_row_off, h_row_off + n_rows + 1, k) - h_row_off) - 1);
        return PEP_OK;
    }
    DevBuf *W = ctx->ws;
    PEP_TRY(group_tables_to_device(ctx, T, L, L.groups.data(), (size_t)n_groups * sizeof(GroupRec), {{K15_WS_OUT, nullptr, (L.pairs + 1) * 12, 0}}, times.ms[0]));
    pep_timed_stage(ctx, times.ms[1], [&] {
        hipLaunchKernelGGL(kimura_pairs, dim3((unsigned)L.tiles.size()), dim3(256), 0, ctx->stream, W[K15_WS_TILES].as<const DiffTile>(), W[K15_WS_GROUPS].as<const GroupRec>(),
                           W[K15_WS_GRP_ROWS].as<const uint32_t>(), W[K15_WS_PLANE_OFF].as<const uint64_t>(), W[K15_WS_PLANES].as<const unsigned long long>(), W[K15_WS_OUT].as<int32_t>());
    });
    PEP_TRY(group_tables_finish(ctx, S));
    // groups that follow each other in the caller's buffer as they do on the device leave in one copy
    uint64_t dev_at = 0, run_dev = 0, run_host = 0, run = 0;
    for (uint32_t g = 0; g <= n_groups; ++g) {
        if (g < n_groups && !need[g]) continue;
        if (g < n_groups && run && h_out_off[g] == run_host + run) {
            run += need[g];
        } else {
            if (run) PEP_TRY(pep_d2h_queue(ctx, h_out + run_host, W[K15_WS_OUT].as<const int32_t>() + run_dev, run * 4));
            if (g == n_groups) break;
            run_host = h_out_off[g]; run_dev = dev_at; run = need[g];
        }
        dev_at += need[g];
    }
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    return PEP_OK;
}

int pep_nj_trees_check(const uint32_t *n_leaves, uint32_t n_trees, const uint64_t *dist_off, const uint64_t *out_off, char *msg, uint64_t msg_cap)
{
    std::string text;
    const int rc = nj_check(n_leaves, n_trees, dist_off, out_off, text);
    return pep_message_out(rc, text, msg, msg_cap);
}

int pep_nj_trees(pep_ctx *ctx, const double *h_dist, const uint64_t *h_dist_off, const uint32_t *h_n, uint32_t n_trees, uint32_t *h_node, double *h_len,
                 const uint64_t *h_out_off)
{
    if (!ctx) return PEP_ERR_ARG;
    CallTimes &times = ctx->calls[PEP_CALL_NJ_TREES];
    times = {};
    std::string msg;
    const int rc = nj_check(h_n, n_trees, h_dist_off, h_out_off, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    if (n_trees == 0) return PEP_OK;
    if (!h_dist || !h_node || !h_len) return pep_fail(ctx, PEP_ERR_ARG, std::string(K21_NJ_ME) + "null table");
    // the trees as the kernels read them (offsets into the device copies, which start at the first tree), by class; the distances that are read
    const uint64_t dist0 = h_dist_off[0], out0 = h_out_off[0], n_dist = h_dist_off[n_trees] - dist0, n_out = h_out_off[n_trees] - out0;
    std::vector<NjTree> trees(n_trees);
    std::vector<uint32_t> cls[3], chain;                // LDS small, LDS mid, in place; the launch chains
    uint32_t chain_max = 0;
    for (uint32_t t = 0; t < n_trees; ++t) {
        const uint32_t n = h_n[t];
        const double *d = h_dist + h_dist_off[t];
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j = i + 1; j < n; ++j)
                if (!std::isfinite(d[(uint64_t)i * n + j]))
                    return pep_fail(ctx, PEP_ERR_ARG, K21_NJ_ME + ("distance [" + std::to_string(i) + ", " + std::to_string(j) + "] of tree " + std::to_string(t)) + " is not finite");
        trees[t] = NjTree{h_dist_off[t] - dist0, h_out_off[t] - out0, n, 0u};
        if (n > PEP_NJ_BLOCK_LEAVES) { chain.push_back(t); chain_max = std::max(chain_max, n); }
        else cls[n <= NJ_LDS_SMALL ? 0 : n <= NJ_LDS_MID ? 1 : 2].push_back(t);
    }
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> which;
    for (const auto &c : cls) which.insert(which.end(), c.begin(), c.end());
    DevBuf *B = ctx->k21;
    // the state of a chain behind the class lists: r, pq (doubles), then pkey, live0, live1, node (words)
    const size_t which_bytes = (which.size() * 4 + 7) & ~(size_t)7;
    const size_t state_bytes = which_bytes + ((size_t)chain_max + NJ_CHAIN_PARTS) * 8 + ((size_t)NJ_CHAIN_PARTS + 3 * (size_t)chain_max) * 4;
    PEP_TRY(pep_tables_to_device(ctx, B, {{K21_DIST, h_dist + dist0, n_dist * 8, 0}, {K21_TREES, trees.data(), trees.size() * sizeof(NjTree), 0},
                                          {K21_STATE, which.data(), which.size() * 4, state_bytes - which.size() * 4},
                                          {K21_NODE, nullptr, n_out * 4, 0}, {K21_LEN, nullptr, n_out * 8, 0}}));
    PEP_HIP(ctx, hipMemsetAsync(B[K21_NODE].p, 0, n_out * 4, ctx->stream));          // (the entries between two trees)
    PEP_HIP(ctx, hipMemsetAsync(B[K21_LEN].p, 0, n_out * 8, ctx->stream));
    double *d_dist = B[K21_DIST].as<double>();
    uint32_t *d_node = B[K21_NODE].as<uint32_t>();
    double *d_len = B[K21_LEN].as<double>();
    const NjTree *d_trees = B[K21_TREES].as<const NjTree>();
    const uint32_t *d_which = B[K21_STATE].as<const uint32_t>();
    if (!which.empty())
        pep_timed_stage(ctx, times.ms[0], [&] {
            size_t first = 0;
            if (!cls[0].empty()) hipLaunchKernelGGL(nj_block<NJ_LDS_SMALL>, dim3((unsigned)cls[0].size()), dim3(NJ_BLOCK), 0, ctx->stream, d_trees, d_which + first, d_dist, d_node, d_len);
            first += cls[0].size();
            if (!cls[1].empty()) hipLaunchKernelGGL(nj_block<NJ_LDS_MID>, dim3((unsigned)cls[1].size()), dim3(NJ_BLOCK), 0, ctx->stream, d_trees, d_which + first, d_dist, d_node, d_len);
            first += cls[1].size();
            if (!cls[2].empty()) hipLaunchKernelGGL(nj_block<0>, dim3((unsigned)cls[2].size()), dim3(NJ_BLOCK), 0, ctx->stream, d_trees, d_which + first, d_dist, d_node, d_len);
        });
    PEP_HIP(ctx, hipGetLastError());
    if (!chain.empty()) {
        uint8_t *st = B[K21_STATE].as<uint8_t>() + which_bytes;
        NjChain C{};
        C.r = reinterpret_cast<double *>(st);
        C.pq = C.r + chain_max;
        C.pkey = reinterpret_cast<uint32_t *>(C.pq + NJ_CHAIN_PARTS);
        C.live0 = C.pkey + NJ_CHAIN_PARTS;
        C.live1 = C.live0 + chain_max;
        C.node = C.live1 + chain_max;
        pep_timed_stage(ctx, times.ms[1], [&] {
            for (uint32_t t : chain) {
                const uint32_t n = h_n[t];
                C.D = d_dist + trees[t].dist_off;
                C.node_out = d_node + trees[t].out_off;
                C.len_out = d_len + trees[t].out_off;
                C.n = n;
                hipLaunchKernelGGL(nj_chain_fill, dim3((unsigned)ceil_div((uint64_t)n * n, NJ_BLOCK)), dim3(NJ_BLOCK), 0, ctx->stream, C);
                hipLaunchKernelGGL(nj_chain_rows, dim3((unsigned)ceil_div(n, NJ_BLOCK)), dim3(NJ_BLOCK), 0, ctx->stream, C);
                uint32_t parity = 0;
                for (uint32_t m = n, s = 0; m > 3; --m, ++s, parity ^= 1) {
                    const uint32_t parts = (uint32_t)std::min<uint64_t>(NJ_CHAIN_PARTS, ceil_div(m - 1, NJ_WAVES));
                    hipLaunchKernelGGL(nj_chain_argmin, dim3(parts), dim3(NJ_BLOCK), 0, ctx->stream, C, m, parity);
                    hipLaunchKernelGGL(nj_chain_update, dim3((unsigned)ceil_div(m, NJ_BLOCK)), dim3(NJ_BLOCK), 0, ctx->stream, C, m, s, parity, parts);
                }
                hipLaunchKernelGGL(nj_chain_last, dim3(1), dim3(64), 0, ctx->stream, C, parity);
            }
        });
        PEP_HIP(ctx, hipGetLastError());
    }
    PEP_TRY(pep_d2h_queue(ctx, h_node + out0, d_node, n_out * 4));
    PEP_TRY(pep_d2h_queue(ctx, h_len + out0, d_len, n_out * 8));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    return PEP_OK;
}

}  // extern "C"
