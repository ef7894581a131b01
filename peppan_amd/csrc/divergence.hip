// K16: divergence verdicts of gene groups (the float layer of filt_per_group that decides whether a group is looked at per pair at all:
// checkDiv PEPPAN.py:335-344 over the edge rows :346-366, the distances test :371-382, the leader grouping :383-392).  K15 ships n^2 pairs per
// group to the host, which reduces nearly every group to one bit; here that reduction stays on the device:
//   allele_planes    K15's bit planes of the packed rows (allelediff.hip)
//   verdict_edge     one wavefront per few row pairs of a host-built list - (first, b), (last, b) of every group and, for in-paralog groups,
//                    of every genome's sub-group: lanes stride over the plane words, population counts, wave reduction, lane 0 evaluates
//                    mut / aln / denX > 1 and ORs bit 0 into flags[g].
//   verdict_pairs    K15's 64 x 64 tile loop (allelediff_tile.h) over all pairs a < b; a tile leaves at once when bit 0 of its group is
//                    clear.  Epilogue: the packed upper triangle goes to a device buffer, "d / gd0 > 1 / gd0" of the thread's 16 pairs is
//                    ORed over the workgroup and one atomicOr sets bit 1 of flags[g].
//   verdict_leaders  one workgroup per group, leaving at once unless bit 1 is set (after turning flags[g] into the verdict byte).  Rows in
//                    order; the leaders found so far sit in LDS (beyond 4 096: in a global list), the threads test them in parallel in chunks of
//                    256, the first match in leader order wins (ballot + find-first per wavefront, atomicMin in LDS over the four wavefronts).
// Every float decision is a chain of single correctly rounded double operations (__ddiv_rn / __dmul_rn: nothing to contract); the only
// transcendental of the reference, exp, depends on the genome pair alone and arrives in a host-made table (gd0, denX, den) sorted by
// g1 << 32 | g2, looked up by binary search.  Same-genome pairs use gd0 = fmax(self_id, 2 / aln) for all three.
// The checks of the row and group tables, their layout and the device prologue up to allele_planes are K15's (grouptable.h); here: the same-genome
// rule of the gd table (the table, its search and its check: gdtable.h), the grp_inparalog check, the edge-pair list and the 24-byte group record of the three kernels.
#include "common.h"
#include "allelediff_tile.h"
#include "grouptable.h"
#include "gdtable.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

struct pep_verdict_result {
    pep_ctx *ctx = nullptr;
    uint64_t serial = 0;                    // the context's call counter when this result was made: its device data lives until the next call
    std::vector<uint8_t> verdict;
    std::vector<uint64_t> rows_off, tri_off;
    std::vector<uint32_t> n;
};

namespace {

constexpr uint32_t K16_EDGE_PER_WAVE = 4;
constexpr uint32_t K16_LDS_LEADERS = 4096;

struct VGroup {                     // a GroupRec as the three kernels here read it
    uint64_t rows_off, tri_off;
    uint32_t n, words;
};
struct EdgePair { uint32_t g, a, b; };      // rows a, b (positions inside group g)
__device__ __forceinline__ void k16_gd(const GdTable &T, uint32_t ga, uint32_t gb, double aln, double &gd0, double &denX, double &den)
{
    if (ga == gb) {
        gd0 = fmax(T.self_id, __ddiv_rn(2.0, aln));
        denX = den = gd0;                               // gd0 * exp(0 * x) == gd0
        return;
    }
    const uint64_t row = gd_row(T, ga, gb);
    gd0 = T.val[3 * row]; denX = T.val[3 * row + 1]; den = T.val[3 * row + 2];
}

__global__ __launch_bounds__(256) void verdict_edge(uint64_t n_pairs, const EdgePair *__restrict__ pairs, const VGroup *__restrict__ groups,
                                                    const uint32_t *__restrict__ grp_rows, const uint32_t *__restrict__ grp_genome,
                                                    const uint64_t *__restrict__ plane_off, const unsigned long long *__restrict__ planes,
                                                    const GdTable gd, uint32_t *flags)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t first = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * K16_EDGE_PER_WAVE;
    for (uint32_t k = 0; k < K16_EDGE_PER_WAVE && first + k < n_pairs; ++k) {
        const EdgePair P = pairs[first + k];
        if (__atomic_load_n(&flags[P.g], __ATOMIC_RELAXED) & 1u) continue;          // (already divergent: the tests are OR-ed)
        const VGroup G = groups[P.g];
        const unsigned long long *pa = planes + plane_off[grp_rows[G.rows_off + P.a]], *pb = planes + plane_off[grp_rows[G.rows_off + P.b]];
        uint32_t mis = 0, cmp = 0;
        for (uint32_t w = lane; w < G.words; w += 64) {
            const unsigned long long c = pa[w] & pb[w];
            cmp += (uint32_t)__popcll(c);
            mis += (uint32_t)__popcll(c & ((pa[G.words + w] ^ pb[G.words + w]) | (pa[2 * G.words + w] ^ pb[2 * G.words + w])));
        }
        for (int d = 32; d > 0; d >>= 1) {
            mis += __shfl_xor(mis, d, 64);
            cmp += __shfl_xor(cmp, d, 64);
        }
        if (lane == 0) {
            const double mut = (double)(mis + 1), aln = (double)(cmp + 2);
            double gd0, denX, den;
            k16_gd(gd, grp_genome[G.rows_off + P.a], grp_genome[G.rows_off + P.b], aln, gd0, denX, den);
            if (__ddiv_rn(__ddiv_rn(mut, aln), denX) > 1.0) atomicOr(&flags[P.g], 1u);
        }
    }
}

__global__ __launch_bounds__(256) void verdict_pairs(const DiffTile *__restrict__ tiles, const VGroup *__restrict__ groups,
                                                     const uint32_t *__restrict__ grp_rows, const uint32_t *__restrict__ grp_genome,
                                                     const uint64_t *__restrict__ plane_off, const unsigned long long *__restrict__ planes,
                                                     const GdTable gd, uint32_t *flags, int2 *__restrict__ tri)
{
    const DiffTile T = tiles[blockIdx.x];
    if (!(__atomic_load_n(&flags[T.g], __ATOMIC_RELAXED) & 1u)) return;             // not divergent (verdict_edge ran in front): the same word for the whole workgroup
    const VGroup G = groups[T.g];
    const uint32_t tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    uint32_t mis[4][4], cmp[4][4];
    k15_tile_counts(grp_rows + G.rows_off, G.n, G.words, T, plane_off, planes, mis, cmp);
    const uint64_t n = G.n;
    uint32_t ga[4], gb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint64_t a = (uint64_t)T.ti * K15_TILE + ty * 4 + i, b = (uint64_t)T.tj * K15_TILE + tx + 16 * i;
        ga[i] = a < n ? grp_genome[G.rows_off + a] : 0u;
        gb[i] = b < n ? grp_genome[G.rows_off + b] : 0u;
    }
    int beyond = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t a = (uint64_t)T.ti * K15_TILE + ty * 4 + i, b = (uint64_t)T.tj * K15_TILE + tx + 16 * j;
            if (a < b && b < n) {
                tri[G.tri_off + a * (2 * n - a - 1) / 2 + (b - a - 1)] = make_int2((int)mis[i][j] + 1, (int)cmp[i][j] + 2);
                if (!beyond) {
                    const double mut = (double)(mis[i][j] + 1), aln = (double)(cmp[i][j] + 2);
                    double gd0, denX, den;
                    k16_gd(gd, ga[i], gb[j], aln, gd0, denX, den);
                    const double d = __ddiv_rn(__ddiv_rn(mut, aln), den);
                    beyond = __ddiv_rn(d, gd0) > __ddiv_rn(1.0, gd0);
                }
            }
        }
    const int any = __syncthreads_or(beyond);
    if (threadIdx.x == 0 && any) atomicOr(&flags[T.g], 2u);
}

__global__ __launch_bounds__(256) void verdict_leaders(const VGroup *__restrict__ groups, const uint32_t *__restrict__ flags, const int2 *__restrict__ tri,
                                                       uint32_t *__restrict__ leader, uint32_t *spill, uint8_t *__restrict__ verdict)
{
    __shared__ uint32_t list[K16_LDS_LEADERS];
    __shared__ uint32_t s_best, s_nl;
    const uint32_t g = blockIdx.x, tid = threadIdx.x, f = flags[g];
    if (tid == 0) verdict[g] = (f & 2u) ? 2 : (f & 1u) ? 1 : 0;
    if (!(f & 2u)) return;
    const VGroup G = groups[g];
    const uint64_t n = G.n;
    uint32_t *out = leader + G.rows_off, *far = spill + G.rows_off;
    if (tid == 0) { s_best = 0xFFFFFFFFu; s_nl = 1; list[0] = 0; out[0] = 0; }      // row 0 is the first leader (n >= 2 here)
    __syncthreads();
    for (uint64_t j = 1; j < n; ++j) {                                              // nl >= 1: every round passes a barrier between reading s_nl and tid 0 writing it
        const uint32_t nl = s_nl;
        int found = 0;
        for (uint32_t c0 = 0; c0 < nl && !found; c0 += 256) {
            const uint32_t k = c0 + tid;
            bool match = false;
            if (k < nl) {
                const uint64_t l = k < K16_LDS_LEADERS ? list[k] : far[k];                     // l < j always
                const int2 v = tri[G.tri_off + l * (2 * n - l - 1) / 2 + (j - l - 1)];
                match = (double)v.x <= __dmul_rn(0.01, (double)v.y);
            }
            const unsigned long long hit = __ballot(match);
            if (hit && (tid & 63) == 0) atomicMin(&s_best, c0 + (tid & ~63u) + (uint32_t)__ffsll((long long)hit) - 1u);
            found = __syncthreads_or(match);
        }
        if (tid == 0) {
            if (found) {
                const uint32_t best = s_best;
                out[j] = best < K16_LDS_LEADERS ? list[best] : far[best];
                s_best = 0xFFFFFFFFu;
            } else {
                if (nl < K16_LDS_LEADERS) list[nl] = (uint32_t)j; else far[nl] = (uint32_t)j;
                out[j] = (uint32_t)j;
                s_nl = nl + 1;
            }
        }
        __syncthreads();
    }
}

struct Layout : GroupLayout {
    std::vector<EdgePair> edges;
    std::vector<double> gd;         // [n_gd + 1][3]
};

const GroupSpec K16_SPEC{"pep_group_verdicts: ", "triangles", "tiles or edge pairs", 2};

// every check of the tables, on the host, before anything is launched; also lays the device buffers out (the row and group tables: grouptable.h)
int k16_check(const GroupTables &T, const uint32_t *h_grp_genome, const uint8_t *h_inparalog, const uint64_t *gd_key, const double *gd_val, uint64_t n_gd,
              const double *gd_default, double self_id, Layout &L, std::string &msg)
{
    const auto bad = [&](int code, const std::string &text) { msg = K16_SPEC.me + text; return code; };
    if (!T.row_off || (T.n_rows && !T.row_len) || (T.n_groups && (!T.grp_off || !h_inparalog)) || (n_gd && (!gd_key || !gd_val)) || !gd_default) return bad(PEP_ERR_ARG, "null table");
    if (T.n_groups && T.grp_off[T.n_groups] && (!T.grp_rows || !h_grp_genome)) return bad(PEP_ERR_ARG, "null table");
    if (T.n_rows && T.row_off[T.n_rows] && !T.packed) return bad(PEP_ERR_ARG, "null table");
    if (!gd_good(self_id)) return bad(PEP_ERR_ARG, "self_id must be finite and > 0");
    const std::string fault = gd_table_fault(gd_key, gd_val, n_gd, gd_default);
    if (!fault.empty()) return bad(PEP_ERR_ARG, fault);
    L.gd.assign(gd_val, gd_val + 3 * n_gd);
    L.gd.insert(L.gd.end(), gd_default, gd_default + 3);
    std::vector<std::pair<uint32_t, uint32_t>> by_genome;
    return group_tables_check(T, K16_SPEC,
        [&](uint32_t g, unsigned &want) { want = 1; return h_inparalog[g] > 1 ? "grp_inparalog of group " + std::to_string(g) + " is neither 0 nor 1" : std::string(); },
        [&](uint32_t g, const GroupRec &G, uint64_t) {
            const uint32_t last = G.n - 1;
            for (uint32_t b = 0; b <= last; ++b) {
                if (b != 0) L.edges.push_back(EdgePair{g, 0u, b});
                if (b != last) L.edges.push_back(EdgePair{g, last, b});
            }
            if (h_inparalog[g]) {                                       // the first and the last row of every genome's sub-group against its rows (:352-366)
                by_genome.clear();
                for (uint32_t k = 0; k <= last; ++k) by_genome.emplace_back(h_grp_genome[G.rows_off + k], k);
                std::sort(by_genome.begin(), by_genome.end());
                for (size_t lo = 0; lo < by_genome.size();) {
                    size_t hi = lo;
                    while (hi < by_genome.size() && by_genome[hi].first == by_genome[lo].first) ++hi;
                    const uint32_t sf = by_genome[lo].second, sl = by_genome[hi - 1].second;
                    for (size_t k = lo; hi - lo > 1 && k < hi; ++k) {
                        const uint32_t b = by_genome[k].second;
                        if (b != sf) L.edges.push_back(EdgePair{g, sf, b});
                        if (b != sl) L.edges.push_back(EdgePair{g, sl, b});
                    }
                    lo = hi;
                }
            }
            return L.edges.size();
        }, L, msg);
}

}  // namespace

extern "C" {

// every table check, no device
int pep_group_verdicts_check(const uint8_t *h_packed, const uint64_t *h_row_off, const uint32_t *h_row_len, uint64_t n_rows, uint32_t n_groups, const uint64_t *h_grp_off,
                             const uint32_t *h_grp_rows, const uint32_t *h_grp_genome, const uint8_t *h_inparalog, const uint64_t *gd_key, const double *gd_val,
                             uint64_t n_gd, const double *gd_default, double self_id, char *msg, uint64_t msg_cap)
{
    Layout L;
    std::string text;
    const int rc = k16_check(GroupTables{h_packed, h_row_off, h_row_len, n_rows, n_groups, h_grp_off, h_grp_rows}, h_grp_genome, h_inparalog, gd_key, gd_val, n_gd, gd_default,
                             self_id, L, text);
    return pep_message_out(rc, text, msg, msg_cap);
}

int pep_group_verdicts(pep_ctx *ctx, const uint8_t *h_packed, const uint64_t *h_row_off, const uint32_t *h_row_len, uint64_t n_rows, uint32_t n_groups,
                       const uint64_t *h_grp_off, const uint32_t *h_grp_rows, const uint32_t *h_grp_genome, const uint8_t *h_inparalog, const uint64_t *gd_key,
                       const double *gd_val, uint64_t n_gd, const double *gd_default, double self_id, uint8_t *h_verdict, pep_verdict_result **detail)
{
    if (!ctx) return PEP_ERR_ARG;
    if (!detail || (n_groups && !h_verdict)) return pep_fail(ctx, PEP_ERR_ARG, "pep_group_verdicts: null table");
    *detail = nullptr;
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    CallTimes &times = ctx->calls[PEP_CALL_GROUP_VERDICTS];
    times = {};
    ++ctx->k16_serial;                                              // whatever an earlier result held on the device is about to be overwritten
    const GroupTables T{h_packed, h_row_off, h_row_len, n_rows, n_groups, h_grp_off, h_grp_rows};
    Layout L;
    std::string msg;
    const int rc = k16_check(T, h_grp_genome, h_inparalog, gd_key, gd_val, n_gd, gd_default, self_id, L, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    pep_verdict_result *res = new (std::nothrow) pep_verdict_result();
    if (!res) return pep_fail(ctx, PEP_ERR_INTERNAL, "pep_group_verdicts: out of memory");
    res->ctx = ctx;
    res->serial = ctx->k16_serial;
    res->verdict.assign(n_groups, 0);
    res->rows_off.resize(n_groups); res->tri_off.resize(n_groups); res->n.resize(n_groups);
    for (uint32_t g = 0; g < n_groups; ++g) { res->rows_off[g] = L.groups[g].rows_off; res->tri_off[g] = L.groups[g].tri_off; res->n[g] = L.groups[g].n; }
    *detail = res;
    if (n_groups == 0) return PEP_OK;
    const auto run = [&]() -> int {
        const uint64_t n_idx = h_grp_off[n_groups];
        static_assert(K16_WS_SLOTS <= PEP_WS_HITS_OUT, "leaves the device-resident hit table alone");
        DevBuf *W = ctx->ws;
        hipStream_t st = ctx->stream;
        std::vector<VGroup> dev_groups(n_groups);
        for (uint32_t g = 0; g < n_groups; ++g) dev_groups[g] = VGroup{L.groups[g].rows_off, L.groups[g].tri_off, L.groups[g].n, L.groups[g].words};
        PEP_TRY(dev_reserve(ctx, ctx->k16_tri, (L.pairs + 1) * 8));
        PEP_TRY(dev_reserve(ctx, ctx->k16_leader, (n_idx + 1) * 4));
        PEP_TRY(group_tables_to_device(ctx, T, L, dev_groups.data(), (size_t)n_groups * sizeof(VGroup),
                                       {{K16_WS_GENOME, h_grp_genome, n_idx * 4, 4}, {K16_WS_EDGES, L.edges.data(), L.edges.size() * sizeof(EdgePair), sizeof(EdgePair)},
                                        {K16_WS_GD_KEY, gd_key, n_gd * 8, 8}, {K16_WS_GD_VAL, L.gd.data(), L.gd.size() * 8, 0},
                                        {K16_WS_FLAGS, nullptr, (size_t)n_groups * 4, 0}, {K16_WS_VERDICT, nullptr, (size_t)n_groups, 0}, {K16_WS_SPILL, nullptr, (n_idx + 1) * 4, 0}},
                                       times.ms[0]));
        PEP_HIP(ctx, hipMemsetAsync(W[K16_WS_FLAGS].p, 0, (size_t)n_groups * 4, st));
        const GdTable gd{W[K16_WS_GD_KEY].as<const uint64_t>(), W[K16_WS_GD_VAL].as<const double>(), n_gd, self_id};
        const VGroup *d_groups = W[K15_WS_GROUPS].as<const VGroup>();
        const uint32_t *d_grp_rows = W[K15_WS_GRP_ROWS].as<const uint32_t>(), *d_genome = W[K16_WS_GENOME].as<const uint32_t>();
        const uint64_t *d_plane_off = W[K15_WS_PLANE_OFF].as<const uint64_t>();
        const unsigned long long *d_planes = W[K15_WS_PLANES].as<const unsigned long long>();
        uint32_t *d_flags = W[K16_WS_FLAGS].as<uint32_t>();
        if (!L.edges.empty())
            pep_timed_stage(ctx, times.ms[1], [&] {
                hipLaunchKernelGGL(verdict_edge, dim3((unsigned)ceil_div(L.edges.size(), 4 * K16_EDGE_PER_WAVE)), dim3(256), 0, st, (uint64_t)L.edges.size(),
                                   W[K16_WS_EDGES].as<const EdgePair>(), d_groups, d_grp_rows, d_genome, d_plane_off, d_planes, gd, d_flags);
            });
        if (!L.tiles.empty())
            pep_timed_stage(ctx, times.ms[2], [&] {
                hipLaunchKernelGGL(verdict_pairs, dim3((unsigned)L.tiles.size()), dim3(256), 0, st, W[K15_WS_TILES].as<const DiffTile>(), d_groups, d_grp_rows, d_genome,
                                   d_plane_off, d_planes, gd, d_flags, ctx->k16_tri.as<int2>());
            });
        pep_timed_stage(ctx, times.ms[3], [&] {
            hipLaunchKernelGGL(verdict_leaders, dim3(n_groups), dim3(256), 0, st, d_groups, (const uint32_t *)d_flags, ctx->k16_tri.as<const int2>(),
                               ctx->k16_leader.as<uint32_t>(), W[K16_WS_SPILL].as<uint32_t>(), W[K16_WS_VERDICT].as<uint8_t>());
        });
        PEP_TRY(pep_d2h_queue(ctx, res->verdict.data(), W[K16_WS_VERDICT].p, n_groups));
        times.bytes_to_host = (uint64_t)n_groups + 4;
        return group_tables_finish(ctx, K16_SPEC);
    };
    const int rc2 = run();
    if (rc2 != PEP_OK) {
        delete res;
        *detail = nullptr;
        return rc2;
    }
    memcpy(h_verdict, res->verdict.data(), n_groups);
    return PEP_OK;
}

int pep_verdict_detail_size(const pep_verdict_result *res, uint32_t g, uint64_t *n_pairs)
{
    if (!res || !n_pairs) return PEP_ERR_ARG;
    if (g >= res->verdict.size()) return PEP_ERR_ARG;
    const uint64_t n = res->n[g];
    *n_pairs = res->verdict[g] == 2 ? n * (n - 1) / 2 : 0;
    return PEP_OK;
}

int pep_verdict_detail_copy(pep_verdict_result *res, uint32_t g, int32_t *h_tri, uint32_t *h_leader)
{
    if (!res) return PEP_ERR_ARG;
    pep_ctx *ctx = res->ctx;
    if (g >= res->verdict.size()) return pep_fail(ctx, PEP_ERR_ARG, "pep_verdict_detail_copy: no such group");
    if (res->serial != ctx->k16_serial) return pep_fail(ctx, PEP_ERR_STATE, "pep_verdict_detail_copy: a newer pep_group_verdicts of this context has replaced the device data of this result");
    if (res->verdict[g] != 2) return PEP_OK;
    const uint64_t n = res->n[g], pairs = n * (n - 1) / 2;
    if (h_tri) PEP_TRY(pep_d2h_queue(ctx, h_tri, ctx->k16_tri.as<const int2>() + res->tri_off[g], pairs * 8));
    if (h_leader) PEP_TRY(pep_d2h_queue(ctx, h_leader, ctx->k16_leader.as<const uint32_t>() + res->rows_off[g], n * 4));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    ctx->calls[PEP_CALL_GROUP_VERDICTS].bytes_to_host += (h_tri ? pairs * 8 : 0) + (h_leader ? n * 4 : 0);
    return PEP_OK;
}

void pep_verdict_result_free(pep_verdict_result *res) { delete res; }

}  // extern "C"
