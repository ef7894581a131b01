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
#include "common.h"
#include "allelediff_tile.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <optional>

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

struct VGroup {
    uint64_t rows_off;              // first entry of the group in grp_rows / grp_genome / leader
    uint64_t tri_off;               // first int32 pair of the group's packed triangle
    uint32_t n, words;
};
struct EdgePair { uint32_t g, a, b; };      // rows a, b (positions inside group g)
struct GdTable {
    const uint64_t *key;            // [n] sorted
    const double *val;              // [n + 1][3]: gd0, denX, den; row n = the default
    uint64_t n;
    double self_id;
};

__device__ __forceinline__ void k16_gd(const GdTable &T, uint32_t ga, uint32_t gb, double aln, double &gd0, double &denX, double &den)
{
    if (ga == gb) {
        gd0 = fmax(T.self_id, __ddiv_rn(2.0, aln));
        denX = den = gd0;                               // gd0 * exp(0 * x) == gd0
        return;
    }
    const uint64_t key = ga < gb ? ((uint64_t)ga << 32 | gb) : ((uint64_t)gb << 32 | ga);
    uint64_t lo = 0, hi = T.n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (T.key[mid] < key) lo = mid + 1; else hi = mid;
    }
    const uint64_t row = (lo < T.n && T.key[lo] == key) ? lo : T.n;
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

struct Layout {
    std::vector<uint64_t> plane_off;
    std::vector<VGroup> groups;
    std::vector<DiffTile> tiles;
    std::vector<EdgePair> edges;
    std::vector<double> gd;         // [n_gd + 1][3]
    uint64_t pairs = 0;
};

bool k16_good(double v) { return std::isfinite(v) && v > 0.; }

// every check of the tables, on the host, before anything is launched; also lays the device buffers out
int k16_check(const uint8_t *h_packed, const uint64_t *h_row_off, const uint32_t *h_row_len, uint64_t n_rows, uint32_t n_groups, const uint64_t *h_grp_off,
              const uint32_t *h_grp_rows, const uint32_t *h_grp_genome, const uint8_t *h_inparalog, const uint64_t *gd_key, const double *gd_val, uint64_t n_gd,
              const double *gd_default, double self_id, Layout &L, std::string &msg)
{
    const std::string me = "pep_group_verdicts: ";
    const auto bad = [&](int code, const std::string &text) { msg = me + text; return code; };
    if (!h_row_off || (n_rows && !h_row_len) || (n_groups && (!h_grp_off || !h_inparalog)) || (n_gd && (!gd_key || !gd_val)) || !gd_default) return bad(PEP_ERR_ARG, "null table");
    if (n_groups && h_grp_off[n_groups] && (!h_grp_rows || !h_grp_genome)) return bad(PEP_ERR_ARG, "null table");
    if (n_rows && h_row_off[n_rows] && !h_packed) return bad(PEP_ERR_ARG, "null table");
    if (!k16_good(self_id)) return bad(PEP_ERR_ARG, "self_id must be finite and > 0");
    for (uint64_t i = 0; i < n_gd; ++i) {
        if ((gd_key[i] >> 32) > (gd_key[i] & 0xFFFFFFFFull)) return bad(PEP_ERR_ARG, "gd_key " + std::to_string(i) + " has g1 > g2");
        if (i && gd_key[i] <= gd_key[i - 1]) return bad(PEP_ERR_ARG, "gd_key must be strictly increasing (entry " + std::to_string(i) + ")");
    }
    for (uint64_t i = 0; i <= n_gd; ++i) {
        const double *v = i < n_gd ? gd_val + 3 * i : gd_default;
        if (!k16_good(v[0]) || !k16_good(v[1]) || !k16_good(v[2]))
            return bad(PEP_ERR_ARG, (i < n_gd ? "gd_val row " + std::to_string(i) : std::string("gd_default")) + " must be finite and > 0 in all three columns");
    }
    L.gd.assign(gd_val, gd_val + 3 * n_gd);
    L.gd.insert(L.gd.end(), gd_default, gd_default + 3);
    if (n_rows >= 0xFFFFFFFFull) return bad(PEP_ERR_LIMIT, "more than 2^32 - 2 rows");
    L.plane_off.assign(n_rows + 1, 0);
    for (uint64_t r = 0; r < n_rows; ++r) {
        const uint64_t s = ((uint64_t)h_row_len[r] + 2) / 3;
        if (h_row_off[r + 1] < h_row_off[r] || h_row_off[r + 1] - h_row_off[r] != s)
            return bad(PEP_ERR_ARG, "row " + std::to_string(r) + " does not hold ceil(row_len / 3) bytes");
        L.plane_off[r + 1] = L.plane_off[r] + 3 * ((3 * s + 63) / 64);
    }
    if (n_groups && h_grp_off[0] != 0) return bad(PEP_ERR_ARG, "grp_off must start at 0");
    L.groups.resize(n_groups);
    std::vector<std::pair<uint32_t, uint32_t>> by_genome;
    for (uint32_t g = 0; g < n_groups; ++g) {
        if (h_grp_off[g + 1] < h_grp_off[g]) return bad(PEP_ERR_ARG, "grp_off must be non-decreasing");
        const uint64_t n = h_grp_off[g + 1] - h_grp_off[g];
        if (n >= 0x7FFFFFFFull) return bad(PEP_ERR_LIMIT, "more than 2^31 - 2 rows in one group");
        if (h_inparalog[g] > 1) return bad(PEP_ERR_ARG, "grp_inparalog of group " + std::to_string(g) + " is neither 0 nor 1");
        VGroup &G = L.groups[g];
        G.rows_off = h_grp_off[g]; G.n = (uint32_t)n; G.words = 0; G.tri_off = L.pairs;
        for (uint64_t k = h_grp_off[g]; k < h_grp_off[g + 1]; ++k) {
            const uint32_t r = h_grp_rows[k];
            if (r >= n_rows) return bad(PEP_ERR_ARG, "row index " + std::to_string(r) + " of group " + std::to_string(g) + " out of range");
            if (h_row_len[r] != h_row_len[h_grp_rows[h_grp_off[g]]]) return bad(PEP_ERR_ARG, "group " + std::to_string(g) + " mixes rows of different row_len");
        }
        if (n < 2) continue;
        const uint32_t r0 = h_grp_rows[h_grp_off[g]];
        G.words = (uint32_t)((L.plane_off[r0 + 1] - L.plane_off[r0]) / 3);
        L.pairs += n * (n - 1) / 2;
        if (L.pairs * 8 > PEP_ALLELE_DIFF_MAX_BYTES)
            return bad(PEP_ERR_LIMIT, std::to_string(L.pairs * 8) + " bytes of triangles asked for, the device budget of one call is " +
                                          std::to_string((uint64_t)PEP_ALLELE_DIFF_MAX_BYTES) + " (reached at group " + std::to_string(g) + ": split the batch)");
        const uint64_t nt = (n + K15_TILE - 1) / K15_TILE;
        for (uint64_t ti = 0; ti < nt; ++ti)
            for (uint64_t tj = ti; tj < nt; ++tj) L.tiles.push_back(DiffTile{g, (uint32_t)ti, (uint32_t)tj, 0u});
        const uint32_t last = (uint32_t)n - 1;
        for (uint32_t b = 0; b <= last; ++b) {
            if (b != 0) L.edges.push_back(EdgePair{g, 0u, b});
            if (b != last) L.edges.push_back(EdgePair{g, last, b});
        }
        if (h_inparalog[g]) {                                       // the first and the last row of every genome's sub-group against its rows (:352-366)
            by_genome.clear();
            for (uint32_t k = 0; k <= last; ++k) by_genome.emplace_back(h_grp_genome[h_grp_off[g] + k], k);
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
    }
    if (L.tiles.size() > 0x7FFFFFFFull || L.edges.size() > 0x7FFFFFFFull) return bad(PEP_ERR_LIMIT, "more than 2^31 - 1 tiles or edge pairs in one call (split the batch)");
    if (L.plane_off[n_rows] * 8 > PEP_ALLELE_DIFF_MAX_BYTES)
        return bad(PEP_ERR_LIMIT, std::to_string(L.plane_off[n_rows] * 8) + " bytes of bit planes asked for, the device budget of one call is " +
                                      std::to_string((uint64_t)PEP_ALLELE_DIFF_MAX_BYTES) + " (split the batch)");
    return PEP_OK;
}

}  // namespace

int pep_k16_check(const uint8_t *h_packed, const uint64_t *h_row_off, const uint32_t *h_row_len, uint64_t n_rows, uint32_t n_groups, const uint64_t *h_grp_off,
                  const uint32_t *h_grp_rows, const uint32_t *h_grp_genome, const uint8_t *h_inparalog, const uint64_t *gd_key, const double *gd_val, uint64_t n_gd,
                  const double *gd_default, double self_id, std::string &msg)
{
    Layout L;
    return k16_check(h_packed, h_row_off, h_row_len, n_rows, n_groups, h_grp_off, h_grp_rows, h_grp_genome, h_inparalog, gd_key, gd_val, n_gd, gd_default, self_id, L, msg);
}

int pep_k16_group_verdicts(pep_ctx *ctx, const uint8_t *h_packed, const uint64_t *h_row_off, const uint32_t *h_row_len, uint64_t n_rows, uint32_t n_groups,
                           const uint64_t *h_grp_off, const uint32_t *h_grp_rows, const uint32_t *h_grp_genome, const uint8_t *h_inparalog, const uint64_t *gd_key,
                           const double *gd_val, uint64_t n_gd, const double *gd_default, double self_id, uint8_t *h_verdict, pep_verdict_result **detail)
{
    for (double &ms : ctx->k16_ms) ms = 0.;
    ctx->k16_bytes_to_host = 0;
    ++ctx->k16_serial;                                              // whatever an earlier result held on the device is about to be overwritten
    Layout L;
    std::string msg;
    const int rc = k16_check(h_packed, h_row_off, h_row_len, n_rows, n_groups, h_grp_off, h_grp_rows, h_grp_genome, h_inparalog, gd_key, gd_val, n_gd, gd_default, self_id, L, msg);
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
        const uint64_t n_idx = h_grp_off[n_groups], n_bytes = h_row_off[n_rows];
        DevBuf *W = ctx->ws;
        hipStream_t st = ctx->stream;
        PEP_TRY(dev_reserve(ctx, W[0], n_bytes + 1));
        PEP_TRY(dev_reserve(ctx, W[1], (n_rows + 1) * 8));
        PEP_TRY(dev_reserve(ctx, W[2], (n_rows + 1) * 4));
        PEP_TRY(dev_reserve(ctx, W[3], (n_rows + 1) * 8));
        PEP_TRY(dev_reserve(ctx, W[4], (L.plane_off[n_rows] + 1) * 8));
        PEP_TRY(dev_reserve(ctx, W[5], (n_idx + 1) * 4));
        PEP_TRY(dev_reserve(ctx, W[6], (size_t)n_groups * sizeof(VGroup)));
        PEP_TRY(dev_reserve(ctx, W[7], (L.tiles.size() + 1) * sizeof(DiffTile)));
        PEP_TRY(dev_reserve(ctx, W[9], 256));
        PEP_TRY(dev_reserve(ctx, W[10], (n_idx + 1) * 4));
        PEP_TRY(dev_reserve(ctx, W[11], (L.edges.size() + 1) * sizeof(EdgePair)));
        PEP_TRY(dev_reserve(ctx, W[12], (n_gd + 1) * 8));
        PEP_TRY(dev_reserve(ctx, W[13], L.gd.size() * 8));
        PEP_TRY(dev_reserve(ctx, W[14], (size_t)n_groups * 4));
        PEP_TRY(dev_reserve(ctx, W[15], (size_t)n_groups));
        PEP_TRY(dev_reserve(ctx, W[16], (n_idx + 1) * 4));
        PEP_TRY(dev_reserve(ctx, ctx->k16_tri, (L.pairs + 1) * 8));
        PEP_TRY(dev_reserve(ctx, ctx->k16_leader, (n_idx + 1) * 4));
        PEP_TRY(pep_h2d(ctx, W[0].p, h_packed, n_bytes));
        PEP_TRY(pep_h2d(ctx, W[1].p, h_row_off, (n_rows + 1) * 8));
        PEP_TRY(pep_h2d(ctx, W[2].p, h_row_len, n_rows * 4));
        PEP_TRY(pep_h2d(ctx, W[3].p, L.plane_off.data(), (n_rows + 1) * 8));
        PEP_TRY(pep_h2d(ctx, W[5].p, h_grp_rows, n_idx * 4));
        PEP_TRY(pep_h2d(ctx, W[6].p, L.groups.data(), (size_t)n_groups * sizeof(VGroup)));
        PEP_TRY(pep_h2d(ctx, W[7].p, L.tiles.data(), L.tiles.size() * sizeof(DiffTile)));
        PEP_TRY(pep_h2d(ctx, W[10].p, h_grp_genome, n_idx * 4));
        PEP_TRY(pep_h2d(ctx, W[11].p, L.edges.data(), L.edges.size() * sizeof(EdgePair)));
        PEP_TRY(pep_h2d(ctx, W[12].p, gd_key, n_gd * 8));
        PEP_TRY(pep_h2d(ctx, W[13].p, L.gd.data(), L.gd.size() * 8));
        PEP_HIP(ctx, hipMemsetAsync(W[9].p, 0xFF, 4, st));
        PEP_HIP(ctx, hipMemsetAsync(W[14].p, 0, (size_t)n_groups * 4, st));
        const GdTable gd{W[12].as<const uint64_t>(), W[13].as<const double>(), n_gd, self_id};
        const bool timed = ctx->timing_level >= 2;
        const auto stage = [&](int which, const auto &launch) {
            std::optional<EventTimer> tm;
            if (timed) tm.emplace(st);
            launch();
            if (timed) ctx->k16_ms[which] = tm->stop();
        };
        if (n_rows)
            stage(0, [&] { pep_k15_queue_planes(st, n_rows, W[0].as<const uint8_t>(), W[1].as<const uint64_t>(), W[2].as<const uint32_t>(), W[3].as<const uint64_t>(),
                                                W[4].as<unsigned long long>(), W[9].as<uint32_t>()); });
        if (!L.edges.empty())
            stage(1, [&] { hipLaunchKernelGGL(verdict_edge, dim3((unsigned)ceil_div(L.edges.size(), 4 * K16_EDGE_PER_WAVE)), dim3(256), 0, st, (uint64_t)L.edges.size(),
                                              W[11].as<const EdgePair>(), W[6].as<const VGroup>(), W[5].as<const uint32_t>(), W[10].as<const uint32_t>(),
                                              W[3].as<const uint64_t>(), W[4].as<const unsigned long long>(), gd, W[14].as<uint32_t>()); });
        if (!L.tiles.empty())
            stage(2, [&] { hipLaunchKernelGGL(verdict_pairs, dim3((unsigned)L.tiles.size()), dim3(256), 0, st, W[7].as<const DiffTile>(), W[6].as<const VGroup>(),
                                              W[5].as<const uint32_t>(), W[10].as<const uint32_t>(), W[3].as<const uint64_t>(), W[4].as<const unsigned long long>(), gd,
                                              W[14].as<uint32_t>(), ctx->k16_tri.as<int2>()); });
        stage(3, [&] { hipLaunchKernelGGL(verdict_leaders, dim3(n_groups), dim3(256), 0, st, W[6].as<const VGroup>(), W[14].as<const uint32_t>(),
                                          ctx->k16_tri.as<const int2>(), ctx->k16_leader.as<uint32_t>(), W[16].as<uint32_t>(), W[15].as<uint8_t>()); });
        PEP_HIP(ctx, hipGetLastError());
        uint32_t bad_row = 0xFFFFFFFFu;
        PEP_TRY(pep_d2h_queue(ctx, &bad_row, W[9].p, 4));
        PEP_TRY(pep_d2h_queue(ctx, res->verdict.data(), W[15].p, n_groups));
        PEP_HIP(ctx, pep_stream_wait(ctx));
        pep_d2h_finish(ctx);
        ctx->k16_bytes_to_host = (uint64_t)n_groups + 4;
        if (bad_row != 0xFFFFFFFFu)
            return pep_fail(ctx, PEP_ERR_ARG, "pep_group_verdicts: row " + std::to_string(bad_row) + " holds a byte above 124 (not three base-5 digits)");
        return PEP_OK;
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

int pep_k16_detail_size(const pep_verdict_result *res, uint32_t g, uint64_t *n_pairs)
{
    if (g >= res->verdict.size()) return PEP_ERR_ARG;
    const uint64_t n = res->n[g];
    *n_pairs = res->verdict[g] == 2 ? n * (n - 1) / 2 : 0;
    return PEP_OK;
}

int pep_k16_detail_copy(pep_verdict_result *res, uint32_t g, int32_t *h_tri, uint32_t *h_leader)
{
    pep_ctx *ctx = res->ctx;
    if (g >= res->verdict.size()) return pep_fail(ctx, PEP_ERR_ARG, "pep_verdict_detail_copy: no such group");
    if (res->serial != ctx->k16_serial) return pep_fail(ctx, PEP_ERR_STATE, "pep_verdict_detail_copy: a newer pep_group_verdicts of this context has replaced the device data of this result");
    if (res->verdict[g] != 2) return PEP_OK;
    const uint64_t n = res->n[g], pairs = n * (n - 1) / 2;
    if (h_tri) PEP_TRY(pep_d2h_queue(ctx, h_tri, ctx->k16_tri.as<const int2>() + res->tri_off[g], pairs * 8));
    if (h_leader) PEP_TRY(pep_d2h_queue(ctx, h_leader, ctx->k16_leader.as<const uint32_t>() + res->rows_off[g], n * 4));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    ctx->k16_bytes_to_host += (h_tri ? pairs * 8 : 0) + (h_leader ? n * 4 : 0);
    return PEP_OK;
}

void pep_k16_result_free(pep_verdict_result *res) { delete res; }
