// K20: the two counting loops of PEPPAN_parser - writeCurve (PEPPAN_parser.py:63-115, its loop :74-80) and getDistance (:172-179, behind writeCGAV).
// Both are integer and data-parallel; the floats made of their counts (curve fits, -log) stay on the host (peppan_amd/panparser.py).
//   rarefaction      the reference adds every genome of a shuffled order to a per-gene counter and sums `genes >= 1` and `genes >= k + 1` over all genes after each,
//                    n_iter x n_genomes times.  Restated over bit rows (include/peppan_hip.h, K20): pan = popcount of the running OR, core = popcount of the running
//                    AND, which starts from the valid-bit mask so that padding never counts.  One workgroup per order.  A slice is 1 024 words (65 536 genes):
//                    every lane keeps the running OR and AND of its four words in registers across the walk, loads its words of row order[k] (consecutive lanes,
//                    consecutive words; the next row is on its way while this one is judged) and forms two deltas - newly in pan, newly out of core.  A ballot that
//                    finds both zero in the whole wavefront skips the rest, late in a walk the normal case; else the deltas are summed over the wavefront and
//                    lane 0 adds them to the step's entry of an LDS array.  After 2 048 steps the workgroup scans that array and stores its own
//                    curves[k][order][:] - nobody else's, so no global atomics, no waiting between workgroups.  More genes: the walk is repeated per slice and the
//                    counts added to what the same thread stored before.  More genomes: more chunks of 2 048 steps.
//   profile_pairs    one workgroup per 64 x 64 tile of pairs, the geometry of K15's tile (allelediff_tile.h: K15_TILE, thread (tx, ty) owns rows ty * 4 + i against
//                    rows tx + 16 j).  K15's bit planes do not fit here - an allele number is any int32, equality over planes would need 32 of them - so the two row
//                    panels are staged as int32, 16 genes per step, A rows recoded absent -> 0 and B rows absent -> -1: shared += (a == b), presence += (min(a, b) > 0).
// Integers only, plain vector stores.  The walk is bound by the latency of one row load per step (the matrix is cache-resident), the pairs by VALU.
#include "common.h"
#include "allelediff_tile.h"
#include <algorithm>

namespace {

// the slots of pep_ctx::k20
enum { K20_BITS = 0, K20_ORDERS, K20_CURVES, K20_PROFILES, K20_SHARED, K20_PRESENCE, K20_SLOTS };
static_assert(K20_SLOTS == sizeof(pep_ctx::k20) / sizeof(DevBuf), "one member of pep_ctx::k20 per slot");

constexpr int K20_BLOCK = 256;
constexpr int K20_WPL = 4;                                  // words of a row per lane and slice
constexpr uint32_t K20_SLICE = K20_BLOCK * K20_WPL;         // words per slice
constexpr uint32_t K20_STEPS = 2048;                        // steps of a walk per LDS chunk
constexpr uint32_t K20_SPT = K20_STEPS / K20_BLOCK;         // steps per thread in the scan
constexpr int K20_KG = 16;                                  // genes of every profile staged per step

__device__ __forceinline__ void k20_load(unsigned long long (&v)[K20_WPL], const unsigned long long *__restrict__ row, uint64_t w_first, uint64_t W)
{
#pragma unroll
    for (int i = 0; i < K20_WPL; ++i) {
        const uint64_t w = w_first + (uint64_t)i * K20_BLOCK;
        v[i] = w < W ? row[w] : 0ull;
    }
}

__global__ __launch_bounds__(K20_BLOCK) void rarefaction(const unsigned long long *__restrict__ bits, uint32_t n, uint64_t n_genes, uint64_t W,
                                                         const uint32_t *__restrict__ orders, uint32_t n_iter, int2 *__restrict__ curves)
{
    __shared__ uint32_t s_new[K20_STEPS], s_lost[K20_STEPS];
    __shared__ uint2 s_scan[K20_BLOCK];
    const uint32_t tid = threadIdx.x, lane = tid & 63, ite = blockIdx.x;
    const uint32_t *order = orders + (uint64_t)ite * n;
    for (uint64_t w0 = 0; w0 < W; w0 += K20_SLICE) {
        const uint32_t slice_genes = (uint32_t)min(n_genes - 64 * w0, (uint64_t)64 * K20_SLICE);
        const uint64_t w_first = w0 + tid;
        unsigned long long acc_or[K20_WPL], acc_and[K20_WPL];
#pragma unroll
        for (int i = 0; i < K20_WPL; ++i) {                                  // the AND starts from the genes that exist
            const uint64_t first_gene = 64 * (w_first + (uint64_t)i * K20_BLOCK);
            acc_or[i] = 0ull;
            acc_and[i] = first_gene >= n_genes ? 0ull : n_genes - first_gene >= 64 ? ~0ull : (1ull << (n_genes - first_gene)) - 1ull;
        }
        uint32_t pan = 0, lost = 0;                                          // of this slice, up to the chunk
        for (uint32_t k0 = 0; k0 < n; k0 += K20_STEPS) {
            const uint32_t steps = min(K20_STEPS, n - k0);
            for (uint32_t e = tid; e < K20_STEPS; e += K20_BLOCK) s_new[e] = s_lost[e] = 0;
            __syncthreads();
            unsigned long long cur[K20_WPL], nxt[K20_WPL] = {};
            k20_load(cur, bits + (uint64_t)order[k0] * W, w_first, W);
            for (uint32_t s = 0; s < steps; ++s) {
                if (s + 1 < steps) k20_load(nxt, bits + (uint64_t)order[k0 + s + 1] * W, w_first, W);
                uint32_t d = 0, l = 0;
#pragma unroll
                for (int i = 0; i < K20_WPL; ++i) {
                    d += (uint32_t)__popcll(cur[i] & ~acc_or[i]);
                    l += (uint32_t)__popcll(acc_and[i] & ~cur[i]);
                    acc_or[i] |= cur[i];
                    acc_and[i] &= cur[i];
                }
                uint32_t both = d | (l << 16);                               // at most 256 each per lane, 16 384 per wavefront
                if (__ballot(both != 0)) {
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) both += __shfl_xor(both, off, 64);
                    if (lane == 0) {
                        if (both & 0xFFFFu) atomicAdd(&s_new[s], both & 0xFFFFu);
                        if (both >> 16) atomicAdd(&s_lost[s], both >> 16);
                    }
                }
#pragma unroll
                for (int i = 0; i < K20_WPL; ++i) cur[i] = nxt[i];
            }
            __syncthreads();
            // inclusive scan of the chunk: every thread its K20_SPT consecutive steps, then the threads' sums
            uint2 own = make_uint2(0, 0);
#pragma unroll
            for (uint32_t j = 0; j < K20_SPT; ++j) { own.x += s_new[tid * K20_SPT + j]; own.y += s_lost[tid * K20_SPT + j]; }
            s_scan[tid] = own;
            for (uint32_t off = 1; off < K20_BLOCK; off <<= 1) {
                __syncthreads();
                const uint2 below = tid >= off ? s_scan[tid - off] : make_uint2(0, 0);
                __syncthreads();
                s_scan[tid].x += below.x;
                s_scan[tid].y += below.y;
            }
            __syncthreads();
            uint32_t run_pan = pan + s_scan[tid].x - own.x, run_lost = lost + s_scan[tid].y - own.y;
#pragma unroll
            for (uint32_t j = 0; j < K20_SPT; ++j) {
                const uint32_t s = tid * K20_SPT + j;
                if (s >= steps) break;
                run_pan += s_new[s];
                run_lost += s_lost[s];
                const uint64_t at = (uint64_t)(k0 + s) * n_iter + ite;
                int2 v = make_int2((int)run_pan, (int)(slice_genes - run_lost));
                if (w0) { const int2 before = curves[at]; v.x += before.x; v.y += before.y; }      // (stored by this thread in the slice before)
                curves[at] = v;
            }
            pan += s_scan[K20_BLOCK - 1].x;
            lost += s_scan[K20_BLOCK - 1].y;
            __syncthreads();                                                 // the arrays are read: the next chunk clears them
        }
    }
}

__global__ __launch_bounds__(256) void profile_pairs(const int32_t *__restrict__ prof, uint32_t n, uint64_t G, int32_t *__restrict__ shared, int32_t *__restrict__ presence)
{
    const uint32_t ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;                                                     // (uniform over the workgroup)
    // [gene][row], a row longer than the tile: the 16 genes of a row are written by 16 consecutive threads into 16 banks
    __shared__ int32_t sA[K20_KG][K15_TILE + 1], sB[K20_KG][K15_TILE + 1];
    const uint32_t tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    uint32_t sh[4][4], pr[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) sh[i][j] = pr[i][j] = 0;
    for (uint64_t g0 = 0; g0 < G; g0 += K20_KG) {
        __syncthreads();                                                     // the previous step's genes are consumed
        for (uint32_t e = tid; e < 2 * K15_TILE * K20_KG; e += 256) {
            const uint32_t panel = e / (K15_TILE * K20_KG), rem = e % (K15_TILE * K20_KG), row = rem / K20_KG, col = rem % K20_KG;
            const uint64_t r = (uint64_t)(panel ? tj : ti) * K15_TILE + row, g = g0 + col;
            const int32_t v = (r < n && g < G) ? prof[r * G + g] : 0;
            if (panel) sB[col][row] = v > 0 ? v : -1; else sA[col][row] = v > 0 ? v : 0;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < K20_KG; ++k) {
            int32_t av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { av[i] = sA[k][ty * 4 + i]; bv[i] = sB[k][tx + 16 * i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    sh[i][j] += av[i] == bv[j] ? 1u : 0u;
                    pr[i][j] += min(av[i], bv[j]) > 0 ? 1u : 0u;
                }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t a = (uint64_t)ti * K15_TILE + ty * 4 + i, b = (uint64_t)tj * K15_TILE + tx + 16 * j;
            if (a < b && b < n) {
                shared[a * n + b] = (int32_t)sh[i][j];
                presence[a * n + b] = (int32_t)pr[i][j];
            }
        }
}

const char *const K20_CURVES_ME = "pep_rarefaction_curves: ";
const char *const K20_PAIRS_ME = "pep_profile_pairs: ";

// every check of the curve tables, on the host, before anything is launched
int k20_curves_check(const uint64_t *bits, uint32_t n, uint64_t n_genes, const uint32_t *orders, uint32_t n_iter, std::string &msg)
{
    const auto bad = [&](int code, const std::string &text) { msg = K20_CURVES_ME + text; return code; };
    if (n == 0 || n_genes == 0 || n_iter == 0) return bad(PEP_ERR_ARG, "n_genomes, n_genes and n_iter must be positive");
    if (!bits || !orders) return bad(PEP_ERR_ARG, "null table");
    if (n_genes >= PEP_PARSER_MAX_GENES) return bad(PEP_ERR_LIMIT, "2^31 genes or more");
    if ((uint64_t)n * n_iter >= PEP_PARSER_MAX_CURVE_POINTS) return bad(PEP_ERR_LIMIT, "n_genomes * n_iter is 2^28 or more");
    const uint64_t W = (n_genes + 63) / 64;
    if (n_genes % 64) {
        const uint64_t padding = ~0ull << (n_genes % 64);
        for (uint32_t g = 0; g < n; ++g)
            if (bits[(uint64_t)g * W + W - 1] & padding) return bad(PEP_ERR_ARG, "genome " + std::to_string(g) + " has a padding bit set");
    }
    std::vector<uint32_t> seen(n, 0u);                                       // the row + 1 that named the genome last
    for (uint32_t t = 0; t < n_iter; ++t)
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t g = orders[(uint64_t)t * n + k];
            if (g >= n) return bad(PEP_ERR_ARG, "entry " + std::to_string(k) + " of order " + std::to_string(t) + " names genome " + std::to_string(g) + " of " + std::to_string(n));
            if (seen[g] == t + 1) return bad(PEP_ERR_ARG, "entry " + std::to_string(k) + " of order " + std::to_string(t) + " names genome " + std::to_string(g) + " again");
            seen[g] = t + 1;
        }
    return PEP_OK;
}

int k20_pairs_check(uint32_t n, uint64_t n_genes, std::string &msg)
{
    const auto bad = [&](int code, const std::string &text) { msg = K20_PAIRS_ME + text; return code; };
    if (n == 0 || n_genes == 0) return bad(PEP_ERR_ARG, "n and n_genes must be positive");
    if (n > PEP_PARSER_MAX_PROFILES) return bad(PEP_ERR_LIMIT, "more than " + std::to_string(PEP_PARSER_MAX_PROFILES) + " profiles");
    if (n_genes >= PEP_PARSER_MAX_GENES) return bad(PEP_ERR_LIMIT, "2^31 genes or more");
    return PEP_OK;
}

}  // namespace

extern "C" {

int pep_rarefaction_curves_check(const uint64_t *bits, uint32_t n_genomes, uint64_t n_genes, const uint32_t *orders, uint32_t n_iter, char *msg, uint64_t msg_cap)
{
    std::string text;
    const int rc = k20_curves_check(bits, n_genomes, n_genes, orders, n_iter, text);
    return pep_message_out(rc, text, msg, msg_cap);
}

int pep_rarefaction_curves(pep_ctx *ctx, const uint64_t *bits, uint32_t n_genomes, uint64_t n_genes, const uint32_t *orders, uint32_t n_iter, int32_t *curves)
{
    if (!ctx) return PEP_ERR_ARG;
    if (!curves) return pep_fail(ctx, PEP_ERR_ARG, std::string(K20_CURVES_ME) + "null table");
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    CallTimes &times = ctx->calls[PEP_CALL_PARSER];                  // shared with pep_profile_pairs: slot 0 is this call's, the byte counts the newer call's
    times.ms[0] = 0.;
    times.bytes_to_device = times.bytes_to_host = 0;
    std::string msg;
    const int rc = k20_curves_check(bits, n_genomes, n_genes, orders, n_iter, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    const uint64_t W = (n_genes + 63) / 64;
    const size_t bits_bytes = (size_t)n_genomes * W * 8, order_bytes = (size_t)n_genomes * n_iter * 4, curve_bytes = (size_t)n_genomes * n_iter * 8;
    DevBuf *B = ctx->k20;
    PEP_TRY(pep_tables_to_device(ctx, B, {{K20_BITS, bits, bits_bytes, 0}, {K20_ORDERS, orders, order_bytes, 0}, {K20_CURVES, nullptr, curve_bytes, 0}}));
    pep_timed_stage(ctx, times.ms[0], [&] {
        hipLaunchKernelGGL(rarefaction, dim3(n_iter), dim3(K20_BLOCK), 0, ctx->stream, B[K20_BITS].as<const unsigned long long>(), n_genomes, n_genes, W,
                           B[K20_ORDERS].as<const uint32_t>(), n_iter, B[K20_CURVES].as<int2>());
    });
    PEP_HIP(ctx, hipGetLastError());
    PEP_TRY(pep_d2h_queue(ctx, curves, B[K20_CURVES].p, curve_bytes));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    times.bytes_to_device = bits_bytes + order_bytes;
    times.bytes_to_host = curve_bytes;
    return PEP_OK;
}

int pep_profile_pairs_check(uint32_t n, uint64_t n_genes, char *msg, uint64_t msg_cap)
{
    std::string text;
    const int rc = k20_pairs_check(n, n_genes, text);
    return pep_message_out(rc, text, msg, msg_cap);
}

int pep_profile_pairs(pep_ctx *ctx, const int32_t *profiles, uint32_t n, uint64_t n_genes, int32_t *shared, int32_t *presence)
{
    if (!ctx) return PEP_ERR_ARG;
    if (!profiles || !shared || !presence) return pep_fail(ctx, PEP_ERR_ARG, std::string(K20_PAIRS_ME) + "null table");
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    CallTimes &times = ctx->calls[PEP_CALL_PARSER];                  // shared with pep_rarefaction_curves: slot 1 is this call's, the byte counts the newer call's
    times.ms[1] = 0.;
    times.bytes_to_device = times.bytes_to_host = 0;
    std::string msg;
    const int rc = k20_pairs_check(n, n_genes, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    const size_t prof_bytes = (size_t)n * n_genes * 4, out_bytes = (size_t)n * n * 4;
    DevBuf *B = ctx->k20;
    PEP_TRY(pep_tables_to_device(ctx, B, {{K20_PROFILES, profiles, prof_bytes, 0}, {K20_SHARED, nullptr, out_bytes, 0}, {K20_PRESENCE, nullptr, out_bytes, 0}}));
    PEP_HIP(ctx, hipMemsetAsync(B[K20_SHARED].p, 0, out_bytes, ctx->stream));         // the kernel stores the pairs i < j alone
    PEP_HIP(ctx, hipMemsetAsync(B[K20_PRESENCE].p, 0, out_bytes, ctx->stream));
    const unsigned tiles = (unsigned)ceil_div(n, K15_TILE);
    pep_timed_stage(ctx, times.ms[1], [&] {
        hipLaunchKernelGGL(profile_pairs, dim3(tiles, tiles), dim3(256), 0, ctx->stream, B[K20_PROFILES].as<const int32_t>(), n, n_genes, B[K20_SHARED].as<int32_t>(),
                           B[K20_PRESENCE].as<int32_t>());
    });
    PEP_HIP(ctx, hipGetLastError());
    PEP_TRY(pep_d2h_queue(ctx, shared, B[K20_SHARED].p, out_bytes));
    PEP_TRY(pep_d2h_queue(ctx, presence, B[K20_PRESENCE].p, out_bytes));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    times.bytes_to_device = prof_bytes;
    times.bytes_to_host = 2 * out_bytes;
    return PEP_OK;
}

}  // extern "C"
