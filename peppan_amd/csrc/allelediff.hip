// K15: pairwise allele differences of gene groups (compare_seq / compare_seqX, PEPPAN.py:296-316, over the rows filt_per_group reads
// from the .seq store and masks, :332-333).  The reference compares n x n x L bytes per group; both of its counts are sums over columns,
// so the column order is free and the base-5 packed rows are never decoded to bytes:
//   allele_planes  one wavefront per packed row: every byte goes through a 125-entry table to three (valid, 2-bit code) digits, and
//                  64 digits at a time become one word of each of three bit planes V (comparable), B0, B1.  Digit d of byte j (column
//                  d * s + j of the reference's decoded row, s = ceil(ref_len / 3)) is bit 3 j + d; columns >= ref_len get V = 0.
//   allele_diff    one workgroup per 64 x 64 tile of pairs of one group (work list over all groups of the batch, built on the host);
//                  the planes of the two row panels are staged in LDS four words at a time, every thread keeps a 4 x 4 micro-tile:
//                  c = Va & Vb, comparable += popc(c), mismatch += popc(c & ((B0a ^ B0b) | (B1a ^ B1b))).  A first/last-row strip
//                  (compare_seqX) is the same loop with a two-row A panel.  Output (mismatch + 1, comparable + 2) as int32 pairs:
//                  the packed upper triangle and / or [2, n, 2], plain vector stores.
// About 14 VALU instructions per pair and 64 columns: the kernel is bound by its n^2 x 8 B of output, the call by the copy to the host.
#include "common.h"
#include "allelediff_tile.h"
#include <algorithm>
#include <chrono>
#include <numeric>
#include <optional>

namespace {

struct DiffGroup {
    uint64_t rows_off;              // first entry of the group in grp_rows
    uint64_t tri_off, edge_off;     // first int32 pair of the group's packed triangle / [2, n, 2] block in the device output
    uint32_t n, words;              // rows; words per plane
};

// Neither kernel is tuned: by the recorded event times (profiles/allele_diff_rate.txt) they are a few per cent of a call that is bound by the
// copy of its output.  Known slack: allele_planes keeps only `words` lanes of a wavefront busy (16 of 64 for 1 002 nt), each walking 64 digits
// with byte loads; allele_diff's staging loop maps consecutive threads to consecutive ROWS (conflict-free LDS writes, but every global load of
// a wavefront touches 64 cache lines for 8 bytes each - the planes are L2-resident); a strip tile computes a full 64 x 64 tile for 2 x 64 results.
__global__ __launch_bounds__(256) void allele_planes(uint64_t n_rows, const uint8_t *__restrict__ packed, const uint64_t *__restrict__ row_off,
                                                     const uint32_t *__restrict__ row_len, const uint64_t *__restrict__ plane_off,
                                                     unsigned long long *__restrict__ planes, uint32_t *__restrict__ bad_row)
{
    __shared__ uint16_t tab[128];           // byte -> 3 x (valid | code << 1), digit d at bits 3 d .. 3 d + 2
    if (threadIdx.x < 128) {
        const uint32_t b = threadIdx.x, dg[3] = {b / 25, (b / 5) % 5, b % 5};
        uint32_t t = 0;
        for (int d = 0; d < 3; ++d)
            if (b < 125 && dg[d]) t |= (1u | ((dg[d] - 1) << 1)) << (3 * d);
        tab[b] = (uint16_t)t;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const uint8_t *src = packed + row_off[r];
    const uint64_t len = row_len[r], s = (len + 2) / 3, words = (3 * s + 63) / 64;
    unsigned long long *out = planes + plane_off[r];
    bool bad = false;
    for (uint64_t w = lane; w < words; w += 64) {
        unsigned long long v = 0, b0 = 0, b1 = 0;
        uint64_t j = (64 * w) / 3;
        uint32_t d = (uint32_t)((64 * w) % 3);
        for (int bit = 0; bit < 64 && j < s; ++bit) {
            const uint32_t byte = src[j];
            if (byte > 124) bad = true;
            const uint32_t dg = byte > 124 ? 0u : (tab[byte] >> (3 * d)) & 7u;
            if ((dg & 1u) && d * s + j < len) {
                v |= 1ull << bit;
                b0 |= (unsigned long long)((dg >> 1) & 1u) << bit;
                b1 |= (unsigned long long)(dg >> 2) << bit;
            }
            if (++d == 3) { d = 0; ++j; }
        }
        out[w] = v;
        out[words + w] = b0;
        out[2 * words + w] = b1;
    }
    if (bad) atomicMin(bad_row, (uint32_t)r);
}

__global__ __launch_bounds__(256) void allele_diff(const DiffTile *__restrict__ tiles, const DiffGroup *__restrict__ groups,
                                                   const uint32_t *__restrict__ grp_rows, const uint64_t *__restrict__ plane_off,
                                                   const unsigned long long *__restrict__ planes, int2 *__restrict__ out)
{
    const DiffTile T = tiles[blockIdx.x];
    const DiffGroup G = groups[T.g];
    const uint32_t tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    uint32_t mis[4][4], cmp[4][4];
    k15_tile_counts(grp_rows + G.rows_off, G.n, G.words, T, plane_off, planes, mis, cmp);     // (allelediff_tile.h: shared with K16)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t b = (uint64_t)T.tj * K15_TILE + tx + 16 * j, n = G.n;
            const int2 val = make_int2((int)mis[i][j] + 1, (int)cmp[i][j] + 2);
            if (T.kind == 0) {
                const uint64_t a = (uint64_t)T.ti * K15_TILE + ty * 4 + i;
                if (a < b && b < n) out[G.tri_off + a * (2 * n - a - 1) / 2 + (b - a - 1)] = val;
            } else if (ty == 0 && i < 2 && b < n) {
                out[G.edge_off + (uint64_t)i * n + b] = val;
            }
        }
}

}  // namespace

void pep_k15_queue_planes(hipStream_t st, uint64_t n_rows, const uint8_t *d_packed, const uint64_t *d_row_off, const uint32_t *d_row_len,
                          const uint64_t *d_plane_off, unsigned long long *d_planes, uint32_t *d_bad_row)
{
    hipLaunchKernelGGL(allele_planes, dim3((unsigned)ceil_div(n_rows, 4)), dim3(256), 0, st, n_rows, d_packed, d_row_off, d_row_len, d_plane_off, d_planes, d_bad_row);
}

int pep_k15_allele_diff(pep_ctx *ctx, const uint8_t *h_packed, const uint64_t *h_row_off, const uint32_t *h_row_len, uint64_t n_rows,
                        uint32_t n_groups, const uint64_t *h_grp_off, const uint32_t *h_grp_rows, const uint8_t *h_grp_mode,
                        int32_t *h_out, const uint64_t *h_out_off, uint64_t out_cap)
{
    ctx->k15_ms[0] = ctx->k15_ms[1] = ctx->k15_ms[2] = 0.;
    if (n_groups == 0) return PEP_OK;
    if (n_rows >= 0xFFFFFFFFull) return pep_fail(ctx, PEP_ERR_LIMIT, "pep_allele_diff: more than 2^32 - 2 rows");
    // validate on the host so that a bad table is an error, not an out-of-bounds access; also lays out the buffers
    std::vector<uint64_t> plane_off(n_rows + 1);
    plane_off[0] = 0;
    for (uint64_t r = 0; r < n_rows; ++r) {
        const uint64_t s = ((uint64_t)h_row_len[r] + 2) / 3;
        if (h_row_off[r + 1] < h_row_off[r] || h_row_off[r + 1] - h_row_off[r] != s)
            return pep_fail(ctx, PEP_ERR_ARG, "pep_allele_diff: row " + std::to_string(r) + " does not hold ceil(row_len / 3) bytes");
        plane_off[r + 1] = plane_off[r] + 3 * ((3 * s + 63) / 64);
    }
    if (h_grp_off[0] != 0) return pep_fail(ctx, PEP_ERR_ARG, "pep_allele_diff: grp_off must start at 0");
    std::vector<DiffGroup> groups(n_groups);
    std::vector<DiffTile> tiles;
    std::vector<uint64_t> need(n_groups);           // int32 values of every group's output
    uint64_t pairs = 0;
    const auto over_budget = [&](uint32_t g) {             // at the first group that crosses it: `pairs` never grows past budget + one group (n < 2^31: no wrap)
        return pep_fail(ctx, PEP_ERR_LIMIT, "pep_allele_diff: " + std::to_string(pairs * 8) + " bytes of output asked for, the device budget of one call is " +
                                             std::to_string((uint64_t)PEP_ALLELE_DIFF_MAX_BYTES) + " (reached at group " + std::to_string(g) + ": split the batch)");
    };
    for (uint32_t g = 0; g < n_groups; ++g) {
        if (h_grp_off[g + 1] < h_grp_off[g]) return pep_fail(ctx, PEP_ERR_ARG, "pep_allele_diff: grp_off must be non-decreasing");
        const uint64_t n = h_grp_off[g + 1] - h_grp_off[g], before = pairs;
        if (n >= 0x7FFFFFFFull) return pep_fail(ctx, PEP_ERR_LIMIT, "pep_allele_diff: more than 2^31 - 2 rows in one group");
        if (h_grp_mode[g] > 3) return pep_fail(ctx, PEP_ERR_ARG, "pep_allele_diff: unknown mode bits of group " + std::to_string(g));
        DiffGroup &G = groups[g];
        G.rows_off = h_grp_off[g]; G.n = (uint32_t)n; G.words = 0; G.tri_off = G.edge_off = 0;
        for (uint64_t k = h_grp_off[g]; k < h_grp_off[g + 1]; ++k) {
            const uint32_t r = h_grp_rows[k];
            if (r >= n_rows) return pep_fail(ctx, PEP_ERR_ARG, "pep_allele_diff: row index " + std::to_string(r) + " of group " + std::to_string(g) + " out of range");
            if (h_row_len[r] != h_row_len[h_grp_rows[h_grp_off[g]]])
                return pep_fail(ctx, PEP_ERR_ARG, "pep_allele_diff: group " + std::to_string(g) + " mixes rows of different row_len");
        }
        if (n) G.words = (uint32_t)((plane_off[h_grp_rows[h_grp_off[g]] + 1] - plane_off[h_grp_rows[h_grp_off[g]]]) / 3);
        const uint64_t nt = (n + K15_TILE - 1) / K15_TILE;
        if ((h_grp_mode[g] & 1) && n > 1) {
            G.tri_off = pairs;
            pairs += n * (n - 1) / 2;
            if (pairs * 8 > PEP_ALLELE_DIFF_MAX_BYTES) return over_budget(g);
            for (uint64_t ti = 0; ti < nt; ++ti)
                for (uint64_t tj = ti; tj < nt; ++tj) tiles.push_back(DiffTile{g, (uint32_t)ti, (uint32_t)tj, 0u});
        }
        if ((h_grp_mode[g] & 2) && n) {
            G.edge_off = pairs;
            pairs += 2 * n;
            if (pairs * 8 > PEP_ALLELE_DIFF_MAX_BYTES) return over_budget(g);
            for (uint64_t tj = 0; tj < nt; ++tj) tiles.push_back(DiffTile{g, 0u, (uint32_t)tj, 1u});
        }
        need[g] = 2 * (pairs - before);
    }
    if (tiles.size() > 0x7FFFFFFFull) return pep_fail(ctx, PEP_ERR_LIMIT, "pep_allele_diff: more than 2^31 - 1 tiles of pairs in one call (split the batch)");
    if (plane_off[n_rows] * 8 > PEP_ALLELE_DIFF_MAX_BYTES)
        return pep_fail(ctx, PEP_ERR_LIMIT, "pep_allele_diff: " + std::to_string(plane_off[n_rows] * 8) + " bytes of bit planes asked for, the device budget of one call is " +
                                             std::to_string((uint64_t)PEP_ALLELE_DIFF_MAX_BYTES) + " (split the batch)");
    // where the caller wants the groups: inside out_cap, no two on the same values
    std::vector<uint32_t> order(n_groups);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return h_out_off[a] < h_out_off[b]; });
    uint64_t end_before = 0;
    for (uint32_t g : order) {
        if (!need[g]) continue;
        if (h_out_off[g] > out_cap || need[g] > out_cap - h_out_off[g])
            return pep_fail(ctx, PEP_ERR_ARG, "pep_allele_diff: output of group " + std::to_string(g) + " runs past out_cap");
        if (h_out_off[g] < end_before) return pep_fail(ctx, PEP_ERR_ARG, "pep_allele_diff: output of group " + std::to_string(g) + " overlaps another group's");
        end_before = h_out_off[g] + need[g];
    }
    const uint64_t n_idx = h_grp_off[n_groups], n_bytes = h_row_off[n_rows];
    if (tiles.empty()) {
        // nothing but empty groups, one-row triangles or groups without a mode bit: no kernel runs, so the bytes are looked at here
        for (uint64_t k = 0; k < n_bytes; ++k)
            if (h_packed[k] > 124) {
                const uint64_t r = (uint64_t)(std::upper_bound(h_row_off, h_row_off + n_rows + 1, k) - h_row_off) - 1;
                return pep_fail(ctx, PEP_ERR_ARG, "pep_allele_diff: row " + std::to_string(r) + " holds a byte above 124 (not three base-5 digits)");
            }
        return PEP_OK;
    }
    DevBuf *W = ctx->ws;
    hipStream_t st = ctx->stream;
    PEP_TRY(dev_reserve(ctx, W[0], n_bytes + 1));
    PEP_TRY(dev_reserve(ctx, W[1], (n_rows + 1) * 8));
    PEP_TRY(dev_reserve(ctx, W[2], (n_rows + 1) * 4));
    PEP_TRY(dev_reserve(ctx, W[3], (n_rows + 1) * 8));
    PEP_TRY(dev_reserve(ctx, W[4], (plane_off[n_rows] + 1) * 8));
    PEP_TRY(dev_reserve(ctx, W[5], (n_idx + 1) * 4));
    PEP_TRY(dev_reserve(ctx, W[6], (size_t)n_groups * sizeof(DiffGroup)));
    PEP_TRY(dev_reserve(ctx, W[7], tiles.size() * sizeof(DiffTile)));
    PEP_TRY(dev_reserve(ctx, W[8], (pairs + 1) * 8));
    PEP_TRY(dev_reserve(ctx, W[9], 256));
    PEP_TRY(pep_h2d(ctx, W[0].p, h_packed, n_bytes));
    PEP_TRY(pep_h2d(ctx, W[1].p, h_row_off, (n_rows + 1) * 8));
    PEP_TRY(pep_h2d(ctx, W[2].p, h_row_len, n_rows * 4));
    PEP_TRY(pep_h2d(ctx, W[3].p, plane_off.data(), (n_rows + 1) * 8));
    PEP_TRY(pep_h2d(ctx, W[5].p, h_grp_rows, n_idx * 4));
    PEP_TRY(pep_h2d(ctx, W[6].p, groups.data(), (size_t)n_groups * sizeof(DiffGroup)));
    PEP_TRY(pep_h2d(ctx, W[7].p, tiles.data(), tiles.size() * sizeof(DiffTile)));
    PEP_HIP(ctx, hipMemsetAsync(W[9].p, 0xFF, 4, st));
    const bool timed = ctx->timing_level >= 2;
    {
        std::optional<EventTimer> tm;
        if (timed) tm.emplace(st);
        pep_k15_queue_planes(st, n_rows, W[0].as<const uint8_t>(), W[1].as<const uint64_t>(), W[2].as<const uint32_t>(), W[3].as<const uint64_t>(),
                             W[4].as<unsigned long long>(), W[9].as<uint32_t>());
        if (timed) ctx->k15_ms[0] = tm->stop();
    }
    {
        std::optional<EventTimer> tm;
        if (timed) tm.emplace(st);
        hipLaunchKernelGGL(allele_diff, dim3((unsigned)tiles.size()), dim3(256), 0, st, W[7].as<const DiffTile>(), W[6].as<const DiffGroup>(),
                           W[5].as<const uint32_t>(), W[3].as<const uint64_t>(), W[4].as<const unsigned long long>(), W[8].as<int2>());
        if (timed) ctx->k15_ms[1] = tm->stop();
    }
    PEP_HIP(ctx, hipGetLastError());
    uint32_t bad_row = 0xFFFFFFFFu;
    PEP_TRY(pep_d2h_queue(ctx, &bad_row, W[9].p, 4));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    if (bad_row != 0xFFFFFFFFu)
        return pep_fail(ctx, PEP_ERR_ARG, "pep_allele_diff: row " + std::to_string(bad_row) + " holds a byte above 124 (not three base-5 digits)");
    // groups that follow each other in the caller's buffer as they do on the device leave in one copy
    const auto copy_t0 = std::chrono::steady_clock::now();
    uint64_t dev_at = 0, run_dev = 0, run_host = 0, run = 0;
    for (uint32_t g = 0; g <= n_groups; ++g) {
        if (g < n_groups && !need[g]) continue;
        if (g < n_groups && run && h_out_off[g] == run_host + run) {
            run += need[g];
        } else {
            if (run) PEP_TRY(pep_d2h_queue(ctx, h_out + run_host, W[8].as<const int32_t>() + run_dev, run * 4));
            if (g == n_groups) break;
            run_host = h_out_off[g]; run_dev = dev_at; run = need[g];
        }
        dev_at += need[g];
    }
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    ctx->k15_ms[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - copy_t0).count();
    return PEP_OK;
}
