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
// The checks of the row and group tables, their layout and the device prologue up to allele_planes are grouptable.h's, shared with K16.
#include "common.h"
#include "allelediff_tile.h"
#include "grouptable.h"
#include <algorithm>
#include <chrono>
#include <numeric>

namespace {

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

__global__ __launch_bounds__(256) void allele_diff(const DiffTile *__restrict__ tiles, const GroupRec *__restrict__ groups,
                                                   const uint32_t *__restrict__ grp_rows, const uint64_t *__restrict__ plane_off,
                                                   const unsigned long long *__restrict__ planes, int2 *__restrict__ out)
{
    const DiffTile T = tiles[blockIdx.x];
    const GroupRec G = groups[T.g];
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

extern "C" {

int pep_allele_diff(pep_ctx *ctx, const uint8_t *h_packed, const uint64_t *h_row_off, const uint32_t *h_row_len, uint64_t n_rows,
                    uint32_t n_groups, const uint64_t *h_grp_off, const uint32_t *h_grp_rows, const uint8_t *h_grp_mode,
                    int32_t *h_out, const uint64_t *h_out_off, uint64_t out_cap)
{
    if (!ctx) return PEP_ERR_ARG;
    if (!h_row_off || (n_rows && !h_row_len) || (n_groups && (!h_grp_off || !h_grp_mode || !h_out_off)) || (out_cap && !h_out))
        return pep_fail(ctx, PEP_ERR_ARG, "pep_allele_diff: null table");
    if (n_groups && h_grp_off[n_groups] && !h_grp_rows) return pep_fail(ctx, PEP_ERR_ARG, "pep_allele_diff: null table");
    if (n_rows && h_row_off[n_rows] && !h_packed) return pep_fail(ctx, PEP_ERR_ARG, "pep_allele_diff: null table");
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    CallTimes &times = ctx->calls[PEP_CALL_ALLELE_DIFF];
    times = {};
    if (n_groups == 0) return PEP_OK;
    const GroupTables T{h_packed, h_row_off, h_row_len, n_rows, n_groups, h_grp_off, h_grp_rows};
    const GroupSpec S{"pep_allele_diff: ", "output", "tiles of pairs", 1};
    GroupLayout L;
    std::vector<uint64_t> need(n_groups);           // int32 values of every group's output
    std::string msg;
    const int rc = group_tables_check(T, S,
        [&](uint32_t g, unsigned &want) { want = h_grp_mode[g]; return want > 3 ? "unknown mode bits of group " + std::to_string(g) : std::string(); },
        [&](uint32_t g, const GroupRec &, uint64_t added) { need[g] = 2 * added; return 0; }, L, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
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
    if (L.tiles.empty()) {
        // nothing but empty groups, one-row triangles or groups without a mode bit: no kernel runs, so the bytes are looked at here
        for (uint64_t k = 0; k < h_row_off[n_rows]; ++k)
            if (h_packed[k] > 124) return group_tables_bad_byte(ctx, S, (uint64_t)(std::upper_bound(h_row_off, h_row_off + n_rows + 1, k) - h_row_off) - 1);
        return PEP_OK;
    }
    static_assert(K15_WS_SLOTS <= PEP_WS_HITS_OUT, "leaves the device-resident hit table alone");
    DevBuf *W = ctx->ws;
    PEP_TRY(group_tables_to_device(ctx, T, L, L.groups.data(), (size_t)n_groups * sizeof(GroupRec), {{K15_WS_OUT, nullptr, (L.pairs + 1) * 8, 0}}, times.ms[0]));
    pep_timed_stage(ctx, times.ms[1], [&] {
        hipLaunchKernelGGL(allele_diff, dim3((unsigned)L.tiles.size()), dim3(256), 0, ctx->stream, W[K15_WS_TILES].as<const DiffTile>(), W[K15_WS_GROUPS].as<const GroupRec>(),
                           W[K15_WS_GRP_ROWS].as<const uint32_t>(), W[K15_WS_PLANE_OFF].as<const uint64_t>(), W[K15_WS_PLANES].as<const unsigned long long>(), W[K15_WS_OUT].as<int2>());
    });
    PEP_TRY(group_tables_finish(ctx, S));
    // groups that follow each other in the caller's buffer as they do on the device leave in one copy
    const auto copy_t0 = std::chrono::steady_clock::now();
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
    times.ms[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - copy_t0).count();
    return PEP_OK;
}

}  // extern "C"
