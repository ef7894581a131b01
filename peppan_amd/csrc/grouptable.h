// The host side that K15 (allelediff.hip) and K16 (divergence.hip) share around K15's bit planes: the record of a group, the checks of the row
// and group tables with the layout they produce, and the device prologue that uploads both and queues allele_planes.  Host code only (the
// shared device code is the tile body in allelediff_tile.h); nothing here needs a device before group_tables_to_device.
#pragma once
#include "common.h"
#include "allelediff_tile.h"
#include <initializer_list>

struct GroupRec {                   // what the checker lays out per group, and the record allele_diff reads (K16's kernels read a shorter one: divergence.hip)
    uint64_t rows_off;              // first entry of the group in grp_rows (K16: also in grp_genome / leader)
    uint64_t tri_off, edge_off;     // first int32 pair of the group's packed triangle / [2, n, 2] block in the device output (K16: no edge block, 0)
    uint32_t n, words;              // rows; words per plane
};

struct GroupLayout {
    std::vector<uint64_t> plane_off;        // [n_rows + 1]: first word of the three planes of every row
    std::vector<GroupRec> groups;
    std::vector<DiffTile> tiles;            // the work list of the 64 x 64 tile kernels, over all groups
    uint64_t pairs = 0;                     // int32 pairs of device output
};

struct GroupTables {                // the caller's tables as both entry points receive them
    const uint8_t *packed; const uint64_t *row_off; const uint32_t *row_len; uint64_t n_rows;
    uint32_t n_groups; const uint64_t *grp_off; const uint32_t *grp_rows;
};

// what differs between the two entry points beside their hooks
struct GroupSpec {
    const char *me;                 // prefix of every message: "pep_allele_diff: "
    const char *noun;               // what the pair budget counts: "output" / "triangles"
    const char *counted;            // what the work-list limit counts: "tiles of pairs" / "tiles or edge pairs"
    uint64_t min_rows;              // groups with fewer rows get no words and no output
};

// the slots of pep_ctx::ws the two kernels use
enum {
    K15_WS_PACKED = 0, K15_WS_ROW_OFF, K15_WS_ROW_LEN, K15_WS_PLANE_OFF, K15_WS_PLANES, K15_WS_GRP_ROWS, K15_WS_GROUPS, K15_WS_TILES,
    K15_WS_OUT,                     // K15 alone: its output
    K15_WS_BAD_ROW,
    K15_WS_SLOTS,                   // K16 goes on where K15 ends
    K16_WS_GENOME = K15_WS_SLOTS, K16_WS_EDGES, K16_WS_GD_KEY, K16_WS_GD_VAL, K16_WS_FLAGS, K16_WS_VERDICT, K16_WS_SPILL,
    K16_WS_SLOTS
};
static_assert(K16_WS_SLOTS <= PEP_WS_HITS_OUT, "leaves the device-resident hit table alone");

// Every check of the row and group tables, on the host, so that a bad table is an error and not an out-of-bounds access; also lays the device
// buffers out.  Returns a code and, for an error, msg.
//   check(g, want)         the entry point's own check of group g (the text of a PEP_ERR_ARG, or empty) and what the group asks for:
//                          want bit 0 = the packed triangle (laid out for n > 1), bit 1 = the first / last row strip
//   laid(g, G, added)      group g (of at least min_rows rows) is laid out and `added` pairs of output are its own; returns how many work items
//                          beside the tiles the entry point has so far (they share the tiles' limit)
template <class Check, class Laid>
int group_tables_check(const GroupTables &T, const GroupSpec &S, Check check, Laid laid, GroupLayout &L, std::string &msg)
{
    const auto bad = [&](int code, const std::string &text) { msg = S.me + text; return code; };
    if (T.n_rows >= 0xFFFFFFFFull) return bad(PEP_ERR_LIMIT, "more than 2^32 - 2 rows");
    L.plane_off.assign(T.n_rows + 1, 0);
    for (uint64_t r = 0; r < T.n_rows; ++r) {
        const uint64_t s = ((uint64_t)T.row_len[r] + 2) / 3;
        if (T.row_off[r + 1] < T.row_off[r] || T.row_off[r + 1] - T.row_off[r] != s)
            return bad(PEP_ERR_ARG, "row " + std::to_string(r) + " does not hold ceil(row_len / 3) bytes");
        L.plane_off[r + 1] = L.plane_off[r] + 3 * ((3 * s + 63) / 64);
    }
    if (T.n_groups && T.grp_off[0] != 0) return bad(PEP_ERR_ARG, "grp_off must start at 0");
    L.groups.resize(T.n_groups);
    uint64_t beside = 0;
    for (uint32_t g = 0; g < T.n_groups; ++g) {
        if (T.grp_off[g + 1] < T.grp_off[g]) return bad(PEP_ERR_ARG, "grp_off must be non-decreasing");
        const uint64_t n = T.grp_off[g + 1] - T.grp_off[g], before = L.pairs;
        if (n >= 0x7FFFFFFFull) return bad(PEP_ERR_LIMIT, "more than 2^31 - 2 rows in one group");
        unsigned want = 0;
        const std::string fault = check(g, want);
        if (!fault.empty()) return bad(PEP_ERR_ARG, fault);
        GroupRec &G = L.groups[g];
        G = GroupRec{T.grp_off[g], 0, 0, (uint32_t)n, 0};
        for (uint64_t k = T.grp_off[g]; k < T.grp_off[g + 1]; ++k) {
            const uint32_t r = T.grp_rows[k];
            if (r >= T.n_rows) return bad(PEP_ERR_ARG, "row index " + std::to_string(r) + " of group " + std::to_string(g) + " out of range");
            if (T.row_len[r] != T.row_len[T.grp_rows[T.grp_off[g]]]) return bad(PEP_ERR_ARG, "group " + std::to_string(g) + " mixes rows of different row_len");
        }
        if (n < S.min_rows) continue;
        const uint32_t r0 = T.grp_rows[T.grp_off[g]];
        G.words = (uint32_t)((L.plane_off[r0 + 1] - L.plane_off[r0]) / 3);
        const uint64_t nt = (n + K15_TILE - 1) / K15_TILE;
        const auto over_budget = [&] {          // at the first group that crosses it: `pairs` never grows past budget + one group (n < 2^31: no wrap)
            return bad(PEP_ERR_LIMIT, std::to_string(L.pairs * 8) + " bytes of " + S.noun + " asked for, the device budget of one call is " +
                                          std::to_string((uint64_t)PEP_ALLELE_DIFF_MAX_BYTES) + " (reached at group " + std::to_string(g) + ": split the batch)");
        };
        if ((want & 1) && n > 1) {
            G.tri_off = L.pairs;
            L.pairs += n * (n - 1) / 2;
            if (L.pairs * 8 > PEP_ALLELE_DIFF_MAX_BYTES) return over_budget();
            for (uint64_t ti = 0; ti < nt; ++ti)
                for (uint64_t tj = ti; tj < nt; ++tj) L.tiles.push_back(DiffTile{g, (uint32_t)ti, (uint32_t)tj, 0u});
        }
        if (want & 2) {
            G.edge_off = L.pairs;
            L.pairs += 2 * n;
            if (L.pairs * 8 > PEP_ALLELE_DIFF_MAX_BYTES) return over_budget();
            for (uint64_t tj = 0; tj < nt; ++tj) L.tiles.push_back(DiffTile{g, 0u, (uint32_t)tj, 1u});
        }
        beside = laid(g, G, L.pairs - before);
    }
    if (L.tiles.size() > 0x7FFFFFFFull || beside > 0x7FFFFFFFull)
        return bad(PEP_ERR_LIMIT, std::string("more than 2^31 - 1 ") + S.counted + " in one call (split the batch)");
    if (L.plane_off[T.n_rows] * 8 > PEP_ALLELE_DIFF_MAX_BYTES)
        return bad(PEP_ERR_LIMIT, std::to_string(L.plane_off[T.n_rows] * 8) + " bytes of bit planes asked for, the device budget of one call is " +
                                      std::to_string((uint64_t)PEP_ALLELE_DIFF_MAX_BYTES) + " (split the batch)");
    return PEP_OK;
}

// The device prologue of both kernels (n_groups >= 1): the tables, the layout and the caller's own tables and buffers (`more`) go to their workspace
// slots (pep_tables_to_device), the bad-row word is cleared and allele_planes is queued (its time -> ms_planes).  dev_groups: the group records as the
// caller's kernels read them.
inline int group_tables_to_device(pep_ctx *ctx, const GroupTables &T, const GroupLayout &L, const void *dev_groups, size_t groups_bytes,
                                  std::initializer_list<WsTable> more, double &ms_planes)
{
    DevBuf *W = ctx->ws;
    std::vector<WsTable> put{{K15_WS_PACKED, T.packed, T.row_off[T.n_rows], 1},
                             {K15_WS_ROW_OFF, T.row_off, (T.n_rows + 1) * 8, 0}, {K15_WS_ROW_LEN, T.row_len, T.n_rows * 4, 4},
                             {K15_WS_PLANE_OFF, L.plane_off.data(), (T.n_rows + 1) * 8, 0}, {K15_WS_GRP_ROWS, T.grp_rows, T.grp_off[T.n_groups] * 4, 4},
                             {K15_WS_GROUPS, dev_groups, groups_bytes, 0},
                             {K15_WS_TILES, L.tiles.data(), L.tiles.size() * sizeof(DiffTile), sizeof(DiffTile)},
                             {K15_WS_PLANES, nullptr, (L.plane_off[T.n_rows] + 1) * 8, 0}, {K15_WS_BAD_ROW, nullptr, 256, 0}};
    put.insert(put.end(), more);
    PEP_TRY(pep_tables_to_device(ctx, W, put));
    PEP_HIP(ctx, hipMemsetAsync(W[K15_WS_BAD_ROW].p, 0xFF, 4, ctx->stream));
    if (T.n_rows)
        pep_timed_stage(ctx, ms_planes, [&] {
            pep_k15_queue_planes(ctx->stream, T.n_rows, W[K15_WS_PACKED].as<const uint8_t>(), W[K15_WS_ROW_OFF].as<const uint64_t>(), W[K15_WS_ROW_LEN].as<const uint32_t>(),
                                 W[K15_WS_PLANE_OFF].as<const uint64_t>(), W[K15_WS_PLANES].as<unsigned long long>(), W[K15_WS_BAD_ROW].as<uint32_t>());
        });
    return PEP_OK;
}

inline int group_tables_bad_byte(pep_ctx *ctx, const GroupSpec &S, uint64_t row)
{
    return pep_fail(ctx, PEP_ERR_ARG, S.me + ("row " + std::to_string(row)) + " holds a byte above 124 (not three base-5 digits)");
}

// after the kernels are queued: waits for them and for the downloads the caller has queued, and fails when allele_planes met a bad byte
inline int group_tables_finish(pep_ctx *ctx, const GroupSpec &S)
{
    PEP_HIP(ctx, hipGetLastError());
    uint32_t bad_row = 0xFFFFFFFFu;         // what the prologue's fill left when no row is bad
    PEP_TRY(pep_d2h_queue(ctx, &bad_row, ctx->ws[K15_WS_BAD_ROW].p, 4));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    return bad_row == 0xFFFFFFFFu ? PEP_OK : group_tables_bad_byte(ctx, S, bad_row);
}
