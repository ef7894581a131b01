// K6 + K8: choose the best band per (query, target), walk the traceback codes written by K5 (one alignment per lane),
// run-length encode the CIGAR, count identities, apply the identity / query-cover filters and the
// per-(query, split) top-k, and emit fixed-size hit records + a CIGAR arena ordered by (q, t).
#include "common.h"
#include "lookback.h"
#include <cstring>

namespace {

struct SelInfo {          // one per selected (q,t) pair
    uint32_t cand;        // index into the compacted key list of selected pairs (== own index)
    int32_t score, iend, jend;
    int32_t istart, jstart;
    uint32_t n_runs, aln_len, n_ident;
    uint32_t pass;        // survived the filters
    uint32_t keep;        // survived top-k
    uint32_t pad;
};

__device__ __forceinline__ uint32_t key_q(uint64_t k) { return (uint32_t)(k >> 43); }
__device__ __forceinline__ uint32_t key_t(uint64_t k) { return (uint32_t)((k >> 18) & ((1u << 25) - 1)); }
__device__ __forceinline__ int key_dlo(uint64_t k) { return (int)(k & ((1u << 18) - 1)) * 64 - (1 << 23) - 32; }

// Selection (group heads pick the best band of their (q, t) group: score desc, then lowest bin = first in sorted order; hsp_mode 1: every band
// that reaches the threshold), compaction and run slots in ONE launch (lookback.h): every thread judges its candidate, the tile scans two
// values at once - selected pairs (their slot in the arrays of the selected) and their run capacity (the slot of their CIGAR runs) - finds
// the totals of the tiles in front of it by look-back and writes the selected pairs' records straight to their slots.  Four launches of a
// dependent chain before (about 5 us each for 50 k candidates).
// The two look-backs of such a kernel.  The tile number comes from the ticket of `count` alone and indexes the status words of both areas:
// the two are always begun together, for the same number of tiles (begin_select), so tile t of this launch owns word t of either, and the
// ticket counter of `runs` (and with it runs.ticket_base) is never read by anyone.
struct SelectState { LbLaunch count, runs; };
int begin_select(pep_ctx *ctx, PepLookback count_slot, PepLookback runs_slot, uint64_t tiles, SelectState *s)
{
    PEP_TRY(pep_lookback_begin(ctx, count_slot, tiles, 1, 32, &s->count));
    return pep_lookback_begin(ctx, runs_slot, tiles, 1, 48, &s->runs);
}
__global__ __launch_bounds__(256) void select_gather(const uint64_t *__restrict__ cands, uint64_t n, const int4 *__restrict__ sw, const int32_t *__restrict__ min_score,
                                                     int hsp_mode, const uint32_t *__restrict__ q_len, const uint32_t *__restrict__ t_len, SelInfo *__restrict__ sel,
                                                     uint64_t *__restrict__ run_off, uint64_t *__restrict__ sel_keys, int32_t *__restrict__ known, int32_t *__restrict__ end_lane,
                                                     uint32_t *__restrict__ counters /* [0] (q, t) groups, [1] selected pairs */, unsigned long long *__restrict__ total_runs,
                                                     SelectState st)
{
    __shared__ uint32_t s_tile, lds32[4];
    __shared__ uint64_t lds64[4], s_pre[2];
    const uint32_t tile = lb_take_tile(st.count.state, st.count.ticket_base, &s_tile);
    const uint64_t c = (uint64_t)tile * 256 + threadIdx.x;
    const bool live = c < n;
    const uint64_t g = live ? cands[c] >> 18 : 0;
    const bool head = live && (c == 0 || (cands[c - 1] >> 18) != g);
    const int heads = __syncthreads_count(head);                 // (q, t) groups that start in this tile: one atomic per block
    if (threadIdx.x == 0 && heads) atomicAdd(&counters[0], (uint32_t)heads);
    uint32_t f = 0, b = (uint32_t)c;
    if (live && hsp_mode != 0) {
        // every band that reaches the threshold is traced; duplicates are removed after the walk (dedupe_bands; hsp_mode 2: cull_hsps)
        if (sw[c].x > 0 && sw[c].x >= min_score[key_q(cands[c])]) f = 1;
    } else if (head) {
        int best = sw[c].x;
        for (uint64_t x = c + 1; x < n && (cands[x] >> 18) == g; ++x)
            if (sw[x].x > best) { best = sw[x].x; b = (uint32_t)x; }
        if (best > 0 && best >= min_score[key_q(cands[c])]) f = 1;
    }
    uint64_t key = 0, cap = 0;
    int4 r = make_int4(0, 0, 0, 0);
    if (f) {
        key = cands[b]; r = sw[b];
        cap = 2ull * min(q_len[key_q(key)], t_len[key_t(key)]) + 2;      // an alignment has at most 2 * min(Lq, Lt) + 1 runs (M runs consume a residue of both sequences)
    }
    uint32_t tot_f;
    uint64_t tot_cap;
    const uint32_t ex_f = block_excl_scan_256<uint32_t>(f, &tot_f, lds32);
    const uint64_t ex_cap = block_excl_scan_256<uint64_t>(cap, &tot_cap, lds64);
    if (threadIdx.x < 64) {
        const uint64_t p0 = lb_tile_prefix<32>(st.count.status(), tile, tot_f, st.count.epoch, (int)threadIdx.x);
        const uint64_t p1 = lb_tile_prefix<48>(st.runs.status(), tile, tot_cap, st.runs.epoch, (int)threadIdx.x);
        if (threadIdx.x == 0) { s_pre[0] = p0; s_pre[1] = p1; }
    }
    __syncthreads();
    if (f) {
        const uint64_t slot = s_pre[0] + ex_f;
        SelInfo s;
        s.cand = (uint32_t)slot; s.score = r.x; s.iend = s.jend = -1;      // the end cell comes from the traceback pass
        s.istart = s.jstart = 0; s.n_runs = s.aln_len = s.n_ident = 0; s.pass = s.keep = 0; s.pad = 0;
        sel[slot] = s;
        sel_keys[slot] = key;
        known[slot] = r.x;              // the traceback pass looks for the first cell that reaches this score ...
        end_lane[slot] = r.y;           // ... in the sub-band around the lane where the score pass met it
        run_off[slot] = s_pre[1] + ex_cap;
    }
    if ((uint64_t)(tile + 1) * 256 >= n && threadIdx.x == 255) {      // the last tile: totals
        counters[1] = (uint32_t)(s_pre[0] + tot_f);
        *total_runs = s_pre[1] + tot_cap;
    }
}

// Rule 5a (oracle: gapless_segment / band_align): before any traceback sweep, the two diagonals of the lowest lane
// that met the band's score T in the score pass are scanned for an UNGAPPED segment scoring T.  Such a segment IS the alignment that ends
// in its last cell (H equals the running ungapped sum all along it - anything larger would end above T - and the diagonal move has
// priority), so the pair is settled as one M run: mode -2, no codes, no walk.
// One wavefront per pair; a diagonal is taken 512 cells at a time, eight consecutive cells per lane (two unaligned 8-byte loads - the
// packed sets carry >= 16 bytes of padding behind every sequence - and eight independent table reads).  With P = prefix sum of the
// scores and M = prefix minimum of P (the 0 in front included), run = P - M is Kadane's running sum with its restart after every cell
// that brings it to <= 0: lane sums and lane minima are scanned across the wavefront with DPP moves (no LDS round trips: a first
// version built on __shfl_up spent 165 us in dependent ds_bpermute chains), then every lane replays its eight cells.  The first cell
// with run == T ends the segment, the last restart before it starts it.
template <class Op>
__device__ __forceinline__ int wave_scan_incl(int v, const int identity, Op op)
{
    v = op(v, __builtin_amdgcn_update_dpp(identity, v, 0x111, 0xf, 0xf, false));      // row_shr:1
    v = op(v, __builtin_amdgcn_update_dpp(identity, v, 0x112, 0xf, 0xf, false));      // row_shr:2
    v = op(v, __builtin_amdgcn_update_dpp(identity, v, 0x114, 0xf, 0xf, false));      // row_shr:4
    v = op(v, __builtin_amdgcn_update_dpp(identity, v, 0x118, 0xf, 0xf, false));      // row_shr:8
    v = op(v, __builtin_amdgcn_update_dpp(identity, v, 0x142, 0xa, 0xf, false));      // row_bcast:15 -> rows 1, 3
    v = op(v, __builtin_amdgcn_update_dpp(identity, v, 0x143, 0xc, 0xf, false));      // row_bcast:31 -> rows 2, 3
    return v;
}

__global__ __launch_bounds__(256) void gapless_check(const uint32_t *__restrict__ d_n_sel, const uint64_t *__restrict__ cands, const int32_t *__restrict__ known,
                                                     const int32_t *__restrict__ end_lane, const uint8_t *__restrict__ q_res, const uint32_t *__restrict__ q_off,
                                                     const uint32_t *__restrict__ q_len, const uint8_t *__restrict__ t_res, const uint32_t *__restrict__ t_off,
                                                     const uint32_t *__restrict__ t_len, const int8_t *__restrict__ sub_g, int4 *__restrict__ out,
                                                     int32_t *__restrict__ mode)
{
    __shared__ int8_t sub[1024];
    reinterpret_cast<uint32_t *>(sub)[threadIdx.x] = reinterpret_cast<const uint32_t *>(sub_g)[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t s = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= *d_n_sel) return;                                  // (whole wavefronts leave together; the grid is sized from an upper bound)
    const uint64_t key = cands[s];
    const uint32_t q = key_q(key), t = key_t(key);
    const int T = known[s];
    const int Lq = (int)q_len[q], Lt = (int)t_len[t];
    const uint8_t *qs = q_res + q_off[q], *ts = t_res + t_off[t];
    constexpr int INF = 0x3fffffff;
    auto add = [](int a, int b) { return a + b; };
    auto mn = [](int a, int b) { return min(a, b); };
    int found_is = -1, found_ie = -1, found_d = 0;
    for (int x = 0; x < 2 && found_is < 0 && T > 0; ++x) {
        const int d = key_dlo(key) + 2 * end_lane[s] + x;
        const int i0 = max(0, -d), n = min(Lq - 1, Lt - 1 - d) - i0 + 1;        // cell k of the diagonal is (i0 + k, i0 + k + d)
        int carry_p = 0, carry_m = 0, last_reset = -1;
        for (int base = 0; base < n; base += 512) {             // wave-uniform trip count
            const int k0 = base + lane * 8;
            uint32_t qw[2] = {0u, 0u}, tw[2] = {0u, 0u};
            if (k0 < n) { __builtin_memcpy(qw, qs + i0 + k0, 8); __builtin_memcpy(tw, ts + i0 + k0 + d, 8); }
            int sc[8], S = 0, lmin = INF;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int qc = (qw[u >> 2] >> ((u & 3) * 8)) & 31, tc = (tw[u >> 2] >> ((u & 3) * 8)) & 31;
                sc[u] = k0 + u < n ? (int)sub[qc * 32 + tc] : 0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { S += sc[u]; lmin = min(lmin, S); }
            const int p_start = carry_p + wave_scan_incl(S, 0, add) - S;
            const int m_incl = wave_scan_incl(p_start + lmin, INF, mn);
            const int m_start = min(carry_m, __builtin_amdgcn_update_dpp(INF, m_incl, 0x138, 0xf, 0xf, false));      // lane l <- lane l - 1
            int P = p_start, M = m_start, first = -1, reset = -1;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                P += sc[u]; M = min(M, P);
                const bool live = k0 + u < n && first < 0;
                if (live && P - M == T) first = u;
                if (live && P == M) reset = u;
            }
            const unsigned long long hit = __ballot(first >= 0);
            const unsigned long long resets = __ballot(reset >= 0);
            if (hit) {
                const int l = __builtin_ctzll(hit);
                const int f = __builtin_amdgcn_readlane(first, l), r_own = __builtin_amdgcn_readlane(reset, l);
                int start_k = last_reset + 1;
                if (r_own >= 0) start_k = base + l * 8 + r_own + 1;
                else {
                    const unsigned long long before = resets & ((1ull << l) - 1ull);
                    if (before) { const int r = 63 - __builtin_clzll(before); start_k = base + r * 8 + __builtin_amdgcn_readlane(reset, r) + 1; }
                }
                found_is = i0 + start_k; found_ie = i0 + base + l * 8 + f; found_d = d;
                break;
            }
            if (resets) { const int r = 63 - __builtin_clzll(resets); last_reset = base + r * 8 + __builtin_amdgcn_readlane(reset, r); }
            carry_p = __builtin_amdgcn_readlane(P, 63);
            carry_m = __builtin_amdgcn_readlane(M, 63);
        }
    }
    if (lane == 0) {
        if (found_is >= 0) {
            out[s] = make_int4(T, found_ie, found_ie + found_d, found_ie - found_is + 1);       // score, end cell, run length
            mode[s] = -2;
        } else mode[s] = -1;
    }
}

// One THREAD per selected pair.  The walk is a serial chain of tiny decisions; spread over a wavefront (one alignment per wave, as the
// first version did) every decision costs an issue slot of the whole CU - vector or scalar unit alike - and 40 k alignments took
// 0.48 ms.  One alignment per lane instead, WALK_LANES alignments per wavefront, fewer than one wavefront per SIMD.  A wavefront that is
// alone on its SIMD issues an instruction every dozen cycles, and it executes what ANY of its lanes needs: the kernel's time is the number
// of instructions its wavefronts execute (about 5 ns each, fitted from two builds) plus their round trips to memory (about 0.6 us each), and the
// loop is shaped to keep both chains short (profiles/walk_round_trips_ab.txt: 83.7 -> 50.1 us).
//   * A lane holds a WINDOW of the codes: the words of WALK_AHEAD blocks down from the block of its cell, of FOUR neighbouring diagonals
//     (one unaligned 16-byte load per block: the words of neighbouring diagonals of a block are neighbouring dwords).  A straight stretch
//     runs down one column of the window; a gap moves the lane a column per cell, so a short gap and the stretch behind it cost no request
//     (the window starts one diagonal below the lane's, two when the lane is inside a deletion, which moves it downwards).
//   * The window lies in LDS, 16 bytes per lane and block, because a lane indexes it by its own block and diagonal.  In registers that is a
//     4-way select per access and 28 moves per block (built first: the wavefronts' round trips fell from 26 to 8 and their instructions
//     rose by half, 83.7 -> 106 us; the same had been found in round 3, DESIGN_HISTORY.md).  Nobody reads another lane's words: no barrier.
//   * The loads are a ROUND of the wavefront: an outer loop that loads, an inner loop in which every lane steps until its cell leaves its
//     window.  A lane that is through waits (masked off) for the others, so the round trips a wavefront pays are those of its lane with the
//     most rounds - not, as with a refill inside the stepping loop, one per trip in which any lane needs memory.
//   * A trip of the inner loop has one shape for every lane - a gap cell, or the diagonal cells down to the end of the NEXT word, found with
//     one 64-bit count of leading zeros - and one branch, around the store of a run that has ended.  Before, a trip was a nest of branches
//     (refill, state switch, word-by-word fast path) of which a wavefront ran nearly all, about 170 instructions; now it is about 75.
//   * The loads of a round are unconditional (rows above block 0 read block 0 again and are not counted in `have`): a branch around a load
//     makes hipcc wait for each load on its own.
// Window depth, measured with -DWALK_AHEAD: 6 / 8 / 12 / 16 blocks -> 51.6 / 50.5 / 57.0 / 60.9 us - every block is a scattered request,
// and a window is dropped when a gap leaves it sideways.  For the same reason the window behind the current one is NOT fetched ahead: it
// would hide part of a round trip on a straight stretch and add eight requests to every round that ends sideways or ends the alignment.
#ifndef WALK_AHEAD
#define WALK_AHEAD 8          // blocks per window: 64 cells of a diagonal
#endif
#ifndef WALK_LANES               // (16 and 32 measured at the end of round 3 with -DWALK_LANES: no difference; 32 with the window in LDS: 49.5 against 50.5 us, none either)
#define WALK_LANES 64         // alignments per wavefront
#endif
__global__ __launch_bounds__(WALK_LANES) void walk(const uint32_t *__restrict__ d_n_sel, SelInfo *__restrict__ sel, const uint64_t *__restrict__ cands, const int4 *__restrict__ sw,
                                           const uint64_t *__restrict__ dir_off, const uint32_t *__restrict__ dirs, const int32_t *__restrict__ mode,
                                           const uint64_t *__restrict__ run_off, uint32_t *__restrict__ runs)
{
    __shared__ uint32_t win[(WALK_AHEAD + 1) * 4 * WALK_LANES];
    const uint64_t s = (uint64_t)blockIdx.x * WALK_LANES + threadIdx.x;
    if (s >= *d_n_sel) return;
    SelInfo info = sel[s];
    const uint64_t key = cands[info.cand];
    // the codes cover the full band (64 lanes, mode -1) or the sub-band that starts at lane mode[] (32 lanes): the row of one 16-step
    // block holds 2 dwords per lane
    const int md = mode[info.cand];
    if (md == -2) {
        // settled by the gapless shortcut (gapless_check): sw[] holds score, end cell and the length of the one M run
        const int4 g = sw[info.cand];
        info.iend = g.y; info.jend = g.z; info.istart = g.y - g.w + 1; info.jstart = g.z - g.w + 1;
        info.n_runs = 1; info.aln_len = (uint32_t)g.w;
        runs[run_off[s]] = ((uint32_t)g.w << 2);
        sel[s] = info;
        return;
    }
    const int dlo = key_dlo(key) + (md > 0 ? 2 * md : 0);
    const int row = md < 0 ? 128 : 64;
    const int4 cell = sw[info.cand];
    const int a0 = cell.w;
    // word of (block b, diagonal rel): dword ((b * lanes + (rel >> 1)) * 2 + (rel & 1)) = b * row + rel of this pair's traceback area
    const uint32_t *dir = dirs + dir_off[info.cand] * 128;
    uint32_t *out = runs + run_off[s];

    uint32_t *const wl = win + threadIdx.x * 4;               // this lane's four dwords of row 0; row k lies k * 4 * WALK_LANES dwords on
    info.iend = cell.y; info.jend = cell.z;     // (the trace pass recomputes the same score)
    int i = info.iend, j = info.jend, state = 0;
    int istart = i, jstart = j;
    uint32_t n_runs = 0, aln_len = 0, cur_op = 3, cur_len = 0;
    bool done = false;
    while (!done) {
        // ---- a round: the window around cell (i, j), which is the (m & 7)-th cell of block m >> 3 of diagonal rel
        const int rel0 = j - i - dlo;
        const int top = (i - a0 + (rel0 >> 1)) >> 3;
        if ((unsigned)rel0 >= (unsigned)row || top < 0) break;                  // (no path leaves its band: nothing is read outside the rows)
        const int base = min(max(rel0 - (state == 1 ? 2 : 1), 0), row - 4);     // never in front of the row's first dword or behind its last
        const uint32_t *col = dir + base;
        uint4 v[WALK_AHEAD];
#pragma unroll
        for (int k = 0; k < WALK_AHEAD; ++k) __builtin_memcpy(&v[k], col + (size_t)max(top - k, 0) * row, 16);
#pragma unroll
        for (int k = 0; k < WALK_AHEAD; ++k) {
            uint32_t *r = wl + k * 4 * WALK_LANES;
            r[0] = v[k].x; r[1] = v[k].y; r[2] = v[k].z; r[3] = v[k].w;
        }
        const int have = min(WALK_AHEAD, top + 1);                              // the look-ahead ends at block 0
        // ---- every lane steps until its cell leaves its window.  One trip takes a gap cell, or the diagonal cells from (i, j) on to the end of
        // the NEXT word (two words side by side, one count of leading zeros), without a branch but for the run that has ended
        for (;;) {
            const int rel = j - i - dlo, c = rel - base;
            const int m = i - a0 + (rel >> 1);
            const int k = top - (m >> 3), nidx = m & 7;
            if ((unsigned)c > 3u || (unsigned)k >= (unsigned)have) break;
            const uint32_t *p = wl + k * 4 * WALK_LANES + c;
            const uint32_t w0 = p[0], below = p[4 * WALK_LANES];                // (row WALK_AHEAD exists: read, not used)
            const uint32_t w1 = k + 1 < have ? below : 0u;                      // a zero nibble is no diagonal code: the run stops at the window's end
            const uint32_t nib = (w0 >> (nidx * 4)) & 15u;
            const uint32_t src = nib & 3u;
            const int st = state ? state : (int)src - 1;                        // 0: a diagonal cell, 1 / 2: a cell of a gap (a gap opens in the cell that names it), -1: the start
            // a zero nibble of y = a diagonal code; the cells below (i, j) are shifted to the top and counted at once, never past row 0 / column 0
            const uint64_t x = (((uint64_t)w0 << 32) | w1) << ((7 - nidx) * 4);
            const uint64_t y = (x & 0x3333333333333333ull) ^ 0x1111111111111111ull;
            const int lim = min(i, j);
            const int run = min(y ? (__clzll((long long)y) >> 2) : 16, lim + 1);
            const uint32_t op = st <= 0 ? 0u : 3u - (uint32_t)st, cnt = st == 0 ? (uint32_t)run : (st < 0 ? 0u : 1u);
            aln_len += cnt;
            if (op != cur_op && cnt) {                                          // (the one branch of a trip: a run has ended)
                if (cur_len) out[n_runs++] = (cur_len << 2) | cur_op;
                cur_op = op; cur_len = 0;
            }
            cur_len += cnt;
            istart = st == 0 ? i - run + 1 : istart; jstart = st == 0 ? j - run + 1 : jstart;
            done = st < 0 || (st == 0 && run > lim);                            // the start code, or the last cell of the run lies on row 0 or column 0
            i -= st == 0 ? run : (st == 2 ? 1 : 0);
            j -= st == 0 ? run : (st == 1 ? 1 : 0);
            state = st > 0 && ((nib >> (st + 1)) & 1u) ? st : 0;                // bit 2 / bit 3: the gap goes on
            if (done) break;
        }
    }
    if (cur_len) out[n_runs++] = (cur_len << 2) | cur_op;
    info.istart = istart; info.jstart = jstart; info.n_runs = n_runs; info.aln_len = aln_len;
    sel[s] = info;
}

// identities + filters; FIN_LANES lanes per selected pair, parallel over the columns of each M run (a whole wavefront per pair meant
// 38 k wavefronts that each lived for a chain of dependent loads: 0.039 ms; two pairs per wavefront: 0.031 ms, four: 0.030 ms but
// slower once alignments are long)
// An M run is compared four residues per lane and trip: one unaligned 4-byte load per side (the packed sets carry >= 16 bytes of padding behind
// every sequence, so the last load of a run may reach up to 3 bytes past it), the equal bytes counted as the zero bytes of the XOR, the run's last
// 1 - 3 columns by mask.  One byte per lane and trip was a chain of 11 dependent trips for a 330-column run; this is 3.
// A chore rides along: the union-find behind it (topk_emit unites, pack_out flattens) gets its parent array initialised (iota).
constexpr int FIN_LANES = 32;
__device__ __forceinline__ uint32_t load_u32_unaligned(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__global__ __launch_bounds__(256) void finalize(const uint32_t *__restrict__ d_n_sel, SelInfo *__restrict__ sel, const uint64_t *__restrict__ cands,
                                                const uint8_t *__restrict__ q_res, const uint32_t *__restrict__ q_off, const uint32_t *__restrict__ q_len,
                                                const uint8_t *__restrict__ t_res, const uint32_t *__restrict__ t_off,
                                                const uint64_t *__restrict__ run_off, const uint32_t *__restrict__ runs, double min_id_pct, double min_qcov_pct,
                                                uint32_t *__restrict__ iota, uint32_t n_iota)
{
    for (uint32_t x = blockIdx.x * 256 + threadIdx.x; x < n_iota; x += gridDim.x * 256) iota[x] = x;
    const int lane = threadIdx.x & (FIN_LANES - 1);
    const uint64_t s = (uint64_t)blockIdx.x * (256 / FIN_LANES) + threadIdx.x / FIN_LANES;
    if (s >= *d_n_sel) return;                                // (whole lane groups leave together)
    const SelInfo info = sel[s];
    const uint64_t key = cands[s];                            // (info.cand == s, select_gather: the key, the record and the run slot leave in one round trip)
    const uint32_t q = key_q(key), t = key_t(key);
    const uint8_t *qs = q_res + q_off[q], *ts = t_res + t_off[t];
    const uint32_t *rv = runs + run_off[s];
    const double Lq = (double)q_len[q];
    int i = info.istart, j = info.jstart;
    uint32_t ident = 0;
    for (uint32_t r0 = 0; r0 < info.n_runs; r0 += FIN_LANES) {
        // the next FIN_LANES runs with one load, a run per lane, and handed round by lane shuffles: a load per run put a memory round trip
        // between every two runs of the pair (the walk stored them end -> start)
        const uint32_t nr = min((uint32_t)FIN_LANES, info.n_runs - r0);
        const uint32_t mine = (uint32_t)lane < nr ? rv[info.n_runs - 1 - (r0 + lane)] : 0u;
        for (uint32_t r = 0; r < nr; ++r) {
            const uint32_t run = __shfl(mine, (int)r, FIN_LANES);
            const int len = (int)(run >> 2);
            const uint32_t op = run & 3u;
            if (op == 0) {
                for (int x = lane * 4; x < len; x += FIN_LANES * 4) {
                    const uint32_t d = load_u32_unaligned(qs + i + x) ^ load_u32_unaligned(ts + j + x);
                    uint32_t z = ~(((d & 0x7f7f7f7fu) + 0x7f7f7f7fu) | d | 0x7f7f7f7fu);      // 0x80 in every byte of d that is zero
                    if (len - x < 4) z &= 0x80808080u >> (8 * (4 - (len - x)));               // columns behind the run do not count
                    ident += (uint32_t)__popc(z);
                }
                i += len; j += len;
            } else if (op == 1) i += len;
            else j += len;
        }
    }
    for (int d = FIN_LANES / 2; d > 0; d >>= 1) ident += __shfl_xor(ident, d, 64);
    if (lane == 0) {
        const double idp = (double)ident * 100.0 / (double)info.aln_len;
        const double qcov = (double)(info.iend - info.istart + 1) * 100.0 / Lq;
        sel[s].n_ident = ident;
        sel[s].pass = (idp >= min_id_pct && qcov >= min_qcov_pct) ? 1u : 0u;
    }
}

// hsp_mode 1: two bands of one (q, t) that end in the same cell found the same alignment: keep the higher score, then the
// lower bin (= lower index, sel is ordered by (q, t, bin)); the decision ignores whether the other one survives its filters
__global__ __launch_bounds__(256) void dedupe_bands(const uint32_t *__restrict__ d_n_sel, SelInfo *__restrict__ sel, const uint64_t *__restrict__ cands)
{
    const uint64_t n_sel = *d_n_sel;
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_sel) return;
    const SelInfo me = sel[s];
    const uint64_t g = cands[me.cand] >> 18;
    bool dead = false;
    for (int dir = -1; dir <= 1 && !dead; dir += 2) {
        for (int64_t x = (int64_t)s + dir; x >= 0 && x < (int64_t)n_sel; x += dir) {
            const SelInfo o = sel[x];
            if ((cands[o.cand] >> 18) != g) break;
            if (o.iend == me.iend && o.jend == me.jend && (o.score > me.score || (o.score == me.score && x < (int64_t)s))) { dead = true; break; }
        }
    }
    if (dead) sel[s].pad = 1u;
}

// hsp_mode 2 (BLAST's way with the HSPs of one subject strand, oracle/align_oracle.c align_group): the alignments of a (q, t) group in the order score
// descending, position ascending; one is dropped when an ACCEPTED one in front of it shares its start cell or its end cell, or holds its query range and
// its subject range inside its own.  Order-dependent, so the group's first thread works the group off alone; groups are a handful of bands (a repeat
// family makes dozens).  pad: 0 not looked at yet, 2 accepted (back to 0 at the end), 1 dropped.
__global__ __launch_bounds__(256) void cull_hsps(const uint32_t *__restrict__ d_n_sel, SelInfo *__restrict__ sel, const uint64_t *__restrict__ cands)
{
    const int64_t n_sel = (int64_t)*d_n_sel;
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_sel) return;
    const uint64_t g = cands[sel[s].cand] >> 18;
    if (s > 0 && (cands[sel[s - 1].cand] >> 18) == g) return;
    int64_t e = s + 1;
    while (e < n_sel && (cands[sel[e].cand] >> 18) == g) ++e;
    if (e - s == 1) return;
    for (int64_t it = s; it < e; ++it) {
        int64_t best = -1;
        int32_t best_score = 0;
        for (int64_t x = s; x < e; ++x)
            if (sel[x].pad == 0u && (best < 0 || sel[x].score > best_score)) { best = x; best_score = sel[x].score; }
        const SelInfo me = sel[best];
        bool dead = false;
        for (int64_t y = s; y < e && !dead; ++y) {
            if (sel[y].pad != 2u) continue;
            const SelInfo o = sel[y];
            dead = (o.iend == me.iend && o.jend == me.jend) || (o.istart == me.istart && o.jstart == me.jstart) ||
                   (o.istart <= me.istart && me.iend <= o.iend && o.jstart <= me.jstart && me.jend <= o.jend);
        }
        sel[best].pad = dead ? 1u : 2u;
    }
    for (int64_t x = s; x < e; ++x)
        if (sel[x].pad == 2u) sel[x].pad = 0u;
}

// hsp_mode 2, in front of topk: keep = 1 for the best alignment of its subject among the query's passing alignments of one competition class
// (score descending, position ascending - the order topk ranks in)
__global__ __launch_bounds__(256) void subject_best(const uint32_t *__restrict__ d_n_sel, SelInfo *__restrict__ sel, const uint64_t *__restrict__ cands, int n_splits, uint32_t t_base,
                                                    const uint32_t *__restrict__ t_class, const uint32_t *__restrict__ t_subject)
{
    const int64_t n_sel = (int64_t)*d_n_sel;
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_sel) return;
    const SelInfo me = sel[s];
    uint32_t best = 0;
    if (me.pass) {
        const uint64_t key = cands[me.cand];
        const uint32_t q = key_q(key), t = key_t(key), split = t_class ? t_class[t] : (t + t_base) % (uint32_t)n_splits, sj = t_subject[t];
        best = 1;
        for (int dir = -1; dir <= 1 && best; dir += 2) {
            for (int64_t x = s + dir; x >= 0 && x < n_sel; x += dir) {
                const SelInfo o = sel[x];
                const uint64_t ko = cands[o.cand];
                if (key_q(ko) != q) break;
                const uint32_t to = key_t(ko);
                if (!o.pass || t_subject[to] != sj || (t_class ? t_class[to] : (to + t_base) % (uint32_t)n_splits) != split) continue;
                if (o.score > me.score || (o.score == me.score && x < s)) { best = 0; break; }
            }
        }
    }
    sel[s].keep = best;
}

__global__ __launch_bounds__(256) void apply_dedupe(const uint32_t *__restrict__ d_n_sel, SelInfo *__restrict__ sel)
{
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < *d_n_sel && sel[s].pad) sel[s].pass = 0u;
}

// rank inside (query, target mod n_splits): score desc, target asc, band asc.  sel is ordered by (q, t, bin).
// t_class (optional): competition class of every target = group * n_splits + (index inside the group) % n_splits, so that a
// batch of reference sets (genomes) searched at once ranks exactly as if each had been searched alone
// the top-k decision of selected pair s (me = sel[s], which passed its filters): its rank among the query's passing pairs of its competition class
__device__ __forceinline__ uint32_t topk_keeps(const SelInfo &me, uint64_t s, uint64_t n_sel, const SelInfo *__restrict__ sel, const uint64_t *__restrict__ cands, int top_k, int n_splits,
                                               uint32_t t_base, const uint32_t *__restrict__ t_class, const uint32_t *__restrict__ t_subject)
{
    // (the key of selected pair x is cands[x]: sel[x].cand == x, select_gather - so a neighbour's key and record are two loads side by side, not a chain)
    const uint64_t key = cands[s];
    const uint32_t q = key_q(key), t = key_t(key), split = t_class ? t_class[t] : (t + t_base) % (uint32_t)n_splits;
    uint32_t rank = 0;
    if (t_subject) {
        // hsp_mode 2: top_k counts subjects.  This alignment's subject is as good as its best alignment (subject_best marked it: keep = 1);
        // its rank = the subjects of the same query and class whose best alignment stands in front of that one
        const uint32_t sj = t_subject[t];
        int64_t mine = (int64_t)s;
        int32_t mine_score = me.score;
        if (!me.keep)
            for (int dir = -1; dir <= 1 && mine == (int64_t)s; dir += 2)
                for (int64_t x = (int64_t)s + dir; x >= 0 && x < (int64_t)n_sel; x += dir) {
                    const SelInfo o = sel[x];
                    const uint64_t ko = cands[x];
                    if (key_q(ko) != q) break;
                    const uint32_t to = key_t(ko);
                    if (o.pass && o.keep && t_subject[to] == sj && (t_class ? t_class[to] : (to + t_base) % (uint32_t)n_splits) == split) { mine = x; mine_score = o.score; break; }
                }
        for (int dir = -1; dir <= 1; dir += 2) {
            for (int64_t x = (int64_t)s + dir; x >= 0 && x < (int64_t)n_sel; x += dir) {
                const SelInfo o = sel[x];
                const uint64_t ko = cands[x];
                if (key_q(ko) != q) break;
                const uint32_t to = key_t(ko);
                if (!o.pass || !o.keep || t_subject[to] == sj || (t_class ? t_class[to] : (to + t_base) % (uint32_t)n_splits) != split) continue;
                if (o.score > mine_score || (o.score == mine_score && x < mine)) ++rank;
            }
        }
    } else
    for (int dir = -1; dir <= 1; dir += 2) {
        for (int64_t x = (int64_t)s + dir; x >= 0 && x < (int64_t)n_sel; x += dir) {
            const SelInfo o = sel[x];
            const uint64_t ko = cands[x];
            if (key_q(ko) != q) break;
            const uint32_t to = key_t(ko);
            if (!o.pass || (t_class ? t_class[to] : (to + t_base) % (uint32_t)n_splits) != split) continue;
            if (o.score > me.score || (o.score == me.score && (to < t || (to == t && x < (int64_t)s)))) ++rank;
        }
    }
    return rank < (uint32_t)top_k ? 1u : 0u;
}

__global__ __launch_bounds__(256) void topk(const uint32_t *__restrict__ d_n_sel, SelInfo *__restrict__ sel, const uint64_t *__restrict__ cands, int top_k, int n_splits, uint32_t t_base,
                                            const uint32_t *__restrict__ t_class, uint32_t *__restrict__ keep_flag, uint32_t *__restrict__ hit_pos, uint64_t *__restrict__ cig_pos,
                                            const unsigned long long *__restrict__ score_hdr, const unsigned long long *__restrict__ trace_hdr, unsigned long long *__restrict__ mail,
                                            SelectState st, const uint32_t *__restrict__ t_subject = nullptr)
{
    // top-k decision per selected pair AND the two compactions behind it (slot of the hit record, slot of its CIGAR runs) in one launch:
    // the tile scans (kept, runs of the kept) and finds the totals in front of it by look-back (lookback.h)
    __shared__ uint32_t s_tile, lds32[4];
    __shared__ uint64_t lds64[4], s_pre[2];
    const uint32_t tile = lb_take_tile(st.count.state, st.count.ticket_base, &s_tile);
    const uint64_t n_sel = *d_n_sel;
    const uint64_t s = (uint64_t)tile * 256 + threadIdx.x;
    if (s == 0) {
        // the totals of the two Smith-Waterman passes into the block the host reads with its last synchronisation (one copy for everything)
        mail[4] = score_hdr[0]; mail[5] = score_hdr[1];
        mail[6] = trace_hdr ? trace_hdr[0] : 0ull; mail[7] = trace_hdr ? trace_hdr[1] : 0ull; mail[8] = trace_hdr ? trace_hdr[5] : 0ull;
        mail[9] = score_hdr[6];                                                  // cells of the candidates the score pass settled without a sweep,
        reinterpret_cast<uint32_t *>(mail)[3] = (uint32_t)score_hdr[7];          // their number
    }
    uint32_t keep = 0;
    uint64_t n_runs = 0;
    if (s < n_sel) {
        const SelInfo me = sel[s];
        if (me.pass) keep = topk_keeps(me, s, n_sel, sel, cands, top_k, n_splits, t_base, t_class, t_subject);
        n_runs = keep ? me.n_runs : 0;
    }
    uint32_t tot_k;
    uint64_t tot_r;
    const uint32_t ex_k = block_excl_scan_256<uint32_t>(keep, &tot_k, lds32);
    const uint64_t ex_r = block_excl_scan_256<uint64_t>(n_runs, &tot_r, lds64);
    if (threadIdx.x < 64) {
        const uint64_t p0 = lb_tile_prefix<32>(st.count.status(), tile, tot_k, st.count.epoch, (int)threadIdx.x);
        const uint64_t p1 = lb_tile_prefix<48>(st.runs.status(), tile, tot_r, st.runs.epoch, (int)threadIdx.x);
        if (threadIdx.x == 0) { s_pre[0] = p0; s_pre[1] = p1; }
    }
    __syncthreads();
    if (s < n_sel) {
        keep_flag[s] = keep;
        hit_pos[s] = (uint32_t)(s_pre[0] + ex_k);
        cig_pos[s] = s_pre[1] + ex_r;
    }
    if (tile == gridDim.x - 1 && threadIdx.x == 255) {          // the last tile: number of hits, number of their CIGAR runs
        reinterpret_cast<uint32_t *>(mail)[2] = (uint32_t)(s_pre[0] + tot_k);
        mail[2] = s_pre[1] + tot_r;
    }
}

__global__ __launch_bounds__(256) void emit(const uint32_t *__restrict__ d_n_sel, const SelInfo *__restrict__ sel, const uint64_t *__restrict__ cands,
                                            const uint32_t *__restrict__ keep_flag, const uint32_t *__restrict__ hit_pos, const uint64_t *__restrict__ cig_pos,
                                            const uint64_t *__restrict__ run_off, const uint32_t *__restrict__ runs, const uint32_t *__restrict__ nblk,
                                            const uint32_t *__restrict__ q_len, const uint32_t *__restrict__ t_len,
                                            pep_hit *__restrict__ hits, uint32_t *__restrict__ cigar,
                                            const unsigned long long *__restrict__ mail = nullptr, unsigned long long *__restrict__ mail_copy = nullptr)
{
    const int lane = threadIdx.x & 63;
    const uint64_t s = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    // the counter block of the stage (final since topk) once more, outside the search's zeroed region: pack_out and K10 read it there, so that
    // pack_out may clear that region for the next search
    if (mail_copy && blockIdx.x == 0 && threadIdx.x < 10) mail_copy[threadIdx.x] = mail[threadIdx.x];
    if (s >= *d_n_sel || !keep_flag[s]) return;
    const SelInfo info = sel[s];
    const uint64_t key = cands[info.cand];
    const uint64_t co = cig_pos[s];
    const uint32_t *rv = runs + run_off[s];
    for (uint32_t r = lane; r < info.n_runs; r += 64) cigar[co + r] = rv[info.n_runs - 1 - r];
    // exact in-band in-matrix cell count of the winning band: the 128 diagonals are spread over the lanes
    const uint32_t q = key_q(key), t = key_t(key);
    const int dlo = key_dlo(key), Lq = (int)q_len[q], Lt = (int)t_len[t];
    const int dl = max(dlo, -(Lq - 1)), dh = min(dlo + 127, Lt - 1);
    unsigned long long cells = 0;
    for (int d = dl + lane; d <= dh; d += 64) cells += (unsigned long long)(min(Lq - 1, Lt - 1 - d) - max(0, -d) + 1);
    for (int x = 32; x > 0; x >>= 1) cells += __shfl_xor(cells, x, 64);
    if (lane == 0) {
        pep_hit h;
        h.q = q; h.t = t;
        h.q_start = (uint32_t)info.istart + 1; h.q_end = (uint32_t)info.iend + 1;
        h.t_start = (uint32_t)info.jstart + 1; h.t_end = (uint32_t)info.jend + 1;
        h.score = info.score; h.n_ident = info.n_ident; h.aln_len = info.aln_len; h.nm = info.aln_len - info.n_ident;
        h.cigar_runs = info.n_runs; h.bin = (int32_t)(key & ((1u << 18) - 1)); h.cigar_off = co;
        h.cells = cells;
        hits[hit_pos[s]] = h;
    }
    (void)nblk;
}

// topk and emit in ONE launch, for the result that leaves through pack_out.  After its look-back a tile knows where its kept hits go: a
// contiguous range of the hit table and a contiguous range of the arena.  So it writes them itself instead of handing keep flag, hit slot
// and CIGAR slot of every pair to a wavefront-per-pair launch through global memory:
//  - the owner of a kept hit builds the 64-byte record in LDS (cells: pep_band_cells, one thread instead of a wavefront's loop over the 128
//    diagonals); the tile writes its records out 16 bytes per lane;
//  - the tile's runs are copied by all threads, one run of the tile's arena range per thread and trip: the hit a run belongs to is found by
//    bisection over the tile's scanned run counts in LDS (9 steps).  Pair by pair with lanes over runs would be a chain of up to 256 dependent
//    round trips per tile for hits of 4 - 5 runs; this way every trip has 256 independent copies in flight, and a hit with more runs than the
//    tile has threads is nothing special.  Reversed as emit does (the walk stored them end -> start);
//  - the owner of a kept hit unites (q + q_base, node of t) where single linkage follows (parent != nullptr; finalize has set the parents);
//  - the last tile writes the stage's counter block, complete, to mail_copy (outside the region pack_out clears).
// The arena range of one tile is counted in 32 bits: the path is taken only below FAST_RUN_BYTES, 2^29 runs for the whole search.
__global__ __launch_bounds__(256) void topk_emit(const uint32_t *__restrict__ d_n_sel, const SelInfo *__restrict__ sel, const uint64_t *__restrict__ cands, int top_k, int n_splits,
                                                 uint32_t t_base, const uint32_t *__restrict__ t_class, const uint32_t *__restrict__ t_subject,
                                                 const uint64_t *__restrict__ run_off, const uint32_t *__restrict__ runs, const uint32_t *__restrict__ q_len,
                                                 const uint32_t *__restrict__ t_len, pep_hit *__restrict__ hits, uint32_t *__restrict__ cigar,
                                                 const unsigned long long *__restrict__ score_hdr, const unsigned long long *__restrict__ trace_hdr,
                                                 const unsigned long long *__restrict__ mail, unsigned long long *__restrict__ mail_copy,
                                                 uint32_t *parent, uint32_t q_base, const uint32_t *__restrict__ node_of_target, SelectState st)
{
    static_assert(sizeof(pep_hit) == 64, "four 16-byte pieces per record");
    __shared__ uint32_t s_tile, lds32[4];
    __shared__ uint64_t lds64[4], s_pre[2];
    __shared__ uint4 s_rec[256 * 4];             // the records of the tile's kept hits, in hit order
    __shared__ uint64_t s_src[256];              // kept hit k: its first run in `runs` (the walk's order)
    __shared__ uint32_t s_first[257];            // kept hit k: its first run in the tile's arena range; [kept hits] = the tile's runs
    const uint32_t tile = lb_take_tile(st.count.state, st.count.ticket_base, &s_tile);
    const uint64_t n_sel = *d_n_sel;
    const uint64_t s = (uint64_t)tile * 256 + threadIdx.x;
    uint32_t keep = 0;
    uint64_t n_runs = 0;
    SelInfo me = {};
    if (s < n_sel) {
        me = sel[s];
        if (me.pass) keep = topk_keeps(me, s, n_sel, sel, cands, top_k, n_splits, t_base, t_class, t_subject);
        n_runs = keep ? me.n_runs : 0;
    }
    uint32_t tot_k;
    uint64_t tot_r;
    const uint32_t ex_k = block_excl_scan_256<uint32_t>(keep, &tot_k, lds32);
    const uint64_t ex_r = block_excl_scan_256<uint64_t>(n_runs, &tot_r, lds64);
    if (threadIdx.x < 64) {
        const uint64_t p0 = lb_tile_prefix<32>(st.count.status(), tile, tot_k, st.count.epoch, (int)threadIdx.x);
        const uint64_t p1 = lb_tile_prefix<48>(st.runs.status(), tile, tot_r, st.runs.epoch, (int)threadIdx.x);
        if (threadIdx.x == 0) { s_pre[0] = p0; s_pre[1] = p1; }
    }
    __syncthreads();
    const uint64_t hit0 = s_pre[0], run0 = s_pre[1];
    uint32_t node_q = 0, node_t = 0;
    if (keep) {
        const uint64_t key = cands[s];                    // (me.cand == s, select_gather)
        const uint32_t q = key_q(key), t = key_t(key);
        pep_hit h;
        h.q = q; h.t = t;
        h.q_start = (uint32_t)me.istart + 1; h.q_end = (uint32_t)me.iend + 1;
        h.t_start = (uint32_t)me.jstart + 1; h.t_end = (uint32_t)me.jend + 1;
        h.score = me.score; h.n_ident = me.n_ident; h.aln_len = me.aln_len; h.nm = me.aln_len - me.n_ident;
        h.cigar_runs = me.n_runs; h.bin = (int32_t)(key & ((1u << 18) - 1)); h.cigar_off = run0 + ex_r;
        h.cells = pep_band_cells((int)q_len[q], (int)t_len[t], key_dlo(key));
        uint4 piece[4];
        __builtin_memcpy(piece, &h, sizeof(h));
#pragma unroll
        for (int x = 0; x < 4; ++x) s_rec[ex_k * 4 + x] = piece[x];
        s_src[ex_k] = run_off[s];
        s_first[ex_k] = (uint32_t)ex_r;
        if (parent) { node_q = q + q_base; node_t = node_of_target[t]; }
    }
    if (threadIdx.x == 0) s_first[tot_k] = (uint32_t)tot_r;
    __syncthreads();
    uint4 *hdst = reinterpret_cast<uint4 *>(hits + hit0);
    for (uint32_t x = threadIdx.x; x < tot_k * 4; x += 256) hdst[x] = s_rec[x];
    uint32_t *cdst = cigar + run0;
    const uint32_t n_tile_runs = (uint32_t)tot_r;
    for (uint32_t x0 = threadIdx.x; x0 < n_tile_runs; x0 += 4 * 256) {      // four copies per thread in flight
        uint32_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t x = x0 + u * 256;
            v[u] = 0;
            if (x < n_tile_runs) {
                uint32_t lo = 0, hi = tot_k;                                 // s_first[lo] <= x < s_first[hi]: the last hit that starts at or in front of x
                while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (s_first[mid] <= x) lo = mid; else hi = mid; }
                const uint32_t first = s_first[lo], n = s_first[lo + 1] - first;
                v[u] = runs[s_src[lo] + (n - 1 - (x - first))];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t x = x0 + u * 256;
            if (x < n_tile_runs) cdst[x] = v[u];
        }
    }
    if (keep && parent) uf_unite(parent, node_q, node_t);
    if (tile == gridDim.x - 1 && threadIdx.x == 255) {
        // the counter block the host reads with its last synchronisation (HostMail): the pair counts and the run capacity as select_gather left them,
        // the hits and their CIGAR runs, the totals of the two Smith-Waterman passes
        mail_copy[0] = mail[0];
        mail_copy[1] = (unsigned long long)(uint32_t)(hit0 + tot_k) | ((unsigned long long)(uint32_t)score_hdr[7] << 32);      // hits, candidates the score pass settled without a sweep
        mail_copy[2] = run0 + tot_r;
        mail_copy[3] = mail[3];
        mail_copy[4] = score_hdr[0]; mail_copy[5] = score_hdr[1];
        mail_copy[6] = trace_hdr ? trace_hdr[0] : 0ull; mail_copy[7] = trace_hdr ? trace_hdr[1] : 0ull; mail_copy[8] = trace_hdr ? trace_hdr[5] : 0ull;
        mail_copy[9] = score_hdr[6];                                         // cells of the settled candidates
    }
}

// The result on its way to the host WITHOUT the host knowing its size: the counter block (72 bytes: hits, CIGAR runs, statistics), the
// hit records and the CIGAR arena are written into the context's pinned staging area by this kernel - header (PACK_HEADER bytes), hits,
// arena back to back - so that the search needs no synchronisation between its candidate count and its end.  A staging area that is too
// small (the first search of a context, a result that grew) gets the header only, with the overflow word set: the host then sizes it
// and copies the classic way.
constexpr size_t PACK_HEADER = 128;
// Two chores ride along (a launch of their own costs 4 - 5 us each): the counters of the NEXT search are cleared (zero_words: the region every
// search needs zeroed - this is its last reader), and single linkage ends here: every union of topk_emit is complete when this launch begins, so
// the label of every node (its root) goes straight into the pinned label array (the body of uf_flatten; n_nodes = 0: no grouping).
__global__ __launch_bounds__(256) void pack_out(const unsigned long long *__restrict__ mail, const pep_hit *__restrict__ hits, const uint32_t *__restrict__ cigar,
                                                unsigned char *__restrict__ pinned, unsigned long long cap, uint32_t *__restrict__ zero_words, uint32_t n_zero_words,
                                                uint32_t *parent, uint32_t *__restrict__ label, uint32_t n_nodes)
{
    for (uint32_t x = blockIdx.x * 256 + threadIdx.x; x < n_zero_words; x += gridDim.x * 256) zero_words[x] = 0u;
    for (uint32_t x = blockIdx.x * 256 + threadIdx.x; x < n_nodes; x += gridDim.x * 256) label[x] = uf_root(parent, x);
    const uint32_t n_hits = reinterpret_cast<const uint32_t *>(mail)[2];
    const unsigned long long n_cig = mail[2];
    const bool fits = PACK_HEADER + (unsigned long long)n_hits * sizeof(pep_hit) + n_cig * 4 <= cap;
    unsigned long long *head = reinterpret_cast<unsigned long long *>(pinned);
    if (blockIdx.x == 0 && threadIdx.x < 16) head[threadIdx.x] = threadIdx.x < 10 ? mail[threadIdx.x] : (threadIdx.x == 15 ? (fits ? 0ull : 1ull) : 0ull);
    if (!fits) return;
    const uint64_t stride = (uint64_t)gridDim.x * 256, t0 = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint4 *src = reinterpret_cast<const uint4 *>(hits);
    uint4 *dst = reinterpret_cast<uint4 *>(pinned + PACK_HEADER);
    for (uint64_t x = t0; x < (uint64_t)n_hits * (sizeof(pep_hit) / 16); x += stride) dst[x] = src[x];
    uint32_t *cdst = reinterpret_cast<uint32_t *>(pinned + PACK_HEADER + (size_t)n_hits * sizeof(pep_hit));
    for (uint64_t x = t0; x < n_cig; x += stride) cdst[x] = cigar[x];
}

}  // namespace

// Workspace slots: PepWsSlot (common.h); the small counters come from pep_zero_block.
//
// Host round trips.  Between the seed stage's count of candidates and the sizes of the result (hits, CIGAR runs) the host does not need
// to see anything: the number of selected pairs stays on the device (every kernel behind the selection reads it there and is launched on
// a grid sized for all n candidates), the traceback area and the run arena are sized from upper bounds (every candidate selected, every
// pair as long as the longest), and the statistics ride on the one read-back at the end.  When those bounds would cost more memory than
// is sensible (FAST_DIR_BYTES / FAST_RUN_BYTES: long sequences times many candidates - searches that are long enough not to care about
// two host round trips), or with params.reserved2 = 1 (tests), the stage synchronises after the selection and sizes everything exactly.
struct HostMail { uint32_t n_pairs, n_sel, n_hits, n_settled; unsigned long long n_cig, run_cap, score_cells, score_blocks, trace_cells, trace_blocks, trace_swept, settled_cells; };
static_assert(sizeof(HostMail) == 80, "layout of the selection stage's counter block");

// the host's half of a search whose result left through pack_out: sizes, statistics and the views of the staging area - called once the
// stream has been waited for (by pep_search behind its one final wait, or by pep_extend itself when the caller wants the result at once)
int pep_extend_finish(pep_ctx *ctx)
{
    if (!ctx->ext.pending) return PEP_OK;
    ctx->ext.pending = false;
    pep_result *res = ctx->ext.res;
    HostMail h;
    std::memcpy(&h, ctx->pin_stage.p, sizeof(h));
    const bool overflow = reinterpret_cast<const unsigned long long *>(ctx->pin_stage.p)[15] != 0;
    ctx->stats.cells += h.score_cells;
    ctx->stats.cells_swept += h.score_blocks * 16 * 64;
    ctx->stats.candidates_settled += h.n_settled;
    ctx->stats.cells_settled += h.settled_cells;
    ctx->stats.cells_trace += h.trace_cells;
    ctx->stats.cells_swept_trace += h.trace_blocks * 16 * 64;
    ctx->stats.dir_bytes += h.trace_blocks * 512;
    ctx->trace_swept = h.trace_swept;
    ctx->stats.tracebacks_gapless = h.n_sel - h.trace_swept;
    ctx->stats.pairs = h.n_pairs;
    ctx->stats.tracebacks = h.n_sel;
    ctx->stats.hits = h.n_hits;
    if (h.n_hits == 0) return PEP_OK;
    const size_t hb = (size_t)h.n_hits * sizeof(pep_hit);
    const pep_hit *d_hits = reinterpret_cast<const pep_hit *>(ctx->ext.d_hits);
    const uint32_t *d_cig = reinterpret_cast<const uint32_t *>(ctx->ext.d_cig);
    if (!overflow) {
        res->st_hits = reinterpret_cast<const pep_hit *>(ctx->pin_stage.p + PACK_HEADER);
        res->st_cigar = reinterpret_cast<const uint32_t *>(ctx->pin_stage.p + PACK_HEADER + hb);
    } else if (pin_reserve(ctx, ctx->pin_stage, PACK_HEADER + hb + (h.n_cig + 1) * 4) == PEP_OK) {
        // the staging area was too small for this result (now it is not: the next search of this size goes through pack_out)
        PEP_HIP(ctx, hipMemcpyAsync(ctx->pin_stage.p + PACK_HEADER, d_hits, hb, hipMemcpyDeviceToHost, ctx->stream));
        if (h.n_cig) PEP_HIP(ctx, hipMemcpyAsync(ctx->pin_stage.p + PACK_HEADER + hb, d_cig, h.n_cig * 4, hipMemcpyDeviceToHost, ctx->stream));
        PEP_HIP(ctx, pep_stream_wait(ctx));
        res->st_hits = reinterpret_cast<const pep_hit *>(ctx->pin_stage.p + PACK_HEADER);
        res->st_cigar = reinterpret_cast<const uint32_t *>(ctx->pin_stage.p + PACK_HEADER + hb);
    } else {
        res->hits.resize(h.n_hits);
        res->cigar.resize(h.n_cig);
        PEP_HIP(ctx, hipMemcpyAsync(res->hits.data(), d_hits, hb, hipMemcpyDeviceToHost, ctx->stream));
        if (h.n_cig) PEP_HIP(ctx, hipMemcpyAsync(res->cigar.data(), d_cig, h.n_cig * 4, hipMemcpyDeviceToHost, ctx->stream));
        PEP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    res->n_hits = h.n_hits; res->n_cigar = h.n_cig;
    res->d_hits = d_hits; res->d_cigar = d_cig;
    return PEP_OK;
}

int pep_extend(pep_ctx *ctx, const uint64_t *d_cands, uint64_t n, const int32_t *h_min_score, pep_result *res, bool defer, bool group)
{
    const pep_search_params &P = ctx->params;
    pep_drop_dev_result(ctx);                     // PEP_WS_HITS_OUT is about to be rewritten
    res->hits.clear();
    res->cigar.clear();
    ctx->stats.candidates = n;
    ctx->stats.pairs = ctx->stats.tracebacks = ctx->stats.hits = 0;
    ctx->stats.cells = ctx->stats.cells_swept = ctx->stats.dir_bytes = 0;
    ctx->stats.candidates_settled = ctx->stats.cells_settled = 0;
    if (n == 0) return PEP_OK;
    hipStream_t st = ctx->stream;
    // ---- pass 1: score-only banded SW over every candidate
    // per-query score thresholds: uploaded from pinned memory BEFORE the score pass is queued (a copy from pageable memory makes the
    // host wait for everything queued ahead of it - behind the score pass that was the whole pass)
    DevBuf &dms = ctx->d_min_score;
    if (h_min_score) {                            // (nullptr: the caller has uploaded them already)
        PEP_TRY(dev_reserve(ctx, dms, (size_t)(ctx->q.n + 1) * 4));
        PEP_TRY(pin_reserve(ctx, ctx->pin_ms, (size_t)(ctx->q.n + 1) * 4));
        std::memcpy(ctx->pin_ms.p, h_min_score, (size_t)ctx->q.n * 4);
        PEP_HIP(ctx, hipMemcpyAsync(dms.p, ctx->pin_ms.p, (size_t)ctx->q.n * 4, hipMemcpyHostToDevice, st));
    }
    unsigned long long *score_hdr = nullptr, *trace_hdr = nullptr;
    PEP_TRY(pep_sw_run(ctx, d_cands, n, false, nullptr, nullptr, nullptr, nullptr, 0, &score_hdr));      // (the pass times come from the context's phase timers, read after the search)

    pep_timer_begin(ctx, TM_TRACE);

    const int4 *sw = ctx->ws[PEP_WS_SW_OUT].as<const int4>();
    // the block the host reads: u32 [0] (q, t) pairs, [1] selected pairs, [2] hits; u64 [2] CIGAR runs of the hits, [3] run capacity of the selected
    // pairs, [4] [5] cells / 16-step blocks of the score pass, [6] [7] [8] cells / blocks / swept pairs of the traceback pass
    void *zb = nullptr;
    PEP_TRY(pep_zero_block(ctx, PEP_ZC_SELECT, PEP_ZERO_SELECT, 256, &zb));
    uint32_t *counters = reinterpret_cast<uint32_t *>(zb);
    unsigned long long *mail = reinterpret_cast<unsigned long long *>(zb);
    const uint32_t *d_n_sel = counters + 1;
    HostMail h_mail;
    std::memset(&h_mail, 0, sizeof(h_mail));
    ctx->ext.pending = ctx->ext.grouped = false;
    const unsigned gb = (unsigned)ceil_div(n, 256);
    // selection, compaction and the run slots of the selected pairs in one launch (select_gather); the arrays of the selected pairs are laid
    // out for n entries (every candidate selected) whatever the count turns out to be
    PEP_TRY(dev_reserve(ctx, ctx->ws[PEP_WS_SEL], (size_t)n * sizeof(SelInfo)));
    PEP_TRY(dev_reserve(ctx, ctx->ws[PEP_WS_SEL_RUNS_KEYS], ((size_t)n + 2) * 8 * 2));
    PEP_TRY(dev_reserve(ctx, ctx->ws[PEP_WS_TRACE_KNOWN], ((size_t)n + 2) * 4 * 2));
    int32_t *known = ctx->ws[PEP_WS_TRACE_KNOWN].as<int32_t>(), *end_lane = known + n + 2;
    SelInfo *sel = ctx->ws[PEP_WS_SEL].as<SelInfo>();
    uint64_t *run_off = ctx->ws[PEP_WS_SEL_RUNS_KEYS].as<uint64_t>(), *sel_keys = run_off + n + 2;
    {
        SelectState ss;
        PEP_TRY(begin_select(ctx, PEP_LB_SELECT_COUNT, PEP_LB_SELECT_RUNS, gb, &ss));
        hipLaunchKernelGGL(select_gather, dim3(gb), dim3(256), 0, st, d_cands, n, sw, dms.as<const int32_t>(), P.hsp_mode, ctx->q.len.as<const uint32_t>(),
                           ctx->t.len.as<const uint32_t>(), sel, run_off, sel_keys, known, end_lane, counters, mail + 3, ss);
    }
    // upper bounds for the buffers of the traceback stage
    constexpr uint64_t FAST_DIR_BYTES = 8ull << 30, FAST_RUN_BYTES = 2ull << 30;
    const uint64_t max_blk = ((uint64_t)ctx->q.max_len + ctx->t.max_len) / 16 + 3;
    const uint64_t dir_blocks_bound = n * max_blk, run_bound = n * (2ull * std::min(ctx->q.max_len, ctx->t.max_len) + 2);
    const bool fast = (P.reserved2 & 1) == 0 && dir_blocks_bound * 512 <= FAST_DIR_BYTES && run_bound * 4 <= FAST_RUN_BYTES;
    uint64_t n_b = n;                            // what the buffers and grids behind the selection are sized for
    if (!fast) {
        PEP_TRY(pep_read_back(ctx, &h_mail, mail, 8));
        PEP_TRY(pep_sync_reads(ctx));
        n_b = h_mail.n_sel;
    }
    uint32_t n_hits = 0;
    uint64_t n_cig = 0;
    uint64_t *cig_pos = nullptr;
    uint32_t *runs = nullptr, *keep_flag = nullptr, *hit_pos = nullptr;
    if (n_b) {
        uint64_t total_runs = run_bound;
        if (!fast) PEP_TRY(pep_read_back(ctx, &total_runs, mail + 3, 8));         // arrives with the synchronisation inside pep_sw_run (block total)
        // ---- rule 5a: pairs whose alignment is one ungapped run are settled without a sweep (the score-pass results in PEP_WS_SW_OUT have been
        // consumed by gather_sel: the slots of the selected pairs are written from here on)
        PEP_TRY(dev_reserve(ctx, ctx->d_trace_mode, ((size_t)n_b + 1) * sizeof(int32_t)));
        PEP_TRY(pep_upload_sub_table(ctx));                                 // (K9 drives this stage without the seed stage in front)
        hipLaunchKernelGGL(gapless_check, dim3((unsigned)ceil_div(n_b, 4)), dim3(256), 0, st, d_n_sel, (const uint64_t *)sel_keys, (const int32_t *)known,
                           (const int32_t *)end_lane, ctx->q.res.as<const uint8_t>(), ctx->q.off.as<const uint32_t>(), ctx->q.len.as<const uint32_t>(),
                           ctx->t.res.as<const uint8_t>(), ctx->t.off.as<const uint32_t>(), ctx->t.len.as<const uint32_t>(), ctx->d_params.as<const int8_t>(),
                           ctx->ws[PEP_WS_SW_OUT].as<int4>(), ctx->d_trace_mode.as<int32_t>());
        // ---- pass 2: the same DP with traceback codes, the remaining selected pairs only
        PEP_TRY(pep_sw_run(ctx, sel_keys, n_b, true, known, end_lane, ctx->d_trace_mode.as<const int32_t>(), d_n_sel, fast ? dir_blocks_bound : 0, &trace_hdr));
        const int4 *sw2 = ctx->ws[PEP_WS_SW_OUT].as<const int4>();
        PEP_TRY(dev_reserve(ctx, ctx->ws[PEP_WS_RUNS], (total_runs + 1) * 4));
        runs = ctx->ws[PEP_WS_RUNS].as<uint32_t>();
        const unsigned gfin = (unsigned)ceil_div(n_b, 256 / FIN_LANES);
        // the result leaves through topk_emit and pack_out: no look at the sizes, no synchronisation behind the selection
        const bool packed = fast && !ctx->device_results && pin_reserve(ctx, ctx->pin_stage, PACK_HEADER) == PEP_OK;
        // ... and single linkage (pep_set_grouping) rides along: parents in finalize, unions in topk_emit, labels in pack_out.  Only with a node map
        // that covers this search's queries and targets - pep_k10_queue refuses the others, and nothing may be united out of bounds before it does
        uint32_t *parent = nullptr, *labels = nullptr;
        if (packed && group && ctx->grp_nodes && ctx->uf_nodes_host.size() >= ctx->t.n && (uint64_t)ctx->q.n + ctx->grp_q_base <= ctx->grp_nodes &&
            pin_reserve(ctx, ctx->pin_labels, (size_t)ctx->grp_nodes * 4) == PEP_OK) {
            PEP_TRY(dev_reserve(ctx, ctx->ws[PEP_WS_UF_PARENT], (size_t)ctx->grp_nodes * 4));
            parent = ctx->ws[PEP_WS_UF_PARENT].as<uint32_t>();
            labels = reinterpret_cast<uint32_t *>(ctx->pin_labels.p);
        }
        const uint32_t n_nodes = parent ? ctx->grp_nodes : 0u;
        hipLaunchKernelGGL(walk, dim3((unsigned)ceil_div(n_b, WALK_LANES)), dim3(WALK_LANES), 0, st, d_n_sel, sel, (const uint64_t *)sel_keys, sw2, ctx->ws[PEP_WS_SW_DIR_OFF].as<const uint64_t>(),
                           ctx->ws[PEP_WS_TRACE_DIRS].as<const uint32_t>(), ctx->d_trace_mode.as<const int32_t>(), (const uint64_t *)run_off, runs);
        hipLaunchKernelGGL(finalize, dim3(gfin), dim3(256), 0, st, d_n_sel, sel, (const uint64_t *)sel_keys, ctx->q.res.as<const uint8_t>(),
                           ctx->q.off.as<const uint32_t>(), ctx->q.len.as<const uint32_t>(), ctx->t.res.as<const uint8_t>(),
                           ctx->t.off.as<const uint32_t>(), (const uint64_t *)run_off, (const uint32_t *)runs, P.min_id_pct, P.min_qcov_pct, parent, n_nodes);
        const uint32_t *t_subject = nullptr;
        if (P.hsp_mode == 1) {
            hipLaunchKernelGGL(dedupe_bands, dim3((unsigned)ceil_div(n_b, 256)), dim3(256), 0, st, d_n_sel, sel, (const uint64_t *)sel_keys);
            hipLaunchKernelGGL(apply_dedupe, dim3((unsigned)ceil_div(n_b, 256)), dim3(256), 0, st, d_n_sel, sel);
        } else if (P.hsp_mode == 2) {
            hipLaunchKernelGGL(cull_hsps, dim3((unsigned)ceil_div(n_b, 256)), dim3(256), 0, st, d_n_sel, sel, (const uint64_t *)sel_keys);
            hipLaunchKernelGGL(apply_dedupe, dim3((unsigned)ceil_div(n_b, 256)), dim3(256), 0, st, d_n_sel, sel);
            // the subject of every target: the reference sequence it is a strand / frame / chunk of (K1's table)
            PEP_TRY(pep_k1_host_tables(ctx, PEP_SIDE_T));
            if (ctx->t_meta.size() != ctx->t.n) return pep_fail(ctx, PEP_ERR_STATE, "hsp_mode 2 needs the targets' sequence table (targets made by pep_translate / pep_use_nt_as_residues)");
            std::vector<uint32_t> subj(ctx->t.n + 1, 0u);
            for (uint32_t t = 0; t < ctx->t.n; ++t) subj[t] = ctx->t_meta[t].seq;
            PEP_TRY(dev_reserve(ctx, ctx->d_t_subject, ((size_t)ctx->t.n + 1) * 4));
            PEP_TRY(pep_h2d(ctx, ctx->d_t_subject.p, subj.data(), ((size_t)ctx->t.n + 1) * 4));
            t_subject = ctx->d_t_subject.as<const uint32_t>();
            hipLaunchKernelGGL(subject_best, dim3((unsigned)ceil_div(n_b, 256)), dim3(256), 0, st, d_n_sel, sel, (const uint64_t *)sel_keys, P.n_splits, (uint32_t)(P.t_index_base % P.n_splits),
                               ctx->t_class_ready ? ctx->d_t_class.as<const uint32_t>() : (const uint32_t *)nullptr, t_subject);
        }
        const uint32_t t_base = (uint32_t)(P.t_index_base % P.n_splits);
        const uint32_t *t_class = ctx->t_class_ready ? ctx->d_t_class.as<const uint32_t>() : (const uint32_t *)nullptr;
        SelectState ts;
        const uint64_t tiles = ceil_div(n_b, 256);
        if (packed) {
            // top-k, compaction and the table itself in one launch; output buffers from the same upper bounds as everything behind the selection
            const size_t hb_bound = (size_t)n_b * sizeof(pep_hit);
            PEP_TRY(dev_reserve(ctx, ctx->ws[PEP_WS_HITS_OUT], hb_bound + (run_bound + 1) * 4));
            pep_hit *d_hits = ctx->ws[PEP_WS_HITS_OUT].as<pep_hit>();
            uint32_t *d_cig = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(ctx->ws[PEP_WS_HITS_OUT].p) + hb_bound);
            PEP_TRY(dev_reserve(ctx, ctx->d_mail_copy, 128));
            unsigned long long *mail_copy = ctx->d_mail_copy.as<unsigned long long>();
            PEP_TRY(begin_select(ctx, PEP_LB_TOPK_HITS, PEP_LB_TOPK_RUNS, tiles, &ts));
            hipLaunchKernelGGL(topk_emit, dim3((unsigned)tiles), dim3(256), 0, st, d_n_sel, (const SelInfo *)sel, (const uint64_t *)sel_keys, P.top_k, P.n_splits, t_base, t_class, t_subject,
                               (const uint64_t *)run_off, (const uint32_t *)runs, ctx->q.len.as<const uint32_t>(), ctx->t.len.as<const uint32_t>(), d_hits, d_cig,
                               (const unsigned long long *)score_hdr, (const unsigned long long *)trace_hdr, (const unsigned long long *)mail, mail_copy,
                               parent, ctx->grp_q_base, ctx->uf_nodes.as<const uint32_t>(), ts);
            hipLaunchKernelGGL(pack_out, dim3(1024), dim3(256), 0, st, (const unsigned long long *)mail_copy, (const pep_hit *)d_hits, (const uint32_t *)d_cig,
                               ctx->pin_stage.p, (unsigned long long)ctx->pin_stage.cap, ctx->d_zero.as<uint32_t>(), (uint32_t)(PEP_ZERO_TOTAL / 4), parent, labels, n_nodes);
            PEP_HIP(ctx, hipGetLastError());
            ctx->ext.pending = true; ctx->ext.res = res; ctx->ext.d_hits = d_hits; ctx->ext.d_cig = d_cig;
            ctx->ext.d_n_hits = reinterpret_cast<const uint32_t *>(mail_copy) + 2; ctx->ext.n_bound = n_b;
            ctx->ext.grouped = parent != nullptr;       // parents, unions and labels are queued: nothing is left for pep_k10_queue
            for (bool &f : ctx->zero_ok) f = true;   // as of this point of the stream every counter block is zero again (pack_out): whatever is queued
            ctx->zero_clean = true;                  // behind it - the next search, K9's alignment stage - needs no fill
            pep_timer_end(ctx, TM_TRACE);
            if (defer) return PEP_OK;
            PEP_HIP(ctx, pep_stream_wait(ctx));
            return pep_extend_finish(ctx);
        }
        // the exactly sized table: top-k and the two compactions, the sizes to the host, then emit into buffers of that size
        PEP_TRY(dev_reserve(ctx, ctx->ws[PEP_WS_KEEP], ((size_t)n_b + 2) * (4 + 4 + 8)));
        keep_flag = ctx->ws[PEP_WS_KEEP].as<uint32_t>(); hit_pos = keep_flag + n_b + 2;
        cig_pos = reinterpret_cast<uint64_t *>(hit_pos + n_b + 2);
        PEP_TRY(begin_select(ctx, PEP_LB_TOPK_HITS, PEP_LB_TOPK_RUNS, tiles, &ts));
        hipLaunchKernelGGL(topk, dim3((unsigned)tiles), dim3(256), 0, st, d_n_sel, sel, (const uint64_t *)sel_keys, P.top_k, P.n_splits, t_base, t_class, keep_flag, hit_pos, cig_pos,
                           (const unsigned long long *)score_hdr, (const unsigned long long *)trace_hdr, mail, ts, t_subject);
        PEP_TRY(pep_read_back(ctx, &h_mail, mail, sizeof(h_mail)));
        PEP_TRY(pep_sync_reads(ctx));
        n_hits = h_mail.n_hits; n_cig = h_mail.n_cig;
        ctx->stats.cells += h_mail.score_cells;
        ctx->stats.cells_swept += h_mail.score_blocks * 16 * 64;
        ctx->stats.candidates_settled += h_mail.n_settled;
        ctx->stats.cells_settled += h_mail.settled_cells;
        if (fast) {                                  // (the exactly sized pass has added its totals itself)
            ctx->stats.cells_trace += h_mail.trace_cells;
            ctx->stats.cells_swept_trace += h_mail.trace_blocks * 16 * 64;
            ctx->stats.dir_bytes += h_mail.trace_blocks * 512;
            ctx->trace_swept = h_mail.trace_swept;
        }
        ctx->stats.tracebacks_gapless = h_mail.n_sel - ctx->trace_swept;   // (counted by the pass's set-up kernel: the pairs that entered the sweep)
    } else {
        unsigned long long h_score[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        PEP_TRY(pep_read_back(ctx, h_score, score_hdr, sizeof(h_score)));
        PEP_TRY(pep_sync_reads(ctx));
        ctx->stats.cells += h_score[0];
        ctx->stats.cells_swept += h_score[1] * 16 * 64;
        ctx->stats.cells_settled += h_score[6];
        ctx->stats.candidates_settled += h_score[7];
    }
    ctx->stats.pairs = h_mail.n_pairs;
    ctx->stats.tracebacks = h_mail.n_sel;
    ctx->stats.hits = n_hits;
    if (n_hits) {
        const uint32_t n_sel = h_mail.n_sel;
        const size_t hb = (size_t)n_hits * sizeof(pep_hit);
        PEP_TRY(dev_reserve(ctx, ctx->ws[PEP_WS_HITS_OUT], hb + (n_cig + 1) * 4));
        pep_hit *d_hits = ctx->ws[PEP_WS_HITS_OUT].as<pep_hit>();
        uint32_t *d_cig = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(ctx->ws[PEP_WS_HITS_OUT].p) + hb);
        hipLaunchKernelGGL(emit, dim3((unsigned)ceil_div(n_sel, 4)), dim3(256), 0, st, d_n_sel, (const SelInfo *)sel, (const uint64_t *)sel_keys, (const uint32_t *)keep_flag,
                           (const uint32_t *)hit_pos, (const uint64_t *)cig_pos, (const uint64_t *)run_off, (const uint32_t *)runs,
                           ctx->ws[PEP_WS_SW_NBLK].as<const uint32_t>(), ctx->q.len.as<const uint32_t>(), ctx->t.len.as<const uint32_t>(), d_hits, d_cig);
        PEP_HIP(ctx, hipGetLastError());
        // the table goes to the context's pinned staging area (DMA speed, no page faults); pep_result_copy reads it from there.
        // If the host refuses that much pinned memory the result owns ordinary vectors instead.  In device-result mode
        // (pep_set_result_mode) nothing is copied here: whoever wants the host copy fetches it later (pep_fetch_result).
        if (ctx->device_results) {
        } else if (pin_reserve(ctx, ctx->pin_stage, hb + (n_cig + 1) * 4) == PEP_OK) {
            PEP_HIP(ctx, hipMemcpyAsync(ctx->pin_stage.p, d_hits, hb + n_cig * 4, hipMemcpyDeviceToHost, st));       // hits and arena are adjacent in PEP_WS_HITS_OUT
            res->st_hits = reinterpret_cast<const pep_hit *>(ctx->pin_stage.p);
            res->st_cigar = reinterpret_cast<const uint32_t *>(ctx->pin_stage.p + hb);
        } else {
            res->hits.resize(n_hits);
            res->cigar.resize(n_cig);
            PEP_HIP(ctx, hipMemcpyAsync(res->hits.data(), d_hits, hb, hipMemcpyDeviceToHost, st));
            if (n_cig) PEP_HIP(ctx, hipMemcpyAsync(res->cigar.data(), d_cig, n_cig * 4, hipMemcpyDeviceToHost, st));
        }
        res->n_hits = n_hits; res->n_cigar = n_cig;
        res->d_hits = d_hits; res->d_cigar = d_cig;
    }
    pep_timer_end(ctx, TM_TRACE);
    PEP_HIP(ctx, hipGetLastError());
    return PEP_OK;
}
