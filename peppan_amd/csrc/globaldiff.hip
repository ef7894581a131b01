// K22: the genome-pair identity statistics of get_global_difference (PEPPAN.py:1611-1666), the (mean, sigma) table K16 and K17 read.
//   pep_global_diff_walk (host C++)  the ORDER-DEPENDENT part, :1632-1659 without the two inner loops: the dictionary of member lists over the selected clu and
//                                    bsn rows.  It only decides which two lists meet at each row, costs the sum of the list lengths, and leaves one event per
//                                    row: two prefixes of lists in an append-only arena of genome ranks, the row's value, and whether same-genome pairs drop out.
//   pep_global_diff      (K22, GPU)  the QUADRATIC part: the cross product of every event, grouped by genome pair in event order, and numpy's two means per pair.
//       gd_count         one thread per item: its key's count and smallest sequence number, by atomics into the dense triangular key table; the counts
//                        are scanned into list offsets (pep_scan_u64), the keys in use compacted into records (pep_scan_u32)
//       gd_emit          per chunk of sequence numbers: key << k | event-in-chunk of every item (an item that does not exist: the key past the last one),
//                        sorted by pep_sort_u64 - all items of an event carry one value, so (key, event) order IS the order of the reference's list
//       gd_heads/scatter the head of a key's run notes where the run goes (the key's cursor - its own position), every item stores its event's value code
//                        (uint16) there, the tail of the run moves the cursor on: a key is one run per chunk, so its cursor has one reader and one writer
//       gd_bufsum        one wavefront per 8192-element buffer of a key's list: numpy's pairwise sum, eight lanes per 128-element leaf as its eight
//                        accumulators, the leaf sums folded along numpy's tree (as numpy_sum of similar.hip does for K14)
//       gd_fold          one thread per key: its buffer sums left to right from 0.0, then the division
//                        ... and both again with m for the squared deviations: a key of 10^8 values is as parallel as a million keys of 1000.
// The definition, operation by operation, is in include/peppan_hip.h (K22) and restated in numpy by tests/globaldiff_helpers.py; the device equals it bit
// for bit, so contraction into fused multiply-adds is switched off for the whole file.  The logarithm is a table the host makes with numpy (the device K16
// uses for its exp).  Not tuned: the rates are in profiles/globaldiff_rate.txt.  Known slack: every item finds its event by a binary search of its own, in
// both passes; the leaves of a buffer are listed and folded by one lane.
#include "common.h"
#include <algorithm>
#include <cstring>
#include <numeric>
#include <unordered_map>

#pragma clang fp contract(off)

namespace {

// the slots of pep_ctx::k22
enum { K22_IN = 0,      // the events (GdEvent), behind them base[n_events + 1] (u64)
       K22_ARENA,       // the arena (u32 ranks), behind it the logarithm table (double)
       K22_CNT,         // items per key, u64[T]; once the records are made: where the run of the chunk goes, minus its position (gd_heads)
       K22_MINSEQ,      // smallest sequence number per key, u64[T]
       K22_OFF,         // first entry of every key's list, u64[T + 1]
       K22_NEXT,        // the cursor: where the key's next entry goes, u64[T]
       K22_SLOT,        // key in use u32[T + 1], behind it its record's index u32[T + 1]
       K22_SORT,        // a chunk's sort words, twice
       K22_CODES,       // the lists: value codes, u16[items]
       K22_KEYS,        // per key in use: its record (GdKey), behind them buffers per key u64[n_keys + 1] and their scan u64[n_keys + 1]
       K22_BSUM,        // the sum of every buffer, double
       K22_OUT,         // m[n_keys], v[n_keys]
       K22_SCAN_TMP,
       K22_SLOTS };
static_assert(K22_SLOTS == sizeof(pep_ctx::k22) / sizeof(DevBuf), "one member of pep_ctx::k22 per slot");

constexpr int GD_BLOCK = 256;
constexpr int NP_BUFFER = 8192;          // elements numpy's reduction sums in one go (its default buffer size)
constexpr int PW_BLOCK = 128;            // numpy's pairwise sum: blocks of at most 128 elements through 8 accumulators
constexpr int LEAF_MAX = 128;            // leaves of one buffer: at most 65 for n <= 8192
static_assert(PEP_GDIFF_MAX_ITEMS <= (1ull << 32) && PEP_GDIFF_TABLE <= 65536, "an item's place inside its event is 32 bits; a value code is 16");
static_assert((uint64_t)PEP_GDIFF_MAX_GENOMES * (PEP_GDIFF_MAX_GENOMES + 1) / 2 < (1ull << 31), "a key is 32 bits, the key past the last one too");
static_assert(PEP_GDIFF_MAX_CHUNK_ITEMS < (1u << 30), "pep_sort_u64 takes fewer than 2^30 keys");

struct GdEvent { uint32_t a_off, a_len, b_off, b_len, value, drop; };
struct GdKey { uint64_t off, n, minseq; uint32_t g1, g2; };        // a key in use: its list, its first item, its two ranks g1 <= g2
struct GdIn {
    const GdEvent *ev;
    const uint64_t *base;                // [n_ev + 1]
    const uint32_t *arena;
    uint64_t n_ev;
    uint64_t G;
};

// item `s` (a sequence number below base[n_ev]): its event, and its key unless it does not exist
__device__ __forceinline__ bool gd_item(const GdIn &A, uint64_t s, uint64_t &e, uint32_t &key)
{
    uint64_t lo = 0, hi = A.n_ev;                       // base[lo] <= s < base[hi]
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (A.base[mid] <= s) lo = mid; else hi = mid;
    }
    e = lo;
    const GdEvent E = A.ev[lo];
    const uint32_t r = (uint32_t)(s - A.base[lo]), a = r / E.b_len, b = r - a * E.b_len;
    const uint32_t ga = A.arena[E.a_off + a], gb = A.arena[E.b_off + b];
    if (E.drop && ga == gb) return false;
    const uint64_t g1 = min(ga, gb), g2 = max(ga, gb);
    key = (uint32_t)(g1 * (2 * A.G - g1 + 1) / 2 + (g2 - g1));
    return true;
}

__global__ __launch_bounds__(GD_BLOCK) void gd_count(GdIn A, uint64_t total, unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ minseq)
{
    const uint64_t s = (uint64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    if (s >= total) return;
    uint64_t e;
    uint32_t key;
    if (!gd_item(A, s, e, key)) return;
    atomicAdd(&cnt[key], 1ull);
    atomicMin(&minseq[key], (unsigned long long)s);
}

__global__ __launch_bounds__(GD_BLOCK) void gd_flags(const uint64_t *__restrict__ cnt, uint32_t *__restrict__ flag, uint64_t T)
{
    const uint64_t k = (uint64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    if (k < T) flag[k] = cnt[k] ? 1u : 0u;
}

__global__ __launch_bounds__(GD_BLOCK) void gd_records(const uint64_t *__restrict__ cnt, const uint64_t *__restrict__ off, const uint64_t *__restrict__ minseq,
                                                       const uint32_t *__restrict__ slot, uint64_t T, uint64_t G, GdKey *__restrict__ rec, uint64_t *__restrict__ n_buf)
{
    const uint64_t k = (uint64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    if (k >= T || !cnt[k]) return;
    const uint32_t j = slot[k];
    uint64_t lo = 0, hi = G;                                // row lo of the triangle starts at or before k, row hi behind it
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (mid * (2 * G - mid + 1) / 2 <= k) lo = mid; else hi = mid;
    }
    rec[j] = GdKey{off[k], cnt[k], minseq[k], (uint32_t)lo, (uint32_t)(lo + (k - lo * (2 * G - lo + 1) / 2))};
    n_buf[j] = (cnt[k] + NP_BUFFER - 1) / NP_BUFFER;
}

// the sort word of every sequence number s0 .. s0 + n of a chunk whose first event is e0: key << ebits | event - e0; T is the key of an item that does not exist
__global__ __launch_bounds__(GD_BLOCK) void gd_emit(GdIn A, uint64_t s0, uint32_t n, uint64_t e0, int ebits, uint32_t T, uint64_t *__restrict__ words)
{
    const uint32_t i = blockIdx.x * GD_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint64_t e;
    uint32_t key;
    const bool have = gd_item(A, s0 + i, e, key);
    words[i] = have ? ((uint64_t)key << ebits) | (e - e0) : (uint64_t)T << ebits;
}

__global__ __launch_bounds__(GD_BLOCK) void gd_heads(const uint64_t *__restrict__ words, uint32_t n, int ebits, uint32_t T, const uint64_t *__restrict__ next,
                                                     uint64_t *__restrict__ dst_base)
{
    const uint32_t i = blockIdx.x * GD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = words[i] >> ebits;
    if (k < T && (i == 0 || (words[i - 1] >> ebits) != k)) dst_base[k] = next[k] - i;
}

__global__ __launch_bounds__(GD_BLOCK) void gd_scatter(const uint64_t *__restrict__ words, uint32_t n, int ebits, uint32_t T, const GdEvent *__restrict__ ev, uint64_t e0,
                                                       const uint64_t *__restrict__ dst_base, uint64_t *__restrict__ next, uint16_t *__restrict__ codes)
{
    const uint32_t i = blockIdx.x * GD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t w = words[i], k = w >> ebits;
    if (k >= T) return;
    const uint64_t pos = dst_base[k] + i;
    codes[pos] = (uint16_t)ev[e0 + (w & ((1ull << ebits) - 1))].value;
    if (i == n - 1 || (words[i + 1] >> ebits) != k) next[k] = pos + 1;
}

__device__ __forceinline__ int split_left(int n) { const int h = n / 2; return h - h % 8; }

__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// numpy's pairwise sum of v(0) .. v(n - 1), 1 <= n <= NP_BUFFER, by one wavefront; lane 0 returns the sum
template <class V>
__device__ double gd_pairwise(const V &v, int n, int lane, uint32_t *leaf_off, uint32_t *leaf_n, double *leaf_sum)
{
    // the leaves of the summation tree, left to right (lane 0)
    int n_leaf = 0;
    if (lane == 0) {
        int st_off[24], st_n[24], sp = 0;
        st_off[0] = 0; st_n[0] = n; sp = 1;
        while (sp > 0) {
            --sp;
            const int off = st_off[sp], m = st_n[sp];
            if (m <= PW_BLOCK) { if (n_leaf < LEAF_MAX) { leaf_off[n_leaf] = (uint32_t)off; leaf_n[n_leaf] = (uint32_t)m; } ++n_leaf; }
            else { const int l = split_left(m); st_off[sp] = off + l; st_n[sp] = m - l; ++sp; st_off[sp] = off; st_n[sp] = l; ++sp; }
        }
    }
    n_leaf = min(__shfl(n_leaf, 0, 64), LEAF_MAX);
    wave_lds_fence();
    // the leaf sums, 8 lanes per leaf = its 8 accumulators
    const int j = lane & 7, w = lane >> 3;
    for (int l0 = 0; l0 < n_leaf; l0 += 8) {                // (wave-uniform trip count)
        const int l = l0 + w;
        const bool have = l < n_leaf;
        const int off = have ? (int)leaf_off[l] : 0, m = have ? (int)leaf_n[l] : 0;
        double r = 0.;
        if (m >= 8) {
            r = v(off + j);
            for (int i = 8; i < m - (m % 8); i += 8) r = r + v(off + i + j);
        }
        const double t = r + __shfl_down(r, 1, 64);
        const double u = t + __shfl_down(t, 2, 64);
        double res = u + __shfl_down(u, 4, 64);
        if (j == 0 && have) {
            if (m < 8) { res = 0.; for (int i = 0; i < m; ++i) res = res + v(off + i); }
            else for (int i = m - (m % 8); i < m; ++i) res = res + v(off + i);
            leaf_sum[l] = res;
        }
    }
    wave_lds_fence();
    // the leaf sums folded along the tree (lane 0; post-order, the leaves are met left to right)
    double total = 0.;
    if (lane == 0) {
        int fr_n[24], fr_stage[24], sp = 0, li = 0;
        double fr_left[24];
        fr_n[0] = n; fr_stage[0] = 0; sp = 1;
        bool have_val = false;
        double val = 0.;
        while (sp > 0) {
            const int top = sp - 1;
            if (!have_val) {
                if (fr_n[top] <= PW_BLOCK) { val = leaf_sum[min(li, LEAF_MAX - 1)]; ++li; have_val = true; --sp; }
                else { fr_stage[top] = 1; fr_n[sp] = split_left(fr_n[top]); fr_stage[sp] = 0; ++sp; }
            } else if (fr_stage[top] == 1) {
                fr_left[top] = val; fr_stage[top] = 2; have_val = false;
                fr_n[sp] = fr_n[top] - split_left(fr_n[top]); fr_stage[sp] = 0; ++sp;
            } else { val = fr_left[top] + val; --sp; }
        }
        total = val;
    }
    return total;
}

// buffer blockIdx.x of all keys' lists: x = table[code], or (x - m) * (x - m) with the key's m when `mean` is given
__global__ __launch_bounds__(64) void gd_bufsum(const GdKey *__restrict__ rec, const uint64_t *__restrict__ buf_off, uint64_t n_keys, const uint16_t *__restrict__ codes,
                                                const double *__restrict__ table, const double *__restrict__ mean, double *__restrict__ bsum)
{
    __shared__ uint32_t leaf_off[LEAF_MAX], leaf_n[LEAF_MAX];
    __shared__ double leaf_sum[LEAF_MAX];
    const uint64_t b = blockIdx.x;
    const int lane = threadIdx.x;
    uint64_t lo = 0, hi = n_keys;                           // buf_off[lo] <= b < buf_off[hi]
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (buf_off[mid] <= b) lo = mid; else hi = mid;
    }
    const GdKey K = rec[lo];
    const uint64_t first = (b - buf_off[lo]) * NP_BUFFER;
    const int n = (int)min((uint64_t)NP_BUFFER, K.n - first);
    const uint16_t *c = codes + K.off + first;
    double sum;
    if (mean) {
        const double m = mean[lo];
        sum = gd_pairwise([&](int k) { const double d = table[c[k]] - m; return d * d; }, n, lane, leaf_off, leaf_n, leaf_sum);
    } else {
        sum = gd_pairwise([&](int k) { return table[c[k]]; }, n, lane, leaf_off, leaf_n, leaf_sum);
    }
    if (lane == 0) bsum[b] = sum;
}

__global__ __launch_bounds__(GD_BLOCK) void gd_fold(const GdKey *__restrict__ rec, const uint64_t *__restrict__ buf_off, uint64_t n_keys, const double *__restrict__ bsum,
                                                    double *__restrict__ out)
{
    const uint64_t j = (uint64_t)blockIdx.x * GD_BLOCK + threadIdx.x;
    if (j >= n_keys) return;
    double s = 0.0;
    for (uint64_t b = buf_off[j]; b < buf_off[j + 1]; ++b) s = s + bsum[b];
    out[j] = s / (double)rec[j].n;
}

const char *const K22_ME = "pep_global_diff: ";
const char *const K22_WALK_ME = "pep_global_diff_walk: ";

int bit_length(uint64_t x) { int b = 0; while (x) { ++b; x >>= 1; } return b; }

// what pep_global_diff makes of its tables on the host; every check of the call
struct GdPlan {
    std::vector<GdEvent> ev;
    std::vector<uint64_t> base;
    uint64_t T = 0, total = 0, chunk = 0;
};

int gd_check(const int64_t *events, uint64_t n_events, const int32_t *arena, uint64_t arena_len, uint32_t n_genomes, uint64_t chunk_items, GdPlan &P, std::string &msg)
{
    const auto bad = [&](int code, const std::string &text) { msg = K22_ME + text; return code; };
    if (chunk_items > PEP_GDIFF_MAX_CHUNK_ITEMS)
        return bad(PEP_ERR_ARG, "chunk_items = " + std::to_string(chunk_items) + ", more than " + std::to_string((uint64_t)PEP_GDIFF_MAX_CHUNK_ITEMS));
    P.chunk = chunk_items ? chunk_items : PEP_GDIFF_CHUNK_ITEMS;
    if (n_genomes > PEP_GDIFF_MAX_GENOMES)
        return bad(PEP_ERR_LIMIT, std::to_string(n_genomes) + " genomes asked for, the key table holds " + std::to_string(PEP_GDIFF_MAX_GENOMES));
    if ((n_events && !events) || (arena_len && !arena)) return bad(PEP_ERR_ARG, "null table");
    if (arena_len >= (1ull << 32)) return bad(PEP_ERR_LIMIT, std::to_string(arena_len) + " arena entries asked for, more than 2^32 - 1");
    P.T = (uint64_t)n_genomes * ((uint64_t)n_genomes + 1) / 2;
    P.ev.resize(n_events);
    P.base.assign(n_events + 1, 0);
    for (uint64_t e = 0; e < n_events; ++e) {
        const int64_t *r = events + 6 * e;
        const std::string name = "event " + std::to_string(e);
        for (int side = 0; side < 2; ++side) {
            const int64_t off = r[2 * side], len = r[2 * side + 1];
            if (len < 1) return bad(PEP_ERR_ARG, name + " has a list of " + std::to_string(len) + " entries, a list holds 1 at least");
            if (off < 0 || (uint64_t)off > arena_len || (uint64_t)len > arena_len - (uint64_t)off)
                return bad(PEP_ERR_ARG, name + " names entries " + std::to_string(off) + " .. " + std::to_string(off) + " + " + std::to_string(len) + " of an arena of " + std::to_string(arena_len));
        }
        if (r[4] < 0 || r[4] >= PEP_GDIFF_TABLE) return bad(PEP_ERR_ARG, name + " has the value " + std::to_string(r[4]) + ", outside 0 .. " + std::to_string(PEP_GDIFF_TABLE - 1));
        if (r[5] != 0 && r[5] != 1) return bad(PEP_ERR_ARG, name + " has drop_same = " + std::to_string(r[5]));
        P.ev[e] = GdEvent{(uint32_t)r[0], (uint32_t)r[1], (uint32_t)r[2], (uint32_t)r[3], (uint32_t)r[4], (uint32_t)r[5]};
        const uint64_t items = (uint64_t)r[1] * (uint64_t)r[3];          // (both below 2^32: no overflow)
        if (items > PEP_GDIFF_MAX_ITEMS - P.base[e]) {             // (base[e] is within the limit: every event before this one was)
            // the amount asked for, as far as 64 bits say it
            unsigned __int128 all = P.base[e];
            for (uint64_t k = e; k < n_events; ++k) all += (unsigned __int128)(uint64_t)std::max<int64_t>(events[6 * k + 1], 0) * (uint64_t)std::max<int64_t>(events[6 * k + 3], 0);
            const uint64_t shown = all > (unsigned __int128)UINT64_MAX ? UINT64_MAX : (uint64_t)all;
            return bad(PEP_ERR_LIMIT, std::to_string(shown) + " items asked for, more than " + std::to_string((uint64_t)PEP_GDIFF_MAX_ITEMS) + " (select fewer groups)");
        }
        P.base[e + 1] = P.base[e] + items;
    }
    P.total = P.base[n_events];
    if (P.total && n_genomes == 0) return bad(PEP_ERR_ARG, "events, but no genome");
    for (uint64_t k = 0; k < arena_len; ++k)
        if (arena[k] < 0 || (uint32_t)arena[k] >= n_genomes)
            return bad(PEP_ERR_ARG, "arena entry " + std::to_string(k) + " is " + std::to_string(arena[k]) + ", not a rank below " + std::to_string(n_genomes));
    // the workspace, the keys in use counted as min(T, items)
    const uint64_t keys = std::min(P.T, P.total), chunk = std::min(P.chunk, P.total);
    const uint64_t bytes = n_events * (sizeof(GdEvent) + 8) + arena_len * 4 + PEP_GDIFF_TABLE * 8 + P.T * (8 + 8 + 8 + 8 + 4 + 4) + chunk * 16 + P.total * 2 +
                           keys * (sizeof(GdKey) + 16 + 16) + (P.total / NP_BUFFER + keys) * 8;
    if (bytes > PEP_GDIFF_MAX_BYTES)
        return bad(PEP_ERR_LIMIT, std::to_string(bytes) + " bytes of workspace asked for (" + std::to_string(P.total) + " items, " + std::to_string(n_genomes) +
                                      " genomes), the device budget of one call is " + std::to_string((uint64_t)PEP_GDIFF_MAX_BYTES) + " (select fewer groups)");
    return PEP_OK;
}

}  // namespace

// the walk's result: the arena, the events, the genome of every rank
struct pep_gdiff_walk {
    std::vector<int32_t> arena;
    std::vector<int64_t> events;         // six per event
    std::vector<int32_t> genomes;
};

extern "C" {

int pep_global_diff_walk(const int64_t *clu, uint64_t n_clu, const int64_t *bsn, uint64_t n_bsn, const int64_t *genes, const int32_t *genome_of,
                         uint64_t n_genes, pep_gdiff_walk **out, char *msg, uint64_t msg_cap)
{
    const auto bad = [&](const std::string &text) { return pep_message_out(PEP_ERR_ARG, K22_WALK_ME + text, msg, msg_cap); };
    if (!out) return bad("null handle");
    *out = nullptr;
    if ((n_clu && !clu) || (n_bsn && !bsn) || (n_genes && (!genes || !genome_of))) return bad("null table");
    for (uint64_t k = 1; k < n_genes; ++k)
        if (genes[k] <= genes[k - 1]) return bad("gene ids are not strictly ascending at entry " + std::to_string(k));
    pep_gdiff_walk *W = new pep_gdiff_walk;
    struct Guard { pep_gdiff_walk *w; ~Guard() { delete w; } } guard{W};
    W->genomes.assign(genome_of, genome_of + n_genes);
    std::sort(W->genomes.begin(), W->genomes.end());
    W->genomes.erase(std::unique(W->genomes.begin(), W->genomes.end()), W->genomes.end());
    std::vector<int32_t> &arena = W->arena;
    struct List { uint64_t off, len, cap; };
    std::unordered_map<int64_t, List> lists;
    int64_t missing = 0;
    bool is_missing = false;
    const auto rank_of = [&](int64_t gene) -> int32_t {
        const int64_t *at = std::lower_bound(genes, genes + n_genes, gene);
        if (at == genes + n_genes || *at != gene) { if (!is_missing) { is_missing = true; missing = gene; } return 0; }
        return (int32_t)(std::lower_bound(W->genomes.begin(), W->genomes.end(), genome_of[at - genes]) - W->genomes.begin());
    };
    const auto single = [&](int64_t gene) { arena.push_back(rank_of(gene)); return List{(uint64_t)arena.size() - 1, 1, 1}; };
    W->events.reserve(6 * (n_clu + n_bsn));
    for (uint64_t k = 0; k < n_clu + n_bsn; ++k) {
        const bool is_clu = k < n_clu;
        const int64_t *row = is_clu ? clu + 3 * k : bsn + 3 * (k - n_clu);
        const int64_t r = row[0], q = row[1], value = row[2];
        const std::string name = (is_clu ? "clu row " : "bsn row ") + std::to_string(is_clu ? k : k - n_clu);
        if (value < 0 || value >= PEP_GDIFF_TABLE)
            return bad(name + " has the value " + std::to_string(value) + ", outside 0 .. " + std::to_string(PEP_GDIFF_TABLE - 1) + " (the logarithm of 1.005 - value / 10000 is not defined)");
        const auto at_r = lists.find(r);
        List rr = at_r != lists.end() ? at_r->second : single(r);
        const auto at_q = lists.find(q);
        List qq;
        if (at_q != lists.end()) { qq = at_q->second; lists.erase(at_q); } else qq = single(q);
        if (is_missing) return bad("gene " + std::to_string(missing) + " of " + name + " is not in the gene -> genome map");
        const int64_t event[6] = {(int64_t)rr.off, (int64_t)rr.len, (int64_t)qq.off, (int64_t)qq.len, value, is_clu ? 0 : 1};
        W->events.insert(W->events.end(), event, event + 6);
        if (is_clu) {
            const uint64_t need = rr.len + qq.len;
            if (need > rr.cap) {
                const bool last = rr.off + rr.cap == arena.size();
                if ((last ? rr.off + need : arena.size() + 2 * need) >= (1ull << 32)) return bad("the arena passes 2^32 - 1 entries at " + name);      // (before it is asked for)
                if (last) {
                    arena.resize(rr.off + need, 0);
                    rr.cap = need;
                } else {
                    const uint64_t to = arena.size();
                    arena.resize(to + 2 * need, 0);
                    std::copy(arena.begin() + rr.off, arena.begin() + rr.off + rr.len, arena.begin() + to);
                    rr.off = to; rr.cap = 2 * need;
                }
            }
            std::copy(arena.begin() + qq.off, arena.begin() + qq.off + qq.len, arena.begin() + rr.off + rr.len);
            rr.len = need;
            lists[r] = rr;
        }
        if (arena.size() >= (1ull << 32)) return bad("the arena passes 2^32 - 1 entries at " + name);
    }
    guard.w = nullptr;
    *out = W;
    return pep_message_out(PEP_OK, "", msg, msg_cap);
}

int pep_global_diff_walk_size(const pep_gdiff_walk *walk, uint64_t *n_events, uint64_t *arena_len, uint32_t *n_genomes)
{
    if (!walk || !n_events || !arena_len || !n_genomes) return PEP_ERR_ARG;
    *n_events = walk->events.size() / 6;
    *arena_len = walk->arena.size();
    *n_genomes = (uint32_t)walk->genomes.size();
    return PEP_OK;
}

int pep_global_diff_walk_copy(const pep_gdiff_walk *walk, int64_t *events, int32_t *arena, int32_t *genomes)
{
    if (!walk || (!walk->events.empty() && !events) || (!walk->arena.empty() && !arena) || (!walk->genomes.empty() && !genomes)) return PEP_ERR_ARG;
    std::copy(walk->events.begin(), walk->events.end(), events);
    std::copy(walk->arena.begin(), walk->arena.end(), arena);
    std::copy(walk->genomes.begin(), walk->genomes.end(), genomes);
    return PEP_OK;
}

void pep_global_diff_walk_free(pep_gdiff_walk *walk) { delete walk; }

int pep_global_diff_check(const int64_t *events, uint64_t n_events, const int32_t *arena, uint64_t arena_len, uint32_t n_genomes, uint64_t chunk_items,
                          char *msg, uint64_t msg_cap)
{
    GdPlan P;
    std::string text;
    const int rc = gd_check(events, n_events, arena, arena_len, n_genomes, chunk_items, P, text);
    return pep_message_out(rc, text, msg, msg_cap);
}

int pep_global_diff(pep_ctx *ctx, const int64_t *events, uint64_t n_events, const int32_t *arena, uint64_t arena_len, uint32_t n_genomes,
                    const double *table, uint64_t chunk_items, uint64_t *n_keys_out)
{
    if (!ctx) return PEP_ERR_ARG;
    CallTimes &times = ctx->calls[PEP_CALL_GLOBAL_DIFF];
    times = {};
    ctx->k22_n_keys = 0;
    if (!n_keys_out) return pep_fail(ctx, PEP_ERR_ARG, std::string(K22_ME) + "null table");
    *n_keys_out = 0;
    GdPlan P;
    std::string msg;
    const int rc = gd_check(events, n_events, arena, arena_len, n_genomes, chunk_items, P, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    if (P.total == 0) return PEP_OK;
    if (!table) return pep_fail(ctx, PEP_ERR_ARG, std::string(K22_ME) + "null table");
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf *B = ctx->k22;
    const uint64_t T = P.T, total = P.total, chunk = std::min(P.chunk, total);
    const size_t ev_bytes = n_events * sizeof(GdEvent), arena_bytes = (arena_len * 4 + 7) & ~(size_t)7;
    static_assert(sizeof(GdEvent) % 8 == 0, "base[] behind the events is aligned");
    PEP_TRY(pep_tables_to_device(ctx, B, {{K22_IN, P.ev.data(), ev_bytes, (n_events + 1) * 8}, {K22_ARENA, arena, arena_len * 4, arena_bytes - arena_len * 4 + PEP_GDIFF_TABLE * 8},
                                          {K22_CNT, nullptr, T * 8, 0}, {K22_MINSEQ, nullptr, T * 8, 0}, {K22_OFF, nullptr, (T + 1) * 8, 0}, {K22_NEXT, nullptr, T * 8, 0},
                                          {K22_SLOT, nullptr, (T + 1) * 8, 0}, {K22_SORT, nullptr, chunk * 16, 0}, {K22_CODES, nullptr, total * 2, 0}}));
    uint64_t *d_base = reinterpret_cast<uint64_t *>(B[K22_IN].as<uint8_t>() + ev_bytes);
    double *d_table = reinterpret_cast<double *>(B[K22_ARENA].as<uint8_t>() + arena_bytes);
    PEP_TRY(pep_h2d(ctx, d_base, P.base.data(), (n_events + 1) * 8));
    PEP_TRY(pep_h2d(ctx, d_table, table, PEP_GDIFF_TABLE * 8));
    const GdIn A{B[K22_IN].as<const GdEvent>(), d_base, B[K22_ARENA].as<const uint32_t>(), n_events, n_genomes};
    uint64_t *d_cnt = B[K22_CNT].as<uint64_t>(), *d_minseq = B[K22_MINSEQ].as<uint64_t>(), *d_off = B[K22_OFF].as<uint64_t>(), *d_next = B[K22_NEXT].as<uint64_t>();
    uint32_t *d_flag = B[K22_SLOT].as<uint32_t>(), *d_slot = d_flag + (T + 1);
    const unsigned key_blocks = (unsigned)ceil_div(T, GD_BLOCK);
    int stage_rc = PEP_OK;
    // ---- counts, offsets, the keys in use
    PEP_HIP(ctx, hipMemsetAsync(d_cnt, 0, T * 8, ctx->stream));
    PEP_HIP(ctx, hipMemsetAsync(d_minseq, 0xFF, T * 8, ctx->stream));
    pep_timed_stage(ctx, times.ms[0], [&] {
        hipLaunchKernelGGL(gd_count, dim3((unsigned)ceil_div(total, GD_BLOCK)), dim3(GD_BLOCK), 0, ctx->stream, A, total, reinterpret_cast<unsigned long long *>(d_cnt),
                           reinterpret_cast<unsigned long long *>(d_minseq));
        stage_rc = pep_scan_u64(ctx, d_cnt, d_off, T, B[K22_SCAN_TMP]);
        if (stage_rc != PEP_OK) return;
        hipLaunchKernelGGL(gd_flags, dim3(key_blocks), dim3(GD_BLOCK), 0, ctx->stream, (const uint64_t *)d_cnt, d_flag, T);
        stage_rc = pep_scan_u32(ctx, d_flag, d_slot, T, B[K22_SCAN_TMP]);
    });
    PEP_TRY(stage_rc);
    PEP_HIP(ctx, hipGetLastError());
    uint32_t n_keys = 0;
    PEP_TRY(pep_read_back(ctx, &n_keys, d_slot + T, 4));
    PEP_TRY(pep_sync_reads(ctx));
    if (n_keys == 0) return PEP_OK;                         // (only items that do not exist)
    if (n_keys > std::min(T, total)) return pep_fail(ctx, PEP_ERR_INTERNAL, std::string(K22_ME) + "more keys in use than items");
    const size_t rec_bytes = (size_t)n_keys * sizeof(GdKey);
    PEP_TRY(pep_tables_to_device(ctx, B, {{K22_KEYS, nullptr, rec_bytes + 2 * ((size_t)n_keys + 1) * 8, 0}, {K22_OUT, nullptr, (size_t)n_keys * 16, 0}}));
    GdKey *d_rec = B[K22_KEYS].as<GdKey>();
    uint64_t *d_nbuf = reinterpret_cast<uint64_t *>(B[K22_KEYS].as<uint8_t>() + rec_bytes), *d_buf_off = d_nbuf + (n_keys + 1);
    hipLaunchKernelGGL(gd_records, dim3(key_blocks), dim3(GD_BLOCK), 0, ctx->stream, (const uint64_t *)d_cnt, (const uint64_t *)d_off, (const uint64_t *)d_minseq,
                       (const uint32_t *)d_slot, T, (uint64_t)n_genomes, d_rec, d_nbuf);
    PEP_TRY(pep_scan_u64(ctx, d_nbuf, d_buf_off, n_keys, B[K22_SCAN_TMP]));
    uint64_t n_buf = 0;
    PEP_TRY(pep_read_back(ctx, &n_buf, d_buf_off + n_keys, 8));
    PEP_HIP(ctx, hipMemcpyAsync(d_next, d_off, T * 8, hipMemcpyDeviceToDevice, ctx->stream));
    // ---- the lists, chunk by chunk (d_cnt is free now: the records hold the counts)
    uint64_t *d_words = B[K22_SORT].as<uint64_t>(), *d_tmp = d_words + chunk, *d_dst_base = d_cnt;
    uint16_t *d_codes = B[K22_CODES].as<uint16_t>();
    const int kbits = bit_length(T);                        // (T itself is a key: the one of the items that do not exist)
    pep_timed_stage(ctx, times.ms[1], [&] {
        for (uint64_t s0 = 0; s0 < total && stage_rc == PEP_OK; s0 += chunk) {
            const uint32_t n = (uint32_t)std::min(chunk, total - s0);
            const uint64_t e0 = (uint64_t)(std::upper_bound(P.base.begin(), P.base.end(), s0) - P.base.begin()) - 1;
            const uint64_t e1 = (uint64_t)(std::upper_bound(P.base.begin(), P.base.end(), s0 + n - 1) - P.base.begin()) - 1;
            const int ebits = std::max(1, bit_length(e1 - e0));
            const unsigned blocks = (unsigned)ceil_div(n, GD_BLOCK);
            hipLaunchKernelGGL(gd_emit, dim3(blocks), dim3(GD_BLOCK), 0, ctx->stream, A, s0, n, e0, ebits, (uint32_t)T, d_words);
            stage_rc = pep_sort_u64(ctx, d_words, d_tmp, nullptr, n, kbits + ebits, nullptr, nullptr);
            if (stage_rc != PEP_OK) return;
            hipLaunchKernelGGL(gd_heads, dim3(blocks), dim3(GD_BLOCK), 0, ctx->stream, (const uint64_t *)d_words, n, ebits, (uint32_t)T, (const uint64_t *)d_next, d_dst_base);
            hipLaunchKernelGGL(gd_scatter, dim3(blocks), dim3(GD_BLOCK), 0, ctx->stream, (const uint64_t *)d_words, n, ebits, (uint32_t)T, A.ev, e0,
                               (const uint64_t *)d_dst_base, d_next, d_codes);
        }
    });
    PEP_TRY(stage_rc);
    PEP_HIP(ctx, hipGetLastError());
    PEP_TRY(pep_sync_reads(ctx));
    if (n_buf < n_keys || n_buf > total / NP_BUFFER + n_keys || n_buf >= (1ull << 31)) return pep_fail(ctx, PEP_ERR_INTERNAL, std::string(K22_ME) + "buffer count out of range");
    // ---- the two means
    PEP_TRY(dev_reserve(ctx, B[K22_BSUM], n_buf * 8));
    double *d_bsum = B[K22_BSUM].as<double>(), *d_mean = B[K22_OUT].as<double>(), *d_var = d_mean + n_keys;
    pep_timed_stage(ctx, times.ms[2], [&] {
        for (int pass = 0; pass < 2; ++pass) {
            hipLaunchKernelGGL(gd_bufsum, dim3((unsigned)n_buf), dim3(64), 0, ctx->stream, (const GdKey *)d_rec, (const uint64_t *)d_buf_off, (uint64_t)n_keys,
                               (const uint16_t *)d_codes, (const double *)d_table, pass ? (const double *)d_mean : (const double *)nullptr, d_bsum);
            hipLaunchKernelGGL(gd_fold, dim3((unsigned)ceil_div(n_keys, GD_BLOCK)), dim3(GD_BLOCK), 0, ctx->stream, (const GdKey *)d_rec, (const uint64_t *)d_buf_off,
                               (uint64_t)n_keys, (const double *)d_bsum, pass ? d_var : d_mean);
        }
    });
    PEP_HIP(ctx, hipGetLastError());
    PEP_HIP(ctx, pep_stream_wait(ctx));
    ctx->k22_n_keys = n_keys;
    *n_keys_out = n_keys;
    return PEP_OK;
}

int pep_global_diff_copy(pep_ctx *ctx, uint64_t n_keys, int32_t *g1, int32_t *g2, uint64_t *n, double *mean, double *var)
{
    if (!ctx) return PEP_ERR_ARG;
    if (n_keys != ctx->k22_n_keys)
        return pep_fail(ctx, PEP_ERR_ARG, "pep_global_diff_copy: " + std::to_string(n_keys) + " keys asked for, the newest pep_global_diff left " + std::to_string(ctx->k22_n_keys));
    if (n_keys == 0) return PEP_OK;
    if (!g1 || !g2 || !n || !mean || !var) return pep_fail(ctx, PEP_ERR_ARG, "pep_global_diff_copy: null table");
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<GdKey> rec(n_keys);
    std::vector<double> out(2 * n_keys);
    PEP_TRY(pep_d2h_queue(ctx, rec.data(), ctx->k22[K22_KEYS].p, n_keys * sizeof(GdKey)));
    PEP_TRY(pep_d2h_queue(ctx, out.data(), ctx->k22[K22_OUT].p, n_keys * 16));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    // the dictionary's insertion order: by the first item of every key
    std::vector<uint64_t> order(n_keys);
    std::iota(order.begin(), order.end(), (uint64_t)0);
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return rec[a].minseq < rec[b].minseq; });
    for (uint64_t k = 0; k < n_keys; ++k) {
        const GdKey &K = rec[order[k]];
        g1[k] = (int32_t)K.g1; g2[k] = (int32_t)K.g2;
        n[k] = K.n; mean[k] = out[order[k]]; var[k] = out[n_keys + order[k]];
    }
    return PEP_OK;
}

}  // extern "C"
