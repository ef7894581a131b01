// Decoupled look-back, the one protocol of everything here that scans, compacts or sorts in a single launch: the scans of scan.hip, the
// kernels that SCAN WHILE THEY COMPUTE (selection + compaction in one launch instead of flag -> scan -> gather: every launch of a dependent
// chain costs the GPU 4 - 5 us even when it has next to nothing to do) and the radix sort's passes (sort.hip).
//
// A block takes its tile number from a ticket counter (so that a tile only ever waits for tiles that are already running), computes its
// elements, publishes the tile's total in a status word and finds the total of everything in front of it by looking back over the status
// words of the tiles before it; then it publishes its inclusive prefix, where later tiles stop looking.
//
// state area: word 0 = the ticket counter (its low 32 bits), status words from word 1 (LbLaunch::status).
// status word: epoch << (VB + 2) | flag << VB | value; flag LB_SUM = the tile's own total, LB_PREFIX = total up to and including the tile;
// VB = value bits, which leaves 64 - 2 - VB bits for the epoch.  Words left by earlier launches carry another epoch and never match, so
// nothing is cleared between launches.  Epoch 0 is never handed out: a cleared area holds no word that could pass for a published one.
// The host hands out epochs and ticket bases (pep_lookback_begin) and clears the area when it grows, when the epoch wraps and after a
// failure (pep_fail) - nowhere else.
#pragma once
#include "common.h"

constexpr uint64_t LB_SUM = 1, LB_PREFIX = 2;

// what a kernel needs of one launch (pep_lookback_begin), passed by value
struct LbLaunch {
    uint64_t *state;
    uint32_t ticket_base;
    uint64_t epoch;
    __device__ __forceinline__ uint64_t *status() const { return state + 1; }
};

// ---- the status word
template <int VB, uint64_t FLAG> __device__ __forceinline__ uint64_t lb_word(uint64_t epoch, uint64_t value) { return (epoch << (VB + 2)) | (FLAG << VB) | (value & ((1ull << VB) - 1)); }
template <int VB> __device__ __forceinline__ bool lb_epoch_is(uint64_t w, uint64_t epoch) { return (w >> (VB + 2)) == epoch; }
template <int VB> __device__ __forceinline__ bool lb_is_prefix(uint64_t w) { return ((w >> VB) & 3u) == LB_PREFIX; }
template <int VB> __device__ __forceinline__ uint64_t lb_value(uint64_t w) { return w & ((1ull << VB) - 1); }
// the largest epoch a layout can hold (host side: where pep_lookback_begin wraps); value_bits >= 32, the host counts epochs in 32 bits
constexpr uint32_t lb_epoch_mask(int value_bits) { return (1u << (64 - 2 - value_bits)) - 1; }

__device__ __forceinline__ void lb_publish(uint64_t *word, uint64_t w) { __hip_atomic_store(word, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the word of this launch in a status slot: waits until its tile has published one
template <int VB>
__device__ __forceinline__ uint64_t lb_wait(const uint64_t *word, uint64_t epoch)
{
    uint64_t w;
    do { w = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while (!lb_epoch_is<VB>(w, epoch));
    return w;
}

// ticket of this block (call with all threads; returns the tile number, block-uniform)
__device__ __forceinline__ uint32_t lb_take_tile(uint64_t *state, uint32_t ticket_base, uint32_t *s_tile)
{
    if (threadIdx.x == 0) *s_tile = atomicAdd(reinterpret_cast<uint32_t *>(state), 1u) - ticket_base;
    __syncthreads();
    return *s_tile;
}

// exclusive prefix of tile `tile` whose own total is `tot`.  To be called by the 64 threads of the block's FIRST wavefront (lane = threadIdx.x);
// the result is valid in every one of them.  VB: value bits (32 with a 30-bit epoch, 48 with a 14-bit epoch); S: the type the totals are added in.
// MAX: the tiles' values are combined by maximum instead of by sum ("the largest value of any tile in front of this one").
// (A kernel that needs several prefixes at once - K1's reference layout - gives every one a status array of its own, n_tickets words apart, and a wavefront of its own.)
template <int VB, class S = uint64_t, bool MAX = false>
__device__ __forceinline__ S lb_tile_prefix(uint64_t *status, uint32_t tile, uint64_t tot, uint64_t epoch, int lane)
{
    S prefix = 0;
    if (tile > 0) {
        if (lane == 0) lb_publish(&status[tile], lb_word<VB, LB_SUM>(epoch, tot));
        for (int64_t hi = (int64_t)tile - 1; hi >= 0; hi -= 64) {          // a window of 64 predecessors, lane 0 = the nearest
            const int64_t idx = hi - lane;
            uint64_t w = lb_word<VB, LB_PREFIX>(epoch, 0);                  // in front of tile 0: prefix 0
            if (idx >= 0) w = lb_wait<VB>(&status[idx], epoch);
            const uint64_t is_prefix = __ballot(lb_is_prefix<VB>(w));
            const int stop = is_prefix ? __ffsll((unsigned long long)is_prefix) - 1 : 63;      // lanes 0 .. stop contribute
            S part = lane <= stop ? (S)lb_value<VB>(w) : (S)0;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) { const S o = __shfl_xor(part, d, 64); part = MAX ? (o > part ? o : part) : part + o; }
            prefix = MAX ? (part > prefix ? part : prefix) : prefix + part;
            if (is_prefix) break;
        }
    }
    if (lane == 0) lb_publish(&status[tile], lb_word<VB, LB_PREFIX>(epoch, MAX ? ((S)tot > prefix ? (S)tot : prefix) : prefix + (S)tot));
    return prefix;
}

// exclusive scan of one value per thread across a 256-thread block; *total = the block's sum (lds: 4 entries)
template <class T>
__device__ __forceinline__ T block_excl_scan_256(T v, T *total, T *lds)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const T o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const T s = lds[w]; if (w < wave) base += s; tot += s; }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// host side (scan.hip), the only place where a state area is reserved and cleared, an epoch advanced and a ticket base moved: one launch of
// n_tickets blocks on `slot`, every one of which owns words_per_ticket status words of value_bits value bits (1 everywhere but in the sort,
// whose tiles publish a word per digit).  The launch must follow on the context's stream.
int pep_lookback_begin(pep_ctx *ctx, PepLookback slot, uint64_t n_tickets, uint64_t words_per_ticket, int value_bits, LbLaunch *out);
