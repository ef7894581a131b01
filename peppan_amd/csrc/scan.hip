// Exclusive prefix sums over device arrays (u32 / u64), n+1 outputs (out[n] = total).
// ONE launch, by decoupled look-back (lookback.h): reads the input once and writes it once; the searches run a dozen short scans per
// pass, so the two launches saved per scan matter more than the bytes.  u64 sums travel as 48 bits.  (n = 0 or n >= 2^40: per-tile
// reduce -> scan of the tile sums -> per-tile scan + offset.)
#include "common.h"
#include "lookback.h"

namespace {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;

template <class T>
__global__ __launch_bounds__(SCAN_THREADS) void scan_reduce(const T *__restrict__ in, T *__restrict__ partial, uint64_t n)
{
    __shared__ T lds[4];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE;
    T s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        uint64_t i = base + (uint64_t)k * SCAN_THREADS + threadIdx.x;
        if (i < n) s += in[i];
    }
    T tot;
    block_excl_scan_256<T>(s, &tot, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

template <class T>
__global__ __launch_bounds__(SCAN_THREADS) void scan_partials(T *partial, uint64_t nb)
{
    __shared__ T lds[4];
    T carry = 0;
    for (uint64_t b0 = 0; b0 < nb; b0 += SCAN_THREADS) {
        uint64_t i = b0 + threadIdx.x;
        T v = i < nb ? partial[i] : 0, tot;
        T ex = block_excl_scan_256<T>(v, &tot, lds);
        if (i < nb) partial[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) partial[nb] = carry;
}

template <class T>
__global__ __launch_bounds__(SCAN_THREADS) void scan_apply(const T *in, T *out, const T *__restrict__ partial,
                                                           uint64_t n, uint64_t nb)
{
    __shared__ T lds[4];
    // thread t owns items [t*ITEMS, t*ITEMS+ITEMS) of the tile so that the in-thread order is the array order
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    T v[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        v[k] = (base + k < n) ? in[base + k] : 0;
        s += v[k];
    }
    T tot;
    T ex = block_excl_scan_256<T>(s, &tot, lds) + partial[blockIdx.x];
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (base + k < n) out[base + k] = ex;
        ex += v[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = partial[nb];
}

// ---- single-launch scan: a tile scans its elements, publishes its sum and finds the sum of the tiles in front of it by look-back (lookback.h)
// value bits of the status word: u32 sums whole; u64 sums (block / run / CIGAR totals, all far below 2^48) in 48 bits, which leaves a 14-bit
// epoch - that state area is cleared every 2^14 - 1 scans
template <class T> constexpr int SCAN_VB = sizeof(T) == 8 ? 48 : 32;

template <class T>
__global__ __launch_bounds__(SCAN_THREADS) void scan_lookback(const T *in, T *out, uint64_t n, uint32_t nb, LbLaunch lb, T *total_out)
{
    __shared__ T lds[4];
    __shared__ uint32_t s_tile;
    __shared__ T s_prefix;
    const uint32_t tile = lb_take_tile(lb.state, lb.ticket_base, &s_tile);
    const uint64_t base = (uint64_t)tile * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_ITEMS;
    T v[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        v[k] = (base + k < n) ? in[base + k] : 0;
        s += v[k];
    }
    T tot;
    T ex = block_excl_scan_256<T>(s, &tot, lds);
    if (threadIdx.x < 64) {
        const T prefix = lb_tile_prefix<SCAN_VB<T>, T>(lb.status(), tile, tot, lb.epoch, (int)threadIdx.x);
        if (threadIdx.x == 0) s_prefix = prefix;
    }
    __syncthreads();
    ex += s_prefix;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (base + k < n) out[base + k] = ex;
        ex += v[k];
    }
    if (tile == nb - 1 && threadIdx.x == SCAN_THREADS - 1) { out[n] = ex; if (total_out) *total_out = ex; }
}

template <class T>
int scan_onepass(pep_ctx *ctx, const T *d_in, T *d_out, uint64_t n, T *d_total)
{
    const uint64_t nb = ceil_div(n, SCAN_TILE);
    LbLaunch lb;
    PEP_TRY(pep_lookback_begin(ctx, sizeof(T) == 8 ? PEP_LB_SCAN_U64 : PEP_LB_SCAN_U32, nb, 1, SCAN_VB<T>, &lb));
    hipLaunchKernelGGL(scan_lookback<T>, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, ctx->stream, d_in, d_out, n, (uint32_t)nb, lb, d_total);
    PEP_HIP(ctx, hipGetLastError());
    return PEP_OK;
}

template <class T>
int scan_impl(pep_ctx *ctx, const T *d_in, T *d_out, uint64_t n, DevBuf &tmp, T *d_total)
{
    if (n == 0) {
        PEP_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(T), ctx->stream));
        if (d_total) PEP_HIP(ctx, hipMemsetAsync(d_total, 0, sizeof(T), ctx->stream));
        return PEP_OK;
    }
    const uint64_t nb = ceil_div(n, SCAN_TILE);
    PEP_TRY(dev_reserve(ctx, tmp, (nb + 1) * sizeof(T)));
    T *partial = tmp.as<T>();
    hipLaunchKernelGGL(scan_reduce<T>, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, ctx->stream, d_in, partial, n);
    hipLaunchKernelGGL(scan_partials<T>, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, partial, nb);
    hipLaunchKernelGGL(scan_apply<T>, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, ctx->stream, d_in, d_out, (const T *)partial, n, nb);
    if (d_total) PEP_HIP(ctx, hipMemcpyAsync(d_total, d_out + n, sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    PEP_HIP(ctx, hipGetLastError());
    return PEP_OK;
}

}  // namespace

int pep_scan_u32(pep_ctx *ctx, const uint32_t *d_in, uint32_t *d_out, uint64_t n, DevBuf &tmp, uint32_t *d_total)
{
    if (n == 0 || n >= (1ull << 40)) return scan_impl<uint32_t>(ctx, d_in, d_out, n, tmp, d_total);
    return scan_onepass<uint32_t>(ctx, d_in, d_out, n, d_total);
}

// the single launch carries 48-bit sums; callers whose totals could pass 2^48 say so (none does: the u64 scans add up block, run and
// CIGAR counts of one search)
int pep_scan_u64(pep_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, uint64_t n, DevBuf &tmp, uint64_t *d_total)
{
    if (n == 0 || n >= (1ull << 40)) return scan_impl<uint64_t>(ctx, d_in, d_out, n, tmp, d_total);
    return scan_onepass<uint64_t>(ctx, d_in, d_out, n, d_total);
}

// n 32-bit words from pinned host memory into device memory BY A KERNEL (the device reads the host buffer over the bus): between two
// kernels a copy command costs the GPU about 10 us of idle time in front of it, a kernel none
namespace {
__global__ __launch_bounds__(256) void copy_words(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) dst[i] = src[i];
}
}  // namespace

// both directions in one launch: n_up words from pinned host memory into device memory, n_down words from device memory into pinned host memory
namespace {
__global__ __launch_bounds__(256) void exchange_words(uint32_t *__restrict__ up_dst, const uint32_t *__restrict__ up_src, uint64_t n_up,
                                                      uint32_t *__restrict__ down_dst, const uint32_t *__restrict__ down_src, uint64_t n_down)
{
    const uint64_t t0 = (uint64_t)blockIdx.x * 256 + threadIdx.x, stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = t0; i < n_up; i += stride) up_dst[i] = up_src[i];
    for (uint64_t i = t0; i < n_down; i += stride) down_dst[i] = down_src[i];
}
}  // namespace

int pep_exchange_pinned(pep_ctx *ctx, void *d_up_dst, const void *pinned_up_src, uint64_t n_up_words, void *pinned_down_dst, const void *d_down_src, uint64_t n_down_words)
{
    if (n_up_words + n_down_words == 0) return PEP_OK;
    hipLaunchKernelGGL(exchange_words, dim3((unsigned)std::min<uint64_t>(ceil_div(std::max(n_up_words, n_down_words), 256), 1024)), dim3(256), 0, ctx->stream,
                       reinterpret_cast<uint32_t *>(d_up_dst), reinterpret_cast<const uint32_t *>(pinned_up_src), n_up_words,
                       reinterpret_cast<uint32_t *>(pinned_down_dst), reinterpret_cast<const uint32_t *>(d_down_src), n_down_words);
    PEP_HIP(ctx, hipGetLastError());
    return PEP_OK;
}

int pep_copy_from_pinned(pep_ctx *ctx, void *d_dst, const void *pinned_src, uint64_t n_words)
{
    if (n_words == 0) return PEP_OK;
    hipLaunchKernelGGL(copy_words, dim3((unsigned)std::min<uint64_t>(ceil_div(n_words, 256), 1024)), dim3(256), 0, ctx->stream, reinterpret_cast<uint32_t *>(d_dst),
                       reinterpret_cast<const uint32_t *>(pinned_src), n_words);
    PEP_HIP(ctx, hipGetLastError());
    return PEP_OK;
}

// (lookback.h) the state area, ticket base and epoch of one launch of a kernel that looks back
int pep_lookback_begin(pep_ctx *ctx, PepLookback slot, uint64_t n_tickets, uint64_t words_per_ticket, int value_bits, LbLaunch *out)
{
    LookbackState &S = ctx->lookback[slot];
    const size_t need = (n_tickets * words_per_ticket + 1) * sizeof(uint64_t);          // the ticket counter + the status words
    bool clear = false;
    if (need > S.buf.cap) {
        // a new (or larger) state area starts from zeros: epoch 0 is never used, so no word of it can pass for a published one
        PEP_TRY(dev_reserve(ctx, S.buf, need * 2));
        clear = true;
    }
    if (S.dirty) { clear = true; S.dirty = false; }
    S.epoch = (S.epoch + 1) & lb_epoch_mask(value_bits);
    if (S.epoch == 0) { clear = true; S.epoch = 1; }   // wrapped: forget every old word
    if (clear) {
        PEP_HIP(ctx, hipMemsetAsync(S.buf.p, 0, S.buf.cap, ctx->stream));
        S.ticket_base = 0;
    }
    *out = LbLaunch{S.buf.as<uint64_t>(), S.ticket_base, S.epoch};
    S.ticket_base += (uint32_t)n_tickets;
    return PEP_OK;
}
