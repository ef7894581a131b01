// The 64 x 64 tile of pair counts over K15's bit planes, shared by allelediff.hip (K15: stores every pair) and divergence.hip (K16: reduces
// the pairs of a tile to one flag); with SPLIT also the transitions among the mismatches, for njtree.hip (K21: Kimura's pair counts).  See allelediff.hip
// for the layout of the planes.
#pragma once
#include "common.h"

constexpr int K15_TILE = 64;        // pairs per tile side
constexpr int K15_KW = 4;           // words of every plane staged per step
constexpr uint64_t K15_NONE = ~0ull;

struct DiffTile { uint32_t g, ti, tj, kind; };      // kind 0: pairs a < b of tile (ti, tj); 1: rows {0, n - 1} against columns of tile tj

// Called by all 256 threads of a workgroup.  idx: the group's row indices (n of them, rows of `words` words per plane).  Thread (tx, ty) =
// (tid & 15, tid >> 4) gets mis / cmp of rows A = ti * 64 + ty * 4 + i (kind 1: row 0 for ty * 4 + i == 0, row n - 1 for == 1, none else)
// against rows B = tj * 64 + tx + 16 * j; rows past n count as all zero.  SPLIT: ts = the mismatches whose codes differ in plane B1 alone - codes are digit - 1, so
// A = 0, C = 1, G = 2, T = 3 and those are A <-> G and C <-> T; not SPLIT: ts is left alone.
template <bool SPLIT>
__device__ __forceinline__ void k15_tile_counts_of(const uint32_t *__restrict__ idx, uint32_t n, uint32_t words, const DiffTile T,
                                                   const uint64_t *__restrict__ plane_off, const unsigned long long *__restrict__ planes,
                                                   uint32_t (&mis)[4][4], uint32_t (&cmp)[4][4], uint32_t (&ts)[4][4])
{
    // [plane * KW + word][row]: the threads of a wavefront read 16 consecutive B rows (no bank conflict) and 4 A rows (broadcast)
    __shared__ unsigned long long sA[3 * K15_KW][K15_TILE], sB[3 * K15_KW][K15_TILE];
    __shared__ uint64_t offA[K15_TILE], offB[K15_TILE];
    const uint32_t tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    if (tid < K15_TILE) {
        uint64_t a = (uint64_t)T.ti * K15_TILE + tid;
        if (T.kind == 1) a = tid == 0 ? 0 : tid == 1 ? (uint64_t)n - 1 : n;
        offA[tid] = a < n ? plane_off[idx[a]] : K15_NONE;
    } else if (tid < 2 * K15_TILE) {
        const uint64_t b = (uint64_t)T.tj * K15_TILE + (tid - K15_TILE);
        offB[tid - K15_TILE] = b < n ? plane_off[idx[b]] : K15_NONE;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            mis[i][j] = cmp[i][j] = 0;
            if constexpr (SPLIT) ts[i][j] = 0;
        }
    for (uint32_t w0 = 0; w0 < words; w0 += K15_KW) {
        __syncthreads();                                            // the previous step's words are consumed (first step: offA / offB are written)
        for (uint32_t e = tid; e < 2 * 3 * K15_KW * K15_TILE; e += 256) {
            const uint32_t panel = e / (3 * K15_KW * K15_TILE), rem = e % (3 * K15_KW * K15_TILE), pw = rem / K15_TILE, row = rem % K15_TILE;
            const uint32_t plane = pw / K15_KW, w = w0 + pw % K15_KW;
            const uint64_t off = panel ? offB[row] : offA[row];
            const unsigned long long v = (off != K15_NONE && w < words) ? planes[off + (uint64_t)plane * words + w] : 0ull;
            if (panel) sB[pw][row] = v; else sA[pw][row] = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int k = 0; k < K15_KW; ++k) {                          // (unrolled, the four steps' LDS reads are hoisted together: 195 VGPRs instead of 95)
            unsigned long long av[4], a0[4], a1[4], bv[4], b0[4], b1[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                av[i] = sA[k][ty * 4 + i]; a0[i] = sA[K15_KW + k][ty * 4 + i]; a1[i] = sA[2 * K15_KW + k][ty * 4 + i];
                bv[i] = sB[k][tx + 16 * i]; b0[i] = sB[K15_KW + k][tx + 16 * i]; b1[i] = sB[2 * K15_KW + k][tx + 16 * i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned long long c = av[i] & bv[j];
                    cmp[i][j] += (uint32_t)__popcll(c);
                    mis[i][j] += (uint32_t)__popcll(c & ((a0[i] ^ b0[j]) | (a1[i] ^ b1[j])));
                    if constexpr (SPLIT) ts[i][j] += (uint32_t)__popcll(c & ~(a0[i] ^ b0[j]) & (a1[i] ^ b1[j]));
                }
        }
    }
}

__device__ __forceinline__ void k15_tile_counts(const uint32_t *__restrict__ idx, uint32_t n, uint32_t words, const DiffTile T,
                                                const uint64_t *__restrict__ plane_off, const unsigned long long *__restrict__ planes,
                                                uint32_t (&mis)[4][4], uint32_t (&cmp)[4][4])
{
    k15_tile_counts_of<false>(idx, n, words, T, plane_off, planes, mis, cmp, mis);
}

// allelediff.hip: queues K15's bit-plane kernel for n_rows packed rows (d_bad_row: the smallest row holding a byte above 124, untouched otherwise)
void pep_k15_queue_planes(hipStream_t st, uint64_t n_rows, const uint8_t *d_packed, const uint64_t *d_row_off, const uint32_t *d_row_len,
                          const uint64_t *d_plane_off, unsigned long long *d_planes, uint32_t *d_bad_row);
