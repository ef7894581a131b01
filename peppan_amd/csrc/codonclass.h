// The codon classes of a marked-start translation (transeq, modules/configure.py:160-194, with markStarts) straight from window bytes, shared by K19
// (genestruct.hip) and K23 (cdsgenes.hip): a codon is M (ATG GTG TTG), X (a stop, or any character outside ACGT-), '-' (it holds a '-') or neither.
// Internal linkage, as in the kernel files these came from: every translation unit that includes this compiles its own copy.
#pragma once
#include <stdint.h>

namespace {

// codon index c0 << 4 | c1 << 2 | c2 with A0 C1 G2 T3, as transeq builds it: the starts a marked-start translation calls M, and the stops
constexpr unsigned long long GS_STARTS = (1ull << 14) | (1ull << 46) | (1ull << 62);             // ATG GTG TTG
constexpr unsigned long long GS_STOPS = (1ull << 48) | (1ull << 50) | (1ull << 56);              // TAA TAG TGA
constexpr unsigned long long GS_STOPS_TABLE4 = (1ull << 48) | (1ull << 50);                      // TGA is W
constexpr uint32_t GS_BAD = 4, GS_GAP = 5;                                                       // codes of a character outside ACGT and of '-'

// the character at position p of the window as the reference's tables see it: 0..3 ACGT (complemented when read backward), GS_GAP, GS_BAD
__device__ __forceinline__ uint32_t gs_code(uint8_t ch, bool rev)
{
    const uint32_t u = ch & 0xDFu;
    const uint32_t code = ((u >> 1) ^ (u >> 2)) & 3u;                   // A 0x41, C 0x43, G 0x47, T 0x54: bits 1 and 2 spell 0..3 in that order
    if (u == ((0x54474341u >> (code * 8)) & 0xFFu)) return rev ? 3u - code : code;
    return (!rev && ch == '-') ? GS_GAP : GS_BAD;                       // (rc() turns '-' into N)
}

// the three characters of codon 64 c + lane of frame 0, 3 bits each; a position behind the window reads as GS_BAD
__device__ __forceinline__ uint32_t gs_load(const uint8_t *__restrict__ w, uint32_t len, bool rev, uint32_t c, uint32_t lane)
{
    const uint32_t p0 = 3u * (c * 64u + lane);
    uint32_t pk = 0;
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
        const uint32_t p = p0 + k;
        uint32_t code = GS_BAD;
        if (p < len) code = gs_code(rev ? w[len - 1u - p] : w[p], rev);
        pk |= code << (3 * k);
    }
    return pk;
}

__device__ __forceinline__ void gs_classify(uint32_t c0, uint32_t c1, uint32_t c2, unsigned long long stops, bool valid, bool &is_m, bool &is_x)
{
    const bool gap = (c0 == GS_GAP) | (c1 == GS_GAP) | (c2 == GS_GAP);
    const bool bad = ((c0 | c1 | c2) & 4u) != 0;
    const uint32_t idx = ((c0 & 3u) << 4) | ((c1 & 3u) << 2) | (c2 & 3u);
    is_m = valid && !bad && ((GS_STARTS >> idx) & 1ull);
    is_x = valid && !gap && (bad || ((stops >> idx) & 1ull));
}

}  // namespace
