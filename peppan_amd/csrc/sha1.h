// The SHA-1 block function of K13 (dedup.hip: k13_sha1) and K23 (cdsgenes.hip: cds_digest): one 64-byte block, given as sixteen big-endian words, into the
// five state words.  80 rounds of 32-bit integer VALU, the schedule kept in a rolling window of sixteen registers.
// Internal linkage, as in the kernel file it came from: every translation unit that includes this compiles its own copy.
#pragma once
#include <stdint.h>

namespace {

__device__ __forceinline__ uint32_t rol(uint32_t x, int n) { return __builtin_rotateleft32(x, n); }

__device__ void sha1_block(uint32_t h[5], const uint32_t *wi)
{
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = wi[i];
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#pragma unroll
    for (int t = 0; t < 80; ++t) {
        uint32_t x;
        if (t < 16) x = w[t];
        else {
            x = rol(w[(t - 3) & 15] ^ w[(t - 8) & 15] ^ w[(t - 14) & 15] ^ w[t & 15], 1);
            w[t & 15] = x;
        }
        uint32_t f, k;
        if (t < 20) { f = (b & c) | (~b & d); k = 0x5A827999u; }
        else if (t < 40) { f = b ^ c ^ d; k = 0x6ED9EBA1u; }
        else if (t < 60) { f = (b & c) | (b & d) | (c & d); k = 0x8F1BBCDCu; }
        else { f = b ^ c ^ d; k = 0xCA62C1D6u; }
        const uint32_t tmp = rol(a, 5) + f + e + k + x;
        e = d; d = c; c = rol(b, 30); b = a; a = tmp;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e;
}

}  // namespace
