// The SHA-1 block function of K13 (dedup.hip: k13_sha1), K23 (cdsgenes.hip: cds_digest) and K24 (outalleles.hip: oa_digest): one 64-byte block, given as sixteen
// big-endian words, into the five state words.  80 rounds of 32-bit integer VALU, the schedule kept in a rolling window of sixteen registers.
// Behind it sha1_window, the digest of a strand-corrected window read in place (K23, K24), with rc() of a byte and of a dword.
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

// rc() of one byte (modules/configure.py:152-154): upper-cased, A <-> T, C <-> G, everything else N
__device__ __forceinline__ uint32_t sha1_rc_byte(uint32_t b)
{
    const uint32_t u = b & 0xDFu;
    const uint32_t c = ((u >> 1) ^ (u >> 2)) & 3u;                      // (gs_code's test for A C G T)
    return u == ((0x54474341u >> (c * 8)) & 0xFFu) ? (0x41434754u >> (c * 8)) & 0xFFu : (uint32_t)'N';
}

__device__ __forceinline__ uint32_t sha1_rc_word(uint32_t r)
{
    return sha1_rc_byte(r & 0xFFu) | sha1_rc_byte((r >> 8) & 0xFFu) << 8 | sha1_rc_byte((r >> 16) & 0xFFu) << 16 | sha1_rc_byte(r >> 24) << 24;
}

// SHA-1 of the `len` bytes at s - as they stand, or read from the far end and complemented bytewise when rev is set - into h: 64-byte blocks as four
// unaligned 16-byte loads, no copy of the text anywhere.  Nothing outside [s, s + len) is read.
__device__ inline void sha1_window(const uint8_t *s, uint32_t len, bool rev, uint32_t h[5])
{
    h[0] = 0x67452301u; h[1] = 0xEFCDAB89u; h[2] = 0x98BADCFEu; h[3] = 0x10325476u; h[4] = 0xC3D2E1F0u;
    uint32_t w[16];
    uint32_t at = 0;
    for (; at + 64u <= len; at += 64u) {
        if (!rev) {
            __builtin_memcpy(w, s + at, 64);
#pragma unroll
            for (int k = 0; k < 16; ++k) w[k] = __builtin_bswap32(w[k]);
        } else {
            // text bytes at .. at + 63 are window bytes len - 1 - at down to len - 64 - at: byte j of big-endian word k is byte 3 - j of little-endian dword 15 - k
            uint32_t r[16];
            __builtin_memcpy(r, s + (len - at - 64u), 64);
#pragma unroll
            for (int k = 0; k < 16; ++k) w[k] = sha1_rc_word(r[15 - k]);
        }
        sha1_block(h, w);
    }
    // tail: remaining bytes, 0x80, zeros, 64-bit big-endian bit length (one or two blocks)
    const uint32_t rem = len - at;
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k] = 0;
    for (uint32_t k = 0; k < rem; ++k) {
        const uint32_t b = rev ? sha1_rc_byte(s[len - 1u - (at + k)]) : (uint32_t)s[at + k];
        w[k >> 2] |= b << (24 - 8 * (k & 3));
    }
    w[rem >> 2] |= 0x80u << (24 - 8 * (rem & 3));
    if (rem >= 56) {
        sha1_block(h, w);
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = 0;
    }
    const uint64_t bits = (uint64_t)len * 8;
    w[14] = (uint32_t)(bits >> 32);
    w[15] = (uint32_t)bits;
    sha1_block(h, w);
}

}  // namespace
