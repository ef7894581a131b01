// K23: the per-gene work of the GFF front end - iter_readGFF (PEPPAN.py:117-182), checkPseu (:992-1010), addGenes (:1013-1021).  The reference cuts every CDS
// out of its contig, reverse-complements it character by character (rc), translates it with marked starts (transeq: numpy arrays per character, then a
// string), looks at the first, the last and the inner characters of the translation, and hashes what it keeps - one Python round per gene.  Restated
// (include/peppan_hip.h, K23): a CDS is one window of a contig and a strand bit; its verdict is a function of its length, of whether codon 0 is M, codon n - 1 is
// X and any codon before the last is X; its digest is SHA-1 of the window as read.
//   cds_verdict   one wavefront per CDS.  Codes 1 and 2 come from the length alone.  Else chunks of 64 codons = 192 nucleotides as in K19 (codonclass.h): lane l
//                 reads the three characters of codon 64 c + l - forward, or backward and complemented -, a position at or behind the window's end reads as
//                 "outside the alphabet", which is how the reference pads a partial last codon.  One ballot each gives the chunk's M and X masks; three
//                 wave-uniform bits are carried: codon 0 is M, codon n - 1 is X, an X before codon n - 1.  The next chunk is on its way while one is judged;
//                 the walk ends after chunk 0 when code 3 is already fixed.  Integers only, no LDS, the code byte by a plain vector store of lane 0.
//   cds_digest    one thread per CDS of code 0, as K13's k13_sha1: 64-byte blocks as four unaligned 16-byte loads straight from the arena - read from the
//                 window's far end, complemented bytewise and taken in reverse word order when the strand bit is set - into sha1_block (sha1.h: sha1_window).
// What bounds them: byte-granular reads and a short wavefront-serial chain of chunks per CDS (verdict); ~1100 integer operations per 64 bytes with the lanes
// of a wavefront on CDS of different lengths (digest).  DESIGN.md 4.10j.
#include "common.h"
#include "codonclass.h"
#include "sha1.h"
#include <cstring>

namespace {

// the slots of pep_ctx::k23
enum { K23_NT = 0, K23_ITEM, K23_CODE, K23_DIGEST, K23_SLOTS };
static_assert(K23_SLOTS == sizeof(pep_ctx::k23) / sizeof(DevBuf), "one member of pep_ctx::k23 per slot");

constexpr uint32_t K23_MASK_ALL = PEP_CDS_ALLOW_NO_START | PEP_CDS_ALLOW_INNER_STOP | PEP_CDS_ALLOW_FRAMESHIFT | PEP_CDS_ALLOW_NO_STOP;

// one CDS as the kernels read it (made by the host check)
struct CdsItem {
    uint64_t at;                     // where its window starts in the arena
    uint32_t len;
    uint32_t rev;                    // 1: read backward and complemented
};
static_assert(sizeof(CdsItem) == 16, "one 16-byte read per CDS");

__global__ __launch_bounds__(256) void cds_verdict(const uint8_t *__restrict__ nt, const CdsItem *__restrict__ items, uint32_t n_cds, uint32_t min_cds, uint32_t mask,
                                                   unsigned long long stops, uint8_t *__restrict__ code)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_cds) return;                                             // (uniform over the wavefront)
    const CdsItem it = items[i];
    const uint32_t len = it.len;
    uint32_t verdict;
    if (len < min_cds) verdict = 1;
    else if (len % 3u != 0 && !(mask & PEP_CDS_ALLOW_FRAMESHIFT)) verdict = 2;
    else {
        const uint8_t *w = nt + it.at;
        const bool rev = it.rev != 0;
        const uint32_t n = (len + 2u) / 3u;                             // codons, a partial last one counted
        const uint32_t n_chunks = (n + 63u) / 64u;
        bool first_m = false, last_x = false, inner_x = false;
        uint32_t cur = n_chunks ? gs_load(w, len, rev, 0, lane) : 0u;
        for (uint32_t c = 0; c < n_chunks; ++c) {
            const uint32_t nxt = c + 1 < n_chunks ? gs_load(w, len, rev, c + 1, lane) : 0u;       // (on its way while this chunk is judged)
            const uint32_t base = c * 64u;
            bool is_m, is_x;
            gs_classify(cur & 7u, (cur >> 3) & 7u, (cur >> 6) & 7u, stops, base + lane < n, is_m, is_x);
            const unsigned long long M = __ballot(is_m), X = __ballot(is_x);
            if (c == 0) {
                first_m = M & 1ull;
                if (!first_m && !(mask & PEP_CDS_ALLOW_NO_START)) break;                         // code 3 whatever follows
            }
            const uint32_t k = n - 1u - base;                           // where the last codon sits, counted from this chunk's first (base < n)
            if (k < 64u) {
                last_x = (X >> k) & 1ull;
                inner_x |= (X & ((1ull << k) - 1ull)) != 0;
            } else inner_x |= X != 0;
            cur = nxt;
        }
        verdict = (!first_m && !(mask & PEP_CDS_ALLOW_NO_START)) ? 3u : (!last_x && !(mask & PEP_CDS_ALLOW_NO_STOP)) ? 4u
                  : (inner_x && !(mask & PEP_CDS_ALLOW_INNER_STOP)) ? 5u : 0u;
    }
    if (lane == 0) code[i] = (uint8_t)verdict;
}

__global__ __launch_bounds__(256) void cds_digest(const uint8_t *__restrict__ nt, const CdsItem *__restrict__ items, uint32_t n_cds, const uint8_t *__restrict__ code,
                                                  uint32_t *__restrict__ digest)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cds || code[i] != 0) return;
    const CdsItem it = items[i];
    uint32_t h[5];
    sha1_window(nt + it.at, it.len, it.rev != 0, h);
#pragma unroll
    for (int k = 0; k < 5; ++k) digest[(size_t)i * 5 + k] = h[k];
}

const char *const K23_ME = "pep_cds_genes: ";

// every check of the tables, on the host, before anything is launched; also makes the kernels' item records
int k23_check(const uint64_t *contig_off, uint32_t n_contigs, uint32_t n_cds, const uint32_t *contig, const uint64_t *win_off, const uint32_t *win_len,
              const uint8_t *strand, uint32_t mask, std::vector<CdsItem> *items, std::string &msg)
{
    const auto bad = [&](int code, const std::string &text) { msg = K23_ME + text; return code; };
    if (!contig_off || (n_cds && (!contig || !win_off || !win_len || !strand))) return bad(PEP_ERR_ARG, "null table");
    if (mask & ~K23_MASK_ALL) return bad(PEP_ERR_ARG, "mask " + std::to_string(mask) + " has bits beyond the four of s, i, f, e");
    if (contig_off[0] != 0) return bad(PEP_ERR_ARG, "contig_off must start at 0");
    for (uint32_t c = 0; c < n_contigs; ++c)
        if (contig_off[c + 1] < contig_off[c]) return bad(PEP_ERR_ARG, "contig_off must be non-decreasing (contig " + std::to_string(c) + ")");
    if (items) items->resize(n_cds);
    uint32_t p = 0;
    const auto who = [&] { return "CDS " + std::to_string(p); };                   // (made only for a message)
    for (; p < n_cds; ++p) {
        if (contig[p] >= n_contigs) return bad(PEP_ERR_ARG, who() + " names contig " + std::to_string(contig[p]) + " of " + std::to_string(n_contigs));
        if (win_len[p] >= PEP_CDS_MAX_WINDOW) return bad(PEP_ERR_LIMIT, "the window of " + who() + " holds 2^31 bytes or more");
        const uint64_t contig_len = contig_off[contig[p] + 1] - contig_off[contig[p]];
        if (win_off[p] > contig_len || win_len[p] > contig_len - win_off[p])
            return bad(PEP_ERR_ARG, "the window of " + who() + " leaves its contig of " + std::to_string(contig_len) + " bytes");
        if (strand[p] > 1) return bad(PEP_ERR_ARG, "the strand byte of " + who() + " is " + std::to_string(strand[p]) + ", not 0 or 1");
        if (items) (*items)[p] = CdsItem{contig_off[contig[p]] + win_off[p], win_len[p], strand[p]};
    }
    return PEP_OK;
}

}  // namespace

extern "C" {

int pep_cds_genes_check(const uint64_t *contig_off, uint32_t n_contigs, uint32_t n_cds, const uint32_t *contig, const uint64_t *win_off, const uint32_t *win_len,
                        const uint8_t *strand, uint32_t mask, char *msg, uint64_t msg_cap)
{
    std::string text;
    const int rc = k23_check(contig_off, n_contigs, n_cds, contig, win_off, win_len, strand, mask, nullptr, text);
    return pep_message_out(rc, text, msg, msg_cap);
}

int pep_cds_genes(pep_ctx *ctx, const uint8_t *nt, const uint64_t *contig_off, uint32_t n_contigs, uint32_t n_cds, const uint32_t *contig, const uint64_t *win_off,
                  const uint32_t *win_len, const uint8_t *strand, uint32_t min_cds, uint32_t mask, int table4, uint8_t *code, uint8_t *digest)
{
    if (!ctx) return PEP_ERR_ARG;
    CallTimes &times = ctx->calls[PEP_CALL_CDS_GENES];
    times = {};
    if (n_cds && (!code || !digest)) return pep_fail(ctx, PEP_ERR_ARG, std::string(K23_ME) + "null table");
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<CdsItem> items;
    std::string msg;
    const int rc = k23_check(contig_off, n_contigs, n_cds, contig, win_off, win_len, strand, mask, &items, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    if (n_cds == 0) return PEP_OK;
    const uint64_t n_nt = contig_off[n_contigs];
    if (n_nt && !nt) return pep_fail(ctx, PEP_ERR_ARG, std::string(K23_ME) + "null table");
    DevBuf *W = ctx->k23;
    hipStream_t st = ctx->stream;
    PEP_TRY(pep_tables_to_device(ctx, W, {{K23_NT, nt, n_nt, 16}, {K23_ITEM, items.data(), (size_t)n_cds * sizeof(CdsItem), 0}, {K23_CODE, nullptr, n_cds, 0},
                                          {K23_DIGEST, nullptr, (size_t)n_cds * 20, 0}}));
    pep_timed_stage(ctx, times.ms[0], [&] {
        hipLaunchKernelGGL(cds_verdict, dim3((unsigned)ceil_div(n_cds, 4)), dim3(256), 0, st, W[K23_NT].as<const uint8_t>(), W[K23_ITEM].as<const CdsItem>(), n_cds, min_cds,
                           mask, table4 ? GS_STOPS_TABLE4 : GS_STOPS, W[K23_CODE].as<uint8_t>());
    });
    pep_timed_stage(ctx, times.ms[1], [&] {
        hipLaunchKernelGGL(cds_digest, dim3((unsigned)ceil_div(n_cds, 256)), dim3(256), 0, st, W[K23_NT].as<const uint8_t>(), W[K23_ITEM].as<const CdsItem>(), n_cds,
                           W[K23_CODE].as<const uint8_t>(), W[K23_DIGEST].as<uint32_t>());
    });
    PEP_HIP(ctx, hipGetLastError());
    // the results wait in memory of the library until the stream has been waited for: on an error nothing is written
    std::vector<uint8_t> h_code(n_cds);
    std::vector<uint32_t> h_words((size_t)n_cds * 5);
    PEP_TRY(pep_d2h_queue(ctx, h_code.data(), W[K23_CODE].p, n_cds));
    PEP_TRY(pep_d2h_queue(ctx, h_words.data(), W[K23_DIGEST].p, (size_t)n_cds * 20));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    memcpy(code, h_code.data(), n_cds);
    for (uint32_t p = 0; p < n_cds; ++p) {                               // big-endian bytes, as hashlib's digest(); what the digest kernel skipped is zero
        uint8_t *d = digest + (size_t)p * 20;
        if (h_code[p] != 0) { memset(d, 0, 20); continue; }
        for (int k = 0; k < 5; ++k) {
            const uint32_t v = h_words[(size_t)p * 5 + k];
            d[4 * k] = (uint8_t)(v >> 24); d[4 * k + 1] = (uint8_t)(v >> 16); d[4 * k + 2] = (uint8_t)(v >> 8); d[4 * k + 3] = (uint8_t)v;
        }
    }
    return PEP_OK;
}

}  // extern "C"
