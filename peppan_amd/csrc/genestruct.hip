// K19: the gene structure of predictions - determineGeneStructure (PEPPAN.py:1193-1229), which write_output runs for every intact prediction (:1468).
// The reference translates the window in the tried frames with marked starts (transeq, modules/configure.py:160-194: numpy arrays per character, then a
// string) and searches the strings with find / rfind.  Restated (include/peppan_hip.h, K19): per frame the codons are classified M (ATG GTG TTG), X (a stop, or
// any character outside ACGT) or neither; with a = lp / 3, b = (lp + allowed_vary) / 3 the start is the first M in [a, b), else the last M below a, else a; the
// stop the first X from the start; while the stop lies below b and an M follows it below b, the start moves to that M.
//   gene_structure   one wavefront per prediction.  A chunk is 64 codons of frame 0 = 192 nucleotides: lane l reads the three of codon 64 c + l (forward, or
//                    backward and complemented as rc() does) as three 3-bit codes; the two more that frames 1 and 2 need come from lane l + 1, for lane 63 from
//                    the next chunk, which is always one chunk ahead on its way.  No table read: stop and start are bits of two 64-bit codon masks.  One ballot per
//                    frame gives the wave-uniform M and X masks of the chunk, and every tried frame's search advances on them with bit scans - a state of six
//                    integers per frame (GsFrame), forward-only: the last M below a with the first X behind it, the first X from a, then "looking for X" /
//                    "looking for an M below b".  The walk ends when the outcome is fixed: the lowest tried frames are final up to one that is a CDS, or all are.
// Integers only, no LDS, outputs by plain vector stores of lane 0.  What bounds it: byte-granular reads of the window and a short wavefront-serial chain of
// chunks per prediction.
#include "common.h"
#include "codonclass.h"
#include <cstring>

namespace {

// the slots of pep_ctx::k19
enum { K19_NT = 0, K19_ITEM, K19_START, K19_STOP, K19_VERDICT, K19_SLOTS };
static_assert(K19_SLOTS == sizeof(pep_ctx::k19) / sizeof(DevBuf), "one member of pep_ctx::k19 per slot");

// one prediction as the kernel reads it (made by the host check)
struct GsItem {
    uint64_t at;                     // where its window starts in the nucleotide set
    uint32_t len, lp, allowed_vary, ref_len;
    uint32_t flags;                  // bit 0: read backward and complemented; bits 1-3: the tried frames
    uint32_t pad;
};
static_assert(sizeof(GsItem) == 32, "two 16-byte reads per prediction");

enum { GS_PRE = 0, GS_FIND_X, GS_FIND_M, GS_DONE };

// the search of one frame between two chunks (all wave-uniform)
struct GsFrame {
    int phase = GS_PRE;
    int s1 = -1, x1 = -1;            // GS_PRE: the last M below a so far, the first X at or behind it
    int xa = -1;                     // GS_PRE: the first X at or behind a
    int start = 0, stop = -1;
    bool nostart = false;
};

// the bits of a chunk that starts at codon `base` whose codons are >= p
__device__ __forceinline__ unsigned long long gs_from(int p, int base)
{
    const int k = p - base;
    return k <= 0 ? ~0ull : k >= 64 ? 0ull : ~0ull << k;
}

__device__ __forceinline__ int gs_first(unsigned long long m, int base) { return base + __ffsll((long long)m) - 1; }

// frame F takes the M and X masks of the chunk at `base` (bits of codons >= n already cleared)
__device__ __forceinline__ void gs_advance(GsFrame &F, unsigned long long M, unsigned long long X, int base, int a, int b, int n)
{
    if (F.phase == GS_DONE) return;
    const bool last = base + 64 >= n, b_passed = base + 64 >= b;
    const unsigned long long below_b = ~gs_from(b, base);
    if (F.phase == GS_PRE) {
        const unsigned long long m_low = M & ~gs_from(a, base);
        if (m_low) { F.s1 = base + 63 - __clzll((long long)m_low); F.x1 = -1; }
        if (F.s1 >= 0 && F.x1 < 0) {
            const unsigned long long t = X & gs_from(F.s1, base);
            if (t) F.x1 = gs_first(t, base);
        }
        if (F.xa < 0) {
            const unsigned long long t = X & gs_from(a, base);
            if (t) F.xa = gs_first(t, base);
        }
        const unsigned long long m_mid = M & gs_from(a, base) & below_b;
        if (m_mid) {                                                    // s0 of :1201
            F.start = gs_first(m_mid, base);
            F.phase = GS_FIND_X;
        } else if (last || b_passed) {                                  // no M in [a, b): s1, else a
            if (F.s1 >= 0) { F.start = F.s1; F.stop = F.x1; }
            else { F.nostart = true; F.start = a; F.stop = F.xa; }
            F.phase = F.stop < 0 ? GS_FIND_X : F.stop < b ? GS_FIND_M : GS_DONE;
        }
    }
    for (;;) {
        if (F.phase == GS_FIND_X) {
            const unsigned long long t = X & gs_from(F.start, base);
            if (!t) break;
            F.stop = gs_first(t, base);
            F.phase = F.stop < b ? GS_FIND_M : GS_DONE;
        } else if (F.phase == GS_FIND_M) {                              // the loop of :1206-1212
            const unsigned long long t = M & gs_from(F.stop, base) & below_b;
            if (t) {
                F.start = gs_first(t, base);
                F.stop = -1;
                F.phase = GS_FIND_X;
            } else {
                if (b_passed) F.phase = GS_DONE;
                break;
            }
        } else break;
    }
    if (last) F.phase = GS_DONE;                                        // still looking for X: no stop; still looking for M: the stop stands
}

__device__ __forceinline__ uint32_t gs_kind(const GsFrame &F, uint32_t ref_len, uint32_t allowed_vary)
{
    if (F.stop < 0) return PEP_GENESTRUCT_NOSTOP;
    if (((long long)F.stop - F.start + 1) * 3 < (long long)ref_len - (long long)allowed_vary) return PEP_GENESTRUCT_PREMATURE;
    return F.nostart ? PEP_GENESTRUCT_NOSTART : PEP_GENESTRUCT_CDS;
}

__global__ __launch_bounds__(256) void gene_structure(const uint8_t *__restrict__ nt, const GsItem *__restrict__ items, uint32_t n_pred, unsigned long long stops,
                                                      uint32_t *__restrict__ start_aa, uint32_t *__restrict__ stop_aa, uint8_t *__restrict__ verdict)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_pred) return;                                            // (uniform over the wavefront)
    const GsItem it = items[i];
    const uint8_t *w = nt + it.at;
    const uint32_t len = it.len;
    const bool rev = it.flags & 1u;
    const bool tried[3] = {(it.flags & 2u) != 0, (it.flags & 4u) != 0, (it.flags & 8u) != 0};
    const int a = (int)(it.lp / 3u);
    const int b = (int)min(((unsigned long long)it.lp + it.allowed_vary) / 3ull, 0x7FFFFFFFull);
    const int n[3] = {(int)(len / 3u), len >= 1u ? (int)((len - 1u) / 3u) : 0, len >= 2u ? (int)((len - 2u) / 3u) : 0};
    const uint32_t n_chunks = max(1u, ((uint32_t)n[0] + 63u) / 64u);
    GsFrame F[3];
    int found = -1;
    uint32_t cur = gs_load(w, len, rev, 0, lane);
    for (uint32_t c = 0; c < n_chunks; ++c) {
        const uint32_t nxt = gs_load(w, len, rev, c + 1, lane);         // (on its way while this chunk is judged; behind the window it reads nothing)
        const int base = (int)(c * 64u);
        uint32_t nb = __shfl_down(cur, 1, 64);
        const uint32_t first_of_next = __shfl(nxt, 0, 64);
        if (lane == 63) nb = first_of_next;
        const uint32_t ch[5] = {cur & 7u, (cur >> 3) & 7u, (cur >> 6) & 7u, nb & 7u, (nb >> 3) & 7u};
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            if (!tried[f] || F[f].phase == GS_DONE) continue;
            bool is_m, is_x;
            gs_classify(ch[f], ch[f + 1], ch[f + 2], stops, base + (int)lane < n[f], is_m, is_x);
            const unsigned long long M = __ballot(is_m), X = __ballot(is_x);
            gs_advance(F[f], M, X, base, a, b, n[f]);
        }
        // fixed already?  the tried frames in ascending order: final ones up to the first CDS
        bool open = false;
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            if (!tried[f] || open || found >= 0) continue;
            if (F[f].phase != GS_DONE) open = true;
            else if (gs_kind(F[f], it.ref_len, it.allowed_vary) == PEP_GENESTRUCT_CDS) found = f;
        }
        if (!open) break;
        cur = nxt;
    }
    if (lane == 0) {
        const int first = tried[0] ? 0 : tried[1] ? 1 : 2;
        const int of = found >= 0 ? found : first;                      // (values selected, F never indexed by a variable: the frames stay in registers)
        const int start = of == 0 ? F[0].start : of == 1 ? F[1].start : F[2].start;
        const int stop = of == 0 ? F[0].stop : of == 1 ? F[1].stop : F[2].stop;
        const uint32_t k0 = gs_kind(F[0], it.ref_len, it.allowed_vary), k1 = gs_kind(F[1], it.ref_len, it.allowed_vary), k2 = gs_kind(F[2], it.ref_len, it.allowed_vary);
        start_aa[i] = (uint32_t)start;
        stop_aa[i] = stop < 0 ? PEP_GENESTRUCT_NO_STOP : (uint32_t)stop;
        verdict[i] = (uint8_t)((first == 0 ? k0 : first == 1 ? k1 : k2) | ((uint32_t)(found + 1) << 2));
    }
}

const char *const K19_ME = "pep_gene_structure: ";

// every check of the tables, on the host, before anything is launched; also makes the kernel's item records
int k19_check(const uint64_t *seq_off, uint32_t n_seq, uint32_t n_pred, const uint32_t *seq, const uint64_t *win_off, const uint32_t *win_len, const uint8_t *flags,
              const uint32_t *lp, const uint32_t *allowed_vary, const uint32_t *ref_len, std::vector<GsItem> *items, std::string &msg)
{
    const auto bad = [&](int code, const std::string &text) { msg = K19_ME + text; return code; };
    if (!seq_off || (n_pred && (!seq || !win_off || !win_len || !flags || !lp || !allowed_vary || !ref_len))) return bad(PEP_ERR_ARG, "null table");
    if (seq_off[0] != 0) return bad(PEP_ERR_ARG, "seq_off must start at 0");
    for (uint32_t s = 0; s < n_seq; ++s)
        if (seq_off[s + 1] < seq_off[s]) return bad(PEP_ERR_ARG, "seq_off must be non-decreasing (sequence " + std::to_string(s) + ")");
    if (items) items->resize(n_pred);
    uint32_t p = 0;
    const auto who = [&] { return "prediction " + std::to_string(p); };            // (made only for a message)
    for (; p < n_pred; ++p) {
        if (seq[p] >= n_seq) return bad(PEP_ERR_ARG, who() + " names sequence " + std::to_string(seq[p]) + " of " + std::to_string(n_seq));
        if (win_len[p] >= PEP_GENESTRUCT_MAX_WINDOW) return bad(PEP_ERR_LIMIT, "the window of " + who() + " holds 2^31 nucleotides or more");
        const uint64_t seq_len = seq_off[seq[p] + 1] - seq_off[seq[p]];
        if (win_off[p] > seq_len || win_len[p] > seq_len - win_off[p])
            return bad(PEP_ERR_ARG, "the window of " + who() + " leaves its sequence of " + std::to_string(seq_len) + " nucleotides");
        if ((flags[p] & 0x0Eu) == 0) return bad(PEP_ERR_ARG, who() + " has no tried frame");
        if (flags[p] & 0xF0u) return bad(PEP_ERR_ARG, who() + " has flag bits above bit 3");
        if (ref_len[p] == 0) return bad(PEP_ERR_ARG, "ref_len of " + who() + " is 0");
        if (items) (*items)[p] = GsItem{seq_off[seq[p]] + win_off[p], win_len[p], lp[p], allowed_vary[p], ref_len[p], flags[p], 0u};
    }
    return PEP_OK;
}

}  // namespace

extern "C" {

int pep_gene_structure_check(const uint64_t *seq_off, uint32_t n_seq, uint32_t n_pred, const uint32_t *seq, const uint64_t *win_off, const uint32_t *win_len,
                             const uint8_t *flags, const uint32_t *lp, const uint32_t *allowed_vary, const uint32_t *ref_len, char *msg, uint64_t msg_cap)
{
    std::string text;
    const int rc = k19_check(seq_off, n_seq, n_pred, seq, win_off, win_len, flags, lp, allowed_vary, ref_len, nullptr, text);
    return pep_message_out(rc, text, msg, msg_cap);
}

int pep_gene_structure(pep_ctx *ctx, const uint8_t *nt, const uint64_t *seq_off, uint32_t n_seq, uint32_t n_pred, const uint32_t *seq, const uint64_t *win_off,
                       const uint32_t *win_len, const uint8_t *flags, const uint32_t *lp, const uint32_t *allowed_vary, const uint32_t *ref_len, int table4,
                       int32_t *frame, uint32_t *start_aa, uint32_t *stop_aa, uint8_t *kind)
{
    if (!ctx) return PEP_ERR_ARG;
    if (n_pred && (!frame || !start_aa || !stop_aa || !kind)) return pep_fail(ctx, PEP_ERR_ARG, std::string(K19_ME) + "null table");
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    CallTimes &times = ctx->calls[PEP_CALL_GENE_STRUCTURE];
    times = {};
    std::vector<GsItem> items;
    std::string msg;
    const int rc = k19_check(seq_off, n_seq, n_pred, seq, win_off, win_len, flags, lp, allowed_vary, ref_len, &items, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    if (n_pred == 0) return PEP_OK;
    const uint64_t n_nt = seq_off[n_seq];
    if (n_nt && !nt) return pep_fail(ctx, PEP_ERR_ARG, std::string(K19_ME) + "null table");
    DevBuf *W = ctx->k19;
    hipStream_t st = ctx->stream;
    PEP_TRY(pep_tables_to_device(ctx, W, {{K19_NT, nt, n_nt, 16}, {K19_ITEM, items.data(), (size_t)n_pred * sizeof(GsItem), 0}, {K19_START, nullptr, (size_t)n_pred * 4, 0},
                                          {K19_STOP, nullptr, (size_t)n_pred * 4, 0}, {K19_VERDICT, nullptr, n_pred, 0}}));
    pep_timed_stage(ctx, times.ms[0], [&] {
        hipLaunchKernelGGL(gene_structure, dim3((unsigned)ceil_div(n_pred, 4)), dim3(256), 0, st, W[K19_NT].as<const uint8_t>(), W[K19_ITEM].as<const GsItem>(), n_pred,
                           table4 ? GS_STOPS_TABLE4 : GS_STOPS, W[K19_START].as<uint32_t>(), W[K19_STOP].as<uint32_t>(), W[K19_VERDICT].as<uint8_t>());
    });
    PEP_HIP(ctx, hipGetLastError());
    // the results wait in memory of the library until the stream has been waited for: on an error nothing is written
    std::vector<uint32_t> h_start(n_pred), h_stop(n_pred);
    std::vector<uint8_t> h_verdict(n_pred);
    PEP_TRY(pep_d2h_queue(ctx, h_start.data(), W[K19_START].p, (size_t)n_pred * 4));
    PEP_TRY(pep_d2h_queue(ctx, h_stop.data(), W[K19_STOP].p, (size_t)n_pred * 4));
    PEP_TRY(pep_d2h_queue(ctx, h_verdict.data(), W[K19_VERDICT].p, n_pred));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    memcpy(start_aa, h_start.data(), (size_t)n_pred * 4);
    memcpy(stop_aa, h_stop.data(), (size_t)n_pred * 4);
    for (uint32_t p = 0; p < n_pred; ++p) {                              // one byte per prediction came back: the first tried frame's outcome, and the frame found + 1
        kind[p] = h_verdict[p] & 3u;
        frame[p] = (int32_t)(h_verdict[p] >> 2) - 1;
    }
    times.bytes_to_device = n_nt + (uint64_t)n_pred * sizeof(GsItem);
    times.bytes_to_host = 9ull * n_pred;
    return PEP_OK;
}

}  // extern "C"
