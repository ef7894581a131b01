// K7: the integer counts of nucleotide rescoring (the reference's cigar2score, called from RunBlast.reScore uberBlast.py:397-415).  One wavefront per hit in
// every kernel; the float identity / score and numpy's round-half-even are applied on the host in float64 exactly as the reference does.  The pieces:
//   HitStart + k7_start    where a hit starts: its first aligned base in either sequence, its strand, its CIGAR runs, the bases a run's unit stands for -
//                          made from a row of an uploaded table (pep_nt_hit) or from a search's own hit and K1's descriptors of its packed sequences
//   k7_match_columns       mode 1 (uberBlast.py:226-249): the 64 lanes stride over the columns of every M run comparing encoded bases (A0 C1 G3 T4 other 2,
//                          uberBlast.py:270-271; a reverse-strand hit reads the reference backwards as 4 - code, uberBlast.py:412)
//   k7_gap_pass            columns and the three gap counts of a hit: functions of its runs alone, the same in all lanes, taken before the lanes part
//   wave_sum               the xor-shuffle sum over the wavefront
//   k7_table<MODE>         a table of hits: MODE 1 = match walk, 2 + 3 counts per hit; MODE 2 / 3 = the codon grid (uberBlast.py:250-269), 4 + 3 counts
//   k7_hits<TOOL>          the match walk over the hits of a search where they lie, bounded by a count on the device, one uint32 per hit
//   k7_rescore             the one host call behind pep_rescore_nt and pep_rescore_codons
// Mode 1 scans 2 x aligned length bytes per hit; the sequences of a search (tens of MB) stay in the L2 / Infinity Cache, so what bounds it is the latency of
// the byte loads, not HBM bandwidth.  Tried in round 2 and dropped: 16 columns per lane and trip through unaligned 16-byte loads (+ a byte-swapped window
// for reverse-strand hits) - 2 to 2.7x SLOWER (216 - 290 us instead of 107 us per call on the mapping workload of tools/other_kernels.py): the unaligned
// wide loads are split by the memory pipeline and the per-byte decoding then costs more than the 16 short trips of the byte version.
// The codon grid: the columns of a hit are those of its M and I runs; from the query's phase on they are cut into whole codons, and lane l takes the codons
// l, l + 64, ...  A codon may straddle run boundaries (M|I|M inside one codon) and nothing ties it to the 64-lane trip of a run, so every lane finds its
// three columns with a cursor of its own - run index, the run's first column, the query and reference bases in front of the run - which only moves forward:
// at most cigar_runs steps per lane over the whole hit, next to (columns / 64) byte loads.  Nothing is carried from lane to lane or from trip to trip.
// MODE 2 translates the codons without an I column through the caller's tables, staged in LDS once per block (125 + 1 024 bytes); MODE 3 needs neither.
#include <cstring>
#include <type_traits>
#include "common.h"

namespace {

__device__ __forceinline__ int enc(uint8_t ch)
{
    switch (ch & 0xDF) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 3;
        case 'T': return 4;
        default: return 2;
    }
}

struct K7Seqs {                                  // the context's two nucleotide sets on the device
    const uint8_t *q_nt; const uint64_t *q_off;
    const uint8_t *r_nt; const uint64_t *r_off;
};

struct HitStart {
    const uint8_t *q, *r;                        // the first aligned base of the query and of the reference; a reverse-strand hit reads r[0], r[-1], ... complemented
    bool rev;
    const uint32_t *cg;                          // the hit's runs, len << 2 | op
    uint32_t runs;
    int unit;                                    // bases per unit of a run's length
};

__device__ __forceinline__ HitStart k7_start(const pep_nt_hit &hit, const uint32_t *cigar, const K7Seqs &s)
{
    // rs >= re: a one-base range is read complemented - the reference's `t[8] < t[9]` is false there (uberBlast.py:412)
    return {s.q_nt + s.q_off[hit.q] + ((long long)hit.qs - 1), s.r_nt + s.r_off[hit.r] + ((long long)hit.rs - 1), hit.rs >= hit.re, cigar + hit.cigar_off, hit.cigar_runs, 1};
}

// The table row a search's hit becomes is a function of the hit and of K1's descriptors of its two packed sequences (pep_table_from_hits: parseDiamond's /
// parseBlast's coordinate algebra, uberBlast.py:25-58, 275-290), so the walk can start from the hit itself.
//   TOOL 0, translated search: CIGAR runs count residues (x 3), the query's frame and the target's (sequence, frame, chunk offset) give the nucleotide coordinates
//   TOOL 1, nucleotide search: runs count bases, a target is a strand of its sequence
// The strand comes from the target's descriptor, not from rs >= re as for a table row: a search emits no one-base reference range.
template <int TOOL> using k7_desc = std::conditional_t<TOOL == 0, PackDesc, NuclDesc>;

template <int TOOL>
__device__ __forceinline__ HitStart k7_start(const pep_hit &hit, const uint32_t *cigar, const k7_desc<TOOL> *q_desc, const k7_desc<TOOL> *t_desc, const K7Seqs &s)
{
    const k7_desc<TOOL> dt = t_desc[hit.t];
    const long long rl = (long long)(s.r_off[dt.seq + 1] - s.r_off[dt.seq]);
    long long qi, ri;
    bool rev;
    if constexpr (TOOL == 0) {
        const long long rf = dt.frame, rs_aa = (long long)hit.t_start + dt.aa_off;
        rev = rf > 3;
        qi = (long long)hit.q_start * 3 + q_desc[hit.q].frame - 3 - 1;
        ri = (rev ? rl - (rs_aa * 3 + rf - 6) + 1 : rs_aa * 3 + rf - 3) - 1;
    } else {
        rev = dt.rev != 0;
        qi = (long long)hit.q_start - 1;
        ri = (rev ? rl - (long long)hit.t_start + 1 : (long long)hit.t_start) - 1;
    }
    return {s.q_nt + s.q_off[hit.q] + qi, s.r_nt + s.r_off[dt.seq] + ri, rev, cigar + hit.cigar_off, hit.cigar_runs, TOOL == 0 ? 3 : 1};
}

// the lane's share of the hit's identical columns.  32 bits hold it, and the sum over the wavefront: the M columns of a table row are at most its reference
// range, rhi - rlo + 1 <= 2^32 - 1 of uint32 coordinates with rlo >= 1 (k7_check); a search's hit aligns packed sequences of at most PEP_MAX_SEQ_LEN = 2^23 - 256 residues, of 3 bases at the most
__device__ __forceinline__ uint32_t k7_match_columns(const HitStart &s, int lane)
{
    const uint8_t *q = s.q, *r = s.r;
    uint32_t nmatch = 0;
    for (uint32_t k = 0; k < s.runs; ++k) {
        const uint32_t run = s.cg[k], op = run & 3u;
        const long long len = (long long)(run >> 2) * s.unit;
        if (op == 0)
            for (long long x = lane; x < len; x += 64)
                nmatch += enc(q[x]) == (s.rev ? 4 - enc(r[-x]) : enc(r[x])) ? 1u : 0u;
        if (op != 2) q += len;
        if (op != 1) r += s.rev ? -len : len;
    }
    return nmatch;
}

// a table row's columns - the bases of its M runs, on the codon grid (I_COLUMNS) those of its I runs too - and its gap runs, their bases, the bases of
// those longer than 3
struct GapCounts { long long ncol = 0, ngap = 0, bgap = 0, mgap = 0; };

template <bool I_COLUMNS>
__device__ __forceinline__ GapCounts k7_gap_pass(const HitStart &s)
{
    GapCounts g;
    for (uint32_t k = 0; k < s.runs; ++k) {
        const uint32_t run = s.cg[k], op = run & 3u;
        const long long len = run >> 2;
        if (op == 0 || (I_COLUMNS && op == 1)) g.ncol += len;
        if (op != 0) { ++g.ngap; g.bgap += len; if (len > 3) g.mgap += len; }
    }
    return g;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

struct CodonCursor {
    uint32_t k = 0;                              // run the cursor stands in
    long long col0 = 0, q0 = 0, r0 = 0;          // first column of that run; query / reference bases the runs in front of it consume
};

// out[h]: MODE 1 nMatch nMismatch | MODE 3 hit0 hit1 hit2 paired | MODE 2 aa_match codons sub_sum 0, then nGap bGap mGap
template <int MODE>
__global__ __launch_bounds__(256) void k7_table(uint64_t n, const pep_nt_hit *__restrict__ hits, const uint32_t *__restrict__ cigar, K7Seqs seqs,
                                                const uint8_t *__restrict__ tables, long long *__restrict__ out)
{
    __shared__ uint8_t s_aa[128];
    __shared__ int8_t s_sub[1024];
    if (MODE == 2) {
        for (int i = threadIdx.x; i < 125; i += 256) s_aa[i] = tables[i];
        for (int i = threadIdx.x; i < 1024; i += 256) s_sub[i] = (int8_t)tables[128 + i];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const uint64_t h = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (h >= n) return;
    const pep_nt_hit hit = hits[h];
    const HitStart s = k7_start(hit, cigar, seqs);
    const GapCounts g = k7_gap_pass<MODE != 1>(s);
    constexpr int PAYLOAD = MODE == 1 ? 2 : 4;
    long long v[4] = {0, 0, 0, 0};
    if (MODE == 1) {
        v[0] = wave_sum(k7_match_columns(s, lane));
        v[1] = g.ncol - v[0];
    } else {
        const long long phase = ((long long)hit.qs - 1) % 3;
        const long long whole = g.ncol > phase ? (g.ncol - phase) / 3 : 0;
        uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;    // mode 3: hit0 hit1 hit2 paired; mode 2: aa_match codons
        long long sub_sum = 0;
        CodonCursor cur;
        for (long long c = lane; c < whole; c += 64) {
            int a[3], b[3];
            for (int j = 0; j < 3; ++j) {
                const long long p = phase + 3 * c + j;   // < ncol: the cursor stops inside the runs
                uint32_t run = s.cg[cur.k];
                while ((run & 3u) == 2 || p >= cur.col0 + (long long)(run >> 2)) {
                    const long long len = run >> 2;
                    if ((run & 3u) != 2) { cur.col0 += len; cur.q0 += len; }
                    if ((run & 3u) != 1) cur.r0 += len;
                    run = s.cg[++cur.k];
                }
                const long long x = p - cur.col0;
                a[j] = enc(s.q[cur.q0 + x]);
                b[j] = -1;
                if ((run & 3u) == 0) b[j] = s.rev ? 4 - enc(s.r[-(cur.r0 + x)]) : enc(s.r[cur.r0 + x]);
            }
            if (MODE == 3) {
                c0 += a[0] == b[0]; c1 += a[1] == b[1]; c2 += a[2] == b[2];
                c3 += (b[0] >= 0) + (b[1] >= 0) + (b[2] >= 0);
            } else if ((b[0] | b[1] | b[2]) >= 0) {
                const int qa = s_aa[25 * a[0] + 5 * a[1] + a[2]], ra = s_aa[25 * b[0] + 5 * b[1] + b[2]];
                c0 += qa == ra; ++c1;
                sub_sum += s_sub[(qa << 5) + ra];
            }
        }
        v[0] = wave_sum<long long>(c0); v[1] = wave_sum<long long>(c1); v[2] = wave_sum(MODE == 3 ? (long long)c2 : sub_sum);
        if (MODE == 3) v[3] = wave_sum<long long>(c3);
    }
    if (lane == 0) {
        long long *o = out + h * (PAYLOAD + 3);
        for (int j = 0; j < PAYLOAD; ++j) o[j] = v[j];
        o[PAYLOAD] = g.ngap; o[PAYLOAD + 1] = g.bgap; o[PAYLOAD + 2] = g.mgap;
    }
}

// K7 over the hits of a search where they lie - the device copy of the table the search has just emitted (pep_set_nt_match): no table is uploaded again, no
// second round trip, and of K7's five counts only this one needs the sequences - the gap counts are functions of the CIGAR alone and are taken by the host
// while it builds the table.
template <int TOOL>
__global__ __launch_bounds__(256) void k7_hits(uint64_t n_bound, const uint32_t *__restrict__ d_n_hits, const pep_hit *__restrict__ hits, const uint32_t *__restrict__ cigar,
                                               const k7_desc<TOOL> *__restrict__ q_desc, const k7_desc<TOOL> *__restrict__ t_desc, K7Seqs seqs, uint32_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const uint64_t h = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t n = d_n_hits ? min((uint64_t)*d_n_hits, n_bound) : n_bound;
    if (h >= n) return;
    const uint32_t nmatch = wave_sum(k7_match_columns(k7_start<TOOL>(hits[h], cigar, q_desc, t_desc, seqs), lane));
    if (lane == 0) out[h] = nmatch;
}

K7Seqs k7_seqs(const pep_ctx *ctx)
{
    return {ctx->q_nt.nt.as<const uint8_t>(), ctx->q_nt.off.as<const uint64_t>(), ctx->r_nt.nt.as<const uint8_t>(), ctx->r_nt.off.as<const uint64_t>()};
}

}  // namespace

// queued behind a search on its stream: counts for hits [0, n) - or [0, *d_n_hits) with n as the bound when the count is still on the device - into
// ctx->pin_nt_match; the caller waits for the stream.  The packed sets must come from the context's nucleotide sets (K1 or pep_use_nt_as_residues).
int pep_k7_hits_queue(pep_ctx *ctx, uint64_t n, const pep_hit *d_hits, const uint32_t *d_cigar, const uint32_t *d_n_hits)
{
    if (n == 0) return PEP_OK;
    if (!ctx->q_nt.nt.p || !ctx->r_nt.nt.p) return pep_fail(ctx, PEP_ERR_STATE, "pep_set_nt_match needs pep_set_query_nt and pep_set_ref_nt first");
    const bool nucl = ctx->holds == SetsHold::BaseCodes;
    if (!nucl && !(ctx->side[PEP_SIDE_Q].from_nt() && ctx->side[PEP_SIDE_T].from_nt()))
        return pep_fail(ctx, PEP_ERR_STATE, "pep_set_nt_match: the packed sets of this search were not made from the context's nucleotide sets");
    if (nucl ? (!ctx->nucl_q.d_desc.p || !ctx->nucl_t.d_desc.p) : (!ctx->d_k1_desc_q.p || !ctx->d_k1_desc_t.p))
        return pep_fail(ctx, PEP_ERR_STATE, "pep_set_nt_match: no descriptors of the packed sets on the device");
    PEP_TRY(dev_reserve(ctx, ctx->d_nt_match, n * 4));
    PEP_TRY(pin_reserve(ctx, ctx->pin_nt_match, n * 4));
    uint32_t *out = ctx->d_nt_match.as<uint32_t>();
    const auto launch = [&](auto kernel, auto *q_desc, auto *t_desc) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, ctx->stream, n, d_n_hits, d_hits, d_cigar, q_desc, t_desc, k7_seqs(ctx), out);
    };
    if (nucl) launch(k7_hits<1>, ctx->nucl_q.d_desc.as<const NuclDesc>(), ctx->nucl_t.d_desc.as<const NuclDesc>());
    else launch(k7_hits<0>, ctx->d_k1_desc_q.as<const PackDesc>(), ctx->d_k1_desc_t.as<const PackDesc>());
    PEP_HIP(ctx, hipGetLastError());
    PEP_HIP(ctx, hipMemcpyAsync(ctx->pin_nt_match.p, out, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    return PEP_OK;
}

// what both entry points hold a table of hits to before anything is uploaded, so that a bad table is an error, not an out-of-bounds read: indices,
// CIGAR slices, op codes, and coordinates that agree with the runs and lie inside the two sequences (q_off / r_off: offsets of the nucleotide sets)
static int k7_check(const char *who, uint64_t n, const pep_nt_hit *h_hits, const uint32_t *h_cigar, uint64_t n_cigar, const uint64_t *q_off, uint64_t n_q,
                    const uint64_t *r_off, uint64_t n_r, std::string &msg)
{
    for (uint64_t i = 0; i < n; ++i) {
        const pep_nt_hit &h = h_hits[i];
        if (h.q >= n_q || h.r >= n_r || h.cigar_off > n_cigar || h.cigar_runs > n_cigar - h.cigar_off) { msg = std::string(who) + ": hit index out of range"; return PEP_ERR_ARG; }
        const uint64_t ql = q_off[h.q + 1] - q_off[h.q], rl = r_off[h.r + 1] - r_off[h.r];
        uint64_t qa = 0, ra = 0;
        for (uint32_t k = 0; k < h.cigar_runs; ++k) {
            const uint32_t run = h_cigar[h.cigar_off + k];
            if ((run & 3u) == 3) { msg = std::string(who) + ": unknown CIGAR op"; return PEP_ERR_ARG; }
            if ((run & 3u) != 2) qa += run >> 2;
            if ((run & 3u) != 1) ra += run >> 2;
        }
        const bool rev = h.rs >= h.re;
        const uint64_t rlo = rev ? h.re : h.rs, rhi = rev ? h.rs : h.re;
        if (h.qs < 1 || h.qs - 1 + qa > ql || rlo < 1 || rhi > rl || ra != rhi - rlo + 1) { msg = std::string(who) + ": CIGAR inconsistent with the hit coordinates"; return PEP_ERR_ARG; }
    }
    return PEP_OK;
}

// the arguments of pep_rescore_codons that need no table of hits to be judged
static int k7_codons_check_tables(int32_t mode, const uint8_t *aa_of_word, const int8_t *sub, std::string &msg)
{
    if (mode != 2 && mode != 3) { msg = "pep_rescore_codons: mode must be 2 or 3"; return PEP_ERR_ARG; }
    if (mode == 2) {
        if (!aa_of_word || !sub) { msg = "pep_rescore_codons: mode 2 needs aa_of_word and sub"; return PEP_ERR_ARG; }
        for (int w = 0; w < 125; ++w)
            if (aa_of_word[w] >= 32) { msg = "pep_rescore_codons: aa_of_word[" + std::to_string(w) + "] is not below 32"; return PEP_ERR_ARG; }
    }
    return PEP_OK;
}

// every check of pep_rescore_codons, no device
static int k7_codons_check(uint64_t n, const pep_nt_hit *h_hits, const uint32_t *h_cigar, uint64_t n_cigar, int32_t mode, const uint8_t *aa_of_word, const int8_t *sub,
                           const uint64_t *q_off, uint64_t n_q, const uint64_t *r_off, uint64_t n_r, std::string &msg)
{
    const int rc = k7_codons_check_tables(mode, aa_of_word, sub, msg);
    if (rc != PEP_OK || n == 0) return rc;
    if (!h_hits || !h_cigar || !q_off || !r_off) { msg = "pep_rescore_codons: NULL table"; return PEP_ERR_ARG; }
    return k7_check("pep_rescore_codons", n, h_hits, h_cigar, n_cigar, q_off, n_q, r_off, n_r, msg);
}

// the slots of pep_ctx::ws (uploaded tables only: pep_k7_hits_queue reads a search's own hits where they are)
enum { K7_HITS = 0, K7_CIGAR, K7_OUT, K7_TABLES, K7_SLOTS };
static_assert(K7_SLOTS <= PEP_WS_HITS_OUT, "leaves the device-resident hit table alone");

// pep_rescore_nt (mode 1, no tables, width 5) and pep_rescore_codons (its mode and tables, width 7): checks, upload, k7_table<mode>, h_out[n, width]; `who` leads the messages.
// width 5: mode is 1 and no table is read.  width 7: the mode and the tables are the caller's and are judged first, also for n == 0 and before the state.
static int k7_rescore(pep_ctx *ctx, const char *who, uint64_t n, const pep_nt_hit *h_hits, const uint32_t *h_cigar, uint64_t n_cigar, int32_t mode,
                      const uint8_t *aa_of_word, const int8_t *sub, uint32_t width, int64_t *h_out)
{
    std::string msg;
    int rc = width == 7 ? k7_codons_check_tables(mode, aa_of_word, sub, msg) : PEP_OK;
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    if (n == 0) return PEP_OK;
    if (!ctx->q_nt.nt.p || !ctx->r_nt.nt.p) return pep_fail(ctx, PEP_ERR_STATE, std::string(who) + " needs pep_set_query_nt and pep_set_ref_nt first");
    rc = k7_check(who, n, h_hits, h_cigar, n_cigar, ctx->q_nt.h_off.data(), ctx->q_nt.n, ctx->r_nt.h_off.data(), ctx->r_nt.n, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    PEP_TRY(dev_reserve(ctx, ctx->ws[K7_HITS], n * sizeof(pep_nt_hit)));
    PEP_TRY(dev_reserve(ctx, ctx->ws[K7_CIGAR], (n_cigar + 1) * 4));
    PEP_TRY(dev_reserve(ctx, ctx->ws[K7_OUT], n * width * 8));
    PEP_TRY(pep_h2d(ctx, ctx->ws[K7_HITS].p, h_hits, n * sizeof(pep_nt_hit)));
    PEP_TRY(pep_h2d(ctx, ctx->ws[K7_CIGAR].p, h_cigar, n_cigar * 4));
    uint8_t tables[128 + 1024] = {0};            // aa_of_word at 0, sub at 128; alive until the stream has been waited for
    if (mode == 2) {
        memcpy(tables, aa_of_word, 125);
        memcpy(tables + 128, sub, 1024);
        PEP_TRY(dev_reserve(ctx, ctx->ws[K7_TABLES], sizeof(tables)));
        PEP_TRY(pep_h2d(ctx, ctx->ws[K7_TABLES].p, tables, sizeof(tables)));
    }
    hipLaunchKernelGGL(mode == 1 ? k7_table<1> : mode == 2 ? k7_table<2> : k7_table<3>, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, ctx->stream, n,
                       ctx->ws[K7_HITS].as<const pep_nt_hit>(), ctx->ws[K7_CIGAR].as<const uint32_t>(), k7_seqs(ctx), ctx->ws[K7_TABLES].as<const uint8_t>(), ctx->ws[K7_OUT].as<long long>());
    PEP_HIP(ctx, hipGetLastError());
    PEP_TRY(pep_d2h_queue(ctx, h_out, ctx->ws[K7_OUT].p, n * width * 8));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    return PEP_OK;
}

extern "C" {

int pep_rescore_nt(pep_ctx *ctx, uint64_t n, const pep_nt_hit *hits, const uint32_t *cigar, uint64_t n_cigar, int64_t *out)
{
    if (!ctx || (n && (!hits || !cigar || !out))) return PEP_ERR_ARG;
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    return k7_rescore(ctx, "pep_rescore_nt", n, hits, cigar, n_cigar, 1, nullptr, nullptr, 5, out);
}

int pep_rescore_codons(pep_ctx *ctx, uint64_t n, const pep_nt_hit *hits, const uint32_t *cigar, uint64_t n_cigar, int32_t mode, const uint8_t *aa_of_word,
                       const int8_t *sub, int64_t *out)
{
    if (!ctx || (n && (!hits || !cigar || !out))) return PEP_ERR_ARG;
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    return k7_rescore(ctx, "pep_rescore_codons", n, hits, cigar, n_cigar, mode, aa_of_word, sub, 7, out);
}

int pep_rescore_codons_check(uint64_t n, const pep_nt_hit *hits, const uint32_t *cigar, uint64_t n_cigar, int32_t mode, const uint8_t *aa_of_word,
                             const int8_t *sub, const uint64_t *q_off, uint64_t n_q, const uint64_t *r_off, uint64_t n_r, char *msg, uint64_t msg_cap)
{
    std::string text;
    const int rc = k7_codons_check(n, hits, cigar, n_cigar, mode, aa_of_word, sub, q_off, n_q, r_off, n_r, text);
    return pep_message_out(rc, text, msg, msg_cap);
}

}  // extern "C"
