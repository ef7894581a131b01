// K7: nucleotide rescoring counts (the reference's cigar2score, called from RunBlast.reScore uberBlast.py:397-415): mode 1 (uberBlast.py:226-249) in
// k7_rescore / k7_hits, modes 2 and 3 - the codon grid, uberBlast.py:250-269 - in k7_codons further down.  Mode 1:  One wavefront per hit walks the nt CIGAR; the 64 lanes stride over the
// columns of every M run comparing encoded bases (A0 C1 G3 T4 other 2, uberBlast.py:270-271; a reverse-strand hit
// reads the reference backwards as 4 - code, uberBlast.py:412).  Integer outputs only: the float identity / score
// and numpy's round-half-even are applied on the host in float64 exactly as the reference does.
// Scan of 2 x aligned length bytes per hit; the sequences of a search (tens of MB) stay in the L2 / Infinity Cache, so what bounds it is
// the latency of the byte loads, not HBM bandwidth.  Tried in round 2 and dropped: 16 columns per lane and trip through unaligned 16-byte
// loads (+ a byte-swapped window for reverse-strand hits) - 2 to 2.7x SLOWER (216 - 290 us instead of 107 us per call on the mapping
// workload of tools/other_kernels.py): the unaligned wide loads are split by the memory pipeline and the per-byte decoding then costs
// more than the 16 short trips of the byte version.
#include <cstring>
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

__global__ __launch_bounds__(256) void k7_rescore(uint64_t n, const pep_nt_hit *__restrict__ hits, const uint32_t *__restrict__ cigar,
                                                  const uint8_t *__restrict__ q_nt, const uint64_t *__restrict__ q_off,
                                                  const uint8_t *__restrict__ r_nt, const uint64_t *__restrict__ r_off, long long *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const uint64_t h = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (h >= n) return;
    const pep_nt_hit hit = hits[h];
    const uint8_t *q = q_nt + q_off[hit.q], *r = r_nt + r_off[hit.r];
    const bool rev = hit.rs >= hit.re;           // a one-base range is read complemented: the reference's `t[8] < t[9]` is false there (uberBlast.py:412)
    long long qi = (long long)hit.qs - 1, ri = (long long)hit.rs - 1;
    long long nmatch = 0, ncol = 0, ngap = 0, bgap = 0, mgap = 0;
    const uint32_t *cg = cigar + hit.cigar_off;
    for (uint32_t k = 0; k < hit.cigar_runs; ++k) {
        const uint32_t run = cg[k];
        const long long len = run >> 2;
        const uint32_t op = run & 3u;
        if (op == 0) {
            for (long long x = lane; x < len; x += 64) {
                const int a = enc(q[qi + x]);
                const int b = rev ? 4 - enc(r[ri - x]) : enc(r[ri + x]);
                nmatch += (a == b) ? 1 : 0;
            }
            ncol += len;
            qi += len; ri += rev ? -len : len;
        } else {
            ++ngap; bgap += len; if (len > 3) mgap += len;
            if (op == 1) qi += len; else ri += rev ? -len : len;
        }
    }
    for (int d = 32; d > 0; d >>= 1) nmatch += __shfl_xor(nmatch, d, 64);
    if (lane == 0) {
        long long *o = out + h * 5;
        o[0] = nmatch; o[1] = ncol - nmatch; o[2] = ngap; o[3] = bgap; o[4] = mgap;
    }
}

// K7 over the hits of a search where they lie - the device copy of the table the search has just emitted (pep_set_nt_match).  The table row a hit becomes is a
// function of the hit and of K1's descriptors of its two packed sequences (pep_table_from_hits: parseDiamond's / parseBlast's coordinate algebra, uberBlast.py:25-58,
// 275-290), so the walk can start from the hit itself: no table is uploaded again, no second round trip, and of K7's five counts only this one needs the sequences -
// the gap counts are functions of the CIGAR alone and are taken by the host while it builds the table.
//   TOOL 0, translated search: CIGAR runs count residues (x 3), the query's frame and the target's (sequence, frame, chunk offset) give the nucleotide coordinates
//   TOOL 1, nucleotide search: runs count bases, a target is a strand of its sequence
template <int TOOL, typename DESC>
__global__ __launch_bounds__(256) void k7_hits(uint64_t n_bound, const uint32_t *__restrict__ d_n_hits, const pep_hit *__restrict__ hits, const uint32_t *__restrict__ cigar,
                                               const DESC *__restrict__ q_desc, const DESC *__restrict__ t_desc,
                                               const uint8_t *__restrict__ q_nt, const uint64_t *__restrict__ q_off,
                                               const uint8_t *__restrict__ r_nt, const uint64_t *__restrict__ r_off, uint32_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const uint64_t h = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t n = d_n_hits ? min((uint64_t)*d_n_hits, n_bound) : n_bound;
    if (h >= n) return;
    const pep_hit hit = hits[h];
    long long qi, ri;
    bool rev;                                    // from the target's descriptor, not from rs >= re as in k7_rescore: a search emits no one-base reference range
    uint32_t r_seq;
    if (TOOL == 0) {
        const PackDesc dq = reinterpret_cast<const PackDesc *>(q_desc)[hit.q], dt = reinterpret_cast<const PackDesc *>(t_desc)[hit.t];
        r_seq = dt.seq;
        const long long rl = (long long)(r_off[r_seq + 1] - r_off[r_seq]), rf = dt.frame, rs_aa = (long long)hit.t_start + dt.aa_off;
        rev = rf > 3;
        qi = (long long)hit.q_start * 3 + dq.frame - 3 - 1;
        ri = (rev ? rl - (rs_aa * 3 + rf - 6) + 1 : rs_aa * 3 + rf - 3) - 1;
    } else {
        const NuclDesc dt = reinterpret_cast<const NuclDesc *>(t_desc)[hit.t];
        r_seq = dt.seq;
        const long long sl = (long long)(r_off[r_seq + 1] - r_off[r_seq]);
        rev = dt.rev != 0;
        qi = (long long)hit.q_start - 1;
        ri = (rev ? sl - (long long)hit.t_start + 1 : (long long)hit.t_start) - 1;
    }
    const uint8_t *q = q_nt + q_off[hit.q], *r = r_nt + r_off[r_seq];
    uint32_t nmatch = 0;
    const uint32_t *cg = cigar + hit.cigar_off;
    for (uint32_t k = 0; k < hit.cigar_runs; ++k) {
        const uint32_t run = cg[k];
        const long long len = (long long)(run >> 2) * (TOOL == 0 ? 3 : 1);
        const uint32_t op = run & 3u;
        if (op == 0) {
            for (long long x = lane; x < len; x += 64) {
                const int a = enc(q[qi + x]);
                const int b = rev ? 4 - enc(r[ri - x]) : enc(r[ri + x]);
                nmatch += (a == b) ? 1u : 0u;
            }
            qi += len; ri += rev ? -len : len;
        } else if (op == 1) qi += len;
        else ri += rev ? -len : len;
    }
    for (int d = 32; d > 0; d >>= 1) nmatch += __shfl_xor(nmatch, d, 64);
    if (lane == 0) out[h] = nmatch;
}

// K7 over the codon grid: the integer counts of modes 2 and 3 (cigar2score, uberBlast.py:250-269).  The columns of a hit are those of its M and I runs; from
// the query's phase on they are cut into whole codons.  One wavefront per hit as in k7_rescore.  A first pass over the runs - the same for all lanes, so it
// runs on the scalar unit - gives the number of columns and the three gap counts.  Then lane l takes the codons l, l + 64, ... : a codon may straddle run
// boundaries (M|I|M inside one codon) and nothing ties it to the 64-lane trip of a run, so every lane finds its three columns with a cursor of its own - run
// index, the run's first column, the query and reference bases in front of the run - which only moves forward: at most cigar_runs steps per lane over the
// whole hit, next to (columns / 64) byte loads.  Nothing is carried from lane to lane or from trip to trip.
// MODE 2 translates the codons without an I column through the caller's tables, staged in LDS once per block (125 + 1 024 bytes); MODE 3 needs neither.
struct CodonCursor {
    uint32_t k = 0;                              // run the cursor stands in
    long long col0 = 0, q0 = 0, r0 = 0;          // first column of that run; query / reference bases the runs in front of it consume
};

template <int MODE>
__global__ __launch_bounds__(256) void k7_codons(uint64_t n, const pep_nt_hit *__restrict__ hits, const uint32_t *__restrict__ cigar,
                                                 const uint8_t *__restrict__ q_nt, const uint64_t *__restrict__ q_off,
                                                 const uint8_t *__restrict__ r_nt, const uint64_t *__restrict__ r_off,
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
    const uint8_t *q = q_nt + q_off[hit.q] + ((long long)hit.qs - 1), *r = r_nt + r_off[hit.r] + ((long long)hit.rs - 1);
    const bool rev = hit.rs >= hit.re;
    const uint32_t *cg = cigar + hit.cigar_off;
    long long ncol = 0, ngap = 0, bgap = 0, mgap = 0;
    for (uint32_t k = 0; k < hit.cigar_runs; ++k) {
        const uint32_t run = cg[k];
        const long long len = run >> 2;
        if ((run & 3u) != 2) ncol += len;
        if ((run & 3u) != 0) { ++ngap; bgap += len; if (len > 3) mgap += len; }
    }
    const long long phase = ((long long)hit.qs - 1) % 3;
    const long long whole = ncol > phase ? (ncol - phase) / 3 : 0;
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;    // mode 3: hit0 hit1 hit2 paired; mode 2: aa_match codons
    long long sub_sum = 0;
    CodonCursor cur;
    for (long long c = lane; c < whole; c += 64) {
        int a[3], b[3];
        for (int j = 0; j < 3; ++j) {
            const long long p = phase + 3 * c + j;   // < ncol: the cursor stops inside the runs
            uint32_t run = cg[cur.k];
            while ((run & 3u) == 2 || p >= cur.col0 + (long long)(run >> 2)) {
                const long long len = run >> 2;
                if ((run & 3u) != 2) { cur.col0 += len; cur.q0 += len; }
                if ((run & 3u) != 1) cur.r0 += len;
                run = cg[++cur.k];
            }
            const long long x = p - cur.col0;
            a[j] = enc(q[cur.q0 + x]);
            b[j] = -1;
            if ((run & 3u) == 0) b[j] = rev ? 4 - enc(r[-(cur.r0 + x)]) : enc(r[cur.r0 + x]);
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
    long long v0 = c0, v1 = c1, v2 = MODE == 3 ? (long long)c2 : sub_sum, v3 = c3;
    for (int d = 32; d > 0; d >>= 1) {
        v0 += __shfl_xor(v0, d, 64); v1 += __shfl_xor(v1, d, 64); v2 += __shfl_xor(v2, d, 64);
        if (MODE == 3) v3 += __shfl_xor(v3, d, 64);
    }
    if (lane == 0) {
        long long *o = out + h * 7;
        o[0] = v0; o[1] = v1; o[2] = v2; o[3] = v3; o[4] = ngap; o[5] = bgap; o[6] = mgap;
    }
}

}  // namespace

// queued behind a search on its stream: counts for hits [0, n) - or [0, *d_n_hits) with n as the bound when the count is still on the device - into
// ctx->pin_nt_match; the caller waits for the stream.  The packed sets must come from the context's nucleotide sets (K1 or pep_use_nt_as_residues).
int pep_k7_hits_queue(pep_ctx *ctx, uint64_t n, const pep_hit *d_hits, const uint32_t *d_cigar, const uint32_t *d_n_hits)
{
    if (n == 0) return PEP_OK;
    if (!ctx->q_nt.nt.p || !ctx->r_nt.nt.p) return pep_fail(ctx, PEP_ERR_STATE, "pep_set_nt_match needs pep_set_query_nt and pep_set_ref_nt first");
    const bool nucl = ctx->resid_from_nucl;
    if (!nucl && !(ctx->q_from_nt && ctx->t_from_nt))
        return pep_fail(ctx, PEP_ERR_STATE, "pep_set_nt_match: the packed sets of this search were not made from the context's nucleotide sets");
    if (nucl ? (!ctx->nucl_q.d_desc.p || !ctx->nucl_t.d_desc.p) : (!ctx->d_k1_desc_q.p || !ctx->d_k1_desc_t.p))
        return pep_fail(ctx, PEP_ERR_STATE, "pep_set_nt_match: no descriptors of the packed sets on the device");
    PEP_TRY(dev_reserve(ctx, ctx->d_nt_match, n * 4));
    PEP_TRY(pin_reserve(ctx, ctx->pin_nt_match, n * 4));
    const dim3 grid((unsigned)ceil_div(n, 4)), block(256);
    uint32_t *out = ctx->d_nt_match.as<uint32_t>();
    if (nucl)
        hipLaunchKernelGGL((k7_hits<1, NuclDesc>), grid, block, 0, ctx->stream, n, d_n_hits, d_hits, d_cigar, ctx->nucl_q.d_desc.as<const NuclDesc>(), ctx->nucl_t.d_desc.as<const NuclDesc>(),
                           ctx->q_nt.nt.as<const uint8_t>(), ctx->q_nt.off.as<const uint64_t>(), ctx->r_nt.nt.as<const uint8_t>(), ctx->r_nt.off.as<const uint64_t>(), out);
    else
        hipLaunchKernelGGL((k7_hits<0, PackDesc>), grid, block, 0, ctx->stream, n, d_n_hits, d_hits, d_cigar, ctx->d_k1_desc_q.as<const PackDesc>(), ctx->d_k1_desc_t.as<const PackDesc>(),
                           ctx->q_nt.nt.as<const uint8_t>(), ctx->q_nt.off.as<const uint64_t>(), ctx->r_nt.nt.as<const uint8_t>(), ctx->r_nt.off.as<const uint64_t>(), out);
    PEP_HIP(ctx, hipGetLastError());
    PEP_HIP(ctx, hipMemcpyAsync(ctx->pin_nt_match.p, out, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    return PEP_OK;
}

// what both entry points hold a table of hits to before anything is uploaded, so that a bad table is an error, not an out-of-bounds read: indices,
// CIGAR slices, op codes, and coordinates that agree with the runs and lie inside the two sequences (q_off / r_off: offsets of the nucleotide sets)
int pep_k7_check(const char *who, uint64_t n, const pep_nt_hit *h_hits, const uint32_t *h_cigar, uint64_t n_cigar, const uint64_t *q_off, uint64_t n_q,
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

int pep_k7_codons_check(uint64_t n, const pep_nt_hit *h_hits, const uint32_t *h_cigar, uint64_t n_cigar, int32_t mode, const uint8_t *aa_of_word, const int8_t *sub,
                        const uint64_t *q_off, uint64_t n_q, const uint64_t *r_off, uint64_t n_r, std::string &msg)
{
    const int rc = k7_codons_check_tables(mode, aa_of_word, sub, msg);
    if (rc != PEP_OK || n == 0) return rc;
    if (!h_hits || !h_cigar || !q_off || !r_off) { msg = "pep_rescore_codons: NULL table"; return PEP_ERR_ARG; }
    return pep_k7_check("pep_rescore_codons", n, h_hits, h_cigar, n_cigar, q_off, n_q, r_off, n_r, msg);
}

int pep_k7_rescore(pep_ctx *ctx, uint64_t n, const pep_nt_hit *h_hits, const uint32_t *h_cigar, uint64_t n_cigar, int64_t *h_out)
{
    if (n == 0) return PEP_OK;
    if (!ctx->q_nt.nt.p || !ctx->r_nt.nt.p) return pep_fail(ctx, PEP_ERR_STATE, "pep_rescore_nt needs pep_set_query_nt and pep_set_ref_nt first");
    std::string msg;
    const int rc = pep_k7_check("pep_rescore_nt", n, h_hits, h_cigar, n_cigar, ctx->q_nt.h_off.data(), ctx->q_nt.n, ctx->r_nt.h_off.data(), ctx->r_nt.n, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    PEP_TRY(dev_reserve(ctx, ctx->ws[0], n * sizeof(pep_nt_hit)));
    PEP_TRY(dev_reserve(ctx, ctx->ws[1], (n_cigar + 1) * 4));
    PEP_TRY(dev_reserve(ctx, ctx->ws[2], n * 5 * 8));
    PEP_TRY(pep_h2d(ctx, ctx->ws[0].p, h_hits, n * sizeof(pep_nt_hit)));
    PEP_TRY(pep_h2d(ctx, ctx->ws[1].p, h_cigar, n_cigar * 4));
    hipLaunchKernelGGL(k7_rescore, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, ctx->stream, n, ctx->ws[0].as<const pep_nt_hit>(), ctx->ws[1].as<const uint32_t>(),
                       ctx->q_nt.nt.as<const uint8_t>(), ctx->q_nt.off.as<const uint64_t>(), ctx->r_nt.nt.as<const uint8_t>(), ctx->r_nt.off.as<const uint64_t>(),
                       ctx->ws[2].as<long long>());
    PEP_HIP(ctx, hipGetLastError());
    PEP_TRY(pep_d2h_queue(ctx, h_out, ctx->ws[2].p, n * 5 * 8));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    return PEP_OK;
}

int pep_k7_codons(pep_ctx *ctx, uint64_t n, const pep_nt_hit *h_hits, const uint32_t *h_cigar, uint64_t n_cigar, int32_t mode, const uint8_t *aa_of_word,
                  const int8_t *sub, int64_t *h_out)
{
    std::string msg;
    int rc = k7_codons_check_tables(mode, aa_of_word, sub, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    if (n == 0) return PEP_OK;
    if (!ctx->q_nt.nt.p || !ctx->r_nt.nt.p) return pep_fail(ctx, PEP_ERR_STATE, "pep_rescore_codons needs pep_set_query_nt and pep_set_ref_nt first");
    rc = pep_k7_check("pep_rescore_codons", n, h_hits, h_cigar, n_cigar, ctx->q_nt.h_off.data(), ctx->q_nt.n, ctx->r_nt.h_off.data(), ctx->r_nt.n, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    PEP_TRY(dev_reserve(ctx, ctx->ws[0], n * sizeof(pep_nt_hit)));
    PEP_TRY(dev_reserve(ctx, ctx->ws[1], (n_cigar + 1) * 4));
    PEP_TRY(dev_reserve(ctx, ctx->ws[2], n * 7 * 8));
    PEP_TRY(dev_reserve(ctx, ctx->ws[3], 128 + 1024));
    PEP_TRY(pep_h2d(ctx, ctx->ws[0].p, h_hits, n * sizeof(pep_nt_hit)));
    PEP_TRY(pep_h2d(ctx, ctx->ws[1].p, h_cigar, n_cigar * 4));
    uint8_t tables[128 + 1024] = {0};            // aa_of_word at 0, sub at 128; alive until the stream has been waited for
    if (mode == 2) {
        memcpy(tables, aa_of_word, 125);
        memcpy(tables + 128, sub, 1024);
        PEP_TRY(pep_h2d(ctx, ctx->ws[3].p, tables, sizeof(tables)));
    }
    const dim3 grid((unsigned)ceil_div(n, 4)), block(256);
    if (mode == 2)
        hipLaunchKernelGGL(k7_codons<2>, grid, block, 0, ctx->stream, n, ctx->ws[0].as<const pep_nt_hit>(), ctx->ws[1].as<const uint32_t>(), ctx->q_nt.nt.as<const uint8_t>(),
                           ctx->q_nt.off.as<const uint64_t>(), ctx->r_nt.nt.as<const uint8_t>(), ctx->r_nt.off.as<const uint64_t>(), ctx->ws[3].as<const uint8_t>(), ctx->ws[2].as<long long>());
    else
        hipLaunchKernelGGL(k7_codons<3>, grid, block, 0, ctx->stream, n, ctx->ws[0].as<const pep_nt_hit>(), ctx->ws[1].as<const uint32_t>(), ctx->q_nt.nt.as<const uint8_t>(),
                           ctx->q_nt.off.as<const uint64_t>(), ctx->r_nt.nt.as<const uint8_t>(), ctx->r_nt.off.as<const uint64_t>(), ctx->ws[3].as<const uint8_t>(), ctx->ws[2].as<long long>());
    PEP_HIP(ctx, hipGetLastError());
    PEP_TRY(pep_d2h_queue(ctx, h_out, ctx->ws[2].p, n * 7 * 8));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    return PEP_OK;
}
