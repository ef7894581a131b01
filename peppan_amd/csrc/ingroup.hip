// K17: in-group rows and gene scores of `initializing` (determineGroup PEPPAN.py:1041-1056 inside initializing2 :1058-1076): which matches of a
// gene are "in group", and the gene's score over them.  The reference walks the rows of a gene in order and, for every row i with
// iden[i] >= thr, tests the rows behind it that are not in yet - a Python lambda per row through np.vectorize, quadratic in the rows of a gene.
// Only rows with iden >= thr ("seeds") ever act as sources and the flags only grow, so the walk collapses to a test per row without an order:
//   raw[j]  = seed[j] or there is an i < j with seed[i] and (1. - iden[j] / iden[i]) / den(genome[i], genome[j]) < 1
//   keep[j] = raw[first[j]], first[j] = the first row of the gene with genome[j]'s genome (:1054-1055)
//   score   = sum of abs(score[j]) over first[j] == j and keep[j] (:1074; an int64 sum, its order is free)
// den is self_id for two rows of one genome (self_id * exp(nSigma * 0.)), else column 2 of K16's genome-pair table (gdtable.h).
//   ingroup_pairs    one workgroup per (gene, chunk of 256 rows) of a host-built list over all genes of the batch; thread t owns target row
//                    j = 256 * chunk + t.  The source rows [0, 256 * (chunk + 1)) go through LDS in panels of 256 (genome, iden); a thread that
//                    is neither a seed nor in yet walks the panel's rows i < j, skips non-seeds, looks den up and stops at its first pass.  The
//                    workgroup leaves when no thread is pending.  raw[j]: one byte.
//   ingroup_finish   the same list: keep[j] = raw[first[j]], a block reduction of abs(score[j]) over first[j] == j and keep[j], one 64-bit
//                    atomicAdd per workgroup into gene_score[g].
// The float chain is three single correctly rounded double operations (__ddiv_rn, __dsub_rn, __ddiv_rn: nothing to contract) and "< 1.0".
// first[] is made on the host (first occurrence is sequential by definition) with a small open-addressing table, in one linear pass.
// ingroup_pairs is quadratic in the rows of a gene in the worst case - many rows below thr that no seed lets in -, as the reference is.
#include "common.h"
#include "gdtable.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr uint32_t K17_CHUNK = 256;

struct IgWork { uint32_t gene, chunk; };

// the slots of pep_ctx::k17
enum { K17_GENOME = 0, K17_IDEN, K17_SCORE, K17_FIRST, K17_GENE_OFF, K17_WORK, K17_GD_KEY, K17_GD_VAL, K17_RAW, K17_KEEP, K17_GENE_SCORE, K17_SLOTS };
static_assert(K17_SLOTS == sizeof(pep_ctx::k17) / sizeof(DevBuf), "one member of pep_ctx::k17 per slot");

__device__ __forceinline__ double k17_den(const GdTable &T, uint32_t ga, uint32_t gb)
{
    return ga == gb ? T.self_id : T.val[3 * gd_row(T, ga, gb) + 2];       // self_id * exp(nSigma * 0.) == self_id
}

__global__ __launch_bounds__(256) void ingroup_pairs(const IgWork *__restrict__ work, const uint64_t *__restrict__ gene_off, const uint32_t *__restrict__ genome,
                                                     const int32_t *__restrict__ iden, const GdTable gd, const double thr, uint8_t *__restrict__ raw)
{
    __shared__ uint32_t s_genome[K17_CHUNK];
    __shared__ int32_t s_iden[K17_CHUNK];
    const IgWork W = work[blockIdx.x];
    const uint64_t base = gene_off[W.gene], n = gene_off[W.gene + 1] - base;
    const uint32_t tid = threadIdx.x;
    const uint64_t j = (uint64_t)W.chunk * K17_CHUNK + tid;
    const bool have = j < n;
    const uint32_t my_genome = have ? genome[base + j] : 0u;
    const double my_iden = have ? (double)iden[base + j] : 0.;
    int in = have && my_iden >= thr;
    int pending = have && !in;
    for (uint32_t p = 0; p <= W.chunk; ++p) {
        if (__syncthreads_count(pending) == 0) break;                   // (also: every thread is done with the panel before)
        const uint64_t i = (uint64_t)p * K17_CHUNK + tid;
        s_genome[tid] = i < n ? genome[base + i] : 0u;
        s_iden[tid] = i < n ? iden[base + i] : 0;
        __syncthreads();
        if (pending) {
            const uint64_t ahead = j - (uint64_t)p * K17_CHUNK;         // rows of this panel and behind it that lie in front of j (j < n: all of them exist)
            const uint32_t lim = ahead < K17_CHUNK ? (uint32_t)ahead : K17_CHUNK;
            for (uint32_t k = 0; k < lim; ++k) {
                const double src = (double)s_iden[k];
                if (!(src >= thr)) continue;
                const double sc = __ddiv_rn(__dsub_rn(1.0, __ddiv_rn(my_iden, src)), k17_den(gd, s_genome[k], my_genome));
                if (sc < 1.0) { in = 1; pending = 0; break; }
            }
        }
    }
    if (have) raw[base + j] = (uint8_t)in;
}

__global__ __launch_bounds__(256) void ingroup_finish(const IgWork *__restrict__ work, const uint64_t *__restrict__ gene_off, const uint32_t *__restrict__ first,
                                                      const long long *__restrict__ score, const uint8_t *__restrict__ raw, uint8_t *__restrict__ keep,
                                                      unsigned long long *gene_score)
{
    __shared__ unsigned long long s_part[K17_CHUNK / PEP_WAVE];
    const IgWork W = work[blockIdx.x];
    const uint64_t base = gene_off[W.gene], n = gene_off[W.gene + 1] - base;
    const uint32_t tid = threadIdx.x;
    const uint64_t j = (uint64_t)W.chunk * K17_CHUNK + tid;
    unsigned long long sum = 0;
    if (j < n) {
        const uint32_t f = first[base + j];
        const uint8_t k = raw[base + f];
        keep[base + j] = k;
        if (f == j && k) {
            const long long s = score[base + j];
            sum = s < 0 ? 0ull - (unsigned long long)s : (unsigned long long)s;      // abs as numpy's int64 does it (wraps at the one value that has none)
        }
    }
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((tid & 63) == 0) s_part[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        const unsigned long long total = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        if (total) atomicAdd(&gene_score[W.gene], total);
    }
}

struct Layout {
    std::vector<uint32_t> first;            // [n_rows]: position inside its gene of the first row with this row's genome
    std::vector<IgWork> work;
    std::vector<double> gd;                 // [n_gd + 1][3]
};

const char *const K17_ME = "pep_gene_ingroups: ";

// every check of the tables, on the host, before anything is launched; also makes first[] and the work list
int k17_check(const uint32_t *genome, const int32_t *iden, const int64_t *score, uint64_t n_rows, uint32_t n_genes, const uint64_t *gene_off, const uint64_t *gd_key,
              const double *gd_val, uint64_t n_gd, const double *gd_default, double self_id, double thr, Layout &L, std::string &msg)
{
    const auto bad = [&](int code, const std::string &text) { msg = K17_ME + text; return code; };
    if (!gene_off || (n_rows && (!genome || !iden || !score)) || (n_gd && (!gd_key || !gd_val)) || !gd_default) return bad(PEP_ERR_ARG, "null table");
    if (n_rows >= 0x100000000ull) return bad(PEP_ERR_LIMIT, "more than 2^32 - 1 rows");
    if (!std::isfinite(self_id)) return bad(PEP_ERR_ARG, "self_id must be finite");
    if (!std::isfinite(thr)) return bad(PEP_ERR_ARG, "thr must be finite");
    if (gene_off[0] != 0) return bad(PEP_ERR_ARG, "gene_off must start at 0");
    uint64_t longest = 0, chunks = 0;
    for (uint32_t g = 0; g < n_genes; ++g) {
        if (gene_off[g + 1] < gene_off[g]) return bad(PEP_ERR_ARG, "gene_off must be non-decreasing (gene " + std::to_string(g) + ")");
        if (gene_off[g + 1] > n_rows) return bad(PEP_ERR_ARG, "gene_off of gene " + std::to_string(g) + " runs past n_rows");
        longest = std::max(longest, gene_off[g + 1] - gene_off[g]);
        chunks += ceil_div(gene_off[g + 1] - gene_off[g], K17_CHUNK);
    }
    if (gene_off[n_genes] != n_rows) return bad(PEP_ERR_ARG, "gene_off must end at n_rows");
    for (uint64_t r = 0; r < n_rows; ++r)
        if (iden[r] < 0) return bad(PEP_ERR_ARG, "iden of row " + std::to_string(r) + " is negative");
    const std::string fault = gd_table_fault(gd_key, gd_val, n_gd, gd_default);
    if (!fault.empty()) return bad(PEP_ERR_ARG, fault);
    if (chunks > 0x7FFFFFFFull) return bad(PEP_ERR_LIMIT, "more than 2^31 - 1 chunks of 256 rows in one call (split the batch)");
    L.gd.assign(gd_val, gd_val + 3 * n_gd);
    L.gd.insert(L.gd.end(), gd_default, gd_default + 3);
    // first[]: an open-addressing table of (genome -> first position), at most half full, stamped with the gene so that it is never cleared
    unsigned bits = 4;
    while (((uint64_t)1 << bits) < 2 * longest) ++bits;
    const uint64_t mask = ((uint64_t)1 << bits) - 1;
    std::vector<uint32_t> slot_gene((size_t)mask + 1, 0xFFFFFFFFu), slot_genome((size_t)mask + 1), slot_first((size_t)mask + 1);
    L.first.resize(n_rows);
    L.work.reserve(chunks);
    for (uint32_t g = 0; g < n_genes; ++g) {
        const uint64_t base = gene_off[g], n = gene_off[g + 1] - base;
        for (uint64_t j = 0; j < n; ++j) {
            const uint32_t id = genome[base + j];
            uint64_t h = ((uint64_t)id * 0x9E3779B97F4A7C15ull) >> (64 - bits);
            while (slot_gene[h] == g && slot_genome[h] != id) h = (h + 1) & mask;
            if (slot_gene[h] != g) { slot_gene[h] = g; slot_genome[h] = id; slot_first[h] = (uint32_t)j; }
            L.first[base + j] = slot_first[h];
        }
        for (uint64_t c = 0; c < ceil_div(n, K17_CHUNK); ++c) L.work.push_back(IgWork{g, (uint32_t)c});
    }
    return PEP_OK;
}

}  // namespace

extern "C" {

// every table check, no device
int pep_gene_ingroups_check(const uint32_t *genome, const int32_t *iden, const int64_t *score, uint64_t n_rows, uint32_t n_genes, const uint64_t *gene_off,
                            const uint64_t *gd_key, const double *gd_val, uint64_t n_gd, const double *gd_default, double self_id, double thr, char *msg, uint64_t msg_cap)
{
    Layout L;
    std::string text;
    const int rc = k17_check(genome, iden, score, n_rows, n_genes, gene_off, gd_key, gd_val, n_gd, gd_default, self_id, thr, L, text);
    return pep_message_out(rc, text, msg, msg_cap);
}

int pep_gene_ingroups(pep_ctx *ctx, const uint32_t *genome, const int32_t *iden, const int64_t *score, uint64_t n_rows, uint32_t n_genes, const uint64_t *gene_off,
                      const uint64_t *gd_key, const double *gd_val, uint64_t n_gd, const double *gd_default, double self_id, double thr, uint8_t *h_keep,
                      int64_t *h_gene_score)
{
    if (!ctx) return PEP_ERR_ARG;
    if ((n_rows && !h_keep) || (n_genes && !h_gene_score)) return pep_fail(ctx, PEP_ERR_ARG, "pep_gene_ingroups: null table");
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    CallTimes &times = ctx->calls[PEP_CALL_GENE_INGROUPS];
    times = {};
    Layout L;
    std::string msg;
    const int rc = k17_check(genome, iden, score, n_rows, n_genes, gene_off, gd_key, gd_val, n_gd, gd_default, self_id, thr, L, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    if (n_genes == 0) return PEP_OK;
    if (L.work.empty()) {                                               // empty genes only: they score 0
        memset(h_gene_score, 0, (size_t)n_genes * 8);
        times.bytes_to_host = 8ull * n_genes;
        return PEP_OK;
    }
    DevBuf *W = ctx->k17;
    hipStream_t st = ctx->stream;
    PEP_TRY(pep_tables_to_device(ctx, W, {{K17_GENOME, genome, n_rows * 4, 0},          {K17_IDEN, iden, n_rows * 4, 0},
                                          {K17_SCORE, score, n_rows * 8, 0},            {K17_FIRST, L.first.data(), n_rows * 4, 0},
                                          {K17_GENE_OFF, gene_off, ((size_t)n_genes + 1) * 8, 0}, {K17_WORK, L.work.data(), L.work.size() * sizeof(IgWork), 0},
                                          {K17_GD_KEY, gd_key, n_gd * 8, 8},            {K17_GD_VAL, L.gd.data(), L.gd.size() * 8, 0},
                                          {K17_RAW, nullptr, n_rows, 0},                {K17_KEEP, nullptr, n_rows, 0},
                                          {K17_GENE_SCORE, nullptr, (size_t)n_genes * 8, 0}}));
    PEP_HIP(ctx, hipMemsetAsync(W[K17_GENE_SCORE].p, 0, (size_t)n_genes * 8, st));
    const GdTable gd{W[K17_GD_KEY].as<const uint64_t>(), W[K17_GD_VAL].as<const double>(), n_gd, self_id};
    const IgWork *d_work = W[K17_WORK].as<const IgWork>();
    const uint64_t *d_gene_off = W[K17_GENE_OFF].as<const uint64_t>();
    const dim3 grid((unsigned)L.work.size());
    pep_timed_stage(ctx, times.ms[0], [&] {
        hipLaunchKernelGGL(ingroup_pairs, grid, dim3(K17_CHUNK), 0, st, d_work, d_gene_off, W[K17_GENOME].as<const uint32_t>(), W[K17_IDEN].as<const int32_t>(), gd, thr,
                           W[K17_RAW].as<uint8_t>());
    });
    pep_timed_stage(ctx, times.ms[1], [&] {
        hipLaunchKernelGGL(ingroup_finish, grid, dim3(K17_CHUNK), 0, st, d_work, d_gene_off, W[K17_FIRST].as<const uint32_t>(), W[K17_SCORE].as<const long long>(),
                           W[K17_RAW].as<const uint8_t>(), W[K17_KEEP].as<uint8_t>(), W[K17_GENE_SCORE].as<unsigned long long>());
    });
    PEP_HIP(ctx, hipGetLastError());
    // both results wait in memory of the library until the stream has been waited for: on an error nothing is written
    std::vector<int64_t> gene_score(n_genes);
    std::vector<uint8_t> keep(n_rows);
    PEP_TRY(pep_d2h_queue(ctx, keep.data(), W[K17_KEEP].p, n_rows));
    PEP_TRY(pep_d2h_queue(ctx, gene_score.data(), W[K17_GENE_SCORE].p, (size_t)n_genes * 8));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    memcpy(h_keep, keep.data(), n_rows);
    memcpy(h_gene_score, gene_score.data(), (size_t)n_genes * 8);
    times.bytes_to_host = n_rows + 8ull * n_genes;
    return PEP_OK;
}

}  // extern "C"
