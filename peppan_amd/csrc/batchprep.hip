// K26: the front half of a round of filt_genes (PEPPAN.py:546-624, :641-656) for a batch of genes.  The definition, the tie rule of the two sorts and the
// deliberate differences are in include/peppan_hip.h (K26); tests/batchprep_helpers.py restates it in plain Python and the library equals that bit for
// bit, so contraction into fused multiply-adds is switched off for the whole file.
//   prep_screen      stage A, one workgroup per gene: the maximum of column 3, then per row the one float64 quotient, the look-up in used_state and the
//                    maximum of the rows `used` does not hold.
//   prep_prune<LDS>  stage C, one workgroup per gene: the gene's working arrays - the current order, a sort buffer, best - in LDS (LDS = true, up to
//                    PEP_PREP_LDS_ROWS rows) or in the gene's part of the workspace slot K26_SCRATCH (LDS = false); the bitmap of the walk's used2 over the
//                    gene's own rows is in LDS on both paths (PEP_PREP_MAX_ROWS bits).  Both instantiations run the SAME device functions over a PrepView
//                    whose three pointers lead into LDS or device memory, so the paths cannot differ in a bit.
//                    Every sort is one bitonic network over POSITIONS with a comparator that ends in the position itself: the keys of a sort are all different,
//                    the result does not depend on the network, and the tie rule (equal keys keep their order) needs no pass of its own.  The first row per
//                    genome comes from the order sorted by (genome, position): a binary search for the genome's first entry.  Conflict values are translated
//                    to source rows once (a binary search in the rows sorted by locus); values that name loci of other genes become -1.
//                    The walk is sequential over the gene's rows and is done by ONE wavefront, 64 rows at a time: the lanes fetch their rows' list bounds
//                    together; rows with an empty list only read their bit, rows with a list are taken in order, and a kept row's list is scattered by the
//                    whole wavefront into the bitmap (LDS operations of one wavefront are carried out in order).
//   pep_batch_unsure_walk   stage B on the host: one bitmap over the locus ids for the round's used2.
// Not tuned: the rates are in profiles/batchprep_rate.txt.  Known slack: three of a workgroup's four wavefronts wait during the walk; a bitonic network does
// log^2 passes where a radix sort would do a handful; a workgroup of 256 threads for a gene of 5 rows.
#include "common.h"
#include <algorithm>
#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace {

// the slots of ctx->ws this call uses
enum { K26_GENOME = 0, K26_C2, K26_C3, K26_C4, K26_LOCUS, K26_USED, K26_CFL_OFF, K26_CFL, K26_TR, K26_GENES, K26_WHICH, K26_SCRATCH, K26_ROWS, K26_OUT, K26_SLOTS,
       // ... and stage A, a call of its own: its offsets, its two rewritten columns, its two values per gene
       K26_A_GENE_OFF = K26_CFL_OFF, K26_A_OUT3 = K26_C2, K26_A_OUT4 = K26_C4, K26_A_PRESENT = K26_GENOME, K26_A_EXCLUDED = K26_OUT };
static_assert(K26_SLOTS <= PEP_WS_HITS_OUT, "leaves the device-resident hit table alone");

constexpr int PREP_BLOCK = 256;
constexpr int PREP_WAVES = PREP_BLOCK / 64;
constexpr uint32_t PREP_NONE = 0xFFFFFFFFu;
static_assert((PEP_PREP_LDS_ROWS & (PEP_PREP_LDS_ROWS - 1)) == 0 && 3 * 4 * PEP_PREP_LDS_ROWS + PEP_PREP_MAX_ROWS / 8 <= 60 * 1024, "prep_prune's LDS arrays");

// a gene of a call: its first row, the first conflict value of its rows and their number, its rows, the power of two its sorts run over, its part of K26_SCRATCH (in words)
struct PrepGene { uint64_t row0, cfl0, n_cfl, ws0; uint32_t n, P; };
struct PrepOut { uint32_t m, inparalog, is_final, tie; };
struct PrepDev {
    const int64_t *genome, *c2, *c3, *c4, *locus;
    const uint64_t *cfl_off;
    const int64_t *cfl;
    int32_t *tr;
    uint32_t *scratch, *rows;
    PrepOut *out;
    double clust_identity, final_threshold;
    uint32_t mode;
};
// one gene as the device functions see it: the columns from its first row on, cfl_off from its first row on, cfl and tr whole; cur, srt, best in LDS or device memory
struct PrepView {
    const int64_t *genome, *c2, *c3, *c4, *locus;
    const uint64_t *cfl_off;
    const int64_t *cfl;
    int32_t *tr;
    uint32_t *cur, *srt, *best, *flag;
    uint32_t n, P;
};
struct PrepLds { uint32_t scan[PREP_BLOCK]; uint32_t count, tie, flag; int32_t min3; long long part[PREP_WAVES]; };

// the barrier of the steps: the working arrays may lie in device memory, and the barrier instruction itself waits for no memory counter
__device__ __forceinline__ void prep_sync()
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#endif
    __syncthreads();
}

__device__ __forceinline__ uint32_t prep_pow2(uint32_t m)
{
    uint32_t P = 1;
    while (P < m) P <<= 1;
    return P;
}

// srt = the positions 0 .. m - 1 sorted by `less` (a strict total order of the positions)
template <class Less>
__device__ void prep_sort(const PrepView &V, uint32_t m, uint32_t tid, const Less &less)
{
    const uint32_t P = prep_pow2(m);
    for (uint32_t i = tid; i < P; i += PREP_BLOCK) V.srt[i] = i < m ? i : PREP_NONE;
    prep_sync();
    const auto before = [&](uint32_t a, uint32_t b) { return b == PREP_NONE ? a != PREP_NONE : (a != PREP_NONE && less(a, b)); };
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < P; i += PREP_BLOCK) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint32_t a = V.srt[i], b = V.srt[l];
                    if ((i & k) == 0 ? before(b, a) : before(a, b)) { V.srt[i] = b; V.srt[l] = a; }
                }
            }
            prep_sync();
        }
}

// cur = cur taken in the order of srt (best is the buffer in between: whoever needs best makes it afterwards)
__device__ void prep_apply_order(const PrepView &V, uint32_t m, uint32_t tid)
{
    for (uint32_t j = tid; j < m; j += PREP_BLOCK) V.best[j] = V.cur[V.srt[j]];
    prep_sync();
    for (uint32_t j = tid; j < m; j += PREP_BLOCK) V.cur[j] = V.best[j];
    prep_sync();
}

// cur = the positions k with srt[k] != 0, in order; -> how many
__device__ uint32_t prep_compact(const PrepView &V, PrepLds &S, uint32_t m, uint32_t tid)
{
    const uint32_t chunk = (m + PREP_BLOCK - 1) / PREP_BLOCK, lo = min(m, tid * chunk), hi = min(m, lo + chunk);
    uint32_t cnt = 0;
    for (uint32_t k = lo; k < hi; ++k) cnt += V.srt[k] ? 1u : 0u;
    S.scan[tid] = cnt;
    prep_sync();
    uint32_t at = 0, total = 0;
    for (uint32_t t = 0; t < PREP_BLOCK; ++t) { const uint32_t c = S.scan[t]; if (t < tid) at += c; total += c; }
    for (uint32_t k = lo; k < hi; ++k)
        if (V.srt[k]) V.best[at++] = V.cur[k];
    prep_sync();
    for (uint32_t j = tid; j < total; j += PREP_BLOCK) V.cur[j] = V.best[j];
    prep_sync();
    return total;
}

// G of the current order, and best[k] = the SOURCE row of the first position with the genome of position k
__device__ uint32_t prep_genomes(const PrepView &V, PrepLds &S, uint32_t m, uint32_t tid)
{
    if (tid == 0) S.count = 0;
    prep_sort(V, m, tid, [&](uint32_t a, uint32_t b) {
        const int64_t ga = V.genome[V.cur[a]], gb = V.genome[V.cur[b]];
        return ga < gb || (ga == gb && a < b);
    });
    uint32_t heads = 0;
    for (uint32_t k = tid; k < m; k += PREP_BLOCK) {
        if (k == 0 || V.genome[V.cur[V.srt[k]]] != V.genome[V.cur[V.srt[k - 1]]]) ++heads;
        const int64_t g = V.genome[V.cur[k]];
        uint32_t lo = 0, hi = m;                         // the first entry of srt whose genome is not below g
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (V.genome[V.cur[V.srt[mid]]] < g) lo = mid + 1; else hi = mid;
        }
        V.best[k] = V.cur[V.srt[lo]];
    }
    if (heads) atomicAdd(&S.count, heads);
    prep_sync();
    const uint32_t G = S.count;
    prep_sync();
    return G;
}

// NaN for 0 / 0, as the reference's numpy division gives it
__device__ __forceinline__ double prep_quot(int64_t a, int64_t b) { return (double)a / (double)b; }
__device__ __forceinline__ double prep_rs(const PrepView &V, uint32_t k) { return prep_quot(V.c4[V.cur[k]], V.c4[V.best[k]]); }
// the order of the selection: the bit pattern, a NaN above every number (rs is never below zero but for -0.0, which no quotient of two columns of one sign gives ...
// and whose pattern would only place it above the numbers, as a NaN)
__device__ __forceinline__ uint64_t prep_bits(double x) { return x != x ? ~0ull : (uint64_t)__double_as_longlong(x); }

// tr[e] = the source row that carries the locus conflict value e puts into used2, -1 when no row of the gene does
__device__ void prep_translate(const PrepView &V, const PrepGene &R, bool sbh, uint32_t tid)
{
    if (R.n_cfl == 0) return;
    prep_sort(V, V.n, tid, [&](uint32_t a, uint32_t b) { const int64_t la = V.locus[a], lb = V.locus[b]; return la < lb || (la == lb && a < b); });
    for (uint64_t e = R.cfl0 + tid; e < R.cfl0 + R.n_cfl; e += PREP_BLOCK) {
        int64_t loc = V.cfl[e] / 10;
        if (sbh) {                                       // (:653 as numpy computes it: the row's own locus is ADDED to every value of its list)
            uint32_t a = 0, b = V.n;                     // the last row whose list starts at or before e
            while (a + 1 < b) {
                const uint32_t mid = (a + b) >> 1;
                if (V.cfl_off[mid] <= e) a = mid; else b = mid;
            }
            loc += V.locus[a];
        }
        uint32_t lo = 0, hi = V.n;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (V.locus[V.srt[mid]] < loc) lo = mid + 1; else hi = mid;
        }
        V.tr[e] = (lo < V.n && V.locus[V.srt[lo]] == loc) ? (int32_t)V.srt[lo] : -1;
    }
    prep_sync();
}

// the walk over the current order: srt[k] = 1 for a kept position, 0 for a dropped one.  The bitmap is cleared by everybody, the walk is wavefront 0's
__device__ void prep_walk(const PrepView &V, uint32_t m, uint32_t tid)
{
    for (uint32_t w = tid; w < (V.n + 31) / 32; w += PREP_BLOCK) V.flag[w] = 0;
    prep_sync();
    if (tid < 64) {
        const uint32_t lane = tid;
        for (uint32_t k0 = 0; k0 < m; k0 += 64) {
            const uint32_t k = k0 + lane;
            const bool valid = k < m;
            const uint32_t r = valid ? V.cur[k] : 0u;
            const uint64_t a = valid ? V.cfl_off[r] : 0ull, b = valid ? V.cfl_off[r + 1] : 0ull;
            uint64_t todo = __ballot(valid && b > a), pending = __ballot(valid);
            uint32_t kept = 0;
            while (todo) {
                const uint32_t j = (uint32_t)__builtin_ctzll(todo);
                todo &= todo - 1;
                const uint64_t upto = j == 63 ? ~0ull : (1ull << (j + 1)) - 1;
                if (((pending & upto) >> lane) & 1) kept = ((V.flag[r >> 5] >> (r & 31)) & 1) ^ 1u;
                pending &= ~upto;
                if (__shfl(kept, j, 64)) {
                    const uint64_t aj = __shfl(a, j, 64), bj = __shfl(b, j, 64);
                    for (uint64_t e = aj + lane; e < bj; e += 64) {
                        const int32_t t = V.tr[e];
                        if (t >= 0) atomicOr(&V.flag[t >> 5], 1u << (t & 31));
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }
            if ((pending >> lane) & 1) kept = ((V.flag[r >> 5] >> (r & 31)) & 1) ^ 1u;
            if (valid) V.srt[k] = kept;
        }
    }
    prep_sync();
}

__device__ void prep_gene(const PrepDev &D, const PrepGene &R, PrepView &V, PrepLds &S, uint32_t g, uint32_t tid)
{
    uint32_t m = V.n;
    if (tid == 0) { S.tie = 0; S.min3 = 0x7FFFFFFF; }
    for (uint32_t i = tid; i < m; i += PREP_BLOCK) V.cur[i] = i;
    prep_sync();
    prep_translate(V, R, D.mode == PEP_PREP_SBH, tid);
    uint32_t G = prep_genomes(V, S, m, tid);
    if (D.mode == PEP_PREP_NJ) {
        if (m >= 2 * G) {
            prep_sort(V, m, tid, [&](uint32_t a, uint32_t b) { const int64_t x = V.c2[V.cur[a]], y = V.c2[V.cur[b]]; return x > y || (x == y && a < b); });
            bool tie = false;
            for (uint32_t k = tid + 1; k < m; k += PREP_BLOCK) tie = tie || V.c2[V.cur[V.srt[k]]] == V.c2[V.cur[V.srt[k - 1]]];
            if (tie) S.tie = 1;
            prep_sync();
            prep_apply_order(V, m, tid);
            prep_walk(V, m, tid);
            m = prep_compact(V, S, m, tid);
            prep_sort(V, m, tid, [&](uint32_t a, uint32_t b) { const int64_t x = V.c3[V.cur[a]], y = V.c3[V.cur[b]]; return x > y || (x == y && a < b); });
            prep_apply_order(V, m, tid);
            G = prep_genomes(V, S, m, tid);
        }
        if (m > 3 * G && m > 1000) {
            prep_sort(V, m, tid, [&](uint32_t a, uint32_t b) { const uint64_t x = prep_bits(prep_rs(V, a)), y = prep_bits(prep_rs(V, b)); return x > y || (x == y && a < b); });
            double cut = prep_rs(V, V.srt[3 * G - 1]);
            if (cut >= D.clust_identity) cut = m > 6 * G ? prep_rs(V, V.srt[6 * G]) : D.clust_identity;
            prep_sync();                                // (everybody has read its cut out of srt)
            for (uint32_t k = tid; k < m; k += PREP_BLOCK) V.srt[k] = prep_rs(V, k) >= cut ? 1u : 0u;
            prep_sync();
            m = prep_compact(V, S, m, tid);
            G = prep_genomes(V, S, m, tid);
        }
    } else {
        for (uint32_t k = tid; k < m; k += PREP_BLOCK) {
            const double x = prep_quot(V.c2[V.cur[k]], V.c2[V.best[k]]), y = prep_rs(V, k);
            const double rs = (x != x || y != y) ? NAN : (x < y ? x : y);
            V.srt[k] = rs >= D.clust_identity ? 1u : 0u;
        }
        prep_sync();
        m = prep_compact(V, S, m, tid);
        if (m) {
            prep_walk(V, m, tid);
            m = prep_compact(V, S, m, tid);
        }
        G = prep_genomes(V, S, m, tid);
    }
    int32_t low = 0x7FFFFFFF;
    for (uint32_t k = tid; k < m; k += PREP_BLOCK) {
        const uint32_t r = V.cur[k];
        D.rows[R.row0 + k] = r;
        low = min(low, (int32_t)V.c3[r]);
    }
    if (low != 0x7FFFFFFF) atomicMin(&S.min3, low);
    prep_sync();
    if (tid == 0) {
        const uint32_t inparalog = m > G ? 1u : 0u;
        const uint32_t is_final = D.mode == PEP_PREP_SBH || m <= 1 || (!inparalog && (double)S.min3 >= D.final_threshold) ? 1u : 0u;
        D.out[g] = PrepOut{m, inparalog, is_final, S.tie};
    }
}

template <bool LDS>
__global__ __launch_bounds__(PREP_BLOCK) void prep_prune(const PrepGene *__restrict__ genes, const uint32_t *__restrict__ which, PrepDev D)
{
    __shared__ uint32_t s_work[LDS ? 3 * PEP_PREP_LDS_ROWS : 1];
    __shared__ uint32_t s_flag[PEP_PREP_MAX_ROWS / 32];
    __shared__ PrepLds S;
    const uint32_t g = which[blockIdx.x];
    const PrepGene R = genes[g];
    PrepView V;
    V.genome = D.genome + R.row0; V.c2 = D.c2 + R.row0; V.c3 = D.c3 + R.row0; V.c4 = D.c4 + R.row0; V.locus = D.locus + R.row0;
    V.cfl_off = D.cfl_off + R.row0; V.cfl = D.cfl; V.tr = D.tr;
    if (LDS) { V.cur = s_work; V.srt = s_work + PEP_PREP_LDS_ROWS; V.best = s_work + 2 * PEP_PREP_LDS_ROWS; }
    else { V.cur = D.scratch + R.ws0; V.srt = V.cur + R.P; V.best = V.srt + R.P; }
    V.flag = s_flag; V.n = R.n; V.P = R.P;
    prep_gene(D, R, V, S, g, threadIdx.x);
}

__device__ __forceinline__ long long prep_block_max(long long v, long long *part, uint32_t tid)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const long long o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    prep_sync();                                    // (the last round's readers of part are through)
    if ((tid & 63) == 0) part[tid >> 6] = v;
    prep_sync();
    v = part[0];
#pragma unroll
    for (int w = 1; w < PREP_WAVES; ++w) v = part[w] > v ? part[w] : v;
    return v;
}

// ---- stage A: one workgroup per gene
__global__ __launch_bounds__(PREP_BLOCK) void prep_screen(const uint64_t *__restrict__ gene_off, const int64_t *__restrict__ c3, const int64_t *__restrict__ locus,
                                                          const uint8_t *__restrict__ used, double threshold, int64_t *__restrict__ out3, int64_t *__restrict__ out4,
                                                          int64_t *__restrict__ present, uint8_t *__restrict__ excluded)
{
    __shared__ long long part[PREP_WAVES];
    const uint32_t g = blockIdx.x, tid = threadIdx.x;
    const uint64_t lo = gene_off[g], hi = gene_off[g + 1];
    long long top = INT64_MIN;
    for (uint64_t r = lo + tid; r < hi; r += PREP_BLOCK) top = c3[r] > top ? c3[r] : top;
    top = prep_block_max(top, part, tid);
    const double den = (double)top;
    long long seen = 0;
    for (uint64_t r = lo + tid; r < hi; r += PREP_BLOCK) {
        const int64_t x = c3[r];
        const int64_t q = (int64_t)((double)(10000 * x) / den);
        const uint8_t state = used[locus[r]];
        out4[r] = q;
        out3[r] = state == 0 ? x : (state == 1 ? -x : 0);
        if (state == 0 && q > seen) seen = q;
    }
    seen = prep_block_max(seen, part, tid);
    if (tid == 0) { present[g] = seen; excluded[g] = (double)seen < threshold ? 1 : 0; }
}

// ---- the checks, shared by the three stages and their twins
struct PrepCheck {
    const char *me;
    std::string msg;
    int bad(int code, const std::string &text) { msg = std::string(me) + ": " + text; return code; }
};

int prep_check_rows(PrepCheck &K, uint32_t n_genes, const uint64_t *gene_off, const int64_t *locus, uint64_t n_loci, bool empty_ok)
{
    if (n_loci > PEP_PREP_MAX_LOCI) return K.bad(PEP_ERR_ARG, "n_loci " + std::to_string(n_loci) + " is more than " + std::to_string((uint64_t)PEP_PREP_MAX_LOCI));
    if (n_genes == 0) return PEP_OK;
    if (!gene_off || !locus) return K.bad(PEP_ERR_ARG, "null table");
    if (gene_off[0] != 0) return K.bad(PEP_ERR_ARG, "gene_off[0] is " + std::to_string(gene_off[0]) + ", not 0");
    std::vector<int64_t> seen;
    for (uint32_t g = 0; g < n_genes; ++g) {
        const std::string gene = "gene " + std::to_string(g);
        if (gene_off[g + 1] < gene_off[g])
            return K.bad(PEP_ERR_ARG, "the rows of " + gene + " (from " + std::to_string(gene_off[g]) + ") overlap the next gene's (gene_off[" + std::to_string(g + 1) + "] = " +
                                          std::to_string(gene_off[g + 1]) + ")");
        const uint64_t n = gene_off[g + 1] - gene_off[g];
        if (n == 0 && !empty_ok) return K.bad(PEP_ERR_ARG, gene + " has no rows");
        if (n > PEP_PREP_MAX_ROWS) return K.bad(PEP_ERR_LIMIT, gene + " has " + std::to_string(n) + " rows, more than " + std::to_string(PEP_PREP_MAX_ROWS));
        const int64_t *l = locus + gene_off[g];
        for (uint64_t r = 0; r < n; ++r)
            if (l[r] < 0 || (uint64_t)l[r] >= n_loci)
                return K.bad(PEP_ERR_ARG, "row " + std::to_string(r) + " of " + gene + " names locus " + std::to_string(l[r]) + ", outside [0, " + std::to_string(n_loci) + ")");
        seen.assign(l, l + n);
        std::sort(seen.begin(), seen.end());
        const auto twice = std::adjacent_find(seen.begin(), seen.end());
        if (twice != seen.end()) return K.bad(PEP_ERR_ARG, "locus " + std::to_string(*twice) + " comes twice in the table of " + gene);
    }
    return PEP_OK;
}

// a column whose every entry is below `limit` in magnitude (limit a power of two up to 2^62)
int prep_check_column(PrepCheck &K, const char *what, uint32_t n_genes, const uint64_t *gene_off, const int64_t *col, int64_t limit, const char *limit_text)
{
    if (n_genes == 0) return PEP_OK;
    if (!col) return K.bad(PEP_ERR_ARG, "null table");
    for (uint32_t g = 0; g < n_genes; ++g)
        for (uint64_t r = gene_off[g]; r < gene_off[g + 1]; ++r)
            if (col[r] >= limit || col[r] <= -limit)
                return K.bad(PEP_ERR_ARG, std::string(what) + " of row " + std::to_string(r - gene_off[g]) + " of gene " + std::to_string(g) + " is " + std::to_string(col[r]) +
                                              ", " + limit_text + " or more in magnitude");
    return PEP_OK;
}

// the conflict lists over the batch's rows; in_range: every value must name a locus of [0, n_loci)
int prep_check_lists(PrepCheck &K, uint32_t n_genes, const uint64_t *gene_off, const uint64_t *cfl_off, const int64_t *cfl, uint64_t n_loci, bool in_range)
{
    if (n_genes == 0) return PEP_OK;
    if (!cfl_off) return K.bad(PEP_ERR_ARG, "null table");
    if (cfl_off[0] != 0) return K.bad(PEP_ERR_ARG, "cfl_off[0] is " + std::to_string(cfl_off[0]) + ", not 0");
    for (uint32_t g = 0; g < n_genes; ++g)
        for (uint64_t r = gene_off[g]; r < gene_off[g + 1]; ++r) {
            const std::string row = "row " + std::to_string(r - gene_off[g]) + " of gene " + std::to_string(g);
            if (cfl_off[r + 1] < cfl_off[r])
                return K.bad(PEP_ERR_ARG, "the conflict list of " + row + " (from " + std::to_string(cfl_off[r]) + ") overlaps the next row's (cfl_off[" + std::to_string(r + 1) +
                                              "] = " + std::to_string(cfl_off[r + 1]) + ")");
            if (cfl_off[r + 1] > PEP_PREP_MAX_CFL_BYTES / 8)
                return K.bad(PEP_ERR_LIMIT, std::to_string(cfl_off[r + 1]) + " conflict values (8 bytes each) asked for up to " + row + ", the budget of one call is " +
                                                std::to_string((uint64_t)PEP_PREP_MAX_CFL_BYTES) + " bytes (split the batch)");
            if (cfl_off[r + 1] > cfl_off[r] && !cfl) return K.bad(PEP_ERR_ARG, "null table");
            for (uint64_t e = cfl_off[r]; e < cfl_off[r + 1]; ++e)
                if (cfl[e] < 0 || (in_range && (uint64_t)(cfl[e] / 10) >= n_loci))
                    return K.bad(PEP_ERR_ARG, "conflict value " + std::to_string(cfl[e]) + " of " + row + " names no locus of [0, " + std::to_string(n_loci) + ")");
        }
    return PEP_OK;
}

int screen_check(PrepCheck &K, uint32_t n_genes, const uint64_t *gene_off, const int64_t *col3, const int64_t *locus, uint64_t n_loci)
{
    PEP_TRY(prep_check_rows(K, n_genes, gene_off, locus, n_loci, true));
    PEP_TRY(prep_check_column(K, "column 3", n_genes, gene_off, col3, 1ll << 31, "2^31"));
    for (uint32_t g = 0; g < n_genes; ++g) {
        int64_t top = INT64_MIN;
        for (uint64_t r = gene_off[g]; r < gene_off[g + 1]; ++r) top = std::max(top, col3[r]);
        if (top <= 0) return K.bad(PEP_ERR_ARG, "gene " + std::to_string(g) + " has no row with column 3 above 0" + (top == INT64_MIN ? " (no row at all)" : " (its maximum is " + std::to_string(top) + ")"));
    }
    return PEP_OK;
}

int walk_check(PrepCheck &K, uint32_t n_genes, const uint64_t *gene_off, const int64_t *col3, const int64_t *locus, const uint64_t *cfl_off, const int64_t *cfl, uint64_t n_loci)
{
    PEP_TRY(prep_check_rows(K, n_genes, gene_off, locus, n_loci, true));
    PEP_TRY(prep_check_column(K, "column 3", n_genes, gene_off, col3, 1ll << 31, "2^31"));
    return prep_check_lists(K, n_genes, gene_off, cfl_off, cfl, n_loci, true);
}

int prune_check(PrepCheck &K, uint32_t mode, uint32_t n_genes, const uint64_t *gene_off, const int64_t *genome, const int64_t *col2, const int64_t *col3, const int64_t *col4,
                const int64_t *locus, const uint64_t *cfl_off, const int64_t *cfl, uint64_t n_loci, uint32_t path)
{
    if (mode > PEP_PREP_SBH) return K.bad(PEP_ERR_ARG, "mode " + std::to_string(mode) + " is neither PEP_PREP_NJ nor PEP_PREP_SBH");
    if (path > PEP_PREP_WS) return K.bad(PEP_ERR_ARG, "path " + std::to_string(path) + " is none of PEP_PREP_AUTO, PEP_PREP_LDS, PEP_PREP_WS");
    PEP_TRY(prep_check_rows(K, n_genes, gene_off, locus, n_loci, false));
    if (path == PEP_PREP_LDS)
        for (uint32_t g = 0; g < n_genes; ++g)
            if (gene_off[g + 1] - gene_off[g] > PEP_PREP_LDS_ROWS)
                return K.bad(PEP_ERR_LIMIT, "gene " + std::to_string(g) + " has " + std::to_string(gene_off[g + 1] - gene_off[g]) + " rows, the LDS path takes " + std::to_string(PEP_PREP_LDS_ROWS));
    PEP_TRY(prep_check_column(K, "the genome id", n_genes, gene_off, genome, 1ll << 32, "2^32"));
    if (n_genes)
        for (uint32_t g = 0; g < n_genes; ++g)
            for (uint64_t r = gene_off[g]; r < gene_off[g + 1]; ++r)
                if (genome[r] < 0) return K.bad(PEP_ERR_ARG, "the genome id of row " + std::to_string(r - gene_off[g]) + " of gene " + std::to_string(g) + " is " + std::to_string(genome[r]) + ", below 0");
    PEP_TRY(prep_check_column(K, "column 2", n_genes, gene_off, col2, 1ll << 62, "2^62"));
    PEP_TRY(prep_check_column(K, "column 3", n_genes, gene_off, col3, 1ll << 31, "2^31"));
    PEP_TRY(prep_check_column(K, "column 4", n_genes, gene_off, col4, 1ll << 31, "2^31"));
    return prep_check_lists(K, n_genes, gene_off, cfl_off, cfl, n_loci, false);
}

}  // namespace

extern "C" {

int pep_batch_screen_check(uint32_t n_genes, const uint64_t *gene_off, const int64_t *col3, const int64_t *locus, uint64_t n_loci, char *msg, uint64_t msg_cap)
{
    PrepCheck K{"pep_batch_screen"};
    const int rc = screen_check(K, n_genes, gene_off, col3, locus, n_loci);
    return pep_message_out(rc, K.msg, msg, msg_cap);
}

int pep_batch_screen(pep_ctx *ctx, uint32_t n_genes, const uint64_t *gene_off, const int64_t *col3, const int64_t *locus, const uint8_t *used_state, uint64_t n_loci,
                     double threshold, int64_t *out3, int64_t *out4, int64_t *present, uint8_t *excluded)
{
    if (!ctx) return PEP_ERR_ARG;
    CallTimes &times = ctx->calls[PEP_CALL_BATCH_SCREEN];
    times = {};
    PrepCheck K{"pep_batch_screen"};
    const int rc = screen_check(K, n_genes, gene_off, col3, locus, n_loci);
    if (rc != PEP_OK) return pep_fail(ctx, rc, K.msg);
    if (n_genes == 0) return PEP_OK;
    if (!used_state || !out3 || !out4 || !present || !excluded) return pep_fail(ctx, PEP_ERR_ARG, "pep_batch_screen: null table");
    const uint64_t n_rows = gene_off[n_genes];
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf *W = ctx->ws;
    PEP_TRY(pep_tables_to_device(ctx, W, {{K26_A_GENE_OFF, gene_off, ((size_t)n_genes + 1) * 8, 0}, {K26_C3, col3, n_rows * 8, 8}, {K26_LOCUS, locus, n_rows * 8, 8},
                                          {K26_USED, used_state, n_loci, 8}, {K26_A_OUT3, nullptr, n_rows * 8, 8}, {K26_A_OUT4, nullptr, n_rows * 8, 8},
                                          {K26_A_PRESENT, nullptr, (size_t)n_genes * 8, 0}, {K26_A_EXCLUDED, nullptr, n_genes, 0}}));
    pep_timed_stage(ctx, times.ms[0], [&] {
        hipLaunchKernelGGL(prep_screen, dim3(n_genes), dim3(PREP_BLOCK), 0, ctx->stream, W[K26_A_GENE_OFF].as<const uint64_t>(), W[K26_C3].as<const int64_t>(),
                           W[K26_LOCUS].as<const int64_t>(), W[K26_USED].as<const uint8_t>(), threshold, W[K26_A_OUT3].as<int64_t>(), W[K26_A_OUT4].as<int64_t>(),
                           W[K26_A_PRESENT].as<int64_t>(), W[K26_A_EXCLUDED].as<uint8_t>());
    });
    PEP_HIP(ctx, hipGetLastError());
    PEP_TRY(pep_d2h_queue(ctx, out3, W[K26_A_OUT3].p, n_rows * 8));
    PEP_TRY(pep_d2h_queue(ctx, out4, W[K26_A_OUT4].p, n_rows * 8));
    PEP_TRY(pep_d2h_queue(ctx, present, W[K26_A_PRESENT].p, (size_t)n_genes * 8));
    PEP_TRY(pep_d2h_queue(ctx, excluded, W[K26_A_EXCLUDED].p, n_genes));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    return PEP_OK;
}

int pep_batch_unsure_walk_check(uint32_t n_genes, const uint64_t *gene_off, const int64_t *col3, const int64_t *locus, const uint64_t *cfl_off, const int64_t *cfl,
                                uint64_t n_loci, char *msg, uint64_t msg_cap)
{
    PrepCheck K{"pep_batch_unsure_walk"};
    const int rc = walk_check(K, n_genes, gene_off, col3, locus, cfl_off, cfl, n_loci);
    return pep_message_out(rc, K.msg, msg, msg_cap);
}

int pep_batch_unsure_walk(uint32_t n_genes, const uint64_t *gene_off, int64_t *col3, const int64_t *locus, const uint64_t *cfl_off, const int64_t *cfl, uint64_t n_loci,
                          uint8_t *popped, char *msg, uint64_t msg_cap)
{
    PrepCheck K{"pep_batch_unsure_walk"};
    const int rc = walk_check(K, n_genes, gene_off, col3, locus, cfl_off, cfl, n_loci);
    if (rc != PEP_OK) return pep_message_out(rc, K.msg, msg, msg_cap);
    if (n_genes == 0) return PEP_OK;
    if (!popped) return pep_message_out(K.bad(PEP_ERR_ARG, "null table"), K.msg, msg, msg_cap);
    std::vector<uint64_t> used2((size_t)((n_loci + 63) / 64), 0);
    const auto in = [&](int64_t l) { return (used2[(uint64_t)l >> 6] >> ((uint64_t)l & 63)) & 1; };
    for (uint32_t g = 0; g < n_genes; ++g) {
        const uint64_t lo = gene_off[g], hi = gene_off[g + 1];
        uint64_t pos = 0, unsure = 0;
        for (uint64_t r = lo; r < hi; ++r)
            if (col3[r] > 0) { ++pos; unsure += in(locus[r]); }
        popped[g] = (double)unsure >= (double)pos * 0.6 ? 1 : 0;
        if (popped[g]) continue;
        for (uint64_t r = lo; r < hi; ++r)
            if (!in(locus[r]))
                for (uint64_t e = cfl_off[r]; e < cfl_off[r + 1]; ++e) { const uint64_t l = (uint64_t)(cfl[e] / 10); used2[l >> 6] |= 1ull << (l & 63); }
        uint64_t neg = 0;
        for (uint64_t r = lo; r < hi; ++r)
            if (col3[r] < 0 && neg++ % 3 == 0) col3[r] = -col3[r];
    }
    return PEP_OK;
}

int pep_batch_prune_check(uint32_t mode, uint32_t n_genes, const uint64_t *gene_off, const int64_t *genome, const int64_t *col2, const int64_t *col3, const int64_t *col4,
                          const int64_t *locus, const uint64_t *cfl_off, const int64_t *cfl, uint64_t n_loci, uint32_t path, char *msg, uint64_t msg_cap)
{
    PrepCheck K{"pep_batch_prune"};
    const int rc = prune_check(K, mode, n_genes, gene_off, genome, col2, col3, col4, locus, cfl_off, cfl, n_loci, path);
    return pep_message_out(rc, K.msg, msg, msg_cap);
}

int pep_batch_prune(pep_ctx *ctx, uint32_t mode, uint32_t n_genes, const uint64_t *gene_off, const int64_t *genome, const int64_t *col2, const int64_t *col3,
                    const int64_t *col4, const int64_t *locus, const uint64_t *cfl_off, const int64_t *cfl, uint64_t n_loci, double clust_identity, double final_threshold,
                    uint32_t path, uint64_t *out_off, int32_t *rows, uint8_t *inparalog, uint8_t *is_final, uint64_t *n_ties)
{
    if (!ctx) return PEP_ERR_ARG;
    CallTimes &times = ctx->calls[PEP_CALL_BATCH_PRUNE];
    times = {};
    PrepCheck K{"pep_batch_prune"};
    const int rc = prune_check(K, mode, n_genes, gene_off, genome, col2, col3, col4, locus, cfl_off, cfl, n_loci, path);
    if (rc != PEP_OK) return pep_fail(ctx, rc, K.msg);
    if (!out_off || !n_ties) return pep_fail(ctx, PEP_ERR_ARG, "pep_batch_prune: null table");
    out_off[0] = 0;
    *n_ties = 0;
    if (n_genes == 0) return PEP_OK;
    if (!rows || !inparalog || !is_final) return pep_fail(ctx, PEP_ERR_ARG, "pep_batch_prune: null table");
    const uint64_t n_rows = gene_off[n_genes], n_cfl = cfl_off[n_rows];
    std::vector<PrepGene> genes(n_genes);
    std::vector<uint32_t> which, large;
    uint64_t ws_words = 0;
    for (uint32_t g = 0; g < n_genes; ++g) {
        const uint32_t n = (uint32_t)(gene_off[g + 1] - gene_off[g]);
        uint32_t P = 1;
        while (P < n) P <<= 1;
        const bool lds = path == PEP_PREP_LDS || (path == PEP_PREP_AUTO && n <= PEP_PREP_LDS_ROWS);
        genes[g] = PrepGene{gene_off[g], cfl_off[gene_off[g]], cfl_off[gene_off[g + 1]] - cfl_off[gene_off[g]], ws_words, n, P};
        if (lds) which.push_back(g);
        else { large.push_back(g); ws_words += 3ull * P; }
    }
    const size_t n_lds = which.size();
    which.insert(which.end(), large.begin(), large.end());
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf *W = ctx->ws;
    PEP_TRY(pep_tables_to_device(ctx, W, {{K26_GENOME, genome, n_rows * 8, 0}, {K26_C2, col2, n_rows * 8, 0}, {K26_C3, col3, n_rows * 8, 0}, {K26_C4, col4, n_rows * 8, 0},
                                          {K26_LOCUS, locus, n_rows * 8, 0}, {K26_CFL_OFF, cfl_off, (n_rows + 1) * 8, 0}, {K26_CFL, n_cfl ? cfl : nullptr, n_cfl * 8, 8},
                                          {K26_GENES, genes.data(), genes.size() * sizeof(PrepGene), 0}, {K26_WHICH, which.data(), which.size() * 4, 0},
                                          {K26_TR, nullptr, n_cfl * 4, 8}, {K26_SCRATCH, nullptr, ws_words * 4, 8}, {K26_ROWS, nullptr, n_rows * 4, 0},
                                          {K26_OUT, nullptr, (size_t)n_genes * sizeof(PrepOut), 0}}));
    const PrepDev D{W[K26_GENOME].as<const int64_t>(), W[K26_C2].as<const int64_t>(), W[K26_C3].as<const int64_t>(), W[K26_C4].as<const int64_t>(),
                    W[K26_LOCUS].as<const int64_t>(), W[K26_CFL_OFF].as<const uint64_t>(), W[K26_CFL].as<const int64_t>(), W[K26_TR].as<int32_t>(),
                    W[K26_SCRATCH].as<uint32_t>(), W[K26_ROWS].as<uint32_t>(), W[K26_OUT].as<PrepOut>(), clust_identity, final_threshold, mode};
    const PrepGene *d_genes = W[K26_GENES].as<const PrepGene>();
    const uint32_t *d_which = W[K26_WHICH].as<const uint32_t>();
    pep_timed_stage(ctx, times.ms[0], [&] {
        if (n_lds) hipLaunchKernelGGL(prep_prune<true>, dim3((unsigned)n_lds), dim3(PREP_BLOCK), 0, ctx->stream, d_genes, d_which, D);
        if (!large.empty()) hipLaunchKernelGGL(prep_prune<false>, dim3((unsigned)large.size()), dim3(PREP_BLOCK), 0, ctx->stream, d_genes, d_which + n_lds, D);
    });
    PEP_HIP(ctx, hipGetLastError());
    std::vector<uint32_t> h_rows(n_rows);
    std::vector<PrepOut> h_out(n_genes);
    PEP_TRY(pep_d2h_queue(ctx, h_rows.data(), D.rows, n_rows * 4));
    PEP_TRY(pep_d2h_queue(ctx, h_out.data(), D.out, (size_t)n_genes * sizeof(PrepOut)));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    for (uint32_t g = 0; g < n_genes; ++g) {
        const PrepOut &o = h_out[g];
        if (o.m > genes[g].n) return pep_fail(ctx, PEP_ERR_INTERNAL, "pep_batch_prune: gene " + std::to_string(g) + " came back with more rows than it has");
        for (uint32_t k = 0; k < o.m; ++k) rows[out_off[g] + k] = (int32_t)h_rows[gene_off[g] + k];
        out_off[g + 1] = out_off[g] + o.m;
        inparalog[g] = (uint8_t)o.inparalog;
        is_final[g] = (uint8_t)o.is_final;
        *n_ties += o.tie;
    }
    return PEP_OK;
}

}  // extern "C"
