// K25: the tree cutting of filt_per_group (PEPPAN.py:424-482, ete3 there) for a batch of trees, on bit sets of leaves: no tree is rooted, pruned or walked.
// The definition, the summation order and what is NOT restated (the reference's choice at exact ties between different bipartitions, which depends on ete3's
// rooting) are in include/peppan_hip.h (K25); tests/treecut_helpers.py restates it in numpy and the device equals that bit for bit, so contraction into fused
// multiply-adds is switched off for the whole file.
//   cut_prep         a wavefront per matrix row of the batch: the row of M = W1 where W0 > W1, and the row's bits of G = (W0 > W1) by ballot (the test of :438
//                    is then `G[a] & T` over the rows a of T).
//   cut_block        one workgroup per tree of up to PEP_NJ_BLOCK_LEAVES leaves, the whole cut loop in one launch: the branches' bit sets, G, the component T
//                    and the state in LDS (16 + 8 KiB), the three matrices read row-wise from global memory.  Per iteration: a wavefront per branch scores it
//                    (lanes along the columns b, a fixed shuffle tree, rows in ascending order), the workgroup selects the winner, applies the cut and moves on
//                    to the next component that needs scoring.
//   cut_chain_*      larger trees: the same three steps as launches on the context's stream - cut_chain_score over a grid of branches, cut_chain_select by one
//                    workgroup - with everything in device memory between the launches (T and the state in LDS within one); launches behind the tree's `done`
//                    flag return at once, and the host reads the flag once per PEP_CUT_ROUND iterations.  No grid-wide barrier, no cooperative launch, no loop that waits.
// Both paths run the SAME device functions (cut_prepare, cut_score_branch, cut_select) over a CutView whose set pointers lead into LDS or device memory.
// Not tuned: the rates are in profiles/treecut_rate.txt.  Known slack: a workgroup of 256 threads and 24 KiB of LDS for a tree of 3 leaves; a branch is scored
// by one wavefront however many rows its far side has; branches with the same restriction are scored once each.
#include "common.h"
#include <algorithm>
#include <cmath>
#include <numeric>

#pragma clang fp contract(off)

namespace {

// the slots of pep_ctx::k25
enum { K25_W0 = 0, K25_W1, K25_M, K25_G, K25_SETS, K25_LEN, K25_TREES, K25_STRONG, K25_SCORE, K25_FIN, K25_PART, K25_COUNTS, K25_LOGI, K25_LOGV, K25_STATE, K25_SLOTS };
static_assert(K25_SLOTS == sizeof(pep_ctx::k25) / sizeof(DevBuf), "one member of pep_ctx::k25 per slot");

constexpr int CUT_BLOCK = 256;
constexpr int CUT_WAVES = CUT_BLOCK / 64;
constexpr int CUT_BLOCK_WORDS = PEP_NJ_BLOCK_LEAVES / 64;
constexpr int CUT_MAX_WORDS = PEP_NJ_MAX_LEAVES / 64;
constexpr int CUT_SCORE = 5;                            // doubles of a branch's score: s0, s1, m, ic0 (-1: no candidate), key
static_assert(CUT_MAX_WORDS <= CUT_BLOCK, "a word of a bit set per thread");
static_assert(PEP_NJ_BLOCK_LEAVES % 64 == 0 && PEP_NJ_BLOCK_LEAVES <= CUT_BLOCK, "cut_block's LDS arrays");

// offsets into the call's device copies, which start at the first tree
struct CutTree { uint64_t mat_off, g_off, set_off, branch_off, leaf_off, word_off, row0; uint32_t n, B, words, cap; };
struct CutState { uint32_t id, ite, nq, n_cuts, n_ties, done, min_t, steps; };
// the device copies of one call
struct CutDev {
    const double *W0, *W1;
    double *M;
    uint64_t *G;
    const uint64_t *sets, *strong;
    const double *len;
    double *score;
    uint32_t *fin;
    int32_t *part, *counts, *log_i;
    double *log_v;
};
// one tree as the device functions see it; G, sets, T and st are in LDS (cut_block) or in device memory (cut_chain_*)
struct CutView {
    const double *W0, *W1, *M;
    const uint64_t *G, *sets, *strong;
    const double *len;
    double *score;
    uint32_t *fin;
    int32_t *part, *counts, *log_i;
    double *log_v;
    uint64_t *T;
    CutState *st;
    uint32_t n, B, words, cap;
};
struct CutLds {
    double len[CUT_BLOCK], pk[CUT_WAVES], pi[CUT_WAVES];
    uint32_t minf[CUT_BLOCK], e[CUT_BLOCK], cnt[CUT_BLOCK];
    uint32_t flag, win, reps;
};

__device__ __forceinline__ CutView cut_view(const CutDev &D, const CutTree &R, uint32_t t)
{
    CutView V;
    V.W0 = D.W0 + R.mat_off; V.W1 = D.W1 + R.mat_off; V.M = D.M + R.mat_off;
    V.G = D.G + R.g_off; V.sets = D.sets + R.set_off; V.strong = D.strong + R.word_off;
    V.len = D.len + R.branch_off; V.score = D.score + CUT_SCORE * R.branch_off; V.fin = D.fin + R.branch_off;
    V.part = D.part + R.leaf_off; V.counts = D.counts + 4 * (uint64_t)t; V.log_i = D.log_i + 2 * R.leaf_off; V.log_v = D.log_v + 4 * R.leaf_off;
    V.T = nullptr; V.st = nullptr;
    V.n = R.n; V.B = R.B; V.words = R.words; V.cap = R.cap;
    return V;
}

// ---- a wavefront per matrix row of the batch
__global__ __launch_bounds__(CUT_BLOCK) void cut_prep(const CutTree *__restrict__ trees, uint32_t n_trees, uint64_t n_rows, CutDev D)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t row = (uint64_t)blockIdx.x * CUT_WAVES + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    uint32_t lo = 0, hi = n_trees - 1;                  // the last tree whose row0 <= row
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (trees[mid].row0 <= row) lo = mid; else hi = mid - 1;
    }
    const CutTree R = trees[lo];
    const uint32_t a = (uint32_t)(row - R.row0), n = R.n;
    const double *r0 = D.W0 + R.mat_off + (uint64_t)a * n, *r1 = D.W1 + R.mat_off + (uint64_t)a * n;
    double *rm = D.M + R.mat_off + (uint64_t)a * n;
    uint64_t *g = D.G + R.g_off + (uint64_t)a * R.words;
    for (uint32_t k = 0; k < R.words; ++k) {
        const uint32_t b = 64 * k + lane;
        bool over = false;
        if (b < n) {
            const double x0 = r0[b], x1 = r1[b];
            over = x0 > x1;
            rm[b] = over ? x1 : 0.0;
        }
        const uint64_t bits = __ballot(over);
        if (lane == 0) g[k] = bits;
    }
}

// ---- the three steps, shared by both paths

// the barrier of the three steps.  Scores, finalist marks and labels travel between the wavefronts of a workgroup through device memory, and the barrier
// instruction itself waits for no memory counter: every wavefront drains its own stores first
__device__ __forceinline__ void cut_sync()
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    __syncthreads();
}

// word w of branch e's far side within T: the side without the component's smallest leaf
__device__ __forceinline__ uint64_t cut_far(const CutView &V, uint32_t e, bool flip, uint32_t w)
{
    const uint64_t s = V.sets[(uint64_t)e * V.words + w], t = V.T[w];
    return flip ? t & ~s : t & s;
}

__device__ __forceinline__ bool cut_flip(const CutView &V, uint32_t e, uint32_t min_t)
{
    return (V.sets[(uint64_t)e * V.words + (min_t >> 6)] >> (min_t & 63)) & 1;
}

__device__ __forceinline__ bool cut_same(const CutView &V, uint32_t e, bool flip_e, uint32_t f, uint32_t min_t)
{
    const bool flip_f = cut_flip(V, f, min_t);
    for (uint32_t w = 0; w < V.words; ++w)
        if (cut_far(V, e, flip_e, w) != cut_far(V, f, flip_f, w)) return false;
    return true;
}

// the component `id` from the labels (threads 0 .. words - 1)
__device__ __forceinline__ void cut_build_T(const CutView &V, uint32_t id, uint32_t tid)
{
    if (tid >= V.words) return;
    uint64_t w = 0;
    for (uint32_t j = 0; j < 64 && 64 * tid + j < V.n; ++j)
        if (V.part[64 * tid + j] == (int32_t)id) w |= 1ull << j;
    V.T[tid] = w;
}

// by the whole workgroup: on to the first component from st->id that has iterations left and fails the test of :438 - T and min_t are then its leaves and the
// smallest of them - or to the end of the queue (st->done)
__device__ void cut_prepare(const CutView &V, CutLds &S, uint32_t tid)
{
    for (;;) {
        cut_sync();
        const uint32_t id = V.st->id, nq = V.st->nq, ite = V.st->ite;
        if (id >= nq || V.st->steps > 2 * V.n + 2) {        // (every step cuts, fewer than n times, or finishes a component, n at most: the second test never holds)
            if (tid == 0) V.st->done = 1;
            break;
        }
        bool score = false;
        if (ite < V.cap) {
            if (tid == 0) S.flag = 0;
            cut_sync();
            bool hit = false;
            for (uint32_t a = tid; a < V.n && !hit; a += CUT_BLOCK)
                if ((V.T[a >> 6] >> (a & 63)) & 1)
                    for (uint32_t w = 0; w < V.words; ++w)
                        if (V.G[(uint64_t)a * V.words + w] & V.T[w]) { hit = true; break; }
            if (hit) S.flag = 1;
            cut_sync();
            score = S.flag != 0;
        }
        if (score) {
            if (tid == 0) {
                uint32_t w = 0;
                while (w + 1 < V.words && V.T[w] == 0) ++w;          // (T holds a leaf: every component does)
                V.st->min_t = V.T[w] ? 64 * w + (uint32_t)__builtin_ctzll(V.T[w]) : 0u;
            }
            break;
        }
        cut_sync();                                // (everybody has read the state)
        if (id + 1 < nq) cut_build_T(V, id + 1, tid);
        if (tid == 0) { V.st->id = id + 1; V.st->ite = 0; }
    }
    cut_sync();
}

// by one wavefront: the score of branch e against the component T
__device__ void cut_score_branch(const CutView &V, uint32_t e, uint32_t lane)
{
    const uint32_t min_t = V.st->min_t, n = V.n;
    const bool flip = cut_flip(V, e, min_t);
    double s0 = 0.0, s1 = 0.0, m = 0.0;
    bool any = false;
    for (uint32_t w = 0; w < V.words; ++w) {
        uint64_t F = cut_far(V, e, flip, w);
        any = any || F != 0;
        while (F) {
            const uint32_t a = 64 * w + (uint32_t)__builtin_ctzll(F);
            F &= F - 1;
            const double *r0 = V.W0 + (uint64_t)a * n, *r1 = V.W1 + (uint64_t)a * n, *rm = V.M + (uint64_t)a * n;
            double p0 = 0.0, p1 = 0.0, pm = 0.0;
            for (uint32_t k = 0; k < V.words; ++k) {
                const uint64_t C = V.T[k] & ~cut_far(V, e, flip, k);
                if ((C >> lane) & 1) {
                    const uint32_t b = 64 * k + lane;
                    p0 = p0 + r0[b];
                    p1 = p1 + r1[b];
                    pm = pm + rm[b];
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                p0 = p0 + __shfl_xor(p0, off, 64);
                p1 = p1 + __shfl_xor(p1, off, 64);
                pm = pm + __shfl_xor(pm, off, 64);
            }
            s0 = s0 + p0;
            s1 = s1 + p1;
            m = m + pm;
        }
    }
    if (lane == 0) {
        double *o = V.score + (uint64_t)CUT_SCORE * e;
        const double ic0 = any ? s0 / (s1 > 1.0 ? s1 : 1.0) : -1.0;
        o[0] = s0; o[1] = s1; o[2] = m; o[3] = ic0;
        o[4] = any ? ic0 * __dsqrt_rn(m) : 0.0;
    }
}

// whether (ok, oi) is the larger (key, ic0)
__device__ __forceinline__ bool cut_larger(double k, double i, double ok, double oi) { return ok > k || (ok == k && oi > i); }

// by the whole workgroup, the scores of every branch written and visible: the winner, the cut, the log record - or the component is finished.  cut_prepare follows.
__device__ void cut_select(const CutView &V, CutLds &S, uint32_t tid)
{
    const uint32_t lane = tid & 63, wave = tid >> 6, B = V.B;
    const uint32_t id = V.st->id, nq = V.st->nq, min_t = V.st->min_t;
    double k = -INFINITY, i = -INFINITY;
    for (uint32_t e = tid; e < B; e += CUT_BLOCK) {
        const double ic = V.score[(uint64_t)CUT_SCORE * e + 3], ky = V.score[(uint64_t)CUT_SCORE * e + 4];
        if (ic > 1.0 && ky == ky && cut_larger(k, i, ky, ic)) { k = ky; i = ic; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ok = __shfl_xor(k, off, 64), oi = __shfl_xor(i, off, 64);
        if (cut_larger(k, i, ok, oi)) { k = ok; i = oi; }
    }
    if (lane == 0) { S.pk[wave] = k; S.pi[wave] = i; }
    cut_sync();
    k = S.pk[0]; i = S.pi[0];
#pragma unroll
    for (int w = 1; w < CUT_WAVES; ++w)
        if (cut_larger(k, i, S.pk[w], S.pi[w])) { k = S.pk[w]; i = S.pi[w]; }
    const auto finished = [&] {
        // no candidate (:471-472): the next component
        cut_sync();
        if (id + 1 < nq) cut_build_T(V, id + 1, tid);
        if (tid == 0) { V.st->id = id + 1; V.st->ite = 0; V.st->steps += 1; }
    };
    if (!(i > 1.0)) return finished();
    for (uint32_t e = tid; e < B; e += CUT_BLOCK) {
        const double ic = V.score[(uint64_t)CUT_SCORE * e + 3], ky = V.score[(uint64_t)CUT_SCORE * e + 4];
        V.fin[e] = (ic > 1.0 && ky == k && ic == i) ? 1u : 0u;
    }
    cut_sync();
    // the different far sides among the finalists, each at its lowest branch
    double best_len = -INFINITY;
    uint32_t best_minf = 0xFFFFFFFFu, best_e = 0xFFFFFFFFu, cnt = 0;
    for (uint32_t e = tid; e < B; e += CUT_BLOCK) {
        if (!V.fin[e]) continue;
        const bool flip = cut_flip(V, e, min_t);
        bool first = true;
        for (uint32_t f = 0; f < e && first; ++f)
            if (V.fin[f] && cut_same(V, e, flip, f, min_t)) first = false;
        if (!first) continue;
        double sum = 0.0 + V.len[e];
        for (uint32_t f = e + 1; f < B; ++f)
            if (V.fin[f] && cut_same(V, e, flip, f, min_t)) sum = sum + V.len[f];
        uint32_t minf = 0xFFFFFFFFu;
        for (uint32_t w = 0; w < V.words && minf == 0xFFFFFFFFu; ++w)
            if (const uint64_t far = cut_far(V, e, flip, w)) minf = 64 * w + (uint32_t)__builtin_ctzll(far);
        ++cnt;
        if (sum > best_len || (sum == best_len && (minf < best_minf || (minf == best_minf && e < best_e)))) { best_len = sum; best_minf = minf; best_e = e; }
    }
    S.len[tid] = best_len; S.minf[tid] = best_minf; S.e[tid] = best_e; S.cnt[tid] = cnt;
    cut_sync();
    if (tid == 0) {
        uint32_t reps = 0;
        for (uint32_t x = 0; x < CUT_BLOCK; ++x) {
            reps += S.cnt[x];
            if (S.e[x] == 0xFFFFFFFFu) continue;
            if (best_e == 0xFFFFFFFFu || S.len[x] > best_len ||
                (S.len[x] == best_len && (S.minf[x] < best_minf || (S.minf[x] == best_minf && S.e[x] < best_e)))) { best_len = S.len[x]; best_minf = S.minf[x]; best_e = S.e[x]; }
        }
        S.win = best_e; S.reps = reps; S.flag = 0;
    }
    cut_sync();
    const uint32_t win = S.win;
    if (win >= B) return finished();                    // (a finalist always is its own first: never taken)
    const bool flip = cut_flip(V, win, min_t);
    const uint64_t F = tid < V.words ? cut_far(V, win, flip, tid) : 0;
    if (tid < V.words && (F & V.strong[tid])) S.flag = 1;
    cut_sync();                                    // (everybody has read T and the sets of the winner)
    const int32_t label = S.flag ? (int32_t)nq : -1;
    if (tid < V.words) {
        for (uint64_t f = F; f; f &= f - 1) V.part[64 * tid + (uint32_t)__builtin_ctzll(f)] = label;
        V.T[tid] &= ~F;
    }
    if (tid == 0) {
        const uint32_t c = V.st->n_cuts;
        const double *o = V.score + (uint64_t)CUT_SCORE * win;
        if (c + 1 < V.n) {                              // (a cut takes a leaf at least from a component that keeps one: n - 1 cuts at most)
            V.log_i[2 * c] = (int32_t)id; V.log_i[2 * c + 1] = (int32_t)win;
            V.log_v[4 * c] = o[0]; V.log_v[4 * c + 1] = o[1]; V.log_v[4 * c + 2] = o[2]; V.log_v[4 * c + 3] = o[4];
        }
        V.st->n_cuts = c + 1;
        V.st->steps += 1;
        V.st->n_ties += S.reps - 1;
        V.st->nq = nq + (S.flag ? 1u : 0u);
        V.st->ite += 1;
    }
}

// the start: every leaf in component 0 (threads of the whole workgroup)
__device__ __forceinline__ void cut_start(const CutView &V, uint32_t tid)
{
    for (uint32_t l = tid; l < V.n; l += CUT_BLOCK) V.part[l] = 0;
    if (tid < V.words) V.T[tid] = 64 * (tid + 1) <= V.n ? ~0ull : (1ull << (V.n & 63)) - 1;
    if (tid == 0) *V.st = CutState{0u, 0u, 1u, 0u, 0u, 0u, 0u, 0u};
}

__device__ __forceinline__ void cut_counts(const CutView &V)
{
    V.counts[0] = (int32_t)V.st->nq; V.counts[1] = (int32_t)V.st->n_cuts; V.counts[2] = (int32_t)V.st->n_ties; V.counts[3] = 0;
}

// ---- one workgroup per tree
__global__ __launch_bounds__(CUT_BLOCK) void cut_block(const CutTree *__restrict__ trees, const uint32_t *__restrict__ which, CutDev D)
{
    __shared__ uint64_t s_sets[2 * PEP_NJ_BLOCK_LEAVES * CUT_BLOCK_WORDS], s_G[PEP_NJ_BLOCK_LEAVES * CUT_BLOCK_WORDS], s_T[CUT_BLOCK_WORDS];
    __shared__ CutState s_st;
    __shared__ CutLds S;
    const uint32_t t = which[blockIdx.x], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CutTree R = trees[t];
    CutView V = cut_view(D, R, t);
    for (uint32_t x = tid; x < R.B * R.words; x += CUT_BLOCK) s_sets[x] = V.sets[x];
    for (uint32_t x = tid; x < R.n * R.words; x += CUT_BLOCK) s_G[x] = V.G[x];
    V.sets = s_sets; V.G = s_G; V.T = s_T; V.st = &s_st;
    cut_start(V, tid);
    cut_prepare(V, S, tid);
    while (!s_st.done) {
        for (uint32_t e = wave; e < R.B; e += CUT_WAVES) cut_score_branch(V, e, lane);
        cut_sync();
        cut_select(V, S, tid);
        cut_prepare(V, S, tid);
    }
    if (tid == 0) cut_counts(V);
}

// ---- the launch chain of one large tree: the view by value; T and the state live in device memory between the launches and in LDS within one, so that
// no decision a workgroup makes together depends on device memory it wrote itself
struct CutHome { uint64_t *T; CutState *st; };

__device__ __forceinline__ CutHome cut_move_in(CutView &V, uint64_t *s_T, CutState *s_st, bool load, uint32_t tid)
{
    const CutHome home{V.T, V.st};
    if (load) {
        if (tid < V.words) s_T[tid] = home.T[tid];
        if (tid == 0) *s_st = *home.st;
    }
    V.T = s_T; V.st = s_st;
    return home;
}

// behind cut_prepare, whose last act is a barrier
__device__ __forceinline__ void cut_move_out(const CutView &V, const CutHome &home, uint32_t tid)
{
    if (tid < V.words) home.T[tid] = V.T[tid];
    if (tid == 0) { *home.st = *V.st; cut_counts(V); }
}

__global__ __launch_bounds__(CUT_BLOCK) void cut_chain_start(CutView V)
{
    __shared__ CutLds S;
    __shared__ uint64_t s_T[CUT_MAX_WORDS];
    __shared__ CutState s_st;
    const CutHome home = cut_move_in(V, s_T, &s_st, false, threadIdx.x);
    cut_start(V, threadIdx.x);
    cut_prepare(V, S, threadIdx.x);
    cut_move_out(V, home, threadIdx.x);
}

__global__ __launch_bounds__(CUT_BLOCK) void cut_chain_score(CutView V)
{
    if (V.st->done) return;
    const uint32_t e = blockIdx.x * CUT_WAVES + (threadIdx.x >> 6);
    if (e < V.B) cut_score_branch(V, e, threadIdx.x & 63);
}

__global__ __launch_bounds__(CUT_BLOCK) void cut_chain_select(CutView V)
{
    __shared__ CutLds S;
    __shared__ uint64_t s_T[CUT_MAX_WORDS];
    __shared__ CutState s_st;
    if (V.st->done) return;
    const CutHome home = cut_move_in(V, s_T, &s_st, true, threadIdx.x);
    cut_sync();
    cut_select(V, S, threadIdx.x);
    cut_prepare(V, S, threadIdx.x);
    cut_move_out(V, home, threadIdx.x);
}

const char *const K25_ME = "pep_tree_cut: ";

uint32_t cut_words(uint64_t n) { return (uint32_t)((n + 63) / 64); }

// every check of pep_tree_cut that reads no matrix and no length
int cut_check(const uint32_t *n_leaves, uint32_t n_trees, const uint64_t *leaf_off, const uint64_t *mat_off, const uint64_t *branch_off, const uint64_t *set_off,
              const uint64_t *sets, uint32_t path, std::string &msg)
{
    const auto bad = [&](int code, const std::string &text) { msg = K25_ME + text; return code; };
    if (path > PEP_CUT_CHAIN) return bad(PEP_ERR_ARG, "path " + std::to_string(path) + " is none of PEP_CUT_AUTO, PEP_CUT_BLOCK, PEP_CUT_CHAIN");
    if (n_trees == 0) return PEP_OK;
    if (!n_leaves || !leaf_off || !mat_off || !branch_off || !set_off || !sets) return bad(PEP_ERR_ARG, "null table");
    std::vector<uint32_t> order, size, inner;
    for (uint32_t t = 0; t < n_trees; ++t) {
        const uint64_t n = n_leaves[t], words = cut_words(n);
        const std::string tree = "tree " + std::to_string(t);
        if (n < 2) return bad(PEP_ERR_ARG, tree + " has " + std::to_string(n) + " leaves, a tree needs 2");
        if (n > PEP_NJ_MAX_LEAVES) return bad(PEP_ERR_LIMIT, tree + " has " + std::to_string(n) + " leaves, more than " + std::to_string(PEP_NJ_MAX_LEAVES));
        if (path == PEP_CUT_BLOCK && n > PEP_NJ_BLOCK_LEAVES)
            return bad(PEP_ERR_LIMIT, tree + " has " + std::to_string(n) + " leaves, the one-workgroup path takes " + std::to_string(PEP_NJ_BLOCK_LEAVES));
        const auto short_of = [&](const uint64_t *off, uint64_t need) { return off[t + 1] < off[t] || off[t + 1] - off[t] < need; };
        const auto overlap = [&](const char *what, const char *table, const uint64_t *off, uint64_t need) {
            return bad(PEP_ERR_ARG, std::string("the ") + what + " of " + tree + " (" + std::to_string(need) + " from " + std::to_string(off[t]) + ") overlap the next tree's or run past the array (" +
                                        table + "[" + std::to_string(t + 1) + "] = " + std::to_string(off[t + 1]) + ")");
        };
        if (short_of(leaf_off, n)) return overlap("leaves", "leaf_off", leaf_off, n);
        if (short_of(mat_off, n * n)) return overlap("matrix entries", "mat_off", mat_off, n * n);
        if (branch_off[t + 1] < branch_off[t]) return overlap("branches", "branch_off", branch_off, 1);
        const uint64_t B = branch_off[t + 1] - branch_off[t];
        if (B < 1 || B > 2 * n) return bad(PEP_ERR_ARG, tree + " has " + std::to_string(B) + " branches, a tree of " + std::to_string(n) + " leaves has 1 .. " + std::to_string(2 * n));
        if (short_of(set_off, B * words)) return overlap("bit-set words", "set_off", set_off, B * words);
    }
    if ((mat_off[n_trees] - mat_off[0]) > PEP_NJ_MAX_BYTES / 8)
        return bad(PEP_ERR_LIMIT, std::to_string(mat_off[n_trees] - mat_off[0]) + " entries (" + std::to_string((mat_off[n_trees] - mat_off[0]) / 1024 * 8) +
                                      " KiB) per matrix asked for, the device budget of one call is " + std::to_string((uint64_t)PEP_NJ_MAX_BYTES) + " bytes (split the batch)");
    if ((set_off[n_trees] - set_off[0]) > PEP_NJ_MAX_BYTES / 8)
        return bad(PEP_ERR_LIMIT, std::to_string(set_off[n_trees] - set_off[0]) + " bit-set words asked for, more than " + std::to_string((uint64_t)PEP_NJ_MAX_BYTES / 8));
    if (leaf_off[n_trees] - leaf_off[0] > PEP_NJ_MAX_BYTES / 8 || branch_off[n_trees] - branch_off[0] > PEP_NJ_MAX_BYTES / 8)
        return bad(PEP_ERR_LIMIT, std::to_string(leaf_off[n_trees] - leaf_off[0]) + " leaf entries and " + std::to_string(branch_off[n_trees] - branch_off[0]) +
                                      " branches asked for, more than " + std::to_string((uint64_t)PEP_NJ_MAX_BYTES / 8));
    // the branches: bipartitions of the leaves, pairwise compatible.  Each is turned to its side without leaf 0; taken by falling size, every set must lie
    // within ONE innermost set of those before it (a laminar family: the sum of the sides' sizes in work, not B^2 comparisons)
    for (uint32_t t = 0; t < n_trees; ++t) {
        const uint32_t n = n_leaves[t], words = cut_words(n), B = (uint32_t)(branch_off[t + 1] - branch_off[t]);
        const uint64_t *S = sets + set_off[t];
        const uint64_t last = n % 64 ? (1ull << (n % 64)) - 1 : ~0ull;
        size.assign(B, 0);
        for (uint32_t e = 0; e < B; ++e) {
            const uint64_t *s = S + (uint64_t)e * words;
            const std::string branch = "branch " + std::to_string(e) + " of tree " + std::to_string(t);
            if (s[words - 1] & ~last) return bad(PEP_ERR_ARG, branch + " is no bipartition of the leaves: it names a leaf beyond " + std::to_string(n - 1));
            uint32_t c = 0;
            for (uint32_t w = 0; w < words; ++w) c += (uint32_t)__builtin_popcountll(s[w]);
            if (c == 0 || c == n) return bad(PEP_ERR_ARG, branch + " is no bipartition of the leaves: one side is empty");
            size[e] = (s[0] & 1) ? n - c : c;
        }
        order.resize(B);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return size[a] > size[b]; });
        inner.assign(n, 0xFFFFFFFFu);
        for (uint32_t e : order) {
            const uint64_t *s = S + (uint64_t)e * words;
            const bool flip = s[0] & 1;
            bool seen = false;
            uint32_t within = 0;
            for (uint32_t w = 0; w < words; ++w) {
                uint64_t f = flip ? ~s[w] & (w + 1 == words ? last : ~0ull) : s[w];
                for (; f; f &= f - 1) {
                    const uint32_t l = 64 * w + (uint32_t)__builtin_ctzll(f);
                    if (!seen) { within = inner[l]; seen = true; }
                    else if (inner[l] != within)
                        return bad(PEP_ERR_ARG, "the branches of tree " + std::to_string(t) + " are not pairwise compatible: branch " + std::to_string(e) + " crosses another one");
                    inner[l] = e;
                }
            }
        }
    }
    return PEP_OK;
}

}  // namespace

extern "C" {

int pep_tree_cut_check(const uint32_t *n_leaves, uint32_t n_trees, const uint64_t *leaf_off, const uint64_t *mat_off, const uint64_t *branch_off,
                       const uint64_t *set_off, const uint64_t *sets, uint32_t path, char *msg, uint64_t msg_cap)
{
    std::string text;
    const int rc = cut_check(n_leaves, n_trees, leaf_off, mat_off, branch_off, set_off, sets, path, text);
    return pep_message_out(rc, text, msg, msg_cap);
}

int pep_tree_cut(pep_ctx *ctx, const uint32_t *h_n, uint32_t n_trees, const uint64_t *h_leaf_off, const uint64_t *h_mat_off, const uint64_t *h_branch_off,
                 const uint64_t *h_set_off, const uint64_t *h_sets, const double *h_len, const double *h_w0, const double *h_w1, const uint8_t *h_strong,
                 const uint32_t *h_cap, uint32_t path, int32_t *h_part, int32_t *h_counts, int32_t *h_log_i, double *h_log_v)
{
    if (!ctx) return PEP_ERR_ARG;
    CallTimes &times = ctx->calls[PEP_CALL_TREE_CUT];
    times = {};
    std::string msg;
    const int rc = cut_check(h_n, n_trees, h_leaf_off, h_mat_off, h_branch_off, h_set_off, h_sets, path, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    if (n_trees == 0) return PEP_OK;
    if (!h_len || !h_w0 || !h_w1 || !h_strong || !h_cap || !h_part || !h_counts || !h_log_i || !h_log_v) return pep_fail(ctx, PEP_ERR_ARG, std::string(K25_ME) + "null table");
    const uint64_t leaf0 = h_leaf_off[0], mat0 = h_mat_off[0], br0 = h_branch_off[0], set0 = h_set_off[0];
    const uint64_t n_leaf = h_leaf_off[n_trees] - leaf0, n_mat = h_mat_off[n_trees] - mat0, n_br = h_branch_off[n_trees] - br0, n_set = h_set_off[n_trees] - set0;
    std::vector<CutTree> trees(n_trees);
    std::vector<uint32_t> block, chain;
    std::vector<uint64_t> strong;
    uint64_t g_words = 0, rows = 0;
    for (uint32_t t = 0; t < n_trees; ++t) {
        const uint32_t n = h_n[t], words = cut_words(n), B = (uint32_t)(h_branch_off[t + 1] - h_branch_off[t]);
        const std::string tree = " of tree " + std::to_string(t);
        const double *w0 = h_w0 + h_mat_off[t], *w1 = h_w1 + h_mat_off[t];
        for (uint32_t a = 0; a < n; ++a)
            for (uint32_t b = a; b < n; ++b) {
                const uint64_t ab = (uint64_t)a * n + b, ba = (uint64_t)b * n + a;
                const std::string at = " [" + std::to_string(a) + ", " + std::to_string(b) + "]" + tree;
                if (!(std::isfinite(w0[ab]) && w0[ab] >= 0)) return pep_fail(ctx, PEP_ERR_ARG, K25_ME + ("W0" + at) + " is not finite and >= 0");
                if (!(std::isfinite(w1[ab]) && w1[ab] >= 0)) return pep_fail(ctx, PEP_ERR_ARG, K25_ME + ("W1" + at) + " is not finite and >= 0");
                if (w0[ab] != w0[ba]) return pep_fail(ctx, PEP_ERR_ARG, K25_ME + ("W0" + at) + " is not its mirror entry: the matrix is not symmetric");
                if (w1[ab] != w1[ba]) return pep_fail(ctx, PEP_ERR_ARG, K25_ME + ("W1" + at) + " is not its mirror entry: the matrix is not symmetric");
            }
        for (uint32_t e = 0; e < B; ++e)
            if (!std::isfinite(h_len[h_branch_off[t] + e])) return pep_fail(ctx, PEP_ERR_ARG, K25_ME + ("the length of branch " + std::to_string(e)) + tree + " is not finite");
        trees[t] = CutTree{h_mat_off[t] - mat0, g_words, h_set_off[t] - set0, h_branch_off[t] - br0, h_leaf_off[t] - leaf0, (uint64_t)strong.size(), rows, n, B, words, h_cap[t]};
        for (uint32_t w = 0; w < words; ++w) {
            uint64_t bits = 0;
            for (uint32_t j = 0; j < 64 && 64 * w + j < n; ++j)
                if (h_strong[h_leaf_off[t] + 64 * w + j]) bits |= 1ull << j;
            strong.push_back(bits);
        }
        g_words += (uint64_t)n * words;
        rows += n;
        (path == PEP_CUT_CHAIN || (path == PEP_CUT_AUTO && n > PEP_NJ_BLOCK_LEAVES) ? chain : block).push_back(t);
    }
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf *W = ctx->k25;
    const size_t which_bytes = (block.size() * 4 + 7) & ~(size_t)7;
    const size_t state_bytes = sizeof(CutState) + CUT_MAX_WORDS * 8;
    PEP_TRY(pep_tables_to_device(ctx, W, {{K25_W0, h_w0 + mat0, n_mat * 8, 0}, {K25_W1, h_w1 + mat0, n_mat * 8, 0}, {K25_SETS, h_sets + set0, n_set * 8, 0},
                                          {K25_LEN, h_len + br0, n_br * 8, 0}, {K25_TREES, trees.data(), trees.size() * sizeof(CutTree), 0},
                                          {K25_STRONG, strong.data(), strong.size() * 8, 0}, {K25_STATE, block.data(), block.size() * 4, which_bytes - block.size() * 4 + state_bytes},
                                          {K25_M, nullptr, n_mat * 8, 0}, {K25_G, nullptr, g_words * 8, 0}, {K25_SCORE, nullptr, n_br * 8 * CUT_SCORE, 0},
                                          {K25_FIN, nullptr, n_br * 4, 0}, {K25_PART, nullptr, n_leaf * 4, 0}, {K25_COUNTS, nullptr, (size_t)n_trees * 16, 0},
                                          {K25_LOGI, nullptr, n_leaf * 8, 0}, {K25_LOGV, nullptr, n_leaf * 32, 0}}));
    PEP_HIP(ctx, hipMemsetAsync(W[K25_PART].p, 0xFF, n_leaf * 4, ctx->stream));            // (the entries between two trees: -1)
    PEP_HIP(ctx, hipMemsetAsync(W[K25_LOGI].p, 0, n_leaf * 8, ctx->stream));
    PEP_HIP(ctx, hipMemsetAsync(W[K25_LOGV].p, 0, n_leaf * 32, ctx->stream));
    CutDev D{W[K25_W0].as<const double>(), W[K25_W1].as<const double>(), W[K25_M].as<double>(), W[K25_G].as<uint64_t>(), W[K25_SETS].as<const uint64_t>(),
             W[K25_STRONG].as<const uint64_t>(), W[K25_LEN].as<const double>(), W[K25_SCORE].as<double>(), W[K25_FIN].as<uint32_t>(), W[K25_PART].as<int32_t>(),
             W[K25_COUNTS].as<int32_t>(), W[K25_LOGI].as<int32_t>(), W[K25_LOGV].as<double>()};
    const CutTree *d_trees = W[K25_TREES].as<const CutTree>();
    pep_timed_stage(ctx, times.ms[0], [&] {
        hipLaunchKernelGGL(cut_prep, dim3((unsigned)ceil_div(rows, CUT_WAVES)), dim3(CUT_BLOCK), 0, ctx->stream, d_trees, n_trees, rows, D);
        if (!block.empty()) hipLaunchKernelGGL(cut_block, dim3((unsigned)block.size()), dim3(CUT_BLOCK), 0, ctx->stream, d_trees, W[K25_STATE].as<const uint32_t>(), D);
    });
    PEP_HIP(ctx, hipGetLastError());
    if (!chain.empty()) {
        uint8_t *st = W[K25_STATE].as<uint8_t>() + which_bytes;
        int failed = PEP_OK;
        pep_timed_stage(ctx, times.ms[1], [&] {
            for (uint32_t t : chain) {
                const CutTree &R = trees[t];
                CutView V{D.W0 + R.mat_off, D.W1 + R.mat_off, D.M + R.mat_off, D.G + R.g_off, D.sets + R.set_off, D.strong + R.word_off, D.len + R.branch_off,
                          D.score + CUT_SCORE * R.branch_off, D.fin + R.branch_off, D.part + R.leaf_off, D.counts + 4 * (uint64_t)t, D.log_i + 2 * R.leaf_off,
                          D.log_v + 4 * R.leaf_off, reinterpret_cast<uint64_t *>(st + sizeof(CutState)), reinterpret_cast<CutState *>(st), R.n, R.B, R.words, R.cap};
                hipLaunchKernelGGL(cut_chain_start, dim3(1), dim3(CUT_BLOCK), 0, ctx->stream, V);
                // every iteration cuts (fewer than n times) or finishes a component (n at most)
                const uint32_t most_rounds = 2 * R.n / PEP_CUT_ROUND + 2;
                uint32_t done = 0;
                for (uint32_t round = 0; round < most_rounds && !done && failed == PEP_OK; ++round) {
                    for (int it = 0; it < PEP_CUT_ROUND; ++it) {
                        hipLaunchKernelGGL(cut_chain_score, dim3((unsigned)ceil_div(R.B, CUT_WAVES)), dim3(CUT_BLOCK), 0, ctx->stream, V);
                        hipLaunchKernelGGL(cut_chain_select, dim3(1), dim3(CUT_BLOCK), 0, ctx->stream, V);
                    }
                    failed = pep_read_back(ctx, &done, &V.st->done, 4);
                    if (failed == PEP_OK) failed = pep_sync_reads(ctx);
                }
                if (failed == PEP_OK && !done) failed = pep_fail(ctx, PEP_ERR_INTERNAL, K25_ME + ("tree " + std::to_string(t)) + " was not finished by its launch chain");
                if (failed != PEP_OK) break;
            }
        });
        if (failed != PEP_OK) return failed;
        PEP_HIP(ctx, hipGetLastError());
    }
    PEP_TRY(pep_d2h_queue(ctx, h_part + leaf0, D.part, n_leaf * 4));
    PEP_TRY(pep_d2h_queue(ctx, h_counts, D.counts, (size_t)n_trees * 16));
    PEP_TRY(pep_d2h_queue(ctx, h_log_i + 2 * leaf0, D.log_i, n_leaf * 8));
    PEP_TRY(pep_d2h_queue(ctx, h_log_v + 4 * leaf0, D.log_v, n_leaf * 32));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    return PEP_OK;
}

}  // extern "C"
