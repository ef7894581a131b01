// K24: the allele pass of write_output (PEPPAN.py:1391-1472).  For every prediction the reference cuts the predicted region out of its contig, reverse-complements
// it character by character on '-', uses the string as a dictionary key to number the alleles of its gene, and works out the window determineGeneStructure
// (K19) is to look at - one Python round per prediction.  Restated (include/peppan_hip.h, K24): the window and the allele span are integer functions of a
// row and of at most five neighbours; an allele's number is the rank of its class's first row among the first rows of its gene, its 't' that row's property.
//   oa_plan      one thread per row: class, neighbour walk, s2 e2 lp, the allele span -> the plan record and the item (arena position, length, gene, strand).
//                oa_plan_row is the one statement of those rules: the host check runs the same function over every row before anything is launched.
//   oa_digest    one thread per item (seeds in front of the rows), sha1_window of sha1.h as K23's cds_digest: the span read in place, strand-corrected.
//   oa_classes   an open-addressed table of item indices, one slot per (gene, length, digest): an empty slot is claimed with a compare-and-swap, a taken one is
//                compared through the digest of whichever member stands in it and, when equal, lowered with atomicMin - members of a class have equal keys, so
//                the slot may change hands among them while others read it.  What is left is the smallest member: no trace of the order of execution.
//   oa_verify    every item against its class's first member, strand-aware, sixteen bytes of text at a time and a tail by bytes; the smallest offender -> a counter
//                the host reads.  Also emits the sort key: (gene, item) for a first member, beyond every gene for the others.
//   pep_sort_u64 the library's radix sort; then oa_starts marks where every gene's run begins, oa_ranks numbers the first members, oa_assign hands every
//                row its class's rank and 't' flag.
// What bounds them: the digest, ~1100 integer operations per 64 bytes with the lanes of a wavefront on spans of different lengths, and byte-granular reads of
// the comparison.  DESIGN.md 4.10k.
#include "common.h"
#include "sha1.h"
#include <algorithm>
#include <cstring>

namespace {

// the slots of ctx->ws this call uses
enum {
    K24_NT = 0, K24_OFF, K24_ROWS, K24_LOOK, K24_PLAN, K24_ITEM, K24_TFLAG, K24_DIGEST, K24_TABLE, K24_SLOT, K24_FIRST, K24_KEYS, K24_KEYS_TMP, K24_START,
    K24_RANKF, K24_OUT_FIRST, K24_OUT_RANK, K24_OUT_T, K24_BAD, K24_SLOTS
};
static_assert(K24_SLOTS <= PEP_WS_HITS_OUT, "leaves the device-resident hit table alone");

constexpr uint32_t OA_NONE = 0xFFFFFFFFu;
constexpr uint32_t OA_SKIP = 1u << 31, OA_REV = 1u << 30, OA_GENE = OA_REV - 1u;      // an item's meta word
constexpr int OA_BLOCK = 256;

// one allele as the digest and the comparison read it
struct OaItem {
    uint64_t at;                     // where its span starts in the arena
    uint32_t len;
    uint32_t meta;                   // OA_SKIP | OA_REV | gene
};
static_assert(sizeof(OaItem) == 16, "one 16-byte read per item");

enum OaRefusal { OA_OK = 0, OA_S_LOW, OA_E_LOW, OA_E_HIGH, OA_QS_LOW, OA_LP_NEG, OA_NO_WINDOW, OA_E2_HIGH };

struct OaPlan { int32_t cls, s2, e2, lp, a, len; int refusal; };

__host__ __device__ inline int64_t oa_t3(int64_t x) { return 3 * (x / 3); }             // 3 * int(x / 3): C division truncates toward zero as int() does
__host__ __device__ inline int64_t oa_min(int64_t a, int64_t b) { return a < b ? a : b; }

// the plan of row i (the header states it); contig_len: the actual length of the row's contig
__host__ __device__ inline OaPlan oa_plan_row(const int32_t *__restrict__ rows, const int32_t *__restrict__ look9, uint32_t n_rows, uint32_t i, int64_t contig_len)
{
    const int32_t *r = rows + (size_t)i * PEP_OUTA_COLS;
    OaPlan p = {PEP_OUTA_SKIPPED, 0, 0, 0, 0, 0, OA_OK};
    const int32_t flags = r[PEP_OUTA_FLAGS];
    if (flags & (PEP_OUTA_MISC | PEP_OUTA_NONAME)) return p;
    const int64_t s = r[PEP_OUTA_S], e = r[PEP_OUTA_E], c7 = r[PEP_OUTA_QS], c8 = r[PEP_OUTA_QE], c12 = r[PEP_OUTA_REFLEN], clen = r[PEP_OUTA_CLEN];
    if (s < 1) { p.refusal = OA_S_LOW; return p; }
    if (e < s - 1) { p.refusal = OA_E_LOW; return p; }
    if (e > contig_len) { p.refusal = OA_E_HIGH; return p; }
    if (c7 < 1) { p.refusal = OA_QS_LOW; return p; }
    if (r[PEP_OUTA_PART] > 1 || e - s + 1 < c12 - r[PEP_OUTA_VARY]) {
        p.cls = PEP_OUTA_FRAGMENT;
        p.s2 = (int32_t)s; p.e2 = (int32_t)e; p.a = (int32_t)(s - 1); p.len = (int32_t)(e - s + 1);
        return p;
    }
    const int32_t contig = r[PEP_OUTA_CONTIG];
    int64_t s2, e2, lp, a, b;
    int64_t other = -1;                                                 // pred2
    if (!(flags & PEP_OUTA_MINUS)) {
        for (uint32_t j = i + 1; j < n_rows && j <= i + 4; ++j) {
            const int32_t *q = rows + (size_t)j * PEP_OUTA_COLS;
            if (q[PEP_OUTA_CONTIG] != contig) break;
            if (!(q[PEP_OUTA_FLAGS] & PEP_OUTA_MISC)) other = j;       // (the reference's break is commented out: the last one)
        }
        e2 = e + oa_min(oa_t3(clen - e), other >= 0 ? oa_t3((int64_t)rows[(size_t)other * PEP_OUTA_COLS + PEP_OUTA_E] + 300 - e) : 600 + c12 - c8);
        s2 = s - oa_min(oa_t3(s - 1), 60 + c7 - 1);
        lp = s - s2;
        a = s - 1; b = oa_min(e, e2);
    } else {
        for (uint32_t k = 1; k <= 5 && k <= i; ++k) {
            const int32_t *q = rows + (size_t)(i - k) * PEP_OUTA_COLS;
            if (q[PEP_OUTA_CONTIG] != contig) break;
            if (!(q[PEP_OUTA_FLAGS] & PEP_OUTA_MISC)) other = i - k;   // (the farthest one)
        }
        int64_t s9 = 0;
        if (other >= 0) {
            // a row of an earlier batch has had determineGeneStructure's start written back by the time this row is reached
            const bool updated = look9 && (uint32_t)other < i - i % PEP_OUTA_BATCH;
            s9 = updated ? look9[other] : rows[(size_t)other * PEP_OUTA_COLS + PEP_OUTA_S];
        }
        s2 = s - oa_min(oa_t3(s - 1), other >= 0 ? oa_t3(s - s9 + 300) : 600 + c12 - c8);
        e2 = e + oa_min(oa_t3(clen - e), 60 + c7 - 1);
        lp = e2 - e;
        a = (s > s2 ? s : s2) - 1; b = e;
    }
    if (lp < 0) { p.refusal = OA_LP_NEG; return p; }
    if (e2 < s2 - 1) { p.refusal = OA_NO_WINDOW; return p; }
    if (e2 > contig_len) { p.refusal = OA_E2_HIGH; return p; }
    const int64_t len = b > a ? b - a : 0;
    p.s2 = (int32_t)s2; p.e2 = (int32_t)e2; p.lp = (int32_t)lp; p.a = (int32_t)a; p.len = (int32_t)len;
    p.cls = r[PEP_OUTA_SVMIN] && len < r[PEP_OUTA_SVMIN] ? PEP_OUTA_STRUCTVAR : PEP_OUTA_INTACT;
    return p;
}

// the 't' of an id this row would give a new allele (:1420, :1454-1457)
__host__ __device__ inline uint32_t oa_tflag(const int32_t *r, int cls)
{
    return cls == PEP_OUTA_FRAGMENT || (r[PEP_OUTA_FLAGS] & PEP_OUTA_SECONDARY) || r[PEP_OUTA_QS] != 1 || r[PEP_OUTA_QE] != r[PEP_OUTA_REFLEN];
}

// (the host has seen every row pass: no refusal here)
__global__ __launch_bounds__(OA_BLOCK) void oa_plan(const int32_t *__restrict__ rows, const int32_t *__restrict__ look9, uint32_t n_rows, const uint64_t *__restrict__ contig_off,
                                                    int32_t *__restrict__ plan, OaItem *__restrict__ items, uint8_t *__restrict__ tflag)
{
    const uint32_t i = blockIdx.x * OA_BLOCK + threadIdx.x;
    if (i >= n_rows) return;
    const int32_t *r = rows + (size_t)i * PEP_OUTA_COLS;
    const bool skipped = r[PEP_OUTA_FLAGS] & (PEP_OUTA_MISC | PEP_OUTA_NONAME);
    const uint64_t base = skipped ? 0 : contig_off[r[PEP_OUTA_CONTIG]];
    const OaPlan p = oa_plan_row(rows, look9, n_rows, i, skipped ? 0 : (int64_t)(contig_off[r[PEP_OUTA_CONTIG] + 1] - base));
    int32_t *out = plan + (size_t)i * PEP_OUTA_PLAN_COLS;
    out[0] = p.cls; out[1] = p.s2; out[2] = p.e2; out[3] = p.lp; out[4] = p.a; out[5] = p.len;
    if (!items) return;                                                 // (the plan alone was asked for)
    OaItem it;
    it.at = base + (uint64_t)p.a;
    it.len = (uint32_t)p.len;
    it.meta = skipped ? OA_SKIP : (uint32_t)r[PEP_OUTA_GENE] | ((r[PEP_OUTA_FLAGS] & PEP_OUTA_MINUS) ? OA_REV : 0u);
    items[i] = it;
    tflag[i] = skipped ? 0 : (uint8_t)oa_tflag(r, p.cls);
}

__global__ __launch_bounds__(OA_BLOCK) void oa_digest(const uint8_t *__restrict__ nt, const OaItem *__restrict__ items, uint32_t n_items, uint32_t *__restrict__ digest)
{
    const uint32_t i = blockIdx.x * OA_BLOCK + threadIdx.x;
    if (i >= n_items) return;
    const OaItem it = items[i];
    if (it.meta & OA_SKIP) return;
    uint32_t h[5];
    sha1_window(nt + it.at, it.len, (it.meta & OA_REV) != 0, h);
#pragma unroll
    for (int k = 0; k < 5; ++k) digest[(size_t)i * 5 + k] = h[k];
}

// are items i and j of one class: gene, length and digest - or, with key_mask, gene and the masked first word
__device__ __forceinline__ bool oa_same_key(const OaItem *__restrict__ items, const uint32_t *__restrict__ digest, uint32_t i, uint32_t j, uint32_t key_mask)
{
    if (((items[i].meta ^ items[j].meta) & OA_GENE) != 0) return false;
    const uint32_t *x = digest + (size_t)i * 5, *y = digest + (size_t)j * 5;
    if (key_mask) return ((x[0] ^ y[0]) & key_mask) == 0;
    return items[i].len == items[j].len && x[0] == y[0] && x[1] == y[1] && x[2] == y[2] && x[3] == y[3] && x[4] == y[4];
}

// table: 2^k slots >= 2 n_items, all OA_NONE on entry
__global__ __launch_bounds__(OA_BLOCK) void oa_classes(const OaItem *__restrict__ items, const uint32_t *__restrict__ digest, uint32_t n_items, uint32_t key_mask, uint32_t *table,
                                                       uint32_t slot_mask, uint32_t *__restrict__ slot_of)
{
    const uint32_t i = blockIdx.x * OA_BLOCK + threadIdx.x;
    if (i >= n_items) return;
    const uint32_t meta = items[i].meta;
    if (meta & OA_SKIP) { slot_of[i] = OA_NONE; return; }
    const uint32_t d0 = digest[(size_t)i * 5], d1 = digest[(size_t)i * 5 + 1];
    uint32_t slot = ((key_mask ? (d0 & key_mask) * 0x85EBCA6Bu : d0 ^ (d1 * 0x85EBCA6Bu)) ^ ((meta & OA_GENE) * 0x9E3779B1u)) & slot_mask;
    for (;;) {                                                          // (ends: the table has more slots than there are items)
        uint32_t held = atomicCAS(&table[slot], OA_NONE, i);
        if (held == OA_NONE || held == i) break;
        if (oa_same_key(items, digest, i, held, key_mask)) { atomicMin(&table[slot], i); break; }
        slot = (slot + 1) & slot_mask;
    }
    slot_of[i] = slot;
}

// byte k of an item's text
__device__ __forceinline__ uint32_t oa_text(const uint8_t *__restrict__ s, uint32_t len, bool rev, uint32_t k) { return rev ? sha1_rc_byte(s[len - 1u - k]) : (uint32_t)s[k]; }

// ... and bytes k .. k + 15 (k + 16 <= len) as four little-endian dwords in text order: one unaligned 16-byte load, from the span's far end when it is read backward -
// text byte 4 w + b is then byte 3 - b of dword 3 - w of what was loaded, complemented
__device__ __forceinline__ void oa_text16(const uint8_t *__restrict__ s, uint32_t len, bool rev, uint32_t k, uint32_t out[4])
{
    if (!rev) { __builtin_memcpy(out, s + k, 16); return; }
    uint32_t r[4];
    __builtin_memcpy(r, s + (len - k - 16u), 16);
#pragma unroll
    for (int w = 0; w < 4; ++w) out[w] = __builtin_bswap32(sha1_rc_word(r[3 - w]));
}

__global__ __launch_bounds__(OA_BLOCK) void oa_verify(const uint8_t *__restrict__ nt, const OaItem *__restrict__ items, const uint32_t *__restrict__ table,
                                                      const uint32_t *__restrict__ slot_of, uint32_t n_items, uint32_t n_genes, int item_bits, uint32_t *__restrict__ first_of,
                                                      uint64_t *__restrict__ keys, uint32_t *bad)
{
    const uint32_t i = blockIdx.x * OA_BLOCK + threadIdx.x;
    if (i >= n_items) return;
    const OaItem it = items[i];
    const uint32_t slot = slot_of[i];
    const uint32_t f = slot == OA_NONE ? OA_NONE : table[slot];
    first_of[i] = f;
    keys[i] = (uint64_t)(f == i ? it.meta & OA_GENE : n_genes) << item_bits | i;
    if (f == OA_NONE || f == i) return;
    const OaItem ft = items[f];
    bool same = it.len == ft.len;
    if (same) {
        const uint8_t *x = nt + it.at, *y = nt + ft.at;
        const uint32_t len = it.len;
        const bool rx = (it.meta & OA_REV) != 0, ry = (ft.meta & OA_REV) != 0;
        uint32_t k = 0, diff = 0;
        for (; !diff && k + 16u <= len; k += 16u) {
            uint32_t u[4], v[4];
            oa_text16(x, len, rx, k, u);
            oa_text16(y, len, ry, k, v);
            diff = (u[0] ^ v[0]) | (u[1] ^ v[1]) | (u[2] ^ v[2]) | (u[3] ^ v[3]);
        }
        for (; !diff && k < len; ++k) diff = oa_text(x, len, rx, k) ^ oa_text(y, len, ry, k);
        same = diff == 0;
    }
    if (!same) atomicMin(bad, i);
}

// sorted keys: the first members by (gene, item), then everything else
__global__ __launch_bounds__(OA_BLOCK) void oa_starts(const uint64_t *__restrict__ keys, uint32_t n_items, uint32_t n_genes, int item_bits, uint32_t *__restrict__ start)
{
    const uint32_t p = blockIdx.x * OA_BLOCK + threadIdx.x;
    if (p >= n_items) return;
    const uint32_t g = (uint32_t)(keys[p] >> item_bits);
    if (g < n_genes && (p == 0 || (uint32_t)(keys[p - 1] >> item_bits) != g)) start[g] = p;
}

__global__ __launch_bounds__(OA_BLOCK) void oa_ranks(const uint64_t *__restrict__ keys, uint32_t n_items, uint32_t n_genes, int item_bits, const uint32_t *__restrict__ start,
                                                     uint32_t *__restrict__ rank_first)
{
    const uint32_t p = blockIdx.x * OA_BLOCK + threadIdx.x;
    if (p >= n_items) return;
    const uint64_t key = keys[p];
    const uint32_t g = (uint32_t)(key >> item_bits);
    if (g < n_genes) rank_first[(uint32_t)(key & ((1ull << item_bits) - 1ull))] = p - start[g] + 1u;
}

// rows are the items behind the n_seeds seeds
__global__ __launch_bounds__(OA_BLOCK) void oa_assign(const uint32_t *__restrict__ first_of, const uint32_t *__restrict__ rank_first, const uint8_t *__restrict__ tflag,
                                                      uint32_t n_seeds, uint32_t n_rows, int32_t *__restrict__ first, uint32_t *__restrict__ rank, uint8_t *__restrict__ t)
{
    const uint32_t i = blockIdx.x * OA_BLOCK + threadIdx.x;
    if (i >= n_rows) return;
    const uint32_t f = first_of[n_seeds + i];
    if (f == OA_NONE) { first[i] = -2; rank[i] = 0; t[i] = 0; return; }
    first[i] = f < n_seeds ? -1 : (int32_t)(f - n_seeds);
    rank[i] = rank_first[f];
    t[i] = tflag[f];
}

const char *const K24_ME = "pep_out_alleles: ";

int oa_bit_length(uint64_t v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }

// every check of the tables, on the host, before anything is launched; also makes the seeds' item records
int k24_check(const uint64_t *contig_off, uint32_t n_contigs, uint32_t n_genes, const int32_t *seed_contig, uint32_t n_rows, const int32_t *rows, const int32_t *look9,
              uint32_t key_bits, std::vector<OaItem> *seeds, std::string &msg)
{
    const auto bad = [&](int code, const std::string &text) { msg = K24_ME + text; return code; };
    if (!contig_off || (n_genes && !seed_contig) || (n_rows && !rows)) return bad(PEP_ERR_ARG, "null table");
    if (key_bits > 31) return bad(PEP_ERR_ARG, "key_bits " + std::to_string(key_bits) + " is beyond 31");
    if ((uint64_t)n_rows + n_genes >= PEP_OUTA_MAX_ITEMS) return bad(PEP_ERR_LIMIT, "2^30 rows and genes or more");
    if (contig_off[0] != 0) return bad(PEP_ERR_ARG, "contig_off must start at 0");
    for (uint32_t c = 0; c < n_contigs; ++c) {
        if (contig_off[c + 1] < contig_off[c]) return bad(PEP_ERR_ARG, "contig_off must be non-decreasing (contig " + std::to_string(c) + ")");
        if (contig_off[c + 1] - contig_off[c] >= PEP_OUTA_MAX_CONTIG) return bad(PEP_ERR_LIMIT, "contig " + std::to_string(c) + " holds 2^31 bytes or more");
    }
    for (uint32_t g = 0; g < n_genes; ++g) {
        if (seed_contig[g] < -1 || (seed_contig[g] >= 0 && (uint32_t)seed_contig[g] >= n_contigs))
            return bad(PEP_ERR_ARG, "the seed of gene " + std::to_string(g) + " names contig " + std::to_string(seed_contig[g]) + " of " + std::to_string(n_contigs));
        if (seeds && seed_contig[g] >= 0)
            seeds->push_back(OaItem{contig_off[seed_contig[g]], (uint32_t)(contig_off[seed_contig[g] + 1] - contig_off[seed_contig[g]]), g});
    }
    // the indices first: the plan of a row reads its neighbours
    for (uint32_t i = 0; i < n_rows; ++i) {
        const int32_t *r = rows + (size_t)i * PEP_OUTA_COLS;
        const std::string who = "row " + std::to_string(i);
        if (r[PEP_OUTA_FLAGS] & ~(PEP_OUTA_MISC | PEP_OUTA_NONAME | PEP_OUTA_SECONDARY | PEP_OUTA_MINUS))
            return bad(PEP_ERR_ARG, who + " has flag bits beyond the four (" + std::to_string(r[PEP_OUTA_FLAGS]) + ")");
        if (r[PEP_OUTA_CONTIG] < 0 || (uint32_t)r[PEP_OUTA_CONTIG] >= n_contigs)
            return bad(PEP_ERR_ARG, who + " names contig " + std::to_string(r[PEP_OUTA_CONTIG]) + " of " + std::to_string(n_contigs));
        if (r[PEP_OUTA_FLAGS] & (PEP_OUTA_MISC | PEP_OUTA_NONAME)) continue;
        if (r[PEP_OUTA_GENE] < 0 || (uint32_t)r[PEP_OUTA_GENE] >= n_genes)
            return bad(PEP_ERR_ARG, who + " names gene " + std::to_string(r[PEP_OUTA_GENE]) + " of " + std::to_string(n_genes));
        if (r[PEP_OUTA_SVMIN] < 0) return bad(PEP_ERR_ARG, who + " has a negative structural-variation length");
    }
    for (uint32_t i = 0; i < n_rows; ++i) {
        const int32_t *r = rows + (size_t)i * PEP_OUTA_COLS;
        if (r[PEP_OUTA_FLAGS] & (PEP_OUTA_MISC | PEP_OUTA_NONAME)) continue;
        const int64_t contig_len = (int64_t)(contig_off[r[PEP_OUTA_CONTIG] + 1] - contig_off[r[PEP_OUTA_CONTIG]]);
        const OaPlan p = oa_plan_row(rows, look9, n_rows, i, contig_len);
        if (p.refusal == OA_OK) continue;
        const std::string who = "row " + std::to_string(i), se = " (s " + std::to_string(r[PEP_OUTA_S]) + ", e " + std::to_string(r[PEP_OUTA_E]) + ")";
        const std::string of = " of " + std::to_string(contig_len) + " bytes";
        switch (p.refusal) {
            case OA_S_LOW: return bad(PEP_ERR_ARG, who + " starts before its contig" + se);
            case OA_E_LOW: return bad(PEP_ERR_ARG, who + " ends before it starts" + se);
            case OA_E_HIGH: return bad(PEP_ERR_ARG, who + " leaves its contig" + of + se);
            case OA_QS_LOW: return bad(PEP_ERR_ARG, who + " has column 7 = " + std::to_string(r[PEP_OUTA_QS]) + ", below 1");
            case OA_LP_NEG: return bad(PEP_ERR_ARG, "the window of " + who + " starts inside its region: the reference's slice would wrap" + se);
            case OA_NO_WINDOW: return bad(PEP_ERR_ARG, "the window of " + who + " ends before it starts" + se);
            default: return bad(PEP_ERR_ARG, "the window of " + who + " leaves its contig" + of + se);
        }
    }
    return PEP_OK;
}

}  // namespace

extern "C" {

int pep_out_alleles_check(const uint64_t *contig_off, uint32_t n_contigs, uint32_t n_genes, const int32_t *seed_contig, uint32_t n_rows, const int32_t *rows,
                          const int32_t *look9, uint32_t key_bits, char *msg, uint64_t msg_cap)
{
    std::string text;
    const int rc = k24_check(contig_off, n_contigs, n_genes, seed_contig, n_rows, rows, look9, key_bits, nullptr, text);
    return pep_message_out(rc, text, msg, msg_cap);
}

int pep_out_alleles(pep_ctx *ctx, const uint8_t *nt, const uint64_t *contig_off, uint32_t n_contigs, uint32_t n_genes, const int32_t *seed_contig, uint32_t n_rows,
                    const int32_t *rows, const int32_t *look9, int plan_only, uint32_t key_bits, int32_t *plan, int32_t *first, uint32_t *rank, uint8_t *tflag)
{
    if (!ctx) return PEP_ERR_ARG;
    CallTimes &times = ctx->calls[PEP_CALL_OUT_ALLELES];
    times = {};
    if (n_rows && (!plan || (!plan_only && (!first || !rank || !tflag)))) return pep_fail(ctx, PEP_ERR_ARG, std::string(K24_ME) + "null table");
    PEP_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<OaItem> seeds;
    std::string msg;
    const int rc = k24_check(contig_off, n_contigs, n_genes, seed_contig, n_rows, rows, look9, key_bits, &seeds, msg);
    if (rc != PEP_OK) return pep_fail(ctx, rc, msg);
    if (n_rows == 0) return PEP_OK;
    const uint64_t n_nt = contig_off[n_contigs];
    if (!plan_only && n_nt && !nt) return pep_fail(ctx, PEP_ERR_ARG, std::string(K24_ME) + "null table");
    DevBuf *W = ctx->ws;
    hipStream_t st = ctx->stream;
    const uint32_t n_seeds = (uint32_t)seeds.size(), n_items = n_seeds + n_rows;
    const size_t row_bytes = (size_t)n_rows * PEP_OUTA_COLS * 4, plan_bytes = (size_t)n_rows * PEP_OUTA_PLAN_COLS * 4;
    const unsigned row_blocks = (unsigned)ceil_div(n_rows, OA_BLOCK), item_blocks = (unsigned)ceil_div(n_items, OA_BLOCK);
    std::vector<int32_t> h_plan((size_t)n_rows * PEP_OUTA_PLAN_COLS);

    if (plan_only) {
        PEP_TRY(pep_tables_to_device(ctx, W, {{K24_OFF, contig_off, ((size_t)n_contigs + 1) * 8, 0}, {K24_ROWS, rows, row_bytes, 0},
                                              {K24_LOOK, look9, look9 ? (size_t)n_rows * 4 : 0, 4}, {K24_PLAN, nullptr, plan_bytes, 0}}));
        pep_timed_stage(ctx, times.ms[0], [&] {
            hipLaunchKernelGGL(oa_plan, dim3(row_blocks), dim3(OA_BLOCK), 0, st, W[K24_ROWS].as<const int32_t>(), look9 ? W[K24_LOOK].as<const int32_t>() : nullptr, n_rows,
                               W[K24_OFF].as<const uint64_t>(), W[K24_PLAN].as<int32_t>(), (OaItem *)nullptr, (uint8_t *)nullptr);
        });
        PEP_HIP(ctx, hipGetLastError());
        PEP_TRY(pep_d2h_queue(ctx, h_plan.data(), W[K24_PLAN].p, plan_bytes));
        PEP_HIP(ctx, pep_stream_wait(ctx));
        pep_d2h_finish(ctx);
        memcpy(plan, h_plan.data(), plan_bytes);
        return PEP_OK;
    }

    uint32_t slots = 1024;
    while (slots < 2ull * n_items) slots <<= 1;                         // (n_items < 2^30)
    const int item_bits = oa_bit_length(n_items), gene_bits = oa_bit_length(n_genes);
    PEP_TRY(pep_tables_to_device(ctx, W, {{K24_NT, nt, n_nt, 16}, {K24_OFF, contig_off, ((size_t)n_contigs + 1) * 8, 0}, {K24_ROWS, rows, row_bytes, 0},
                                          {K24_LOOK, look9, look9 ? (size_t)n_rows * 4 : 0, 4}, {K24_PLAN, nullptr, plan_bytes, 0},
                                          {K24_ITEM, seeds.data(), (size_t)n_seeds * sizeof(OaItem), (size_t)n_rows * sizeof(OaItem)}, {K24_TFLAG, nullptr, n_items, 0},
                                          {K24_DIGEST, nullptr, (size_t)n_items * 20, 0}, {K24_TABLE, nullptr, (size_t)slots * 4, 0}, {K24_SLOT, nullptr, (size_t)n_items * 4, 0},
                                          {K24_FIRST, nullptr, (size_t)n_items * 4, 0}, {K24_KEYS, nullptr, (size_t)n_items * 8, 0},
                                          {K24_KEYS_TMP, nullptr, (size_t)n_items * 8, 0}, {K24_START, nullptr, (size_t)n_genes * 4, 4},
                                          {K24_RANKF, nullptr, (size_t)n_items * 4, 0}, {K24_OUT_FIRST, nullptr, (size_t)n_rows * 4, 0},
                                          {K24_OUT_RANK, nullptr, (size_t)n_rows * 4, 0}, {K24_OUT_T, nullptr, n_rows, 0}, {K24_BAD, nullptr, 4, 0}}));
    OaItem *d_items = W[K24_ITEM].as<OaItem>();
    uint8_t *d_tflag = W[K24_TFLAG].as<uint8_t>();
    uint32_t *d_digest = W[K24_DIGEST].as<uint32_t>(), *d_table = W[K24_TABLE].as<uint32_t>(), *d_slot = W[K24_SLOT].as<uint32_t>(), *d_first = W[K24_FIRST].as<uint32_t>();
    uint64_t *d_keys = W[K24_KEYS].as<uint64_t>();
    PEP_HIP(ctx, hipMemsetAsync(d_tflag, 0, n_seeds ? n_seeds : 1, st));                             // a seed's id is '1': no 't'
    PEP_HIP(ctx, hipMemsetAsync(d_table, 0xFF, (size_t)slots * 4, st));
    PEP_HIP(ctx, hipMemsetAsync(W[K24_BAD].p, 0xFF, 4, st));
    pep_timed_stage(ctx, times.ms[0], [&] {
        hipLaunchKernelGGL(oa_plan, dim3(row_blocks), dim3(OA_BLOCK), 0, st, W[K24_ROWS].as<const int32_t>(), look9 ? W[K24_LOOK].as<const int32_t>() : nullptr, n_rows,
                           W[K24_OFF].as<const uint64_t>(), W[K24_PLAN].as<int32_t>(), d_items + n_seeds, d_tflag + n_seeds);
    });
    pep_timed_stage(ctx, times.ms[1], [&] {
        hipLaunchKernelGGL(oa_digest, dim3(item_blocks), dim3(OA_BLOCK), 0, st, W[K24_NT].as<const uint8_t>(), (const OaItem *)d_items, n_items, d_digest);
    });
    pep_timed_stage(ctx, times.ms[2], [&] {
        hipLaunchKernelGGL(oa_classes, dim3(item_blocks), dim3(OA_BLOCK), 0, st, (const OaItem *)d_items, (const uint32_t *)d_digest, n_items,
                           key_bits ? (1u << key_bits) - 1u : 0u, d_table, slots - 1u, d_slot);
    });
    pep_timed_stage(ctx, times.ms[3], [&] {
        hipLaunchKernelGGL(oa_verify, dim3(item_blocks), dim3(OA_BLOCK), 0, st, W[K24_NT].as<const uint8_t>(), (const OaItem *)d_items, (const uint32_t *)d_table,
                           (const uint32_t *)d_slot, n_items, n_genes, item_bits, d_first, d_keys, W[K24_BAD].as<uint32_t>());
    });
    PEP_HIP(ctx, hipGetLastError());
    int sort_rc = PEP_OK;
    pep_timed_stage(ctx, times.ms[4], [&] { sort_rc = pep_sort_u64(ctx, d_keys, W[K24_KEYS_TMP].as<uint64_t>(), nullptr, n_items, item_bits + gene_bits, nullptr, nullptr); });
    PEP_TRY(sort_rc);
    pep_timed_stage(ctx, times.ms[5], [&] {
        hipLaunchKernelGGL(oa_starts, dim3(item_blocks), dim3(OA_BLOCK), 0, st, (const uint64_t *)d_keys, n_items, n_genes, item_bits, W[K24_START].as<uint32_t>());
        hipLaunchKernelGGL(oa_ranks, dim3(item_blocks), dim3(OA_BLOCK), 0, st, (const uint64_t *)d_keys, n_items, n_genes, item_bits, W[K24_START].as<const uint32_t>(),
                           W[K24_RANKF].as<uint32_t>());
        hipLaunchKernelGGL(oa_assign, dim3(row_blocks), dim3(OA_BLOCK), 0, st, (const uint32_t *)d_first, W[K24_RANKF].as<const uint32_t>(), (const uint8_t *)d_tflag, n_seeds,
                           n_rows, W[K24_OUT_FIRST].as<int32_t>(), W[K24_OUT_RANK].as<uint32_t>(), W[K24_OUT_T].as<uint8_t>());
    });
    PEP_HIP(ctx, hipGetLastError());
    // the results wait in memory of the library until the stream has been waited for and the comparison is known to have passed: on an error nothing is written
    std::vector<int32_t> h_first(n_rows);
    std::vector<uint32_t> h_rank(n_rows);
    std::vector<uint8_t> h_t(n_rows);
    uint32_t offender = OA_NONE;
    PEP_TRY(pep_d2h_queue(ctx, h_plan.data(), W[K24_PLAN].p, plan_bytes));
    PEP_TRY(pep_d2h_queue(ctx, h_first.data(), W[K24_OUT_FIRST].p, (size_t)n_rows * 4));
    PEP_TRY(pep_d2h_queue(ctx, h_rank.data(), W[K24_OUT_RANK].p, (size_t)n_rows * 4));
    PEP_TRY(pep_d2h_queue(ctx, h_t.data(), W[K24_OUT_T].p, n_rows));
    PEP_TRY(pep_d2h_queue(ctx, &offender, W[K24_BAD].p, 4));
    PEP_HIP(ctx, pep_stream_wait(ctx));
    pep_d2h_finish(ctx);
    if (offender != OA_NONE) {
        times = {};                      // (nothing was merged: the refused call reports no times)
        const auto name = [&](int64_t item) { return item < n_seeds ? std::string("the seed of its gene") : "row " + std::to_string(item - n_seeds); };
        const int32_t f = offender >= n_seeds ? h_first[offender - n_seeds] : -1;
        return pep_fail(ctx, PEP_ERR_ALLELE_CLASS, K24_ME + name(offender) + " and " + name(f < 0 ? -1 : (int64_t)f + n_seeds) +
                                                       " share a digest class and hold different bytes: nothing was merged");
    }
    memcpy(plan, h_plan.data(), plan_bytes);
    memcpy(first, h_first.data(), (size_t)n_rows * 4);
    memcpy(rank, h_rank.data(), (size_t)n_rows * 4);
    memcpy(tflag, h_t.data(), n_rows);
    return PEP_OK;
}

}  // extern "C"
