// Internal declarations shared by the HIP translation units of libpeppan_hip.so.
// gfx950 (MI355X, wave64) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <atomic>
#include <optional>
#include <string>
#include <type_traits>
#include <vector>
#include "../../include/peppan_hip.h"
using CallTimes = struct pep_call_times;     // (the tag alone names the function in C++)

#define PEP_WAVE 64
// copies of the 1 KiB substitution table in LDS (one per bank group): 32 = conflict-free gather, 16 = half the LDS for at most 2-way conflicts
#define PEP_TAB_REP 16

#define PEP_HIP(ctx, expr)                                                                            \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) {                                                                       \
            return pep_fail((ctx), PEP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
        }                                                                                             \
    } while (0)

#define PEP_TRY(expr)                  \
    do {                               \
        int _rc = (expr);              \
        if (_rc != PEP_OK) return _rc; \
    } while (0)

// ---- ownership.  Every device buffer, pinned buffer, event and stream of the library is held by one of the four types below and released by its destructor:
// a new one is a member (of pep_ctx, of a struct inside it) or a local and needs nothing else.  They are the only places that free a HIP resource, and the
// only ones that count what is alive (process-wide: pep_live_resources).  Move-only: a declared move constructor deletes both copies.
struct PepLive { std::atomic<uint64_t> device_bytes{0}, pinned_bytes{0}; std::atomic<uint32_t> events{0}; };
inline PepLive pep_live;

// grow-only device buffer (dev_reserve)
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    ~DevBuf() { release(); }
    void release() { if (p) { (void)hipFree(p); pep_live.device_bytes -= cap; } p = nullptr; cap = 0; }
    hipError_t alloc(size_t bytes)          // exactly `bytes`, in place of what it held
    {
        release();
        const hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) { cap = bytes; pep_live.device_bytes += bytes; } else p = nullptr;
        return e;
    }
};

// packed sequence set on the device.  Residues of sequence i live at res[off[i] .. off[i]+len[i]);
// at least PEP_SEQ_GAP bytes of PEP_PAD_CODE separate consecutive sequences and PEP_END_PAD pad both ends,
// so a spaced seed can never straddle two sequences.
#define PEP_PAD_CODE 31
#define PEP_SEQ_GAP 16
#define PEP_END_PAD 64
struct SeqSet {
    uint32_t n = 0;
    uint64_t total = 0;          // bytes in res (with padding)
    uint64_t residues = 0;       // sum of len
    uint32_t max_len = 0;
    DevBuf res;                  // u8
    DevBuf off;                  // u32[n+1]  (off[n] = total, sentinel for binary search)
    DevBuf len;                  // u32[n]
    DevBuf blk2seq;              // uint2[total/32]: (sequence whose residues a 32-byte block holds, start of that sequence) - starts are 16-aligned, gaps >= 16, so never two; one look-up
                                 // turns a packed position into (sequence, position inside it)
    // host mirrors
    std::vector<uint32_t> h_off, h_len;
};

// nucleotide sequence set (ASCII upper-cased on upload is NOT required: kernels fold case)
struct NtSet {
    uint32_t n = 0;
    uint64_t total = 0;
    DevBuf nt;                   // u8 ASCII, concatenated
    DevBuf off;                  // u64[n+1]
    std::vector<uint64_t> h_off;
};

// pinned host memory of a context: small read-backs (counts) and the staging area of downloaded tables.  A device -> host copy into
// pageable memory costs ~27 us per round trip on this box, into pinned memory ~16 us (tools/micro/sync_cost.hip), and large copies
// run at DMA speed only into pinned memory.
struct PinBuf {
    uint8_t *p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(PinBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    ~PinBuf() { release(); }
    void release() { if (p) { (void)hipHostFree(p); pep_live.pinned_bytes -= cap; } p = nullptr; cap = 0; }
    hipError_t alloc(size_t bytes)
    {
        release();
        const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), bytes, hipHostMallocDefault);
        if (e == hipSuccess) { cap = bytes; pep_live.pinned_bytes += bytes; } else p = nullptr;
        return e;
    }
};

// an event, created when it is first needed
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    ~Event() { if (e) { (void)hipEventDestroy(e); --pep_live.events; } }
    // false: the runtime gave none (every caller has its own way on without one)
    bool ensure(unsigned flags = hipEventDefault) { if (!e && hipEventCreateWithFlags(&e, flags) == hipSuccess) ++pep_live.events; return e != nullptr; }
    operator hipEvent_t() const { return e; }
};

// the context's stream: declared in front of every buffer and event, so the last of them to go
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

static_assert(!std::is_copy_constructible<DevBuf>::value && std::is_nothrow_move_constructible<DevBuf>::value && sizeof(DevBuf) == 16, "DevBuf: move-only, two words");
static_assert(!std::is_copy_constructible<PinBuf>::value && std::is_nothrow_move_constructible<PinBuf>::value, "PinBuf: move-only");
static_assert(!std::is_copy_constructible<Event>::value && std::is_nothrow_move_constructible<Event>::value, "Event: move-only");

struct pep_result;

enum PepSide { PEP_SIDE_Q = 0, PEP_SIDE_T = 1 };         // the state of the context's two packed sequence sets, one record per side (the transitions: setstate.h)
enum class SetSource { None, Nt, Residues };            // what the side was given: nothing yet, nucleotides (K1 packs them), residues (packed by the upload)
enum class Packed { No, Queued, Yes };                  // No: given or invalidated; Queued: K1 is on the stream, its summary not taken; Yes: the summary is in the SeqSet
enum class SetsHold { Inputs, BaseCodes, TakenOver };   // ctx->q / ctx->t hold: the inputs as K1 or an upload packed them; the nucleotide tool's base codes; what K9's gapped stage put there
struct SideState {
    SetSource source = SetSource::None;
    int gtable = 11, frames = 6;            // (frames: reference side)
    Packed packed = Packed::No;
    bool tables_built = true;               // false: the host tables (meta records, h_off, h_len) are still to be made from K1's descriptors on the device (pep_k1_host_tables)
    bool from_nt() const { return source == SetSource::Nt; }
};

// K1's descriptor of a packed sequence (translate.hip): the nucleotide sequence it was translated from, the frame (1 - 3 forward, 4 - 6 reverse strand), the residue its
// chunk starts at inside that frame, its length in residues.  One per query (d_k1_desc_q) / target (d_k1_desc_t), on the device; the host's meta records are made from them.
struct PackDesc {
    uint32_t seq;
    uint32_t frame;
    uint32_t aa_off;
    uint32_t len;
};
// ... and of a packed nucleotide sequence (pep_use_nt_as_residues: NuclSide::d_desc): the sequence and whether it is its reverse complement
struct NuclDesc { uint32_t seq, rev; };

// The slots of pep_ctx::ws that the search pipeline addresses (seed stage -> score pass -> selection -> traceback pass -> emit), and the ones other
// files enter it through.  Per line: what the slot holds, its element type, who writes it, who reads it last.  An alias is a take-over inside one
// search, with the reason the earlier tenant is dead by then.  The stand-alone calls name their slots in their own files and stay below PEP_WS_HITS_OUT.
enum PepWsSlot {
    PEP_WS_BUCKET_CNT = 0,                  // entries per index bucket of the count -> scan -> fill build, u32: seed_count / seed_fill (seeds.hip), read last by seed_fill
    PEP_WS_UF_PARENT = PEP_WS_BUCKET_CNT,   // K10's parent of every node, u32: finalize / uf_init, read last by pack_out / uf_flatten - the bucket counts are dead when the seed stage ends, the parents are written behind walk
    PEP_WS_IDX_START = 1,                   // first entry of every bucket, per seed shape, u32: idx_finish / the scan, read last by the matchers (seed_match, seed_match_stride)
    PEP_WS_IDX_ENTRIES = 2,                 // the query index's entries, per seed shape, u64: idx_finish / seed_fill, read last by the matchers
    // 3: free in the pipeline
    PEP_WS_CANDS = 4,                       // the sorted candidate keys, u64: set_compact and the sort - or the caller's upload (linclust.hip) -, read last by select_gather (as d_cands of pep_extend)
    PEP_WS_CANDS_TMP = 5,                   // the sort's second buffer, u64: sort.hip, read last by its final pass
    // 6: free in the pipeline
    PEP_WS_SEED_SCAN_TMP = 7,               // scratch of the bucket scan (count -> scan -> fill build): pep_scan_u32
    PEP_WS_SEED_HITS = 8,                   // raw seed hits, u64: the matchers, read last by seed_runs_extend
    PEP_WS_TRACE_KNOWN = PEP_WS_SEED_HITS,  // known score + end lane of every selected pair, i32 x 2: select_gather, read last by the traceback sweeps - the raw seed hits are dead once seed_runs_extend has made candidates of them, in the seed stage
    PEP_WS_SEED_FILTER = 9,                 // occupancy bits in front of the index, per seed shape, u64: idx_finish / filter_fill, read last by the matchers
    PEP_WS_DPP_SELFTEST = PEP_WS_SEED_FILTER,   // the two shifted lane rows of pep_selftest_dpp, i32: a call of its own at start-up, waited for before it returns
    PEP_WS_SW_NBLK = 10,                    // 16-step blocks per candidate of the newest pass, u32: sw_prep, read last by emit (trace.hip)
    PEP_WS_SW_DIR_OFF = 11,                 // first traceback block per candidate, u64[n + 1]: sw_prep, read last by walk (trace.hip)
    PEP_WS_SW_OUT = 12,                     // score / end cell / a0 per candidate, int4: identical_check, the sweeps and gapless_check, read last by walk
    PEP_WS_IDX_PART = 13,                   // the partition build's slabs per coarse bucket, u64: idx_slab, read last by idx_finish
    PEP_WS_SW_SKIP_MODE = PEP_WS_IDX_PART,  // score pass: which candidates identical_check settled, i32, read last by sw_order - the slabs are dead once idx_finish has run, in the seed stage
    PEP_WS_TRACE_DIRS = PEP_WS_IDX_PART,    // traceback codes, 512 B per 16-step block, u32: sw_trace_kernel, read last by walk - the skip modes are dead once the score pass is over (the traceback pass reads d_trace_mode)
    PEP_WS_SW_SCAN_IN = 14,                 // blocks per candidate as the look-back scan's input, u64: sw_prep
    PEP_WS_SW_ORDER = 15,                   // the candidates by decreasing length, u32: sw_order, read last by the sweeps
    // 16 - 18: free
    PEP_WS_SEL = 19,                        // the record of every selected pair, SelInfo: select_gather .. finalize, read last by topk_emit (the exactly sized path: emit)
    PEP_WS_SEL_RUNS_KEYS = 20,              // run slot of every selected pair u64[n + 2], then their keys u64[n + 2]: select_gather, read last by topk_emit / emit
    PEP_WS_RUNS = 21,                       // the CIGAR run arena of the selected pairs, u32: walk, read last by topk_emit / emit
    PEP_WS_KEEP = 22,                       // keep flag u32, hit position u32, CIGAR position u64 per selected pair: topk, read last by emit - the exactly sized path only (topk_emit hands nothing over)
    PEP_WS_HITS_OUT = 23,                   // the search's hit table, pep_hit[n_hits] + CIGAR runs u32: topk_emit / emit.  The one slot that outlives a call: intact while ctx->dev_result is set
                                            // (pep_fetch_result and pep_k10_components_dev read it later), so whoever writes it calls pep_drop_dev_result first and every other user of ws stays below it
    PEP_WS_COUNT
};

// The state areas of the kernels that look back (lookback.h): who begins a launch on the slot (pep_lookback_begin), the kernels that read it, the
// value bits of its status words.  A slot serves one launch at a time; two users may share one only if their words have the same layout
// and they begin one after the other on the context's stream.
enum PepLookback {
    PEP_LB_SCAN_U32 = 0,                    // scan_onepass<uint32_t> (pep_scan_u32): scan_lookback<uint32_t>; K1's layout_and_pack and reference side (translate.hip): k1_offsets,
                                            // k1_ref_desc, k1_ref_layout (four status arrays, one per total).  32 value bits.  Co-tenants: all write 32-bit words and are begun one
                                            // after another on the context's stream
    PEP_LB_SCAN_U64,                        // scan_onepass<uint64_t> (pep_scan_u64): scan_lookback<uint64_t>; the traceback pass of pep_sw_run (sw.hip): sw_prep.  48 value bits.
                                            // Co-tenants for the same reason
    PEP_LB_SELECT_COUNT,                    // the alignment stage (trace.hip): select_gather, selected pairs in front of a tile.  32 value bits.  Its ticket numbers the tiles of both select slots
    PEP_LB_SELECT_RUNS,                     // ... begun with it: select_gather, run capacity in front of a tile.  48 value bits
    PEP_LB_TOPK_HITS,                       // the alignment stage: topk, kept hits in front of a tile.  32 value bits.  Its ticket numbers the tiles of both top-k slots
    PEP_LB_TOPK_RUNS,                       // ... begun with it: topk, CIGAR runs of the kept in front of a tile.  48 value bits
    PEP_LB_SORT,                            // sort_passes (once per pass) and pep_sort_u64_two_level (sort.hip): sort_onesweep, one word per (tile, digit).  32 value bits
    PEP_LB_COUNT
};

// dirty: a failure may have left host and device ticket counts apart - the next launch on the slot starts from a cleared area (pep_fail)
struct LookbackState { DevBuf buf; uint32_t epoch = 0, ticket_base = 0; bool dirty = false; };

enum PepTimer { TM_SEED = 0, TM_TOTAL, TM_SW, TM_SW_TRACE, TM_TRACE, TM_MATCH0, TM_MATCH1, TM_MATCH2, TM_MATCH3, TM_COUNT };

struct pep_ctx {
    int device = 0;
    Stream stream;                          // declared before every buffer and event: destroyed after them
    PinBuf pin_small;                       // 16 KiB: counters read back between kernels
    size_t pin_small_used = 0;
    struct PendingRead { void *dst; size_t off, n; } pending[32];
    int n_pending = 0;
    PinBuf pin_k1, pin_k1q;                 // grow-only: what K1's kernels write for the host - the set's summary (reference), summary + lengths (queries)
    DevBuf d_k1_desc_q, d_k1_desc_t;        // K1's descriptors (+ the summary's accumulators behind them): fetched only when the host tables are asked for
    DevBuf d_self_delta, d_self_t;          // seed stage, self-search: per 32-byte block of the target layout the distance to the query that IS that target (pep_self_map, self_prepare);
                                            // per reference sequence the packed sequence its frame 1 starts with (K1: k1_ref_desc)
    const uint32_t *self_first = nullptr;   // what pep_self_map found applicable to the current sets: d_self_t (K1's) or the nucleotide tool's nucl_t.d_first; its entries; may a target be longer than its query
    uint32_t self_first_cnt = 0;
    int self_exact_len = 0;
    Event k1_event;                         // the point of the stream where the reference side's downloads have arrived
    Event k1q_event;                        // ... and the query side's
    Event wait_event;                       // pep_stream_wait: marks the point of the stream the host is waiting for
    Event k1_t0, k1_t1;                     // pep_translate's timing pair (created once)
    PinBuf pin_up;                          // grow-only: staging area of uploads out of pageable memory (pep_h2d)
    size_t pin_up_used = 0;
    Event up_event;                         // the point of the stream where the last upload out of pin_up has left it
    bool up_event_set = false;
    PinBuf pin_down;                        // grow-only: staging area of downloads into pageable memory (pep_d2h_queue / pep_d2h_finish)
    size_t pin_down_used = 0;
    struct PendingDown { void *dst; size_t off, n; } down[16];
    int n_down = 0;
    PinBuf pin_stage;                       // grow-only: the hit table of the newest search
    PinBuf pin_ms;                          // grow-only: per-query score thresholds on their way to the device
    pep_result *staged_result = nullptr;    // the result whose hits still live in pin_stage (materialised before it is overwritten)
    std::string err;
    pep_search_params params;
    // inputs
    NtSet q_nt, r_nt;
    SeqSet q, t;
    std::vector<pep_query_meta> q_meta;     // frame chosen per query (K1)
    std::vector<pep_target_meta> t_meta;    // (seq, frame, chunk offset, length) per target (K1)
    // what q / t hold: assigned by the transitions of setstate.h alone, which also drop what was derived from the sets - nucl_valid .. self_first_n below
    SideState side[2];                      // [PEP_SIDE_Q], [PEP_SIDE_T]
    SetsHold holds = SetsHold::Inputs;
    bool nucl_valid = false, t_class_ready = false;
    int k1_base_frames = 0;                 // 0 = K1's length-derived reference tables (below) are not computed for the current reference set
    uint32_t self_first_n = 0;              // entries of d_self_t (reference sequences of the last K1 of the reference side)
    bool sub_ready = false, codon_ready = false;
    // K1 reference side: chunk-slot prefix per (sequence, frame), a function of the input lengths only - kept between translations
    DevBuf d_k1_base;
    std::vector<uint64_t> k1_base;
    uint64_t k1_upper = 0;
    // ... and the tables of its LONG frames (contigs of genomes: k1_stop_mask / k1_ref_chunks_mask / k1_ref_desc_fill): tiles of the stop mask, the long frames'
    // records (+ frame -> record), the stop mask itself, tiles of chunk slots
    DevBuf d_k1_seg, d_k1_long, d_k1_spec, d_k1_tiles;
    uint32_t k1_n_seg = 0, k1_n_long = 0, k1_n_tiles = 0;
    // ... and of a set without long frames (genes: k1_ref_layout / k1_pack_ref): its frames of more than 1000 characters, whose stops k1_ref_chunks looks for, and the
    // chunk slots of its sequences too long for one wavefront's staging area
    DevBuf d_k1_cut, d_k1_big;
    uint32_t k1_n_cut = 0, k1_n_big = 0;
    // what pep_use_nt_as_residues makes of the nucleotide sets apart from the residues themselves (translate.hip: pep_nucl_sets), kept per pair of uploads
    struct NuclSide {
        uint32_t n = 0, max_len = 0;
        uint64_t total = 0, residues = 0;
        std::vector<uint32_t> h_off, h_len;
        std::vector<pep_query_meta> q_meta;
        std::vector<pep_target_meta> t_meta;
        DevBuf d_off, d_len, d_desc;
        DevBuf d_first;                     // targets: per reference sequence the packed sequence that is its forward strand (seeds.hip: self_prepare)
        uint32_t n_first = 0;
    } nucl_q, nucl_t;
    int nucl_strands = 0;
    DevBuf d_min_score;
    DevBuf d_trace_defer;                   // traceback pass: pairs that left their sub-band, waiting for their full-band sweep (sw.hip: run_deferred)
    DevBuf d_trace_mode;                    // per traced pair: first lane of the sub-band its traceback codes cover, -1 = the full band (sw.hip)
    std::vector<uint32_t> group_of_seq;     // optional: competition group of every reference sequence (pep_set_target_groups)
    DevBuf d_t_class;
    DevBuf d_t_subject;                         // hsp_mode 2: the reference sequence every target is a strand / frame / chunk of (uploaded per search)
    // workspaces (grow-only, reused between searches and between calls: PepWsSlot above)
    DevBuf ws[PEP_WS_COUNT];
    DevBuf sub_lds;                         // replicated substitution table image (32 KiB)
    DevBuf d_params;                        // device copy of seed params
    int8_t d_params_host[1024] = {};        // what d_params holds (uploaded again only when the substitution table changes)
    bool d_params_valid = false;
    // phase timers: events recorded on the stream, read once after the search's final synchronisation (waiting for an end event in
    // the middle of a search costs a host round trip with the GPU idle, and lets nothing be queued behind a running SW pass)
    Event tm_a[TM_COUNT], tm_b[TM_COUNT];
    int tm_state[TM_COUNT] = {};                // 0 idle, 1 begun, 2 ended (waiting to be read)
    int timing_level = 0;                    // pep_set_timing: 0 no phase timers, 1 the score pass only, 2 all of them
    PinBuf pin_labels;                       // grow-only: K10's labels on their way to the caller
    uint64_t trace_swept = 0;               // pairs the last traceback pass swept (the rest were settled by the gapless shortcut)
    LookbackState lookback[PEP_LB_COUNT];   // the state of every kernel that looks back (lookback.h; the slots: PepLookback above)
    DevBuf sort_hist;                       // the radix sort's own digit histograms, for callers that bring none (sort.hip)
    DevBuf d_set;                           // candidate hash set of the seed stage (seeds.hip); set_compact leaves every slot it read EMPTY again
    uint64_t set_clean_slots = 0;           // leading slots of d_set known to be EMPTY (0 while a search is using it)
    DevBuf uf_nodes;                        // K10 over a device-resident hit table: node of every target (uploaded when it changes)
    std::vector<uint32_t> uf_nodes_host;
    struct { bool pending = false; pep_result *res = nullptr; const void *d_hits = nullptr, *d_cig = nullptr; const uint32_t *d_n_hits = nullptr; uint64_t n_bound = 0; bool grouped = false; } ext;
                                            // a search whose result left through pack_out and whose host half (sizes, statistics, views) is still to be done (pep_extend_finish)
    struct { void *d_dst = nullptr; const void *pinned_src = nullptr; uint64_t n_words = 0; } upload;   // an upload out of pinned memory that rides on the next read-back kernel
    bool want_nt_match = false;              // pep_set_nt_match: the searches of this context end with K7's count of identical nucleotide columns per hit (rescore.hip: pep_k7_hits_queue)
    DevBuf d_nt_match;
    PinBuf pin_nt_match;                     // grow-only: those counts on their way to the result
    uint32_t grp_nodes = 0, grp_q_base = 0;  // pep_set_grouping: the searches of this context end with K10 over their own hit table (0 = off)
    bool device_results = false;            // pep_set_result_mode: searches leave their table on the device; the host copy is fetched on demand
    pep_result *dev_result = nullptr;       // the result whose hit table is still intact on the device (PEP_WS_HITS_OUT): the newest search's, until the workspace is reused
    DevBuf d_zero;                          // the small counters of one search, cleared by ONE fill when it starts (layout: PEP_ZERO_* below)
    bool zero_clean = false;                // the seed stage's part of d_zero is zero as of the end of what is queued (pack_out cleared all of d_zero): with every
                                            // zero_ok flag still set the next search needs no fill
    DevBuf d_mail_copy;                     // the alignment stage's counter block outside d_zero (trace.hip: emit -> pack_out, K10)
    bool zero_ok[4] = {false, false, false, false};     // which consumer regions of d_zero are still untouched since that fill (PEP_ZC_*)
    CallTimes calls[PEP_CALL_COUNT] = {};   // pep_call_times: the times and byte counts of the newest call of each of K15 - K26 (the slots: each kernel's section of peppan_hip.h)
    uint64_t k16_serial = 0;                 // counts pep_group_verdicts calls: a pep_verdict_result is live while its serial is the newest
    DevBuf k16_tri, k16_leader;              // grow-only: packed triangles and leaders of the newest pep_group_verdicts (read by pep_verdict_detail_copy)
    DevBuf k17[11];                          // grow-only, pep_gene_ingroups: its tables, work list and outputs (the slots: ingroup.hip)
    uint64_t k18_n_conf = 0, k18_n_walk = 0; // the pairs the two lists of the newest pep_synteny_pairs hold, waiting on the device for pep_synteny_pairs_copy
    DevBuf k18[18];                          // grow-only: its tables, counters and the two lists (the slots: synteny.hip)
    DevBuf k19[5];                           // grow-only, pep_gene_structure: the nucleotide set, the item records and the outputs (the slots: genestruct.hip)
    DevBuf k20[6];                           // grow-only, pep_rarefaction_curves and pep_profile_pairs: bit rows, orders and curves; profiles and the two pair matrices (the slots: parser.hip)
    DevBuf k21[5];                           // grow-only, pep_nj_trees: the matrices, the tree records, the two outputs and the state of a launch chain (the slots: njtree.hip)
    uint64_t k22_n_keys = 0;                 // the keys the newest pep_global_diff left on the device, waiting for pep_global_diff_copy
    DevBuf k22[13];                          // grow-only, pep_global_diff: events, arena, the per-key tables, a chunk's sort buffers, the value lists and the sums (the slots: globaldiff.hip)
    DevBuf k23[4];                           // grow-only, pep_cds_genes: the contig arena, the item records, the codes and the digests (the slots: cdsgenes.hip)
    DevBuf k25[15];                          // grow-only, pep_tree_cut: the matrices, the bit sets, the tree records, the scores, the outputs and the state of a launch chain (the slots: treecut.hip)
    // stats of the last search
    pep_stats stats;
    ~pep_ctx();                 // what only the context can do before its members release themselves: its device current, the results that point into it cut loose
};

inline SeqSet &pep_set_of(pep_ctx *ctx, PepSide s) { return s == PEP_SIDE_Q ? ctx->q : ctx->t; }
struct pep_result {
    pep_ctx *ctx = nullptr;
    std::vector<pep_hit> hits;              // used once the result no longer lives in the context's staging area
    std::vector<uint32_t> cigar;
    const pep_hit *st_hits = nullptr;       // while staged: views into ctx->pin_stage
    const uint32_t *st_cigar = nullptr;
    uint64_t n_hits = 0, n_cigar = 0;
    const pep_hit *d_hits = nullptr;        // device copy (context workspace), valid while ctx->dev_result == this
    const uint32_t *d_cigar = nullptr;
    pep_stats stats;
    std::vector<uint32_t> labels;           // pep_set_grouping: the partition of the search's hit graph (one label per node)
    std::vector<uint32_t> nt_match;         // pep_set_nt_match: identical nucleotide columns per hit (K7's n_match)
};

// HIP-event stopwatch on one stream (the kernel times bench.py reports are taken with it, inside the library,
// on the stream the kernels are launched on); its events go with it on every exit path
hipError_t pep_event_wait(hipEvent_t ev);      // polls before it sleeps (capi.hip)
unsigned pep_wait_event_flags();               // flags of an event that is only ever waited for (blocking when PEPPAN_HIP_SPIN_US=0)

struct EventTimer {
    Event a, b;
    hipStream_t st;
    explicit EventTimer(hipStream_t s) : st(s)
    {
        b.ensure();
        if (a.ensure()) (void)hipEventRecord(a, st);
    }
    float stop()                      // records the end event, waits for it, returns milliseconds (0 on failure)
    {
        float ms = 0.f;
        if (a && b && hipEventRecord(b, st) == hipSuccess && pep_event_wait(b) == hipSuccess) (void)hipEventElapsedTime(&ms, a, b);
        return ms;
    }
};

void pep_timer_begin(pep_ctx *ctx, int id);
void pep_timer_end(pep_ctx *ctx, int id);
void pep_timers_resolve(pep_ctx *ctx);     // after a stream synchronisation: elapsed times -> ctx->stats.ms_*

int pep_fail(pep_ctx *ctx, int code, const std::string &msg);
// small device -> host reads: queue any number with pep_read_back (async copy into the pinned page), then ONE pep_sync_reads
// waits for the stream and stores the values
int pep_read_back(pep_ctx *ctx, void *dst, const void *d_src, size_t n);
int pep_sync_reads(pep_ctx *ctx);
// Waits until everything queued on the context's stream so far has finished - by polling an event for up to a few hundred microseconds
// before falling back to a blocking wait: the searches are chains of short kernels with a handful of host decisions in between, and a
// sleeping host thread adds tens of microseconds of wake-up latency to each of them.
hipError_t pep_stream_wait(pep_ctx *ctx);
int pin_reserve(pep_ctx *ctx, PinBuf &b, size_t bytes);
// stream-ordered upload of caller memory: through the context's pinned staging area for anything of size (a copy command straight out of pageable
// memory has the runtime pin the pages first - 15 ms for the 10 MB of a gene set it has not seen before, 0.2 ms the second time); the caller's buffer
// is free on return
int pep_h2d(pep_ctx *ctx, void *d_dst, const void *h_src, size_t n);
// the way back: pep_d2h_queue queues a download into the pinned staging area (small ones go straight to their destination), pep_d2h_finish - called once
// the stream has been waited for - copies what arrived to where the caller wants it.  A copy command straight into pageable memory makes the driver
// register those pages; when the caller frees them (numpy arrays of a megabyte or more go back to the system at once) the driver evicts the process's
// queues to drop the registration - the NEXT call on the GPU then takes 10 - 30 ms (found in round 5 behind the last gather of RunBlast.run)
int pep_d2h_queue(pep_ctx *ctx, void *h_dst, const void *d_src, size_t n);
void pep_d2h_finish(pep_ctx *ctx);
void pep_materialise_staged(pep_ctx *ctx);
void pep_drop_dev_result(pep_ctx *ctx);
int dev_reserve(pep_ctx *ctx, DevBuf &b, size_t bytes);
inline void dev_release(DevBuf &b) { b.release(); }      // the explicit early release

// a table of a call for slot `slot` of a DevBuf array: bytes + pad are reserved and `bytes` uploaded from src; src == nullptr: reserved only (an output or scratch buffer)
struct WsTable { int slot; const void *src; size_t bytes, pad; };
// every reserve before the first upload, so that no buffer grows with a copy queued in front of it; the uploads go on the stream in the list's order
inline int pep_tables_to_device(pep_ctx *ctx, DevBuf *W, const std::vector<WsTable> &tables)
{
    for (const WsTable &t : tables) PEP_TRY(dev_reserve(ctx, W[t.slot], t.bytes + t.pad));
    for (const WsTable &t : tables)
        if (t.src) PEP_TRY(pep_h2d(ctx, W[t.slot].p, t.src, t.bytes));
    return PEP_OK;
}

// one kernel stage on the context's stream, its HIP-event time left in `ms` when pep_set_timing is 2
template <class Launch>
void pep_timed_stage(pep_ctx *ctx, double &ms, const Launch &launch)
{
    std::optional<EventTimer> tm;
    if (ctx->timing_level >= 2) tm.emplace(ctx->stream);
    launch();
    if (tm) ms = tm->stop();
}

// the text of a device-free table check (pep_*_check) into the caller's char[msg_cap], cut to fit; passes `rc` on
int pep_message_out(int rc, const std::string &text, char *msg, uint64_t msg_cap);

// Layout of pep_ctx::d_zero: every small counter block a search needs starts from zero, and one fill at the start of the search clears
// them all (each used to be a fill of its own in front of its kernel: eleven tiny launches per search).  A stage that runs without the
// seed stage in front (K9 drives the alignment stage alone) finds its flag in zero_ok unset and clears its own block.
#define PEP_ZERO_SEED 0                                         // 64 B: list length, overflow flags, statistics (seeds.hip)
#define PEP_SORT_TOP_BITS 10                                    // two-level candidate sort (sort.hip): buckets by the top 10 bits of the key ...
#define PEP_SORT_TOP_CAP 4096                                   // ... each sorted in LDS when none holds more keys than this
#define PEP_ZERO_TOP (PEP_ZERO_SEED + 64)                       // 1024 x 4 B: candidates per top digit of the dense key (set_compact; read back WITH the 64 bytes in front)
#define PEP_ZERO_SHAPE (PEP_ZERO_TOP + 4096)                    // 4 x 16 B: raw-hit and run counters per seed shape
#define PEP_ZERO_COARSE (PEP_ZERO_SHAPE + 64)                   // 4 x 8192 x 4 B: coarse-bucket counts of the query index per seed shape
#define PEP_ZERO_SORT (PEP_ZERO_COARSE + 4 * 8192 * 4)          // 8 x 2048 x 4 B: digit histograms of the candidate sort
#define PEP_ZERO_SW_BYTES (64 + 2 * 1024 * 4)                   // totals + length histogram + scatter cursors of one Smith-Waterman pass (sw.hip)
#define PEP_ZERO_SW_SCORE (PEP_ZERO_SORT + 8 * 2048 * 4)
#define PEP_ZERO_SW_TRACE (PEP_ZERO_SW_SCORE + PEP_ZERO_SW_BYTES)
#define PEP_ZERO_SELECT (PEP_ZERO_SW_TRACE + PEP_ZERO_SW_BYTES)  // 256 B: counters of the selection stage (trace.hip)
#define PEP_ZERO_TILES (PEP_ZERO_SELECT + 256)                  // 4 x 8 x 128 B: the matchers' tile claims per seed shape: eight counters, a cache line each (seeds.hip: TileClaims)
#define PEP_ZERO_TOTAL (PEP_ZERO_TILES + 4 * 8 * 128)
enum { PEP_ZC_SW_SCORE = 0, PEP_ZC_SW_TRACE, PEP_ZC_SELECT, PEP_ZC_SORT };
// the block of consumer `which` (PEP_ZC_*), zeroed: taken from the search's one fill when it is still untouched, cleared here otherwise
int pep_zero_block(pep_ctx *ctx, int which, size_t offset, size_t bytes, void **out);

// ---- scan.hip
// exclusive; d_out[n] = total (n+1 outputs); d_total (optional): a second place the total is written to (a counter block the host reads in one copy)
int pep_scan_u32(pep_ctx *ctx, const uint32_t *d_in, uint32_t *d_out, uint64_t n, DevBuf &tmp, uint32_t *d_total = nullptr);
int pep_scan_u64(pep_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, uint64_t n, DevBuf &tmp, uint64_t *d_total = nullptr);
int pep_copy_from_pinned(pep_ctx *ctx, void *d_dst, const void *pinned_src, uint64_t n_words);     // a kernel instead of a copy command (scan.hip)
int pep_exchange_pinned(pep_ctx *ctx, void *d_up_dst, const void *pinned_up_src, uint64_t n_up_words, void *pinned_down_dst, const void *d_down_src, uint64_t n_down_words);
// pep_read_back through a kernel that also carries an upload out of pinned memory (one launch for both directions; n a multiple of 4)
int pep_read_back_with_upload(pep_ctx *ctx, void *dst, const void *d_src, size_t n, void *d_up_dst, const void *pinned_up_src, uint64_t n_up_words);
// ---- sort.hip
// the dense candidate-key form q | t | bin - bin_min (tb / bb bits for t / bin) <-> q:21 | t:25 | bin:18 (seeds.hip); on = 0: keys pass unchanged
struct pep_key_unpack { int on, tb, bb; uint32_t bin_min; };
int pep_sort_u64(pep_ctx *ctx, uint64_t *d_keys, uint64_t *d_tmp, const uint32_t *d_n, uint64_t n_bound, int bits, uint32_t *d_hist_zeroed,
                 const pep_key_unpack *unpack);   // result in d_keys
int pep_sort_u64_two_level(pep_ctx *ctx, uint64_t *d_keys, uint64_t *d_tmp, uint64_t n, int bits, const uint32_t *d_top_hist, const pep_key_unpack *unpack);
// ---- translate.hip  (K1)
int pep_k1_query_queue(pep_ctx *ctx, int gtable), pep_k1_query_take(pep_ctx *ctx);     // queue: a side's device work and the download of its summary; take: wait for that download, fill in the SeqSet
int pep_k1_ref_queue(pep_ctx *ctx, int frames, int gtable), pep_k1_ref_take(pep_ctx *ctx);
int pep_k1_host_tables(pep_ctx *ctx, PepSide side);    // the per-sequence host tables of one side, if its last K1 left them to be built on demand
int pep_nucl_sets(pep_ctx *ctx, int strands);      // the nucleotide sets themselves as residue sets (base codes; reference: forward strands + reverse complements)
// ---- seeds.hip  (K2-K4)
// before_sync (optional): host work to do once every kernel of the stage is queued, while the GPU runs them (the stage ends with a synchronisation)
int pep_find_candidates(pep_ctx *ctx, uint64_t **d_cands, uint64_t *n_cands, int (*before_sync)(pep_ctx *) = nullptr, int (*need_targets)(pep_ctx *) = nullptr);
int pep_upload_sub_table(pep_ctx *ctx);       // ctx->params.sub -> ctx->d_params (1 KiB, uploaded when it changed)
// ---- sw.hip / trace.hip (K5, K6, K8)
int pep_sw_run(pep_ctx *ctx, const uint64_t *d_cands, uint64_t n, bool trace, const int32_t *d_known = nullptr, const int32_t *d_end_lane = nullptr, const int32_t *d_skip_mode = nullptr,
               const uint32_t *d_n = nullptr, uint64_t dir_blocks_bound = 0, unsigned long long **d_hdr = nullptr);   // kernel time: phase timers TM_SW / TM_SW_TRACE
// h_min_score: score threshold per query; nullptr = ctx->d_min_score holds them already (pep_search uploads them while the seed stage runs)
// defer: the caller waits for the stream itself and calls pep_extend_finish afterwards (pep_search: one wait for everything)
// group: the caller ends with K10 over this table (pep_set_grouping): where the result leaves through topk_emit / pack_out those two do the unions and the
// labels on their way (ctx->ext.grouped says so; pep_k10_queue then queues nothing)
int pep_extend(pep_ctx *ctx, const uint64_t *d_cands, uint64_t n_cands, const int32_t *h_min_score, pep_result *res, bool defer = false, bool group = false);
int pep_extend_finish(pep_ctx *ctx);
int pep_selftest_dpp(pep_ctx *ctx);
// ---- what another translation unit calls of a kernel's file (an exported function is defined in the file of its kernel and declared in the public header alone)
int pep_k7_hits_queue(pep_ctx *ctx, uint64_t n_hits, const pep_hit *d_hits, const uint32_t *d_cigar, const uint32_t *d_n_hits = nullptr);   // K7's match counts of a search's own hits -> ctx->pin_nt_match (no wait; rescore.hip)
int pep_k10_queue(pep_ctx *ctx, uint64_t n_hits, const pep_hit *d_hits, const uint32_t *d_n_hits = nullptr);   // d_n_hits: the count lives on the device, n_hits bounds it       // K10 behind a search, labels -> ctx->pin_labels (no wait; unionfind.hip)
int pep_k10_components_dev(pep_ctx *ctx, uint32_t n_nodes, uint64_t n_hits, const pep_hit *d_hits, uint32_t q_base, const uint32_t *h_node_of_target,
                           uint64_t n_targets, uint32_t *h_label);      // pep_components_of_result over a hit table that is still on the device (unionfind.hip)

static inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// In-matrix cells of a band: the diagonals dlo .. dlo + 127 (d = j - i) of an Lq x Lt matrix, clipped to dl = max(dlo, -(Lq - 1)) .. dh = min(dlo + 127, Lt - 1).
// Diagonal d holds min(Lq, Lt - d) + min(0, d) cells; their sum in closed form (a loop over the 128 diagonals of every candidate was most of sw_prep's
// time, and a wavefront per hit in the emit stage).  0 for a band that misses the matrix.
__device__ __forceinline__ unsigned long long pep_band_cells(int Lq, int Lt, int dlo)
{
    const int dl = max(dlo, -(Lq - 1)), dh = min(dlo + 127, Lt - 1);
    if (dl > dh) return 0ull;
    auto tri = [](long long a, long long b) { return b < a ? 0ll : (a + b) * (b - a + 1) / 2; };      // a + (a + 1) + ... + b
    const long long k = (long long)Lt - Lq;                       // min(Lq, Lt - d) = Lq for d <= k, Lt - d beyond
    const long long flat_hi = min((long long)dh, k), slope_lo = max((long long)dl, k + 1);
    long long total = (flat_hi >= dl ? (flat_hi - dl + 1) * (long long)Lq : 0ll);
    if (slope_lo <= dh) total += (long long)(dh - slope_lo + 1) * Lt - tri(slope_lo, dh);
    total += tri(dl, min((long long)dh, -1ll));                     // + d for the negative diagonals
    return (unsigned long long)total;
}

// K10's lock-free union-find (unionfind.hip), for every kernel that unites or flattens: a union hooks the larger root under the smaller with an
// atomic compare-and-swap, so the final root of a component is its smallest node id whatever the execution order
__device__ __forceinline__ uint32_t uf_root(uint32_t *parent, uint32_t x)
{
    for (;;) {
        const uint32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ void uf_unite(uint32_t *parent, uint32_t x, uint32_t y)
{
    for (;;) {
        x = uf_root(parent, x);
        y = uf_root(parent, y);
        if (x == y) return;
        if (x < y) { const uint32_t t = x; x = y; y = t; }          // x = larger root, hooked under y
        if (atomicCAS(&parent[x], x, y) == x) return;
    }
}
int pep_upload_blk2seq(pep_ctx *ctx, SeqSet &s);
// translate.hip, for the seed stage of a self-search (seeds.hip: self_prepare): K1 leaves ctx->d_self_t[g] = the packed sequence that frame 1 of reference sequence g
// starts with (PEP_SELF_NONE: none); pep_self_map clears ctx->d_self_delta - one word per 32-byte block of the target layout, PEP_SELF_NO_DELTA - and says whether
// the current sets came out of K1 at all (*on = 0: not applicable, nothing queued).
#define PEP_SELF_NONE 0xFFFFFFFFu
#define PEP_SELF_NO_DELTA ((int32_t)0x80808080)
#define PEP_SELF_SAFE 1          // bit 0 of a distance word (the starts are 16-aligned, so a distance has four free low bits; PEP_SELF_NO_DELTA has it clear): see JoinArgs::self_delta
int pep_self_map(pep_ctx *ctx, int *on);
int pep_upload_codes(pep_ctx *ctx, PepSide side, const uint8_t *codes, const uint64_t *off, uint32_t n, uint32_t max_n);
int pep_upload_sub(pep_ctx *ctx);
