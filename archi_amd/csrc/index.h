// index.h -- the HBM-resident corpus index behind ak_index_* (gfx950 only).
//
// Data layout in HBM (one shard = one process = one GPU):
//   rows  [cap][dim]  storage dtype (f32 / bf16 / f16), row-major, 16-B aligned rows
//   na    [cap] f32   pgvector-order sequential sum a[i]*a[i] of the STORED values
//   ea,eb [cap] f32   per-row epilogue terms of the candidate scan:
//                       cosine: s~ = dot * 1/sqrt(na)          (ea = rsqrt, eb = 0)
//                       l2    : s~ = dot - na/2                (ea = 1, eb = -na/2)
//                       ip    : s~ = dot                       (ea = 1, eb = 0)
//                     dead or zero-norm(cosine) rows: ea = 0, eb = -inf (never a candidate)
//   ids   [cap] i64   document_chunks.id of each row slot
//   alive [cap] u8    0 after ak_index_remove (tombstone)
//   lex_off [cap] i64, lex_cnt [cap] i32, lex_len [cap] i32   the row's sorted (term id, tf) list in the entry arena and its length in
//                     tokens (lexical.hip: the BM25 leg of the hybrid query); a row without a list has cnt = len = 0
#pragma once
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <shared_mutex>
#include <unordered_map>
#include <vector>

#include "coalesce.h"      // request coalescing of ak_index_search: host-only, sanitizer-tested on its own
#include "common.h"
#include "index_book.h"    // id <-> slot map, tombstones, growth plan, layout epoch: host-only, sanitizer-tested on its own
#include "scan_plan.h"     // QPrep, FastPlan and the scan's plan and workspace layout: host-only, sanitizer-tested on its own

namespace ak {

struct Workspace {
    void *buf = nullptr;
    size_t bytes = 0;
    int reserve(size_t need);
    void release();
};

// The host mirror (cap, n, n_alive, epoch, next_id, h_ids, h_alive, id2slot) is the IndexBook base; read and written under `mu`.
struct Index : IndexBook {
    int dim = 0, dtype = 0, metric = 0;
    void *rows = nullptr;
    void *shadow = nullptr;   // f32 corpora only: bf16 copy of the rows that the MFMA candidate scan reads
    float *na = nullptr, *ea = nullptr, *eb = nullptr;
    float *gb = nullptr;      // [ceil(cap/32)][4]: per 32-row block {max ea | rows 8q+0..3, max ea | rows 8q+4..7, max eb .., max eb ..}
    int64_t *ids = nullptr;
    uint8_t *alive = nullptr;
    // ---- lexical store (lexical.hip), doc-major: per slot an offset into the append-only arena of (term id, tf) entries -- 8 bytes
    // each, ascending in term id within a row, every row starting on an even entry (16-byte loads) --, the entry count and the
    // document length. rebuild() carries the three per-slot arrays along and, on a gathering rebuild, copies the arena compacted.
    int64_t *lex_off = nullptr;
    int32_t *lex_cnt = nullptr, *lex_len = nullptr;
    uint2 *lex_arena = nullptr;
    int64_t lex_arena_cap = 0, lex_used = 0;     // entries allocated / entries up to the append position (alignment gaps included)
    int64_t lex_entries = 0, lex_rows = 0;       // entries of attached rows / live rows with a list
    uint64_t lex_gen = 0;                        // whose lists these are (ak_index_lex_clear / ak_index_lex_attach)
    std::vector<int32_t> h_lex_cnt;              // host mirror of lex_cnt (shorter than n: the missing slots hold 0)
    std::vector<uint8_t> h_lex_att;              // 1 = a list was attached to the slot (an empty text attaches an empty list)
    Workspace ws_lex;                            // workspace of the lexical / hybrid query (one at a time: lex_mu)
    Workspace ws_lexb;                           // the batch call's [queries][rows of U] arrays, sized after |U| is known (lex_mu)
    std::mutex lex_mu;
    char *lex_pin = nullptr; size_t lex_pin_cap = 0;       // pinned landing pad of the query's small copies
    hipEvent_t lex_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // ak_index_profile: stage boundaries of the hybrid query
    float max_na = 0.f;  // max over rows of na (for the ip / l2 error bound)
    float max_rho = 0.f; // f32 corpora: max over rows of |a - shadow(a)| / |a| (measured at ingest; certificate term rho_c)
    // ---- int8 shadow of a 16-bit corpus (the i8 scan plan, scan.hip): rows8 [cap in whole tiles][dim] int8, ea8 = scale * ea (the
    // scan-side term), gb8 the filter's per-32-row-block maxima of ea8 / eb. The rows of a filter class (the 16 rows of a 32-row
    // block with one value of row bit 2: gb8's sets) share ONE ea8 wherever they can adopt it, so that the scan's bound
    // max(dot) * gb8 is a site's exact maximum; a row that cannot (zeros, a non-finite value, removed before the build, beyond the
    // cap) keeps scale = max|a| / 127 (shadow8_scale.h has the rule). Built lazily by the first search whose plan asks for it
    // (ensure_shadow8), extended for appended rows -- a row a published shadow holds is never rewritten, so the block an append
    // lands in may be mixed --, dropped when rows moved (a reclaim of tombstones renumbers the slots) or the buffers grew.
    // Removed rows need nothing: the scan takes eb (-inf for a tombstone) from the index itself.
    int8_t *rows8 = nullptr;
    float *ea8 = nullptr, *gb8 = nullptr;
    int64_t s8_n = 0, s8_cap = 0;          // rows covered / rows allocated
    uint64_t s8_epoch = 0;                 // the layout it was built for: IndexBook::reclaims, the epoch changes that renumbered slots
    float max_rho8 = 0.f;                  // max over rows of |a - scale * a8| / |a| with the scale the scan applies (ea8 / ea), rounded up
    int64_t s8_builds = 0;                 // full builds so far (ak_index_i8_info)
    std::atomic<int64_t> s8_searches{0};   // searches that ran the i8 plan
    std::mutex s8_mu;
    Coalescer co;
    HybridCoalescer hco;  // concurrent ak_index_hybrid_search calls (lexical_batch.hip)
    std::shared_mutex mu;
    Workspace ws_dev;     // workspace of ak_index_search_dev (one call at a time: ws_mu + ws_event order its users)
    Workspace ws_fb;      // ak_index_search_dev, AUTO mode: workspace of the re-run of uncertified queries (rare, grow-only)
    std::mutex ws_mu;
    std::mutex prof_mu;   // profile / debug state below (fast_search is reached under the shared lock only)
    // ak_index_search_dev is asynchronous: its kernels may still be using ws_dev (and reading ea/eb/gb/rows) after the call
    // returned. ws_event is recorded behind the last enqueued kernel; the next device search on ANOTHER stream waits for
    // it on the device, writers (add / remove / compaction) wait for it on the host before they touch the index.
    hipEvent_t ws_event = nullptr;
    hipStream_t ws_stream = nullptr;
    bool ws_pending = false;
    // optional per-launch timing of the scan kernel (ak_index_profile): event pairs
    // recorded on the launch stream, read back after the caller synchronised.
    float *max_dev = nullptr;       // landing pad of finish_rows' maxima {norm^2, shadow error} (allocated once, not per add)
    long long *dbg_dev = nullptr;   // AK_SCAN_DBG: per-wave phase cycle counters of the last two scan launches
    bool profile = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
    size_t prof_used = 0;
};

// ---- exact path (exact.hip) -------------------------------------------------
// Reference arithmetic for every (query,row): keys -> hierarchical selection.
// queries_dev [nq][dim] f32, nb_dev [nq] f32 (pgvector-order sum q[i]^2),
// filter_dev NULL or [n] bytes. Outputs on device: [nq][k].
// `ws` holds exact_scratch_bytes(ix, k); nothing is allocated and nothing synchronises inside (asynchronous on st).
size_t exact_scratch_bytes(const Index &ix, int k);
int exact_search(Index &ix, const float *queries_dev, const float *nb_dev, int nq, int k,
                 const uint8_t *filter_dev, int64_t *out_ids_dev, double *out_dist_dev,
                 int *out_cnt_dev, void *ws, hipStream_t st);

// generic selection: smallest k (key,id) pairs per query, hierarchical.
//   keys [nq][n_in]; ids: explicit [nq][n_in] or NULL (then id = idmap ? idmap[i] : i)
//   result: okeys/oids [nq][k] sorted ascending; missing -> KEY_INVALID / -1
// scratch must hold select_scratch_bytes(nq, n_in, k).
size_t select_scratch_bytes(int nq, int64_t n_in, int k);
int select_topk(const uint64_t *keys, const int64_t *ids, const int64_t *idmap, int nq, int64_t n_in,
                int k, uint64_t *okeys, int64_t *oids, void *scratch, hipStream_t st);

int select_topk_strided(const uint64_t *keys, int nq, int64_t n_in, int64_t in_stride, int k, uint64_t *okeys,
                        int64_t *oids, void *scratch, hipStream_t st);

// key-only selection by bitonic sort (select.hip): keys [nq][in_stride] -> okeys [nq][k] ascending
size_t select_keys_scratch_bytes(int nq, int64_t n_in, int k);
int select_keys_topk(const uint64_t *keys, int nq, int64_t n_in, int64_t in_stride, int k, uint64_t *okeys,
                     void *scratch, hipStream_t st);

// exact re-rank of candidates: cand [nq][kp] approx keys (row slot in the low
// 32 bits) -> exact distance keys + global ids, same layout.
// Two kernels: the panel kernel (coalesced row fetch through wave-private LDS images; dim % 64 == 0, dim <= TAIL_MAX_DIM) and the
// thread-per-candidate one (every shape; AK_RERANK_OLD = 1). Same bits from both.
int rerank(Index &ix, const float *queries_dev, const float *nb_dev, int nq, int kp, const uint64_t *cand,
           uint64_t *okeys, int64_t *oids, hipStream_t st);
bool rerank_panel_supported(const Index &ix);
bool rerank_takes_panel(const Index &ix);          // what rerank() launches for this index under the current switches
// one named kernel (kernel-level tests); panel on a shape it does not take is an error, not a fallback
int rerank_with(Index &ix, const float *queries_dev, const float *nb_dev, int nq, int kp, const uint64_t *cand, uint64_t *okeys,
                int64_t *oids, bool panel, hipStream_t st);

// per-query preparation: nb (pgvector-order sum of squares)
int query_norms(const float *queries_dev, int nq, int dim, float *nb_dev, hipStream_t st);

// keys/ids [nq][k] -> distances + counts
int emit_results(const uint64_t *keys, const int64_t *ids, int nq, int k, int64_t *out_ids,
                 double *out_dist, int *out_cnt, hipStream_t st);

// ---- pieces of index.hip the lexical store (lexical.hip) builds on ---------------------------------------------------------
int thread_stream(hipStream_t *out);                  // the calling host thread's stream
char *thread_scratch(size_t bytes);                   // the calling host thread's grow-only device scratch (NULL: hipMalloc failed)
void thread_scratch_trim();
int writer_fence(Index &ix);                          // wait for the last asynchronous device search (caller holds the unique lock)
int filter_is_current(const Index &ix, const void *row_filter, int64_t filter_len, uint64_t filter_epoch, const char *who);
// ak_index_search_dev behind its argument checks; the caller holds ix.mu (shared) and has checked the filter's epoch
// stats4 (nullable, host int64[4]): ak_index_search's out_stats of this call, AUTO mode on the MFMA scan (zeros are left otherwise)
int search_dev_locked(Index &ix, const float *queries_dev, int nq, int k, int mode, const uint8_t *row_filter_dev, int64_t *out_ids_dev,
                      double *out_dist_dev, int *out_cert_dev, hipStream_t st, int64_t *stats4 = nullptr);
// lexical.hip: what rebuild() / ak_index_remove / ak_index_destroy do to the lexical store
struct LexMove { int64_t *off = nullptr; int32_t *cnt = nullptr, *len = nullptr; };   // the new per-slot arrays (zeroed, new capacity)
int lex_rebuild(Index &ix, const LexMove &to, const std::vector<int64_t> *src, hipStream_t st, uint2 **new_arena, int64_t *new_cap,
                int64_t *new_used);
void lex_rebuilt(Index &ix, const std::vector<int64_t> *src, uint2 *new_arena, int64_t new_cap, int64_t new_used);
void lex_removed(Index &ix, const std::vector<int64_t> &slots);
void lex_release(Index &ix);
// pieces of lexical.hip the batch call (lexical_batch.hip) builds on
int lex_unique_terms(const int32_t *terms, int T, std::vector<uint32_t> &out, const char *who);      // distinct, first-occurrence order
int lex_pin_reserve(Index &ix, size_t need);
hipEvent_t *lex_events(Index &ix);                    // ix.lex_ev when ak_index_profile is on, else NULL
void lex_also_slots(const Index &ix, const int64_t *also_ids, int64_t n_also, std::vector<int64_t> &also);
// ak_index_hybrid_search behind its argument checks and locks (ix.mu shared, ix.lex_mu)
int lex_hybrid_one(Index &ix, const float *query, const std::vector<uint32_t> &uq, double k1, double b, double sign, double w_s,
                   double w_b, const std::vector<int64_t> &also, const uint8_t *row_filter, int k, int64_t *out_hit_ids,
                   double *out_hit_combined, int *n_hit, int64_t *out_scan_ids, double *out_scan_dist, int *n_scan, int64_t *out_info);
// ak_index_hybrid_search: the call itself (uncoalesced) -- what a group of one runs
int lex_hybrid_single(Index &ix, const HybridReq &r);
// lexical_batch.hip: one group of same-keyed concurrent calls as one batch call; fills every request's outputs, rc and err
void lex_hybrid_group(Index &ix, std::vector<HybridReq *> &g);

// ---- max-marginal-relevance selection (mmr.hip) ------------------------------------------------------------------------------
// The second half of ak_index_mmr_search: the candidate search has run (index.hip), the host has resolved the candidates' row
// slots. k_mmr_gram writes the float32 accumulator of every candidate pair i < j of a query -- exact_distance's chain over the two
// stored rows -- into a packed upper triangle; k_mmr_select, one wave per query, finishes pairs to float64 on the fly and runs the
// greedy pick. Cosine indexes only (the caller has checked).
constexpr int MMR_MAX_FETCH = 128;
struct MmrWs {                  // one block of the calling thread's scratch
    int *slots = nullptr;       // [nq][fetch_k] row slot of candidate rank r; ranks >= the query's count are never read
    float *acc = nullptr;       // [nq][fetch_k (fetch_k - 1) / 2] pair (i < j) at i * fetch_k - i (i + 1) / 2 + (j - i - 1)
    int64_t *ids = nullptr;     // [nq][k] results, pick order
    double *dist = nullptr;     // [nq][k]
    int *rank = nullptr;        // [nq][k]
    size_t bytes = 0;
};
MmrWs mmr_layout(void *base, int nq, int k, int fetch_k);      // base == NULL: only .bytes means anything
// dq_dev [nq][fetch_k] float64 distances and cnt_dev [nq] counts of the candidate search, rank order; everything on `st`
int mmr_run(Index &ix, int nq, int k, int fetch_k, double lambda_mult, const double *dq_dev, const int *cnt_dev, const MmrWs &w,
            hipStream_t st);

// ---- grouped search (group.hip) ----------------------------------------------------------------------------------------------
// The device side of ak_index_group_search. The searches run through search_dev_locked (index.hip), the host resolves the returned
// ids to row slots between a search and its collapse.
constexpr int GROUP_MAX_K = 32, GROUP_MAX_SIZE = 8, GROUP_MAX_FETCH = 128;
struct GroupWs {                          // one block of the calling thread's scratch
    float *q = nullptr, *nb = nullptr;    // [nq][dim] queries, [nq] their norms (stage B)
    int64_t *sids = nullptr;              // [nq][fetch] a round's search results: query q's row, whichever round wrote it last
    double *sdist = nullptr;              // [nq][fetch]
    int *scert = nullptr;                 // [nq]
    int *slots = nullptr;                 // [nq][fetch] row slot of each returned id, -1 behind the list's end
    int32_t *keys = nullptr;              // [slots, rounded up to 16] the caller's row_group
    uint8_t *filter = nullptr;            // [same] the caller's row_filter, or NULL
    uint8_t *mask = nullptr;              // [same] a later round's mask
    int32_t *wkey = nullptr, *wslot = nullptr;   // [nq][GROUP_MAX_K] winners in rank order: group key, representative slot
    int *wcnt = nullptr;                  // [nq] winners so far
    unsigned long long *mcnt = nullptr, *cursor = nullptr;   // [nq] rows the members pass matched / the fill pass's write position
    int64_t *off = nullptr;               // [nq] start of the query's list in its batch
    int *overflow = nullptr;
    int64_t *rid = nullptr;               // [nq][k][g] results
    double *rdist = nullptr;              // [nq][k][g]
    int32_t *rgroup = nullptr;            // [nq][k]
    int *rsizes = nullptr;                // [nq][k]
    size_t bytes = 0;
};
GroupWs group_layout(void *base, int nq, int k, int g, int fetch, int64_t n, int dim, bool has_filter);   // base == NULL: only .bytes
int group_init(const GroupWs &w, int nq, int k, int g, hipStream_t st);                                   // padding, zero counts
int group_collapse(Index &ix, const GroupWs &w, int q0, int nqr, int fetch, int k, int g, hipStream_t st);  // queries q0 .. q0 + nqr
int group_exclude(Index &ix, const GroupWs &w, int q, int64_t n, hipStream_t st);                         // w.mask for query q
int group_members(Index &ix, const GroupWs &w, int nq, int k, int g, int64_t n, const std::function<void *(size_t)> &reserve,
                  hipStream_t st, int64_t *matched);

// ---- fast path (scan.hip) ----------------------------------------------------
// Fused tail of the fast path (exact.hip), one workgroup per query: the dense candidate list the scans appended to
// (list [nq][lcap], cnt [nq]) -> drop candidates below the main-pass starting threshold thr0 -> best kp = 64 by approximate
// score -> exact re-rank in the reference arithmetic (rows staged through LDS) -> top-k by (distance, id) + certificate.
// thr_max [nq]: atomicMax over the workgroups' final thresholds as ascending-order uints (~score_key).
int fused_tail(Index &ix, const float *queries_dev, const float *nb_dev, int nq, int k, const uint64_t *list, int64_t lcap,
               const int *cnt, const unsigned int *thr_max, const float *thr0, const QPrep *prep, int64_t *out_ids_dev,
               double *out_dist_dev, int *out_cnt_dev, int *cert_dev, int64_t *stats_dev, hipStream_t st);

// int8 shadow (index.hip): make it cover rows [0, ix.n) of the current layout; synchronises `st` when it had to build
// AK_SHADOW8_NOMEM: the device has no room for it (nothing is left allocated; the caller runs the 16-bit plan)
constexpr int AK_SHADOW8_NOMEM = -1008;
int ensure_shadow8(Index &ix, hipStream_t st);
void release_shadow8(Index &ix);
bool fast_supported(const Index &ix, int nq, int k);
FastPlan fast_plan(const Index &ix, int nq, int k, bool widest = false, bool allow_i8 = true);
// Candidate scan + select + exact re-rank + certification, all on `st`.
// cert_dev [nq] int32: 1 = top-k proven identical to the exact path.
// nb_dev [nq]: the queries' sums of squares in the reference arithmetic -- an INPUT when nb_ready, otherwise computed here
// (fused into the query set-up launch) and left for the caller. stats_dev (nullable, int64[4]) is zeroed here.
int fast_search(Index &ix, const float *queries_dev, float *nb_dev, bool nb_ready, int nq, int k,
                const uint8_t *filter_dev, int64_t *out_ids_dev, double *out_dist_dev,
                int *out_cnt_dev, int *cert_dev, int64_t *stats_dev, void *ws, const FastPlan &plan,
                hipStream_t st);

}  // namespace ak
