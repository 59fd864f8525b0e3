// lexical.hip -- the BM25 leg of the hybrid query in HBM (gfx950 only): a doc-major lexical store inside the index and the
// whole hybrid query (reference postgres_vectorstore.py:366-491) as one call in slot space under the index's shared lock.
//
// Store: per row slot a sorted list of (term id, tf) entries in an append-only arena (index.h). An append is an append, a delete
// is the `alive` byte, reclaim / compaction is the row permutation of every other per-slot array (lex_rebuild, called by
// rebuild() in index.hip). Entry: 8 bytes, {uint32 term id, uint32 tf} -- any term id below 2^31 and any tf a text can produce
// are held exactly; every row starts on an even entry so that a lane's 16-byte load covers two entries of ONE row.
//
// Query: two streaming passes over the lists, one wave per row, 16-byte coalesced loads along a row's entries, the query terms
// in LDS as sorted chunks of 64 (binary search per entry):
//   k_lex_stats  over ALL live rows: n, sum of lengths, df per query term, a match byte per slot
//   k_lex_compact  the matching rows that pass the WHERE mask -> a dense slot list; the scan leg's mask (WHERE and not a hit)
//   host: avg, idf with the C library's log (T + 3 integers come back: df[T], n, sum_len, hits)
//   k_lex_score  over the listed rows: float64 BM25 in the scalar formulation's order of operations, terms in query order
//   hit leg: rerank() (exact.hip) -> k_lex_combine -> select_topk -> k_lex_emit; scan leg: the certified search with the mask
// The float64 sums are per row, in a fixed order, by one wave: no floating-point atomics anywhere. Integer counters (df, n,
// sum_len, the list cursor) are atomic adds: their results do not depend on the order.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_set>
#include <vector>

#include "index.h"
#include "switches.h"

namespace ak {

constexpr int LEX_QCH = 64;             // query terms per chunk: one per lane in the score pass
constexpr int LEX_WAVES = 4;            // waves per workgroup
constexpr uint32_t LEX_NOTERM = 0xffffffffu;

// position of `t` in the sorted chunk s_q[0, tc), or -1
__device__ inline int lex_find(const uint32_t *s_q, int tc, uint32_t t) {
    int lo = 0, hi = tc;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_q[mid] < t) lo = mid + 1; else hi = mid;
    }
    return (lo < tc && s_q[lo] == t) ? lo : -1;
}

// ---- statistics pass -----------------------------------------------------------------------------------------------------
// qsorted [nch][64]: the query's terms, chunk c = terms [64 c, 64 c + 64) of the query order, SORTED by term id inside the chunk
// and padded with LEX_NOTERM; qpos [nch][64]: the term's place in the query order. counters: {n live, sum_len, list cursor, -}.
__global__ __launch_bounds__(LEX_WAVES * 64) void k_lex_stats(int64_t n_slots, const uint8_t *__restrict__ alive, const int64_t *__restrict__ off,
                                                              const int32_t *__restrict__ cnt, const int32_t *__restrict__ len,
                                                              const uint2 *__restrict__ arena, const uint32_t *__restrict__ qsorted,
                                                              const int32_t *__restrict__ qpos, int T, unsigned int *__restrict__ df,
                                                              unsigned long long *__restrict__ counters, uint8_t *__restrict__ match) {
    __shared__ uint32_t s_q[LEX_QCH];
    __shared__ int s_p[LEX_QCH];
    __shared__ unsigned int s_df[LEX_QCH];
    __shared__ unsigned long long s_tot[2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t w0 = (int64_t)blockIdx.x * LEX_WAVES + wave, wstride = (int64_t)gridDim.x * LEX_WAVES;
    const int nch = (T + LEX_QCH - 1) / LEX_QCH;
    if (threadIdx.x < 2) s_tot[threadIdx.x] = 0;
    for (int c = 0; c < nch; c++) {
        const int tc = T - c * LEX_QCH < LEX_QCH ? T - c * LEX_QCH : LEX_QCH;
        __syncthreads();
        if (threadIdx.x < LEX_QCH) {
            s_q[threadIdx.x] = qsorted[c * LEX_QCH + threadIdx.x];
            s_p[threadIdx.x] = qpos[c * LEX_QCH + threadIdx.x];
            s_df[threadIdx.x] = 0;
        }
        __syncthreads();
        unsigned long long w_n = 0, w_len = 0;
        for (int64_t r = w0; r < n_slots; r += wstride) {
            if (!alive[r]) {                    // wave-uniform
                if (c == 0 && lane == 0) match[r] = 0;
                continue;
            }
            const int m = cnt[r];
            const uint2 *e = arena + off[r];
            bool any = false;
            for (int i = lane * 2; i < m; i += 128) {
                const uint4 v = *(const uint4 *)(e + i);          // entries i, i + 1 of this row (the arena is padded past its end)
                int j = lex_find(s_q, tc, v.x);
                if (j >= 0) { atomicAdd(&s_df[j], 1u); any = true; }
                if (i + 1 < m) {
                    j = lex_find(s_q, tc, v.z);
                    if (j >= 0) { atomicAdd(&s_df[j], 1u); any = true; }
                }
            }
            const bool hit = __ballot(any) != 0;
            if (lane == 0) {
                if (c == 0) { w_n += 1; w_len += (unsigned long long)len[r]; match[r] = hit ? 1 : 0; }
                else if (hit) match[r] = 1;
            }
        }
        if (c == 0 && lane == 0) { atomicAdd(&s_tot[0], w_n); atomicAdd(&s_tot[1], w_len); }
        __syncthreads();
        if (threadIdx.x < tc && s_df[threadIdx.x]) atomicAdd(&df[s_p[threadIdx.x]], s_df[threadIdx.x]);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_tot[threadIdx.x]) atomicAdd(&counters[threadIdx.x], s_tot[threadIdx.x]);
}

// The hit set in slot space: matching rows that pass the WHERE mask, appended to `list` as re-rank candidates (the row slot
// in the low 32 bits, as rerank() reads them); mask = WHERE and not a hit, for the scan leg. match[r] becomes 2 for listed rows.
__global__ __launch_bounds__(256) void k_lex_compact(int64_t n_slots, const uint8_t *__restrict__ filter, uint8_t *__restrict__ match,
                                                     uint64_t *__restrict__ list, unsigned long long *__restrict__ counters,
                                                     uint8_t *__restrict__ mask) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = r < n_slots;
    const bool pass = in && (!filter || filter[r]);
    const bool take = pass && match[r] == 1;
    const unsigned long long b = __ballot(take);
    if (b) {
        unsigned long long base = 0;
        const int leader = __ffsll((long long)b) - 1;
        if (lane == leader) base = atomicAdd(&counters[2], (unsigned long long)__popcll(b));
        base = __shfl(base, leader);
        if (take) {
            list[base + __popcll(b & ((1ull << lane) - 1ull))] = (uint64_t)r;
            match[r] = 2;
        }
    }
    if (in) mask[r] = (pass && !take) ? 1 : 0;
}

// Rows whose distance can be NaN (the store's suspects) join the hit set with a BM25 of +0.0 unless they are listed already.
__global__ void k_lex_also(const int64_t *__restrict__ also, int n_also, int64_t n_slots, const uint8_t *__restrict__ alive,
                           const uint8_t *__restrict__ filter, uint8_t *__restrict__ match, uint8_t *__restrict__ mask,
                           uint64_t *__restrict__ list_tail, double *__restrict__ bm_tail) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_also) return;
    const int64_t s = also[i];
    const bool ok = s >= 0 && s < n_slots && alive[s] && (!filter || filter[s]) && match[s] != 2;
    list_tail[i] = ok ? (uint64_t)s : KEY_INVALID;
    bm_tail[i] = 0.0;
    if (ok) mask[s] = 0;
}

// ---- score pass -----------------------------------------------------------------------------------------------------------
// One wave per listed row. The surviving terms (df > 0) in query order, chunks of 64 as above; idf [T]. Per chunk the row's
// matching tfs land in the wave's LDS line, lane j evaluates term j's contribution, and the contributions are added to the row's
// accumulator one by one in query order: acc = acc + ((idf tf)(k1 + 1)) / (tf + k1 ((1 - b) + (b len) / avg)).
__global__ __launch_bounds__(LEX_WAVES * 64) void k_lex_score(int64_t n_list, const uint64_t *__restrict__ list, const int64_t *__restrict__ off,
                                                              const int32_t *__restrict__ cnt, const int32_t *__restrict__ len,
                                                              const uint2 *__restrict__ arena, const uint32_t *__restrict__ qsorted,
                                                              const int32_t *__restrict__ qpos, int T, const double *__restrict__ idf,
                                                              double k1, double b, double avg, double sign, double *__restrict__ bm) {
    __shared__ uint32_t s_q[LEX_QCH];
    __shared__ int s_p[LEX_QCH];
    __shared__ uint32_t s_tf[LEX_WAVES][LEX_QCH];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t w0 = (int64_t)blockIdx.x * LEX_WAVES + wave, wstride = (int64_t)gridDim.x * LEX_WAVES;
    const int nch = (T + LEX_QCH - 1) / LEX_QCH;
    const double k1p = k1 + 1.0, omb = 1.0 - b;
    for (int c = 0; c < nch; c++) {
        const int tc = T - c * LEX_QCH < LEX_QCH ? T - c * LEX_QCH : LEX_QCH;
        __syncthreads();
        if (threadIdx.x < LEX_QCH) {
            s_q[threadIdx.x] = qsorted[c * LEX_QCH + threadIdx.x];
            s_p[threadIdx.x] = qpos[c * LEX_QCH + threadIdx.x] - c * LEX_QCH;        // place inside the chunk
        }
        __syncthreads();
        const double my_idf = lane < tc ? idf[c * LEX_QCH + lane] : 0.0;
        for (int64_t j = w0; j < n_list; j += wstride) {
            const int64_t r = (int64_t)(uint32_t)list[j];
            const int m = cnt[r];
            const uint2 *e = arena + off[r];
            s_tf[wave][lane] = 0;
            __builtin_amdgcn_wave_barrier();
            for (int i = lane * 2; i < m; i += 128) {
                const uint4 v = *(const uint4 *)(e + i);
                int p = lex_find(s_q, tc, v.x);
                if (p >= 0) s_tf[wave][s_p[p]] = v.y;
                if (i + 1 < m) {
                    p = lex_find(s_q, tc, v.z);
                    if (p >= 0) s_tf[wave][s_p[p]] = v.w;
                }
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xc07f);        // lgkmcnt(0): the wave's LDS writes have landed
            const uint32_t tfu = s_tf[wave][lane];
            __builtin_amdgcn_wave_barrier();
            const double tf = (double)tfu, dl = (double)len[r];
            const double norm = avg > 0.0 ? tf + k1 * (omb + (b * dl) / avg) : tf + k1 * omb;
            const double contrib = ((my_idf * tf) * k1p) / norm;
            unsigned long long present = __ballot(tfu != 0);
            double acc = c == 0 ? 0.0 : bm[j];
            while (present) {
                const int t = __ffsll((long long)present) - 1;
                present &= present - 1;
                acc = acc + __shfl(contrib, t);
            }
            if (lane == 0) bm[j] = c == nch - 1 ? sign * acc : acc;
        }
    }
}

// combined = (1.0 - d) w_s + bm w_b per listed row; the selection key orders NaN first, then combined descending (select_topk
// breaks ties by ascending id)
__global__ void k_lex_combine(int64_t n_list, const uint64_t *__restrict__ dkeys, const double *__restrict__ bm, double w_s, double w_b,
                              double *__restrict__ comb, uint64_t *__restrict__ ckeys) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_list) return;
    const uint64_t dk = dkeys[j];
    if (dk == KEY_INVALID) { ckeys[j] = KEY_INVALID; comb[j] = 0.0; return; }
    const double d = key_dist(dk);
    const double c = (1.0 - d) * w_s + bm[j] * w_b;
    comb[j] = c;
    ckeys[j] = c != c ? 0ull : ~dist_key(c);
}

// the selected rows' combined scores as computed (the key does not tell -0.0 from 0.0)
__global__ void k_lex_emit(int64_t n_list, const uint64_t *__restrict__ ckeys, const int64_t *__restrict__ ids, const double *__restrict__ comb,
                           int k, const uint64_t *__restrict__ skeys, const int64_t *__restrict__ sids, double *__restrict__ out_comb) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_list) return;
    const uint64_t key = ckeys[j];
    if (key == KEY_INVALID || key > skeys[k - 1]) return;
    const int64_t id = ids[j];
    for (int i = 0; i < k; i++)
        if (skeys[i] == key && sids[i] == id) out_comb[i] = comb[j];
}

// ---- growth / compaction ---------------------------------------------------------------------------------------------------
// new row i <- old row src[i]: one wave per row, 16-byte pieces (both lists start on even entries)
__global__ __launch_bounds__(256) void k_lex_gather(const int64_t *__restrict__ src, int64_t m, const int64_t *__restrict__ off,
                                                    const int32_t *__restrict__ cnt, const int32_t *__restrict__ len,
                                                    const uint2 *__restrict__ arena, const int64_t *__restrict__ off2_in,
                                                    int64_t *__restrict__ off2, int32_t *__restrict__ cnt2, int32_t *__restrict__ len2,
                                                    uint2 *__restrict__ arena2) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= m) return;
    const int64_t s = src[i];
    const int c = cnt[s];
    const int64_t o2 = off2_in[i];
    const uint2 *from = arena + off[s];
    uint2 *to = arena2 + o2;
    for (int e = lane * 2; e < c; e += 128) *(uint4 *)(to + e) = *(const uint4 *)(from + e);
    if (lane == 0) { off2[i] = o2; cnt2[i] = c; len2[i] = len[s]; }
}

__global__ void k_lex_scatter(const int64_t *__restrict__ slots, const int64_t *__restrict__ offs, const int32_t *__restrict__ cnts,
                              const int32_t *__restrict__ lens, int64_t n, int64_t *__restrict__ off, int32_t *__restrict__ cnt,
                              int32_t *__restrict__ len) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t s = slots[i];
    off[s] = offs[i]; cnt[s] = cnts[i]; len[s] = lens[i];
}

static inline int64_t even_up(int64_t x) { return (x + 1) & ~(int64_t)1; }
static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
// an arena of `entries` entries: two more are allocated, the last lane's 16-byte load may reach one entry past a row's end
static hipError_t arena_alloc(uint2 **out, int64_t entries) { return hipMalloc((void **)out, (size_t)(entries + 2) * sizeof(uint2)); }

// rebuild() of index.hip, lexical part. src == NULL: every slot keeps its number, the per-slot arrays are copied and the arena
// stays. Otherwise new slot i <- old slot (*src)[i]: the arena is copied compacted in the new slot order -- offsets from the host
// mirror of the entry counts --, so a dead row's entries do not survive. Enqueued on st; the caller synchronises and then calls
// lex_rebuilt() (success) or frees *new_arena (failure).
int lex_rebuild(Index &ix, const LexMove &to, const std::vector<int64_t> *src, hipStream_t st, uint2 **new_arena, int64_t *new_cap,
                int64_t *new_used) {
    *new_arena = nullptr; *new_cap = 0; *new_used = 0;
    if (!src) {
        if (ix.n == 0) return 0;
        if (hipMemcpyAsync(to.off, ix.lex_off, (size_t)ix.n * 8, hipMemcpyDeviceToDevice, st) != hipSuccess ||
            hipMemcpyAsync(to.cnt, ix.lex_cnt, (size_t)ix.n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
            hipMemcpyAsync(to.len, ix.lex_len, (size_t)ix.n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return -10;
        return 0;
    }
    const int64_t m = (int64_t)src->size();
    if (m == 0 || ix.lex_used == 0) return 0;       // no lists at all: the new arrays are zeroed already
    ix.h_lex_cnt.resize((size_t)ix.n, 0);
    std::vector<int64_t> up((size_t)2 * m);          // [src | new offsets]
    int64_t used = 0;
    for (int64_t i = 0; i < m; i++) {
        up[i] = (*src)[i];
        up[m + i] = used;
        used = even_up(used + ix.h_lex_cnt[(*src)[i]]);
    }
    uint2 *a2 = nullptr;
    int64_t *d = nullptr;
    if (arena_alloc(&a2, used) != hipSuccess) return -10;
    if (hipMalloc((void **)&d, (size_t)2 * m * 8) != hipSuccess) { hipFree(a2); return -10; }
    int rc = 0;
    if (hipMemcpyAsync(d, up.data(), (size_t)2 * m * 8, hipMemcpyHostToDevice, st) != hipSuccess) rc = -10;
    if (!rc) {
        k_lex_gather<<<(unsigned)((m + 3) / 4), 256, 0, st>>>(d, m, ix.lex_off, ix.lex_cnt, ix.lex_len, ix.lex_arena, d + m, to.off, to.cnt,
                                                              to.len, a2);
        if (hipGetLastError() != hipSuccess) rc = -10;
    }
    if (hipStreamSynchronize(st) != hipSuccess) rc = -10;      // `up` and `d` end here
    hipFree(d);
    if (rc) { hipFree(a2); return rc; }
    *new_arena = a2; *new_cap = used; *new_used = used;
    return 0;
}

// the host mirror follows; called before IndexBook::rebuilt renumbers the slots
void lex_rebuilt(Index &ix, const std::vector<int64_t> *src, uint2 *new_arena, int64_t new_cap, int64_t new_used) {
    if (!src) return;
    const int64_t m = (int64_t)src->size();
    ix.h_lex_cnt.resize((size_t)ix.n, 0);
    ix.h_lex_att.resize((size_t)ix.n, 0);
    std::vector<int32_t> c2((size_t)m);
    std::vector<uint8_t> a2((size_t)m);
    int64_t entries = 0, rows = 0;
    for (int64_t i = 0; i < m; i++) {
        c2[i] = ix.h_lex_cnt[(*src)[i]];
        a2[i] = ix.h_lex_att[(*src)[i]];
        entries += c2[i]; rows += a2[i];
    }
    ix.h_lex_cnt.swap(c2);
    ix.h_lex_att.swap(a2);
    if (ix.lex_arena) hipFree(ix.lex_arena);
    ix.lex_arena = new_arena; ix.lex_arena_cap = new_cap; ix.lex_used = new_used;
    ix.lex_entries = entries; ix.lex_rows = rows;
}

void lex_removed(Index &ix, const std::vector<int64_t> &slots) {
    for (int64_t s : slots)
        if ((size_t)s < ix.h_lex_att.size() && ix.h_lex_att[s]) { ix.h_lex_att[s] = 0; ix.lex_rows--; }
}

void lex_release(Index &ix) {
    if (ix.lex_arena) hipFree(ix.lex_arena);
    ix.lex_arena = nullptr; ix.lex_arena_cap = ix.lex_used = 0;
    ix.ws_lex.release();
    ix.ws_lexb.release();
    if (ix.lex_pin) hipHostFree(ix.lex_pin);
    ix.lex_pin = nullptr; ix.lex_pin_cap = 0;
    for (auto &e : ix.lex_ev) if (e) { hipEventDestroy(e); e = nullptr; }
}

// ---- the query ----------------------------------------------------------------------------------------------------------------
namespace {

struct QueryTable {       // the query's terms as the kernels read them
    std::vector<uint32_t> sorted;
    std::vector<int32_t> pos;
    int T = 0;
    void build(const std::vector<uint32_t> &terms) {
        T = (int)terms.size();
        const int nch = (T + LEX_QCH - 1) / LEX_QCH;
        sorted.assign((size_t)std::max(nch, 1) * LEX_QCH, LEX_NOTERM);
        pos.assign((size_t)std::max(nch, 1) * LEX_QCH, 0);
        for (int c = 0; c < nch; c++) {
            const int lo = c * LEX_QCH, tc = std::min(LEX_QCH, T - lo);
            std::vector<int> o(tc);
            for (int i = 0; i < tc; i++) o[i] = lo + i;
            std::sort(o.begin(), o.end(), [&](int a, int b) { return terms[a] < terms[b]; });
            for (int i = 0; i < tc; i++) { sorted[lo + i] = terms[o[i]]; pos[lo + i] = o[i]; }
        }
    }
    size_t bytes() const { return sorted.size() * 8; }
};

}  // namespace

// the query's distinct terms in first-occurrence order
int lex_unique_terms(const int32_t *terms, int T, std::vector<uint32_t> &out, const char *who) {
    out.clear();
    if (T < 0 || (T > 0 && !terms)) AK_FAIL(-1, std::string(who) + ": bad terms");
    std::unordered_set<uint32_t> seen;
    for (int i = 0; i < T; i++) {
        if (terms[i] < 0) AK_FAIL(-1, std::string(who) + ": term ids must be >= 0");
        if (seen.insert((uint32_t)terms[i]).second) out.push_back((uint32_t)terms[i]);
    }
    return 0;
}

int lex_pin_reserve(Index &ix, size_t need) {
    if (need <= ix.lex_pin_cap) return 0;
    if (ix.lex_pin) hipHostFree(ix.lex_pin);
    ix.lex_pin = nullptr; ix.lex_pin_cap = 0;
    need = (need + 4095) & ~(size_t)4095;
    AK_HIP(hipHostMalloc((void **)&ix.lex_pin, need, hipHostMallocDefault));
    ix.lex_pin_cap = need;
    return 0;
}

namespace {

struct LexPlan {          // workspace of one query; every array sized for the worst case so that nothing grows after the counts are known
    uint8_t *match, *mask, *filter;
    uint64_t *list, *dkeys, *ckeys, *skeys;
    int64_t *oids, *sids, *also, *scan_ids;
    double *bm, *comb, *out_comb, *scan_dist, *idf;
    uint32_t *qsorted; int32_t *qpos;
    unsigned int *df;
    unsigned long long *counters;
    float *dq, *dnb;
    int *cert;
    void *sel;
    size_t bytes;
};

LexPlan lex_plan(char *base, int64_t n, int T, int n_also, int k, int dim, bool with_filter) {
    LexPlan p;
    size_t o = 0;
    auto take = [&](size_t b) { char *r = base ? base + o : nullptr; o += al256(b); return r; };
    const size_t L = (size_t)n + (size_t)n_also, tq = (size_t)std::max((T + LEX_QCH - 1) / LEX_QCH, 1) * LEX_QCH;
    p.match = (uint8_t *)take((size_t)n); p.mask = (uint8_t *)take((size_t)n); p.filter = (uint8_t *)take(with_filter ? (size_t)n : 0);
    p.list = (uint64_t *)take(L * 8); p.dkeys = (uint64_t *)take(L * 8); p.ckeys = (uint64_t *)take(L * 8);
    p.oids = (int64_t *)take(L * 8); p.bm = (double *)take(L * 8); p.comb = (double *)take(L * 8);
    p.skeys = (uint64_t *)take((size_t)k * 8); p.sids = (int64_t *)take((size_t)k * 8); p.out_comb = (double *)take((size_t)k * 8);
    p.scan_ids = (int64_t *)take((size_t)k * 8); p.scan_dist = (double *)take((size_t)k * 8);
    p.also = (int64_t *)take((size_t)n_also * 8);
    p.idf = (double *)take(tq * 8); p.qsorted = (uint32_t *)take(tq * 4); p.qpos = (int32_t *)take(tq * 4);
    p.df = (unsigned int *)take(tq * 4 + 32);             // df [tq] and, behind it, the four 64-bit counters: one memset, one copy back
    p.counters = (unsigned long long *)((char *)p.df + tq * 4);
    p.dq = (float *)take((size_t)dim * 4); p.dnb = (float *)take(256); p.cert = (int *)take(256);
    p.sel = take(select_scratch_bytes(1, (int64_t)L, std::max(k, 1)));
    p.bytes = o;
    return p;
}

struct LexStats { int64_t n_live = 0, sum_len = 0, n_list = 0; int T_used = 0; double avg = 0.0; };
// host sources of the asynchronous uploads: they live in the caller's frame, until it has synchronised the stream
struct LexHost { QueryTable qt, q2; std::vector<double> idf; };

unsigned lex_grid(int64_t rows) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + LEX_WAVES - 1) / LEX_WAVES, 4096)); }

// statistics pass + list compaction + the host's idf step + score pass. On return (stream synchronised once, after the
// compaction) p.list [st.n_list] and -- enqueued, not yet synchronised -- p.bm [st.n_list] describe the hit rows.
int lex_passes(Index &ix, LexPlan &p, const std::vector<uint32_t> &terms, const uint8_t *filter_dev, double k1, double b, double sign,
               hipStream_t st, LexStats &out, hipEvent_t *ev, LexHost &hs) {
    const int64_t n = ix.n;
    QueryTable &qt = hs.qt, &q2 = hs.q2;
    std::vector<double> &idf = hs.idf;
    qt.build(terms);
    const size_t tq = qt.sorted.size();
    AK_HIP(hipMemsetAsync(p.df, 0, tq * 4 + 32, st));
    if (ev) AK_HIP(hipEventRecord(ev[0], st));
    if (qt.T > 0 && ix.lex_used > 0) {
        AK_HIP(hipMemcpyAsync(p.qsorted, qt.sorted.data(), tq * 4, hipMemcpyHostToDevice, st));
        AK_HIP(hipMemcpyAsync(p.qpos, qt.pos.data(), tq * 4, hipMemcpyHostToDevice, st));
        k_lex_stats<<<lex_grid(n), LEX_WAVES * 64, 0, st>>>(n, ix.alive, ix.lex_off, ix.lex_cnt, ix.lex_len, ix.lex_arena, p.qsorted, p.qpos,
                                                            qt.T, p.df, p.counters, p.match);
    } else {
        AK_HIP(hipMemsetAsync(p.match, 0, (size_t)n, st));
    }
    AK_HIP(hipGetLastError());
    k_lex_compact<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, filter_dev, p.match, p.list, p.counters, p.mask);
    AK_HIP(hipGetLastError());
    if (ev) AK_HIP(hipEventRecord(ev[1], st));
    // the one small copy: df [T] | n | sum_len | hits
    if (lex_pin_reserve(ix, tq * 4 + 32 + 4096)) return -10;
    AK_HIP(hipMemcpyAsync(ix.lex_pin, p.df, tq * 4 + 32, hipMemcpyDeviceToHost, st));
    AK_HIP(hipStreamSynchronize(st));
    const unsigned int *df = (const unsigned int *)ix.lex_pin;
    const unsigned long long *cn = (const unsigned long long *)(ix.lex_pin + tq * 4);
    out.n_live = (int64_t)cn[0]; out.sum_len = (int64_t)cn[1]; out.n_list = (int64_t)cn[2];
    if (out.n_list == 0 || out.n_live == 0) { out.n_list = 0; if (ev) AK_HIP(hipEventRecord(ev[2], st)); return 0; }
    const double nd = (double)out.n_live;
    out.avg = (double)out.sum_len / nd;
    std::vector<uint32_t> used;
    idf.clear();
    for (int t = 0; t < qt.T; t++) {
        if (!df[t]) continue;                      // no live row holds it: the term drops out
        const double d = (double)df[t];
        used.push_back(terms[t]);
        idf.push_back(log(1.0 + ((double)(out.n_live - (int64_t)df[t]) + 0.5) / (d + 0.5)));
    }
    out.T_used = (int)used.size();
    q2.build(used);
    idf.resize(q2.sorted.size(), 0.0);
    AK_HIP(hipMemcpyAsync(p.qsorted, q2.sorted.data(), q2.sorted.size() * 4, hipMemcpyHostToDevice, st));
    AK_HIP(hipMemcpyAsync(p.qpos, q2.pos.data(), q2.sorted.size() * 4, hipMemcpyHostToDevice, st));
    AK_HIP(hipMemcpyAsync(p.idf, idf.data(), idf.size() * 8, hipMemcpyHostToDevice, st));
    k_lex_score<<<lex_grid(out.n_list), LEX_WAVES * 64, 0, st>>>(out.n_list, p.list, ix.lex_off, ix.lex_cnt, ix.lex_len, ix.lex_arena, p.qsorted,
                                                                 p.qpos, q2.T, p.idf, k1, b, out.avg, sign, p.bm);
    AK_HIP(hipGetLastError());
    if (ev) AK_HIP(hipEventRecord(ev[2], st));
    return 0;
}

}  // namespace

hipEvent_t *lex_events(Index &ix) {
    if (!ix.profile) return nullptr;
    for (auto &e : ix.lex_ev)
        if (!e && hipEventCreate(&e) != hipSuccess) return nullptr;
    return ix.lex_ev;
}

// also_ids -> the distinct live slots they name: a const look at the id map (the shared lock allows no lazy build; generated rows
// go by the id array)
void lex_also_slots(const Index &ix, const int64_t *also_ids, int64_t n_also, std::vector<int64_t> &also) {
    also.clear();
    const int64_t n = ix.n;
    std::unordered_set<int64_t> seen;
    for (int64_t i = 0; i < n_also; i++) {
        int64_t s = -1;
        if (ix.map_built) {
            auto it = ix.id2slot.find(also_ids[i]);
            if (it != ix.id2slot.end()) s = it->second;
        } else {
            for (int64_t r = 0; r < n; r++) if (ix.h_ids[r] == also_ids[i] && ix.h_alive[r]) { s = r; break; }
        }
        if (s >= 0 && ix.h_alive[s] && seen.insert(s).second) also.push_back(s);
    }
}

}  // namespace ak

using namespace ak;

extern "C" {

int ak_index_lex_attach(ak_index_t h, const int64_t *ids, int64_t n, const int64_t *row_offsets, const int32_t *terms, const int32_t *tfs,
                        const int32_t *doc_len, uint64_t generation) {
    AK_BIND();
    if (!h) AK_FAIL(-1, "ak_index_lex_attach: NULL index");
    Index &ix = *(Index *)h;
    if (n == 0) return 0;
    if (n < 0 || !ids || !row_offsets || !doc_len) AK_FAIL(-1, "ak_index_lex_attach: bad arguments");
    const int64_t total = row_offsets[n];
    if (row_offsets[0] != 0 || total < 0 || (total > 0 && (!terms || !tfs))) AK_FAIL(-1, "ak_index_lex_attach: bad row_offsets");
    std::unique_lock<std::shared_mutex> lk(ix.mu);
    if (generation != ix.lex_gen)
        AK_FAIL(-1, "ak_index_lex_attach: the lists of this index belong to generation " + std::to_string(ix.lex_gen) + ", not " +
                        std::to_string(generation) + " (ak_index_lex_clear starts a generation)");
    // pass 1 checks everything, nothing is touched: unknown or dead ids, unsorted lists and zero tfs are errors
    std::vector<int64_t> slots((size_t)n), offs((size_t)n);
    std::vector<int32_t> cnts((size_t)n);
    std::unordered_set<int64_t> seen;
    int64_t used = even_up(ix.lex_used);
    for (int64_t i = 0; i < n; i++) {
        const int64_t s = ix.alive_slot_of(ids[i]);
        if (s < 0) AK_FAIL(-1, "ak_index_lex_attach: id " + std::to_string(ids[i]) + " is not a live row of the index");
        if (!seen.insert(s).second) AK_FAIL(-1, "ak_index_lex_attach: id " + std::to_string(ids[i]) + " listed twice");
        const int64_t lo = row_offsets[i], hi = row_offsets[i + 1];
        if (hi < lo || hi > total || hi - lo > 0x7fffffff) AK_FAIL(-1, "ak_index_lex_attach: bad row_offsets");
        if (doc_len[i] < 0) AK_FAIL(-1, "ak_index_lex_attach: negative document length");
        for (int64_t e = lo; e < hi; e++) {
            if (terms[e] < 0 || tfs[e] <= 0) AK_FAIL(-1, "ak_index_lex_attach: term ids must be >= 0 and tfs > 0");
            if (e > lo && terms[e] <= terms[e - 1]) AK_FAIL(-1, "ak_index_lex_attach: a row's term ids must ascend");
        }
        slots[i] = s; offs[i] = used; cnts[i] = (int32_t)(hi - lo);
        used = even_up(used + (hi - lo));
    }
    hipStream_t st;
    if (thread_stream(&st)) return -10;
    if (writer_fence(ix)) return -10;
    const int64_t base = even_up(ix.lex_used), span = used - base;
    if (used > ix.lex_arena_cap) {         // the arena doubles
        int64_t cap2 = std::max<int64_t>(ix.lex_arena_cap * 2, 1 << 16);
        while (cap2 < used) cap2 *= 2;
        uint2 *a2 = nullptr;
        hipError_t e = arena_alloc(&a2, cap2);
        if (e != hipSuccess) AK_FAIL(-10, std::string("ak_index_lex_attach: hipMalloc failed: ") + hipGetErrorString(e));
        if (ix.lex_used > 0 && (hipMemcpy(a2, ix.lex_arena, (size_t)ix.lex_used * sizeof(uint2), hipMemcpyDeviceToDevice) != hipSuccess ||
                                hipStreamSynchronize(nullptr) != hipSuccess)) {
            hipFree(a2);
            AK_FAIL(-10, "ak_index_lex_attach: arena copy failed");
        }
        if (ix.lex_arena) hipFree(ix.lex_arena);
        ix.lex_arena = a2; ix.lex_arena_cap = cap2;
    }
    // entries (with the alignment gaps zeroed) | slots | offsets | counts | lengths, one staging block
    std::vector<uint2> ent((size_t)span, make_uint2(0, 0));
    for (int64_t i = 0; i < n; i++) {
        uint2 *d = ent.data() + (offs[i] - base);
        for (int64_t e = row_offsets[i]; e < row_offsets[i + 1]; e++) *d++ = make_uint2((uint32_t)terms[e], (uint32_t)tfs[e]);
    }
    const size_t b_sl = al256((size_t)n * 8), b_c = al256((size_t)n * 4);
    char *blk = thread_scratch(2 * b_sl + 2 * b_c);
    if (!blk) return -10;
    int64_t *d_sl = (int64_t *)blk, *d_of = (int64_t *)(blk + b_sl);
    int32_t *d_c = (int32_t *)(blk + 2 * b_sl), *d_l = (int32_t *)(blk + 2 * b_sl + b_c);
    if (span > 0) AK_HIP(hipMemcpyAsync(ix.lex_arena + base, ent.data(), (size_t)span * sizeof(uint2), hipMemcpyHostToDevice, st));
    AK_HIP(hipMemcpyAsync(d_sl, slots.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    AK_HIP(hipMemcpyAsync(d_of, offs.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    AK_HIP(hipMemcpyAsync(d_c, cnts.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    AK_HIP(hipMemcpyAsync(d_l, doc_len, (size_t)n * 4, hipMemcpyHostToDevice, st));
    k_lex_scatter<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(d_sl, d_of, d_c, d_l, n, ix.lex_off, ix.lex_cnt, ix.lex_len);
    AK_HIP(hipGetLastError());
    AK_HIP(hipStreamSynchronize(st));
    // the device holds the lists: the mirror follows
    ix.h_lex_cnt.resize((size_t)ix.n, 0);
    ix.h_lex_att.resize((size_t)ix.n, 0);
    for (int64_t i = 0; i < n; i++) {
        const int64_t s = slots[i];
        ix.lex_entries += cnts[i] - ix.h_lex_cnt[s];
        if (!ix.h_lex_att[s]) { ix.h_lex_att[s] = 1; ix.lex_rows++; }
        ix.h_lex_cnt[s] = cnts[i];
    }
    ix.lex_used = used;
    thread_scratch_trim();
    return 0;
}

int ak_index_lex_clear(ak_index_t h, uint64_t new_generation) {
    AK_BIND();
    if (!h) AK_FAIL(-1, "ak_index_lex_clear: NULL index");
    Index &ix = *(Index *)h;
    std::unique_lock<std::shared_mutex> lk(ix.mu);
    if (writer_fence(ix)) return -10;
    if (ix.n > 0) {
        AK_HIP(hipMemset(ix.lex_off, 0, (size_t)ix.n * 8));
        AK_HIP(hipMemset(ix.lex_cnt, 0, (size_t)ix.n * 4));
        AK_HIP(hipMemset(ix.lex_len, 0, (size_t)ix.n * 4));
        AK_HIP(hipStreamSynchronize(nullptr));        // null-stream fills; the next attach writes on its thread's stream
    }
    if (ix.lex_arena) hipFree(ix.lex_arena);
    ix.lex_arena = nullptr; ix.lex_arena_cap = ix.lex_used = ix.lex_entries = ix.lex_rows = 0;
    ix.h_lex_cnt.clear(); ix.h_lex_att.clear();
    ix.lex_gen = new_generation;
    return 0;
}

int ak_index_lex_info(ak_index_t h, uint64_t *generation, int64_t *rows_attached, int64_t *entries, int64_t *arena_bytes) {
    if (!h) AK_FAIL(-1, "ak_index_lex_info: NULL index");
    Index &ix = *(Index *)h;
    std::shared_lock<std::shared_mutex> lk(ix.mu);
    if (generation) *generation = ix.lex_gen;
    if (rows_attached) *rows_attached = ix.lex_rows;
    if (entries) *entries = ix.lex_entries;
    if (arena_bytes) *arena_bytes = ix.lex_used * (int64_t)sizeof(uint2);
    return 0;
}

int ak_index_lex_scores(ak_index_t h, const int32_t *terms, int T, double k1, double b, double sign, double *out_bm, uint8_t *out_hit,
                        int64_t *out_info) {
    AK_BIND();
    if (!h) AK_FAIL(-1, "ak_index_lex_scores: NULL index");
    Index &ix = *(Index *)h;
    if (out_info) memset(out_info, 0, 4 * sizeof(int64_t));
    std::vector<uint32_t> uq;
    if (int rc = lex_unique_terms(terms, T, uq, "ak_index_lex_scores")) return rc;
    std::shared_lock<std::shared_mutex> lk(ix.mu);
    const int64_t n = ix.n;
    if (n == 0) return 0;
    if (!out_bm || !out_hit) AK_FAIL(-1, "ak_index_lex_scores: NULL output");
    memset(out_bm, 0, (size_t)n * 8);
    memset(out_hit, 0, (size_t)n);
    std::lock_guard<std::mutex> ql(ix.lex_mu);
    hipStream_t st;
    if (thread_stream(&st)) return -10;
    const size_t need = lex_plan(nullptr, n, (int)uq.size(), 0, 1, ix.dim, false).bytes;
    if (ix.ws_lex.reserve(need)) return -10;
    LexPlan p = lex_plan((char *)ix.ws_lex.buf, n, (int)uq.size(), 0, 1, ix.dim, false);
    LexStats ls;
    LexHost hs;
    int rc = lex_passes(ix, p, uq, nullptr, k1, b, sign, st, ls, nullptr, hs);
    std::vector<uint64_t> list((size_t)ls.n_list);
    std::vector<double> bm((size_t)ls.n_list);
    if (!rc && ls.n_list > 0 &&
        (hipMemcpyAsync(list.data(), p.list, (size_t)ls.n_list * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
         hipMemcpyAsync(bm.data(), p.bm, (size_t)ls.n_list * 8, hipMemcpyDeviceToHost, st) != hipSuccess)) rc = -10;
    if (hipStreamSynchronize(st) != hipSuccess) rc = -10;
    if (rc == -10) AK_FAIL(-10, std::string("ak_index_lex_scores: HIP error: ") + hipGetErrorString(hipGetLastError()));
    if (rc) return rc;
    for (int64_t j = 0; j < ls.n_list; j++) {
        const int64_t s = (int64_t)(uint32_t)list[j];
        out_hit[s] = 1; out_bm[s] = bm[j];
    }
    if (out_info) { out_info[0] = ls.n_live; out_info[1] = ls.sum_len; out_info[2] = ls.n_list; out_info[3] = ls.T_used; }
    return 0;
}

int ak_index_hybrid_search(ak_index_t h, const float *query, const int32_t *terms, int T, double k1, double b, double sign, double w_s,
                           double w_b, const int64_t *also_ids, int64_t n_also, const uint8_t *row_filter, int64_t filter_len,
                           uint64_t filter_epoch, int k, int64_t *out_hit_ids, double *out_hit_combined, int *n_hit, int64_t *out_scan_ids,
                           double *out_scan_dist, int *n_scan, int64_t *out_info) {
    AK_BIND();
    if (!h) AK_FAIL(-1, "ak_index_hybrid_search: NULL index");
    Index &ix = *(Index *)h;
    if (out_info) memset(out_info, 0, 12 * sizeof(int64_t));
    if (!query || k <= 0 || k > 4096 || !out_hit_ids || !out_hit_combined || !n_hit || !out_scan_ids || !out_scan_dist || !n_scan ||
        n_also < 0 || n_also > (1 << 24) || (n_also > 0 && !also_ids))
        AK_FAIL(-1, "ak_index_hybrid_search: bad arguments");
    *n_hit = 0; *n_scan = 0;
    {
        std::vector<uint32_t> uq;          // a caller's bad terms are its own error, not its group's
        if (int rc = lex_unique_terms(terms, T, uq, "ak_index_hybrid_search")) return rc;
    }
    RoctxRange range("ak_index_hybrid_search");
    HybridReq me{query, terms, T, k1, b, sign, w_s, w_b, also_ids, n_also, row_filter, filter_len, filter_epoch, k,
                 out_hit_ids, out_hit_combined, n_hit, out_scan_ids, out_scan_dist, n_scan, out_info};
    if (!switches().coalesce.load(std::memory_order_relaxed)) return lex_hybrid_single(ix, me);
    // concurrent calls meet in the coalescer (coalesce.h): a caller on an idle index serves itself at once through the single-query
    // path; calls that queued behind a running one are served per (k, k1, b, sign, w_s, w_b, filter) group by ONE batch call
    const int rc = ix.hco.submit(me, [&](std::vector<HybridReq *> &g) { lex_hybrid_group(ix, g); });
    if (rc) set_error(me.err);
    return rc;
}

}  // extern "C"

int ak::lex_hybrid_single(Index &ix, const HybridReq &r) {
    std::vector<uint32_t> uq;
    if (int rc = lex_unique_terms(r.terms, r.T, uq, "ak_index_hybrid_search")) return rc;
    std::shared_lock<std::shared_mutex> lk(ix.mu);
    if (int frc = filter_is_current(ix, r.filter, r.flen, r.fepoch, "ak_index_hybrid_search")) return frc;
    if (ix.n == 0) return 0;
    std::vector<int64_t> also;
    lex_also_slots(ix, r.also, r.n_also, also);
    std::lock_guard<std::mutex> ql(ix.lex_mu);
    return lex_hybrid_one(ix, r.q, uq, r.k1, r.b, r.sign, r.w_s, r.w_b, also, r.filter, r.k, r.out_hit_ids, r.out_hit_comb, r.n_hit,
                          r.out_scan_ids, r.out_scan_dist, r.n_scan, r.out_info);
}

// ak_index_hybrid_search behind its argument checks: the caller holds ix.mu (shared) and ix.lex_mu, has checked the filter's epoch
// and zeroed the outputs' counts and out_info; ix.n > 0
int ak::lex_hybrid_one(Index &ix, const float *query, const std::vector<uint32_t> &uq, double k1, double b, double sign, double w_s,
                       double w_b, const std::vector<int64_t> &also, const uint8_t *row_filter, int k, int64_t *out_hit_ids,
                       double *out_hit_combined, int *n_hit, int64_t *out_scan_ids, double *out_scan_dist, int *n_scan,
                       int64_t *out_info) {
    const int64_t n = ix.n;
    const int na = (int)also.size();
    hipStream_t st;
    if (thread_stream(&st)) return -10;
    const size_t need = lex_plan(nullptr, n, (int)uq.size(), na, k, ix.dim, row_filter != nullptr).bytes;
    if (ix.ws_lex.reserve(need)) return -10;
    LexPlan p = lex_plan((char *)ix.ws_lex.buf, n, (int)uq.size(), na, k, ix.dim, row_filter != nullptr);
    hipEvent_t *ev = lex_events(ix);
    int rc = 0;
    LexStats ls;
    LexHost hs;
    int64_t n_list = 0;
    const size_t ob = (size_t)k * 8;
    do {
        if (hipMemcpyAsync(p.dq, query, (size_t)ix.dim * 4, hipMemcpyHostToDevice, st) != hipSuccess) { rc = -10; break; }
        if (row_filter && hipMemcpyAsync(p.filter, row_filter, (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess) { rc = -10; break; }
        const uint8_t *dfl = row_filter ? p.filter : nullptr;
        if ((rc = lex_passes(ix, p, uq, dfl, k1, b, sign, st, ls, ev, hs))) break;
        n_list = ls.n_list;
        if (na > 0) {
            if (hipMemcpyAsync(p.also, also.data(), (size_t)na * 8, hipMemcpyHostToDevice, st) != hipSuccess) { rc = -10; break; }
            k_lex_also<<<(na + 255) / 256, 256, 0, st>>>(p.also, na, n, ix.alive, dfl, p.match, p.mask, p.list + n_list, p.bm + n_list);
            if (hipGetLastError() != hipSuccess) { rc = -10; break; }
            n_list += na;
        }
        // hit leg: exact distances in slot space, combined score, top k by (NaN first, combined descending, id ascending)
        if (n_list > 0) {
            if ((rc = query_norms(p.dq, 1, ix.dim, p.dnb, st))) break;
            if ((rc = rerank(ix, p.dq, p.dnb, 1, (int)n_list, p.list, p.dkeys, p.oids, st))) break;
            k_lex_combine<<<(unsigned)((n_list + 255) / 256), 256, 0, st>>>(n_list, p.dkeys, p.bm, w_s, w_b, p.comb, p.ckeys);
            if (hipGetLastError() != hipSuccess) { rc = -10; break; }
            if ((rc = select_topk(p.ckeys, p.oids, nullptr, 1, n_list, k, p.skeys, p.sids, p.sel, st))) break;
            k_lex_emit<<<(unsigned)((n_list + 255) / 256), 256, 0, st>>>(n_list, p.ckeys, p.oids, p.comb, k, p.skeys, p.sids, p.out_comb);
            if (hipGetLastError() != hipSuccess) { rc = -10; break; }
        }
        if (ev && hipEventRecord(ev[3], st) != hipSuccess) { rc = -10; break; }
        // scan leg: the certified search over WHERE and not a hit -- the mask never leaves the device
        const bool masked = row_filter || n_list > 0;
        if ((rc = search_dev_locked(ix, p.dq, 1, k, AK_SEARCH_AUTO, masked ? p.mask : nullptr, p.scan_ids, p.scan_dist, p.cert, st))) break;
        if (ev && hipEventRecord(ev[4], st) != hipSuccess) { rc = -10; break; }
        if (lex_pin_reserve(ix, 4 * ob)) { rc = -10; break; }
        char *pin = ix.lex_pin;
        if (n_list > 0 && (hipMemcpyAsync(pin, p.sids, ob, hipMemcpyDeviceToHost, st) != hipSuccess ||
                           hipMemcpyAsync(pin + ob, p.out_comb, ob, hipMemcpyDeviceToHost, st) != hipSuccess)) { rc = -10; break; }
        if (hipMemcpyAsync(pin + 2 * ob, p.scan_ids, ob, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(pin + 3 * ob, p.scan_dist, ob, hipMemcpyDeviceToHost, st) != hipSuccess) { rc = -10; break; }
        if (hipStreamSynchronize(st) != hipSuccess) { rc = -10; break; }
        if (n_list > 0) {
            memcpy(out_hit_ids, pin, ob);
            memcpy(out_hit_combined, pin + ob, ob);
            int c = 0;
            while (c < k && out_hit_ids[c] >= 0) c++;
            *n_hit = c;
        }
        memcpy(out_scan_ids, pin + 2 * ob, ob);
        memcpy(out_scan_dist, pin + 3 * ob, ob);
        int c = 0;
        while (c < k && out_scan_ids[c] >= 0) c++;
        *n_scan = c;
    } while (0);
    if (rc) hipStreamSynchronize(st);          // nothing of a failed call may still be running on the workspace
    if (rc == -10) AK_FAIL(-10, std::string("ak_index_hybrid_search: HIP error: ") + hipGetErrorString(hipGetLastError()));
    if (rc) return rc;
    if (out_info) {
        out_info[0] = ls.n_live; out_info[1] = ls.sum_len; out_info[2] = ls.n_list; out_info[3] = n_list; out_info[4] = ls.T_used;
        out_info[5] = ix.lex_used;
        if (ev) {
            for (int i = 0; i < 4; i++) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) out_info[6 + i] = (int64_t)((double)ms * 1e6);
            }
        }
    }
    return 0;
}
