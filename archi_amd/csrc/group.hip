// group.hip -- grouped search behind ak_index_group_search (include/archi_knn.h): the k nearest GROUPS of rows (documents) and the
// best rows (chunks) of each. No counterpart in the reference's store, whose callers collapse the retriever's k chunks by document
// on the host. The searches themselves are the index's own (search_dev_locked); the kernels here work on what they return.
//
//   stage A, which groups -- exact by the prefix property: a certified search returns exactly the first k' rows of the query's
//   complete list, so the distinct groups among them, in order of first appearance, are the first groups of the true ranking.
//     k_group_collapse   one wave per query: the group keys at the returned rows' slots -> first occurrences, in list order,
//                        appended to the query's winners table (key, representative slot) and to the results (the representative
//                        is the group's best row: its id and the search's own distance).
//     k_group_exclude    later rounds of a query that still misses groups: one pass over the slots, mask = caller's filter AND
//                        "group not among the winners" (a negative key is a group of one row: "slot not among the winners'").
//   stage B, the members (group_size > 1):
//     k_group_members    one pass over the slots per query: live AND filter AND key >= 0 AND key among the query's winners (sorted
//                        in LDS, binary search). Run twice: COUNT (one global add per wave), then, the host having sized the list
//                        from the counts, FILL (wave-level compaction: prefix sum over the lanes' match counts, one global add per
//                        wave for the wave's range). Nothing is truncated: a list always has room for every match, and a query
//                        batch whose lists would not fit a budget is cut into smaller batches.
//     k_group_dist<DT>   exact_distance (exact_arith.h: the search's own arithmetic) of every listed (query, row).
//     k_group_select     one workgroup per (query, winner): the best group_size listed rows of that winner by (distance key, id),
//                        one block-wide minimum per row returned.
//
// The slot passes read 16 slots per thread with 16-byte loads (4 x int4 of keys, one uint4 of each byte column) and write 16 mask
// bytes with one 16-byte store; a thread whose 16 slots cross the end of the arrays walks them one by one.
#include "exact_arith.h"
#include "index.h"

namespace ak {

constexpr int GP_THREADS = 256, GP_PER = 16;
constexpr int GROUP_Q_SHIFT = 37, GROUP_W_SHIFT = 32;        // list entry: query << 37 | winner << 32 | slot

// The query's winners with a key >= 0, sorted by key into s_key / s_idx (winner index); the slots of the winners with a negative
// key into s_neg. Called by every thread of the workgroup; returns through *m / *mneg after a barrier.
__device__ inline void load_winners(const int32_t *__restrict__ wkey, const int32_t *__restrict__ wslot, int cnt, int32_t *s_raw,
                                    int32_t *s_key, int32_t *s_idx, int32_t *s_neg, int *s_m) {
    const int t = threadIdx.x;
    if (t < GROUP_MAX_K) s_raw[t] = t < cnt ? wkey[t] : -1;
    __syncthreads();
    if (t < GROUP_MAX_K) {
        const bool valid = t < cnt && s_raw[t] >= 0;
        const uint32_t mine = valid ? (uint32_t)s_raw[t] : 0x80000000u + (uint32_t)t;
        int rank = 0, nvalid = 0, negrank = 0;
#pragma unroll 1
        for (int j = 0; j < GROUP_MAX_K; j++) {
            const bool vj = j < cnt && s_raw[j] >= 0;
            const uint32_t other = vj ? (uint32_t)s_raw[j] : 0x80000000u + (uint32_t)j;
            rank += other < mine;
            nvalid += vj;
            negrank += (j < cnt && !vj && j < t);
        }
        s_key[rank] = valid ? s_raw[t] : INT32_MAX;          // the invalid ones rank behind every valid one: the padding
        s_idx[rank] = t;
        if (!valid && t < cnt) s_neg[negrank] = wslot[t];
        if (t == 0) { s_m[0] = nvalid; s_m[1] = cnt - nvalid; }
    }
    __syncthreads();
}

// Branch-free lower bound over the 32 sorted entries (s_key is padded with INT32_MAX behind the m valid ones): the winner index of
// `key`, or -1. Five selects, no divergence among the lanes of a wave.
__device__ inline int find_winner(const int32_t *s_key, const int32_t *s_idx, int m, int32_t key) {
    int pos = 0;
#pragma unroll
    for (int step = GROUP_MAX_K / 2; step >= 1; step >>= 1) pos += s_key[pos + step - 1] < key ? step : 0;
    return (pos < m && s_key[pos] == key) ? s_idx[pos] : -1;
}

__global__ __launch_bounds__(256) void k_group_init(int64_t *__restrict__ rid, double *__restrict__ rdist, int32_t *__restrict__ rgroup,
                                                    int *__restrict__ rsizes, int *__restrict__ wcnt, unsigned long long *__restrict__ mcnt,
                                                    int64_t rows, int64_t groups, int nq) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows) { rid[i] = -1; rdist[i] = __builtin_nan(""); }
    if (i < groups) { rgroup[i] = -1; rsizes[i] = 0; }
    if (i < nq) { wcnt[i] = 0; mcnt[i] = 0ull; }
}

// One wave per query (blockIdx.x + q0). sids / sdist / slots: the query's row of the search's output, [fetch] each; a slot < 0 ends
// the list. Appends first occurrences to the winners table until it holds k groups.
__global__ __launch_bounds__(WAVE) void k_group_collapse(const int32_t *__restrict__ keys, int q0, int fetch, int k, int g,
                                                         const int64_t *__restrict__ sids, const double *__restrict__ sdist,
                                                         const int *__restrict__ slots, int32_t *__restrict__ wkey,
                                                         int32_t *__restrict__ wslot, int *__restrict__ wcnt, int64_t *__restrict__ rid,
                                                         double *__restrict__ rdist, int32_t *__restrict__ rgroup, int *__restrict__ rsizes) {
    __shared__ int32_t s_k[GROUP_MAX_FETCH], s_s[GROUP_MAX_FETCH];
    const int q = q0 + blockIdx.x, lane = threadIdx.x;
    const int64_t so = (int64_t)q * fetch;
    const int base = wcnt[q];
    int32_t *wk = wkey + (int64_t)q * GROUP_MAX_K, *wsl = wslot + (int64_t)q * GROUP_MAX_K;
    for (int r = lane; r < GROUP_MAX_FETCH; r += WAVE) {
        const int s = r < fetch ? slots[so + r] : -1;
        s_s[r] = s;
        s_k[r] = s >= 0 ? keys[s] : 0;
    }
    __syncthreads();
    bool first[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int r = lane + h * WAVE;
        const int s = s_s[r], key = s_k[r];
        bool f = s >= 0;
        if (f && key >= 0) {
            for (int j = 0; j < r && f; j++) f = !(s_s[j] >= 0 && s_k[j] == key);
            for (int j = 0; j < base && f; j++) f = wk[j] != key;
        } else if (f) {
            for (int j = 0; j < base && f; j++) f = !(wk[j] < 0 && wsl[j] == s);
        }
        first[h] = f;
    }
    const unsigned long long b0 = __ballot(first[0]), b1 = __ballot(first[1]);
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    const int n0 = __popcll(b0);
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int r = lane + h * WAVE;
        const int pos = base + (h ? n0 + __popcll(b1 & below) : __popcll(b0 & below));
        if (first[h] && pos < k) {
            wk[pos] = s_k[r];
            wsl[pos] = s_s[r];
            const int64_t o = ((int64_t)q * k + pos) * g;
            rid[o] = sids[so + r];
            rdist[o] = sdist[so + r];
            rgroup[(int64_t)q * k + pos] = s_k[r];
            rsizes[(int64_t)q * k + pos] = 1;
        }
    }
    if (lane == 0) {
        const int total = base + n0 + __popcll(b1);
        wcnt[q] = total < k ? total : k;
    }
}

// mask[s] = (filter ? filter[s] : 1) AND the slot's group is not among the query's winners. One query.
__global__ __launch_bounds__(GP_THREADS) void k_group_exclude(const int32_t *__restrict__ keys, const uint8_t *__restrict__ filter,
                                                               int64_t n, const int32_t *__restrict__ wkey,
                                                               const int32_t *__restrict__ wslot, const int *__restrict__ wcnt,
                                                               uint8_t *__restrict__ mask) {
    __shared__ int32_t s_raw[GROUP_MAX_K], s_key[GROUP_MAX_K], s_idx[GROUP_MAX_K], s_neg[GROUP_MAX_K];
    __shared__ int s_m[2];
    load_winners(wkey, wslot, wcnt[0], s_raw, s_key, s_idx, s_neg, s_m);
    const int m = s_m[0], mneg = s_m[1];
    const int64_t base = ((int64_t)blockIdx.x * GP_THREADS + threadIdx.x) * GP_PER;
    if (base >= n) return;
    auto keep = [&](int64_t s, int32_t key) -> bool {      // both tests for every slot: no divergence
        const bool in_key = find_winner(s_key, s_idx, m, key) >= 0;
        bool in_slot = false;
        for (int j = 0; j < mneg; j++) in_slot |= (int64_t)(uint32_t)s_neg[j] == s;
        return key >= 0 ? !in_key : !in_slot;
    };
    if (base + GP_PER <= n) {
        int32_t kk[GP_PER];
        uint8_t ff[GP_PER];
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const int4 x = *(const int4 *)(keys + base + 4 * v);
            kk[4 * v] = x.x; kk[4 * v + 1] = x.y; kk[4 * v + 2] = x.z; kk[4 * v + 3] = x.w;
        }
        uint4 f = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
        if (filter) f = *(const uint4 *)(filter + base);
        __builtin_memcpy(ff, &f, 16);
#pragma unroll
        for (int j = 0; j < GP_PER; j++) ff[j] = (ff[j] && keep(base + j, kk[j])) ? 1 : 0;
        uint4 o;
        __builtin_memcpy(&o, ff, 16);
        *(uint4 *)(mask + base) = o;
    } else {
        for (int64_t s = base; s < n; s++) mask[s] = ((!filter || filter[s]) && keep(s, keys[s])) ? 1 : 0;
    }
}

// The members pass of query q0 + blockIdx.y. COUNT: mcnt[q] += matches. FILL: entries go to list[off[q] ..), at most mcnt[q] of them
// (a match beyond that -- the two passes saw different data, which one hold of the reader lock excludes -- raises *overflow and is
// not written).
template <bool FILL>
__global__ __launch_bounds__(GP_THREADS) void k_group_members(const int32_t *__restrict__ keys, const uint8_t *__restrict__ filter,
                                                               const uint8_t *__restrict__ alive, int64_t n, int q0,
                                                               const int32_t *__restrict__ wkey, const int32_t *__restrict__ wslot,
                                                               const int *__restrict__ wcnt, unsigned long long *__restrict__ mcnt,
                                                               unsigned long long *__restrict__ cursor, const int64_t *__restrict__ off,
                                                               uint64_t *__restrict__ list, int *__restrict__ overflow) {
    __shared__ int32_t s_raw[GROUP_MAX_K], s_key[GROUP_MAX_K], s_idx[GROUP_MAX_K], s_neg[GROUP_MAX_K];
    __shared__ int s_m[2];
    const int q = q0 + blockIdx.y;
    load_winners(wkey + (int64_t)q * GROUP_MAX_K, wslot + (int64_t)q * GROUP_MAX_K, wcnt[q], s_raw, s_key, s_idx, s_neg, s_m);
    const int m = s_m[0];
    if (m == 0) return;                                   // the whole workgroup: only single-row groups, nothing to list
    const int64_t base = ((int64_t)blockIdx.x * GP_THREADS + threadIdx.x) * GP_PER;
    int8_t win[GP_PER];
    int c = 0;
#pragma unroll
    for (int j = 0; j < GP_PER; j++) win[j] = -1;
    if (base + GP_PER <= n) {
        int32_t kk[GP_PER];
        uint8_t ff[GP_PER], aa[GP_PER];
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const int4 x = *(const int4 *)(keys + base + 4 * v);
            kk[4 * v] = x.x; kk[4 * v + 1] = x.y; kk[4 * v + 2] = x.z; kk[4 * v + 3] = x.w;
        }
        uint4 f = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
        if (filter) f = *(const uint4 *)(filter + base);
        const uint4 a = *(const uint4 *)(alive + base);
        __builtin_memcpy(ff, &f, 16);
        __builtin_memcpy(aa, &a, 16);
#pragma unroll
        for (int j = 0; j < GP_PER; j++) {
            const int w = find_winner(s_key, s_idx, m, kk[j]);
            win[j] = (int8_t)((aa[j] && ff[j] && kk[j] >= 0) ? w : -1);
            c += win[j] >= 0;
        }
    } else {
        for (int j = 0; j < GP_PER && base + j < n; j++) {
            const int64_t s = base + j;
            if (alive[s] && (!filter || filter[s]) && keys[s] >= 0) {
                const int w = find_winner(s_key, s_idx, m, keys[s]);
                win[j] = (int8_t)w;
                c += w >= 0;
            }
        }
    }
    // wave-level compaction: inclusive prefix sum of the lanes' match counts, one global add per wave
    const int lane = threadIdx.x & (WAVE - 1);
    int incl = c;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    const int total = __shfl(incl, WAVE - 1);
    if (total == 0) return;
    if (!FILL) {
        if (lane == 0) atomicAdd(mcnt + q, (unsigned long long)total);
        return;
    }
    unsigned long long start = 0;
    if (lane == 0) start = atomicAdd(cursor + q, (unsigned long long)total);
    start = __shfl(start, 0);
    unsigned long long at = start + (unsigned long long)(incl - c);
    const unsigned long long cap = mcnt[q];
    uint64_t *dst = list + off[q];
#pragma unroll
    for (int j = 0; j < GP_PER; j++)
        if (win[j] >= 0) {
            if (at < cap) dst[at] = ((uint64_t)q << GROUP_Q_SHIFT) | ((uint64_t)win[j] << GROUP_W_SHIFT) | (uint64_t)(uint32_t)(base + j);
            else *overflow = 1;
            at++;
        }
}

// Exact distance key and id of every list entry.
template <int DT>
__global__ __launch_bounds__(256) void k_group_dist(const typename Store<DT>::T *__restrict__ rows, const float *__restrict__ na,
                                                    const int64_t *__restrict__ ids, int dim, int metric,
                                                    const float *__restrict__ queries, const float *__restrict__ nb,
                                                    const uint64_t *__restrict__ list, int64_t total, uint64_t *__restrict__ ekey,
                                                    int64_t *__restrict__ eid) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const uint64_t x = list[e];
    const int64_t r = (int64_t)(uint32_t)x;
    const int q = (int)(x >> GROUP_Q_SHIFT);
    const double d = exact_distance<DT>(rows + r * (int64_t)dim, queries + (int64_t)q * dim, dim, metric, na[r], nb[q]);
    ekey[e] = dist_key(d);
    eid[e] = ids[r];
}

// Workgroup (w, q0 + blockIdx.y): the best g entries of winner w in the query's list by (distance key, id). Row j is the smallest
// pair above row j - 1's: ids are unique, so pairs are.
__global__ __launch_bounds__(256) void k_group_select(int q0, int k, int g, const int32_t *__restrict__ wkey, const int *__restrict__ wcnt,
                                                      const unsigned long long *__restrict__ mcnt, const int64_t *__restrict__ off,
                                                      const uint64_t *__restrict__ list, const uint64_t *__restrict__ ekey,
                                                      const int64_t *__restrict__ eid, int64_t *__restrict__ rid,
                                                      double *__restrict__ rdist, int *__restrict__ rsizes) {
    __shared__ uint64_t s_bk[4];
    __shared__ int64_t s_bi[4];
    const int w = blockIdx.x, q = q0 + blockIdx.y, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    if (w >= wcnt[q] || wkey[(int64_t)q * GROUP_MAX_K + w] < 0) return;
    const int64_t o = off[q], cnt = (int64_t)mcnt[q];
    uint64_t pk = 0;
    int64_t pi = INT64_MIN;
    bool have_prev = false;
    int found = 0;
    for (int j = 0; j < g; j++) {
        uint64_t bk = KEY_INVALID;
        int64_t bi = INT64_MAX;
        for (int64_t e = tid; e < cnt; e += 256) {
            if ((int)((list[o + e] >> GROUP_W_SHIFT) & 31) != w) continue;
            const uint64_t key = ekey[o + e];
            const int64_t id = eid[o + e];
            if (have_prev && !(key > pk || (key == pk && id > pi))) continue;
            if (key < bk || (key == bk && id < bi)) { bk = key; bi = id; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint64_t ok = __shfl_xor(bk, d);
            const int64_t oi = __shfl_xor(bi, d);
            if (ok < bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; }
        }
        __syncthreads();                                  // the previous round's reads of s_bk / s_bi are done
        if (lane == 0) { s_bk[wave] = bk; s_bi[wave] = bi; }
        __syncthreads();
        bk = s_bk[0]; bi = s_bi[0];
#pragma unroll
        for (int v = 1; v < 4; v++)
            if (s_bk[v] < bk || (s_bk[v] == bk && s_bi[v] < bi)) { bk = s_bk[v]; bi = s_bi[v]; }
        if (bk == KEY_INVALID) break;                     // the same value in every thread
        if (tid == 0) {
            rid[((int64_t)q * k + w) * g + j] = bi;
            rdist[((int64_t)q * k + w) * g + j] = key_dist(bk);
        }
        pk = bk; pi = bi; have_prev = true;
        found++;
    }
    if (tid == 0 && found > 0) rsizes[(int64_t)q * k + w] = found;
}

static inline size_t group_al(size_t x) { return (x + 255) & ~(size_t)255; }

GroupWs group_layout(void *base, int nq, int k, int g, int fetch, int64_t n, int dim, bool has_filter) {
    GroupWs w;
    char *p = (char *)base;
    size_t o = 0;
    const size_t n16 = ((size_t)n + 15) & ~(size_t)15, nf = (size_t)nq * fetch, nw = (size_t)nq * GROUP_MAX_K;
    w.q = (float *)(p + o); o += group_al((size_t)nq * dim * 4);
    w.nb = (float *)(p + o); o += group_al((size_t)nq * 4);
    w.sids = (int64_t *)(p + o); o += group_al(nf * 8);
    w.sdist = (double *)(p + o); o += group_al(nf * 8);
    w.scert = (int *)(p + o); o += group_al((size_t)nq * 4);
    w.slots = (int *)(p + o); o += group_al(nf * 4);
    w.keys = (int32_t *)(p + o); o += group_al(n16 * 4);
    w.filter = has_filter ? (uint8_t *)(p + o) : nullptr; o += has_filter ? group_al(n16) : 0;
    w.mask = (uint8_t *)(p + o); o += group_al(n16);
    w.wkey = (int32_t *)(p + o); o += group_al(nw * 4);
    w.wslot = (int32_t *)(p + o); o += group_al(nw * 4);
    w.wcnt = (int *)(p + o); o += group_al((size_t)nq * 4);
    w.mcnt = (unsigned long long *)(p + o); o += group_al((size_t)nq * 8);
    w.cursor = (unsigned long long *)(p + o); o += group_al((size_t)nq * 8);
    w.off = (int64_t *)(p + o); o += group_al((size_t)nq * 8);
    w.overflow = (int *)(p + o); o += 256;
    w.rid = (int64_t *)(p + o); o += group_al((size_t)nq * k * g * 8);
    w.rdist = (double *)(p + o); o += group_al((size_t)nq * k * g * 8);
    w.rgroup = (int32_t *)(p + o); o += group_al((size_t)nq * k * 4);
    w.rsizes = (int *)(p + o); o += group_al((size_t)nq * k * 4);
    w.bytes = o;
    return w;
}

// ak_index_profile: one event pair per kernel launch, appended to the index's list behind the scan's (ak_index_profile_read)
static int group_prof_pair(Index &ix, hipEvent_t *a, hipEvent_t *b) {
    *a = *b = nullptr;
    std::lock_guard<std::mutex> lk(ix.prof_mu);
    if (!ix.profile) return 0;
    if (ix.prof_used == ix.prof_events.size()) {
        hipEvent_t x, y;
        AK_HIP(hipEventCreate(&x));
        AK_HIP(hipEventCreate(&y));
        ix.prof_events.emplace_back(x, y);
    }
    *a = ix.prof_events[ix.prof_used].first;
    *b = ix.prof_events[ix.prof_used].second;
    ix.prof_used++;
    return 0;
}

int group_init(const GroupWs &w, int nq, int k, int g, hipStream_t st) {
    const int64_t rows = (int64_t)nq * k * g;
    k_group_init<<<(unsigned)((rows + 255) / 256), 256, 0, st>>>(w.rid, w.rdist, w.rgroup, w.rsizes, w.wcnt, w.mcnt, rows, (int64_t)nq * k, nq);
    AK_HIP(hipGetLastError());
    return 0;
}

int group_collapse(Index &ix, const GroupWs &w, int q0, int nqr, int fetch, int k, int g, hipStream_t st) {
    if (nqr <= 0) return 0;
    if (fetch < 1 || fetch > GROUP_MAX_FETCH || k < 1 || k > GROUP_MAX_K) AK_FAIL(-1, "group_collapse: fetch / k out of range");
    hipEvent_t a, b;
    if (group_prof_pair(ix, &a, &b)) return -10;
    if (a) AK_HIP(hipEventRecord(a, st));
    k_group_collapse<<<nqr, WAVE, 0, st>>>(w.keys, q0, fetch, k, g, w.sids, w.sdist, w.slots, w.wkey, w.wslot, w.wcnt, w.rid, w.rdist,
                                           w.rgroup, w.rsizes);
    AK_HIP(hipGetLastError());
    if (b) AK_HIP(hipEventRecord(b, st));
    return 0;
}

static unsigned slot_blocks(int64_t n) { return (unsigned)((n + (int64_t)GP_THREADS * GP_PER - 1) / ((int64_t)GP_THREADS * GP_PER)); }

int group_exclude(Index &ix, const GroupWs &w, int q, int64_t n, hipStream_t st) {
    hipEvent_t a, b;
    if (group_prof_pair(ix, &a, &b)) return -10;
    if (a) AK_HIP(hipEventRecord(a, st));
    k_group_exclude<<<slot_blocks(n), GP_THREADS, 0, st>>>(w.keys, w.filter, n, w.wkey + (int64_t)q * GROUP_MAX_K,
                                                           w.wslot + (int64_t)q * GROUP_MAX_K, w.wcnt + q, w.mask);
    AK_HIP(hipGetLastError());
    if (b) AK_HIP(hipEventRecord(b, st));
    return 0;
}

// Stage B for every query. reserve(bytes): a device buffer that stays valid until its next call. *matched: rows listed, summed over the queries.
int group_members(Index &ix, const GroupWs &w, int nq, int k, int g, int64_t n, const std::function<void *(size_t)> &reserve, hipStream_t st, int64_t *matched) {
    *matched = 0;
    if (nq <= 0 || g <= 1 || n <= 0) return 0;
    if (n > 0xffffffffll) AK_FAIL(-1, "group_members: more than 2^32 row slots");
    hipEvent_t a, b;
    if (query_norms(w.q, nq, ix.dim, w.nb, st)) return -10;
    if (group_prof_pair(ix, &a, &b)) return -10;
    if (a) AK_HIP(hipEventRecord(a, st));
    for (int q0 = 0; q0 < nq; q0 += 65535) {               // gridDim.y
        const int qc = std::min(nq - q0, 65535);
        k_group_members<false><<<dim3(slot_blocks(n), qc), GP_THREADS, 0, st>>>(w.keys, w.filter, ix.alive, n, q0, w.wkey, w.wslot, w.wcnt,
                                                                                  w.mcnt, nullptr, nullptr, nullptr, nullptr);
        AK_HIP(hipGetLastError());
    }
    if (b) AK_HIP(hipEventRecord(b, st));
    std::vector<unsigned long long> cnt((size_t)nq);
    std::vector<int64_t> off((size_t)nq);
    AK_HIP(hipMemcpyAsync(cnt.data(), w.mcnt, (size_t)nq * 8, hipMemcpyDeviceToHost, st));
    AK_HIP(hipStreamSynchronize(st));
    // batches of consecutive queries whose lists fit the budget together; one query's list always fits (it has its own batch)
    const int64_t budget = 1ll << 22;
    for (int q0 = 0; q0 < nq;) {
        int64_t total = 0;
        int q1 = q0;
        while (q1 < nq && q1 - q0 < 65535 && (q1 == q0 || total + (int64_t)cnt[q1] <= budget)) { off[q1] = total; total += (int64_t)cnt[q1]; q1++; }
        if (total > 0) {
            const size_t lb = group_al((size_t)total * 8);
            char *blk = (char *)reserve(3 * lb);
            if (!blk) return -10;
            uint64_t *list = (uint64_t *)blk, *ekey = (uint64_t *)(blk + lb);
            int64_t *eid = (int64_t *)(blk + 2 * lb);
            AK_HIP(hipMemcpyAsync(w.off + q0, off.data() + q0, (size_t)(q1 - q0) * 8, hipMemcpyHostToDevice, st));
            AK_HIP(hipMemsetAsync(w.cursor + q0, 0, (size_t)(q1 - q0) * 8, st));
            AK_HIP(hipMemsetAsync(w.overflow, 0, 4, st));
            if (group_prof_pair(ix, &a, &b)) return -10;
            if (a) AK_HIP(hipEventRecord(a, st));
            k_group_members<true><<<dim3(slot_blocks(n), q1 - q0), GP_THREADS, 0, st>>>(w.keys, w.filter, ix.alive, n, q0, w.wkey, w.wslot,
                                                                                          w.wcnt, w.mcnt, w.cursor, w.off, list, w.overflow);
            AK_HIP(hipGetLastError());
            if (b) AK_HIP(hipEventRecord(b, st));
            const unsigned db = (unsigned)((total + 255) / 256);
#define LAUNCH(DT)                                                                                                                      \
    k_group_dist<DT><<<db, 256, 0, st>>>((const Store<DT>::T *)ix.rows, ix.na, ix.ids, ix.dim, ix.metric, w.q, w.nb, list, total, ekey, eid)
            if (ix.dtype == AK_DTYPE_F32) LAUNCH(AK_DTYPE_F32);
            else if (ix.dtype == AK_DTYPE_BF16) LAUNCH(AK_DTYPE_BF16);
            else LAUNCH(AK_DTYPE_F16);
#undef LAUNCH
            AK_HIP(hipGetLastError());
            k_group_select<<<dim3(k, q1 - q0), 256, 0, st>>>(q0, k, g, w.wkey, w.wcnt, w.mcnt, w.off, list, ekey, eid, w.rid, w.rdist, w.rsizes);
            AK_HIP(hipGetLastError());
            int over = 0;
            AK_HIP(hipMemcpyAsync(&over, w.overflow, 4, hipMemcpyDeviceToHost, st));
            AK_HIP(hipStreamSynchronize(st));              // `off` (pageable) was a copy's source; the list is reused by the next batch
            if (over) AK_FAIL(-1, "group_members: the fill pass matched more rows than the count pass");
            *matched += total;
        }
        q0 = q1;
    }
    return 0;
}

}  // namespace ak
