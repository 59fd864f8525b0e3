// lexical_batch.hip -- the hybrid query for a BATCH of queries (gfx950 only): one statistics pass over the lists, one host step,
// one score pass and one scan for up to 32 queries, beside the single-query kernels of lexical.hip, which stay as they are.
//
// The scan (scan.hip) takes ONE byte mask for all its queries, so the batch is evaluated the way also_ids rows are:
//   U        = every live row that passes the WHERE mask and holds a term of ANY query of the batch, plus the also rows
//   hit leg  : per query q the exact distance of EVERY row of U; bm_q = the single-query BM25 for rows holding a term of q and +0.0
//              for the rest of U; combined = (1.0 - d) w_s + bm_q w_b; best k by (NaN first, combined descending, id ascending)
//   scan leg : ONE certified search for all queries with mask = WHERE and not in U
// A row of U without a term of q gets (1.0 - d) w_s + 0.0 w_b in the hit leg, the expression the caller evaluates for a scan row:
// which leg such a row goes through cannot change its score, and the merged top k per query equals the single call's.
//
//   k_lex_stats_b    over ALL live rows, one wave per row: the union of the batch's distinct terms as ONE sorted table in LDS with
//                    a query bitmask (uint32: <= 32 queries) beside each term -> df per union term, n, sum of lengths, and per slot
//                    the uint32 of queries the row holds a term of. The arena is streamed once whatever the number of terms.
//   k_lex_compact_b  U -> a dense slot list with each row's query bits; the batch's scan mask; k_lex_also_b appends the also rows
//   host             avg and idf per union term with the C library's log (the one synchronisation of a sub-batch)
//   k_lex_score_b    one wave per listed row: the row's entries are read ONCE, their tfs parked in the wave's LDS line by union
//                    index; then per query whose bit is set the float64 sum of k_lex_score, operation for operation: surviving
//                    terms in that query's first-occurrence order from acc = 0.0, absent terms skipped, sign * acc at the end
//   hit leg          k_lex_spread -> rerank() (nq = G) -> k_lex_combine_b -> select_topk (nq = G) -> k_lex_emit_b
// LEX_BT_CAP terms fit the table: a batch whose union is larger, or that has more than 32 queries, runs as consecutive sub-batches;
// the [G][|U|] arrays of the hit leg are allocated after the host has read |U| and bounded by AK_LEX_BATCH_PAIRS pairs -- above it
// the hit leg (score pass included) runs in query groups while the statistics pass and the scan stay shared.
// No floating-point atomics: the float64 sums are per (row, query), in a fixed order, by one wave.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "index.h"
#include "switches.h"

namespace ak {

constexpr int LEX_BT_CAP = 2048;        // distinct terms of a sub-batch: the LDS table of the two passes
constexpr int LEX_BQ = 32;              // queries of a sub-batch: one bit each in a uint32
constexpr int LEXB_WAVES = 4;           // waves per workgroup

// position of `t` in the sorted table s_t[0, tu), or -1
__device__ inline int lexb_find(const uint32_t *s_t, int tu, uint32_t t) {
    int lo = 0, hi = tu;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_t[mid] < t) lo = mid + 1; else hi = mid;
    }
    return (lo < tu && s_t[lo] == t) ? lo : -1;
}

// ---- statistics pass -----------------------------------------------------------------------------------------------------
// uterm [tu] ascending, umask [tu]: bit q = query q of the sub-batch holds the term. counters: {n live, sum_len, list cursor,
// sum over listed rows of their number of queries}. match [n_slots]: the row's query bits (0 for a dead row).
__global__ __launch_bounds__(LEXB_WAVES * 64) void k_lex_stats_b(int64_t n_slots, const uint8_t *__restrict__ alive, const int64_t *__restrict__ off,
                                                                 const int32_t *__restrict__ cnt, const int32_t *__restrict__ len,
                                                                 const uint2 *__restrict__ arena, const uint32_t *__restrict__ uterm,
                                                                 const uint32_t *__restrict__ umask, int tu, unsigned int *__restrict__ df,
                                                                 unsigned long long *__restrict__ counters, uint32_t *__restrict__ match) {
    __shared__ uint32_t s_t[LEX_BT_CAP];
    __shared__ uint32_t s_m[LEX_BT_CAP];
    __shared__ unsigned int s_df[LEX_BT_CAP];
    __shared__ unsigned long long s_tot[2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t w0 = (int64_t)blockIdx.x * LEXB_WAVES + wave, wstride = (int64_t)gridDim.x * LEXB_WAVES;
    for (int i = threadIdx.x; i < tu; i += LEXB_WAVES * 64) { s_t[i] = uterm[i]; s_m[i] = umask[i]; s_df[i] = 0; }
    if (threadIdx.x < 2) s_tot[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long w_n = 0, w_len = 0;
    for (int64_t r = w0; r < n_slots; r += wstride) {
        if (!alive[r]) {                    // wave-uniform
            if (lane == 0) match[r] = 0u;
            continue;
        }
        const int m = cnt[r];
        const uint2 *e = arena + off[r];
        uint32_t bits = 0u;
        for (int i = lane * 2; i < m; i += 128) {
            const uint4 v = *(const uint4 *)(e + i);          // entries i, i + 1 of this row (the arena is padded past its end)
            int j = lexb_find(s_t, tu, v.x);
            if (j >= 0) { atomicAdd(&s_df[j], 1u); bits |= s_m[j]; }
            if (i + 1 < m) {
                j = lexb_find(s_t, tu, v.z);
                if (j >= 0) { atomicAdd(&s_df[j], 1u); bits |= s_m[j]; }
            }
        }
        // OR over the wave; the bits travel as unsigned (bit 31 is a query like any other)
        for (int o = 32; o > 0; o >>= 1) bits |= (uint32_t)__shfl_xor((int)bits, o);
        if (lane == 0) { w_n += 1; w_len += (unsigned long long)len[r]; match[r] = bits; }
    }
    if (lane == 0) { atomicAdd(&s_tot[0], w_n); atomicAdd(&s_tot[1], w_len); }
    __syncthreads();
    for (int i = threadIdx.x; i < tu; i += LEXB_WAVES * 64)
        if (s_df[i]) atomicAdd(&df[i], s_df[i]);
    if (threadIdx.x < 2 && s_tot[threadIdx.x]) atomicAdd(&counters[threadIdx.x], s_tot[threadIdx.x]);
}

// U in slot space: rows with a query bit that pass the WHERE mask, appended to `list` (the row slot in the low 32 bits, as rerank()
// reads it) with their bits in lbits; mask = WHERE and not in U, for the scan leg of the whole batch.
__global__ __launch_bounds__(256) void k_lex_compact_b(int64_t n_slots, const uint8_t *__restrict__ filter, const uint32_t *__restrict__ match,
                                                       uint64_t *__restrict__ list, uint32_t *__restrict__ lbits,
                                                       unsigned long long *__restrict__ counters, uint8_t *__restrict__ mask) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = r < n_slots;
    const bool pass = in && (!filter || filter[r]);
    const uint32_t bits = pass ? match[r] : 0u;
    const bool take = bits != 0u;
    const unsigned long long b = __ballot(take);
    if (b) {
        int nq_rows = __popc(bits);
        for (int o = 32; o > 0; o >>= 1) nq_rows += __shfl_xor(nq_rows, o);
        unsigned long long base = 0;
        const int leader = __ffsll((long long)b) - 1;
        if (lane == leader) {
            base = atomicAdd(&counters[2], (unsigned long long)__popcll(b));
            atomicAdd(&counters[3], (unsigned long long)nq_rows);
        }
        base = __shfl(base, leader);
        if (take) {
            const unsigned long long at = base + __popcll(b & ((1ull << lane) - 1ull));
            list[at] = (uint64_t)r;
            lbits[at] = bits;
        }
    }
    if (in) mask[r] = (pass && !take) ? 1 : 0;
}

// The batch's also rows join U with no query bit (BM25 +0.0 for every query) unless they are listed already. mask[s] == 1 says
// exactly that: the row passes the WHERE mask and is not in U. The host has dropped repeats.
__global__ void k_lex_also_b(const int64_t *__restrict__ also, int n_also, int64_t n_slots, const uint8_t *__restrict__ alive,
                             uint8_t *__restrict__ mask, uint64_t *__restrict__ list_tail, uint32_t *__restrict__ lbits_tail) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_also) return;
    const int64_t s = also[i];
    const bool ok = s >= 0 && s < n_slots && alive[s] && mask[s] == 1;
    list_tail[i] = ok ? (uint64_t)s : KEY_INVALID;
    lbits_tail[i] = 0u;
    if (ok) mask[s] = 0;
}

// ---- score pass -----------------------------------------------------------------------------------------------------------
// One wave per listed row, queries [q0, q1) of the sub-batch. uterm [tu] as above, uidf [tu] the idf by union index; query q's
// surviving terms (df > 0) in its first-occurrence order are the union indices qidx [qoff[q], qoff[q + 1]). The row's entries are
// read once and their tfs parked by union index in the wave's LDS line; per query, lane t evaluates term t's contribution and the
// contributions are added one by one in query order (chunks of 64), as k_lex_score does:
//   acc = acc + ((idf tf)(k1 + 1)) / (tf + k1 ((1 - b) + (b len) / avg)).
// bm [q1 - q0][stride]; +0.0 where the row has no term of the query (rows j >= n_scored, the also rows, have none at all).
__global__ __launch_bounds__(LEXB_WAVES * 64) void k_lex_score_b(int64_t n_rows, int64_t n_scored, int64_t stride, const uint64_t *__restrict__ list,
                                                                 const uint32_t *__restrict__ lbits, const int64_t *__restrict__ off,
                                                                 const int32_t *__restrict__ cnt, const int32_t *__restrict__ len,
                                                                 const uint2 *__restrict__ arena, const uint32_t *__restrict__ uterm, int tu,
                                                                 const double *__restrict__ uidf, const int32_t *__restrict__ qoff,
                                                                 const int32_t *__restrict__ qidx, int q0, int q1, double k1, double b,
                                                                 double avg, double sign, double *__restrict__ bm) {
    __shared__ uint32_t s_t[LEX_BT_CAP];
    __shared__ uint32_t s_tf[LEXB_WAVES][LEX_BT_CAP];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t w0 = (int64_t)blockIdx.x * LEXB_WAVES + wave, wstride = (int64_t)gridDim.x * LEXB_WAVES;
    for (int i = threadIdx.x; i < tu; i += LEXB_WAVES * 64) s_t[i] = uterm[i];
    __syncthreads();
    const double k1p = k1 + 1.0, omb = 1.0 - b;
    const int nqg = q1 - q0;
    const uint32_t gmask = (nqg >= 32 ? 0xffffffffu : ((1u << nqg) - 1u)) << q0;
    for (int64_t j = w0; j < n_rows; j += wstride) {
        const uint32_t bits = j < n_scored ? (lbits[j] & gmask) : 0u;       // wave-uniform
        if (bits == 0u) {
            if (lane < nqg) bm[(int64_t)lane * stride + j] = 0.0;
            continue;
        }
        const int64_t r = (int64_t)(uint32_t)list[j];
        const int m = cnt[r];
        const uint2 *e = arena + off[r];
        for (int i = lane; i < tu; i += 64) s_tf[wave][i] = 0u;
        __builtin_amdgcn_wave_barrier();
        for (int i = lane * 2; i < m; i += 128) {
            const uint4 v = *(const uint4 *)(e + i);
            int p = lexb_find(s_t, tu, v.x);
            if (p >= 0) s_tf[wave][p] = v.y;
            if (i + 1 < m) {
                p = lexb_find(s_t, tu, v.z);
                if (p >= 0) s_tf[wave][p] = v.w;
            }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);        // lgkmcnt(0): the wave's LDS writes have landed
        const double dl = (double)len[r];
        for (int q = q0; q < q1; q++) {
            if (!((bits >> q) & 1u)) {
                if (lane == 0) bm[(int64_t)(q - q0) * stride + j] = 0.0;
                continue;
            }
            const int t0 = qoff[q], t1 = qoff[q + 1];
            double acc = 0.0;
            for (int c = t0; c < t1; c += 64) {
                const bool have = c + lane < t1;
                const int ui = have ? qidx[c + lane] : 0;
                const uint32_t tfu = have ? s_tf[wave][ui] : 0u;
                const double my_idf = have ? uidf[ui] : 0.0;
                const double tf = (double)tfu;
                const double norm = avg > 0.0 ? tf + k1 * (omb + (b * dl) / avg) : tf + k1 * omb;
                const double contrib = ((my_idf * tf) * k1p) / norm;
                unsigned long long present = __ballot(tfu != 0u);
                while (present) {
                    const int t = __ffsll((long long)present) - 1;
                    present &= present - 1;
                    acc = acc + __shfl(contrib, t);
                }
            }
            if (lane == 0) bm[(int64_t)(q - q0) * stride + j] = sign * acc;
        }
        __builtin_amdgcn_wave_barrier();           // the line is zeroed for the next row only after every lane has read it
    }
}

// ---- hit leg over [G][L] -----------------------------------------------------------------------------------------------------
// every query of the group re-ranks the same rows: cand [g][j] = list [j]
__global__ void k_lex_spread(const uint64_t *__restrict__ list, int64_t L, int64_t total, uint64_t *__restrict__ cand) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    cand[t] = list[t % L];
}

// combined = (1.0 - d) w_s + bm w_b per (query, listed row); the selection key orders NaN first, then combined descending
// (select_topk breaks ties by ascending id) -- k_lex_combine over the flattened [G][L] arrays
__global__ void k_lex_combine_b(int64_t total, const uint64_t *__restrict__ dkeys, const double *__restrict__ bm, double w_s, double w_b,
                                double *__restrict__ comb, uint64_t *__restrict__ ckeys) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= total) return;
    const uint64_t dk = dkeys[j];
    if (dk == KEY_INVALID) { ckeys[j] = KEY_INVALID; comb[j] = 0.0; return; }
    const double d = key_dist(dk);
    const double c = (1.0 - d) * w_s + bm[j] * w_b;
    comb[j] = c;
    ckeys[j] = c != c ? 0ull : ~dist_key(c);
}

// the selected rows' combined scores as computed (the key does not tell -0.0 from 0.0); skeys / sids / out_comb [G][k]
__global__ void k_lex_emit_b(int64_t L, int64_t total, const uint64_t *__restrict__ ckeys, const int64_t *__restrict__ ids,
                             const double *__restrict__ comb, int k, const uint64_t *__restrict__ skeys, const int64_t *__restrict__ sids,
                             double *__restrict__ out_comb) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int64_t g = t / L;
    const uint64_t key = ckeys[t];
    const uint64_t *sk = skeys + g * k;
    if (key == KEY_INVALID || key > sk[k - 1]) return;
    const int64_t id = ids[t];
    for (int i = 0; i < k; i++)
        if (sk[i] == key && sids[g * k + i] == id) out_comb[g * k + i] = comb[t];
}

// ---- the batch query ----------------------------------------------------------------------------------------------------------
namespace {

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
unsigned lexb_grid(int64_t rows) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + LEXB_WAVES - 1) / LEXB_WAVES, 4096)); }

struct SubBatch {               // queries [first, first + nq) of the call and their union table
    int first = 0, nq = 0;
    std::vector<uint32_t> uterm, umask;
};

struct BatchPlan {              // the part of the workspace whose size is known before the passes (ix.ws_lex)
    uint32_t *match; uint8_t *mask, *filter;
    uint64_t *list; uint32_t *lbits;
    uint32_t *uterm, *umask; double *uidf; unsigned int *df; unsigned long long *counters;
    int32_t *qoff, *qidx;
    float *dq, *dnb; int *cert;
    uint64_t *skeys; int64_t *sids, *scan_ids, *also; double *out_comb, *scan_dist;
    size_t bytes;
};

BatchPlan batch_plan(char *base, int64_t n, int Q, int64_t n_qterms, int n_also, int k, int dim, bool with_filter) {
    BatchPlan p;
    size_t o = 0;
    auto take = [&](size_t b) { char *r = base ? base + o : nullptr; o += al256(b); return r; };
    const size_t L = (size_t)n + (size_t)n_also, qk = (size_t)Q * (size_t)k;
    p.match = (uint32_t *)take((size_t)n * 4); p.mask = (uint8_t *)take((size_t)n); p.filter = (uint8_t *)take(with_filter ? (size_t)n : 0);
    p.list = (uint64_t *)take(L * 8); p.lbits = (uint32_t *)take(L * 4);
    p.uterm = (uint32_t *)take(LEX_BT_CAP * 4); p.umask = (uint32_t *)take(LEX_BT_CAP * 4); p.uidf = (double *)take(LEX_BT_CAP * 8);
    p.df = (unsigned int *)take(LEX_BT_CAP * 4 + 32);       // df [cap] and, behind it, the four 64-bit counters: one memset, one copy back
    p.counters = (unsigned long long *)((char *)p.df + LEX_BT_CAP * 4);
    p.qoff = (int32_t *)take((LEX_BQ + 1) * 4); p.qidx = (int32_t *)take((size_t)std::max<int64_t>(n_qterms, 1) * 4);
    p.dq = (float *)take((size_t)Q * dim * 4); p.dnb = (float *)take((size_t)Q * 4); p.cert = (int *)take((size_t)Q * 4);
    p.skeys = (uint64_t *)take(qk * 8); p.sids = (int64_t *)take(qk * 8); p.out_comb = (double *)take(qk * 8);
    p.scan_ids = (int64_t *)take(qk * 8); p.scan_dist = (double *)take(qk * 8);
    p.also = (int64_t *)take((size_t)n_also * 8);
    p.bytes = o;
    return p;
}

struct PairPlan {               // the [G][L] arrays of the hit leg (ix.ws_lexb), sized after the host has read |U|
    uint64_t *cand, *dkeys, *ckeys; int64_t *oids; double *bm, *comb; void *sel;
    size_t bytes;
};

PairPlan pair_plan(char *base, int G, int64_t L, int k) {
    PairPlan p;
    size_t o = 0;
    auto take = [&](size_t b) { char *r = base ? base + o : nullptr; o += al256(b); return r; };
    const size_t pairs = (size_t)G * (size_t)L;
    p.cand = (uint64_t *)take(pairs * 8); p.dkeys = (uint64_t *)take(pairs * 8); p.ckeys = (uint64_t *)take(pairs * 8);
    p.oids = (int64_t *)take(pairs * 8); p.bm = (double *)take(pairs * 8); p.comb = (double *)take(pairs * 8);
    p.sel = take(select_scratch_bytes(G, L, std::max(k, 1)));
    p.bytes = o;
    return p;
}

struct BatchArgs {
    const float *queries; int nq; const std::vector<std::vector<uint32_t>> *uq;       // per query: distinct terms, first-occurrence order
    double k1, b, sign, w_s, w_b; const std::vector<int64_t> *also; const uint8_t *row_filter; int k;
    int64_t *out_hit_ids; double *out_hit_comb; int *n_hit; int64_t *out_scan_ids; double *out_scan_dist; int *n_scan;
    int64_t *info;              // int64[16], zeroed by the caller
};

// one sub-batch; the caller holds ix.mu (shared) and ix.lex_mu. p: the fixed workspace, the filter (if any) already in p.filter.
int run_sub_batch(Index &ix, const BatchArgs &a, const SubBatch &sb, BatchPlan &p, hipStream_t st, hipEvent_t *ev) {
    const int64_t n = ix.n;
    const int Q = sb.nq, k = a.k, tu = (int)sb.uterm.size(), na = (int)a.also->size();
    const uint8_t *dfl = a.row_filter ? p.filter : nullptr;
    const size_t dfb = (size_t)LEX_BT_CAP * 4 + 32;
    AK_HIP(hipMemcpyAsync(p.dq, a.queries + (size_t)sb.first * ix.dim, (size_t)Q * ix.dim * 4, hipMemcpyHostToDevice, st));
    AK_HIP(hipMemsetAsync(p.df, 0, dfb, st));
    if (ev) AK_HIP(hipEventRecord(ev[0], st));
    const bool lists = tu > 0 && ix.lex_used > 0;
    if (lists) {
        AK_HIP(hipMemcpyAsync(p.uterm, sb.uterm.data(), (size_t)tu * 4, hipMemcpyHostToDevice, st));
        AK_HIP(hipMemcpyAsync(p.umask, sb.umask.data(), (size_t)tu * 4, hipMemcpyHostToDevice, st));
        k_lex_stats_b<<<lexb_grid(n), LEXB_WAVES * 64, 0, st>>>(n, ix.alive, ix.lex_off, ix.lex_cnt, ix.lex_len, ix.lex_arena, p.uterm, p.umask, tu,
                                                                p.df, p.counters, p.match);
        a.info[10] += 1;
    } else {
        AK_HIP(hipMemsetAsync(p.match, 0, (size_t)n * 4, st));
    }
    AK_HIP(hipGetLastError());
    k_lex_compact_b<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(n, dfl, p.match, p.list, p.lbits, p.counters, p.mask);
    AK_HIP(hipGetLastError());
    if (ev) AK_HIP(hipEventRecord(ev[1], st));
    // the one small copy: df [cap] | n | sum_len | |U| | sum of |H_q|
    if (lex_pin_reserve(ix, std::max(dfb, (size_t)4 * Q * k * 8) + 4096)) return -10;
    AK_HIP(hipMemcpyAsync(ix.lex_pin, p.df, dfb, hipMemcpyDeviceToHost, st));
    AK_HIP(hipStreamSynchronize(st));
    const unsigned int *df = (const unsigned int *)ix.lex_pin;
    const unsigned long long *cn = (const unsigned long long *)(ix.lex_pin + (size_t)LEX_BT_CAP * 4);
    const int64_t n_live = (int64_t)cn[0], sum_len = (int64_t)cn[1];
    int64_t nU = (int64_t)cn[2];
    const int64_t sumH = (int64_t)cn[3];
    if (n_live == 0) nU = 0;
    double avg = 0.0;
    std::vector<double> uidf;
    std::vector<int32_t> qoff((size_t)LEX_BQ + 1, 0), qidx;
    int t_used = 0;
    if (nU > 0) {
        avg = (double)sum_len / (double)n_live;
        uidf.assign((size_t)tu, 0.0);
        for (int t = 0; t < tu; t++) {
            if (!df[t]) continue;                      // no live row holds it: the term drops out of every query
            const double d = (double)df[t];
            uidf[t] = log(1.0 + ((double)(n_live - (int64_t)df[t]) + 0.5) / (d + 0.5));
            t_used++;
        }
        for (int q = 0; q < Q; q++) {
            for (uint32_t term : (*a.uq)[(size_t)sb.first + q]) {
                const int ui = (int)(std::lower_bound(sb.uterm.begin(), sb.uterm.end(), term) - sb.uterm.begin());
                if (df[ui]) qidx.push_back(ui);
            }
            qoff[(size_t)q + 1] = (int32_t)qidx.size();
        }
        AK_HIP(hipMemcpyAsync(p.uidf, uidf.data(), (size_t)tu * 8, hipMemcpyHostToDevice, st));
        AK_HIP(hipMemcpyAsync(p.qoff, qoff.data(), qoff.size() * 4, hipMemcpyHostToDevice, st));
        if (!qidx.empty()) AK_HIP(hipMemcpyAsync(p.qidx, qidx.data(), qidx.size() * 4, hipMemcpyHostToDevice, st));
    }
    int64_t L = nU;
    if (na > 0) {
        AK_HIP(hipMemcpyAsync(p.also, a.also->data(), (size_t)na * 8, hipMemcpyHostToDevice, st));
        k_lex_also_b<<<(na + 255) / 256, 256, 0, st>>>(p.also, na, n, ix.alive, p.mask, p.list + nU, p.lbits + nU);
        AK_HIP(hipGetLastError());
        L += na;
    }
    // hit leg: exact distances of every row of U for every query, in groups of G queries whose [G][L] arrays fit the pair budget
    int rc = 0;
    if (L > 0) {
        if (L > 0x7fffffff) AK_FAIL(-1, "ak_index_hybrid_search_batch: more than 2^31 rows in the hit leg");
        const int64_t budget = std::max<int64_t>(1, switches().lex_batch_pairs.load(std::memory_order_relaxed));
        const int G = (int)std::max<int64_t>(1, std::min<int64_t>(Q, std::min<int64_t>(budget, 0x7fffffff) / L));
        if (ix.ws_lexb.reserve(pair_plan(nullptr, G, L, k).bytes)) return -10;
        PairPlan pp = pair_plan((char *)ix.ws_lexb.buf, G, L, k);
        if ((rc = query_norms(p.dq, Q, ix.dim, p.dnb, st))) return rc;
        for (int q0 = 0; q0 < Q; q0 += G) {
            const int g = std::min(G, Q - q0);
            const int64_t total = (int64_t)g * L;
            const unsigned tb = (unsigned)((total + 255) / 256);
            if (nU > 0) {
                k_lex_score_b<<<lexb_grid(L), LEXB_WAVES * 64, 0, st>>>(L, nU, L, p.list, p.lbits, ix.lex_off, ix.lex_cnt, ix.lex_len, ix.lex_arena,
                                                                        p.uterm, tu, p.uidf, p.qoff, p.qidx, q0, q0 + g, a.k1, a.b, avg, a.sign,
                                                                        pp.bm);
                AK_HIP(hipGetLastError());
                a.info[11] += 1;
            } else {
                AK_HIP(hipMemsetAsync(pp.bm, 0, (size_t)total * 8, st));
            }
            if (ev && q0 == 0) AK_HIP(hipEventRecord(ev[2], st));
            k_lex_spread<<<tb, 256, 0, st>>>(p.list, L, total, pp.cand);
            AK_HIP(hipGetLastError());
            if ((rc = rerank(ix, p.dq + (size_t)q0 * ix.dim, p.dnb + q0, g, (int)L, pp.cand, pp.dkeys, pp.oids, st))) return rc;
            k_lex_combine_b<<<tb, 256, 0, st>>>(total, pp.dkeys, pp.bm, a.w_s, a.w_b, pp.comb, pp.ckeys);
            AK_HIP(hipGetLastError());
            if ((rc = select_topk(pp.ckeys, pp.oids, nullptr, g, L, k, p.skeys + (size_t)q0 * k, p.sids + (size_t)q0 * k, pp.sel, st))) return rc;
            k_lex_emit_b<<<tb, 256, 0, st>>>(L, total, pp.ckeys, pp.oids, pp.comb, k, p.skeys + (size_t)q0 * k, p.sids + (size_t)q0 * k,
                                             p.out_comb + (size_t)q0 * k);
            AK_HIP(hipGetLastError());
            a.info[15] += total;
        }
    } else if (ev) {
        AK_HIP(hipEventRecord(ev[2], st));
    }
    if (ev) AK_HIP(hipEventRecord(ev[3], st));
    // scan leg: ONE certified search for the sub-batch over WHERE and not in U -- the mask never leaves the device
    const bool masked = a.row_filter || L > 0;
    if ((rc = search_dev_locked(ix, p.dq, Q, k, AK_SEARCH_AUTO, masked ? p.mask : nullptr, p.scan_ids, p.scan_dist, p.cert, st))) return rc;
    a.info[12] += 1;
    if (ev) AK_HIP(hipEventRecord(ev[4], st));
    const size_t ob = (size_t)Q * k * 8;
    char *pin = ix.lex_pin;
    if (L > 0) {
        AK_HIP(hipMemcpyAsync(pin, p.sids, ob, hipMemcpyDeviceToHost, st));
        AK_HIP(hipMemcpyAsync(pin + ob, p.out_comb, ob, hipMemcpyDeviceToHost, st));
    }
    AK_HIP(hipMemcpyAsync(pin + 2 * ob, p.scan_ids, ob, hipMemcpyDeviceToHost, st));
    AK_HIP(hipMemcpyAsync(pin + 3 * ob, p.scan_dist, ob, hipMemcpyDeviceToHost, st));
    AK_HIP(hipStreamSynchronize(st));
    const size_t o0 = (size_t)sb.first * k;
    if (L > 0) {
        memcpy(a.out_hit_ids + o0, pin, ob);
        memcpy(a.out_hit_comb + o0, pin + ob, ob);
    }
    memcpy(a.out_scan_ids + o0, pin + 2 * ob, ob);
    memcpy(a.out_scan_dist + o0, pin + 3 * ob, ob);
    for (int q = 0; q < Q; q++) {
        int c = 0;
        if (L > 0) while (c < k && a.out_hit_ids[o0 + (size_t)q * k + c] >= 0) c++;
        a.n_hit[sb.first + q] = c;
        c = 0;
        while (c < k && a.out_scan_ids[o0 + (size_t)q * k + c] >= 0) c++;
        a.n_scan[sb.first + q] = c;
    }
    a.info[0] = n_live; a.info[1] = sum_len; a.info[2] += nU; a.info[3] += L; a.info[4] += t_used; a.info[5] = ix.lex_used;
    a.info[13] += 1; a.info[14] += nU > 0 ? sumH : 0;
    if (ev) {
        for (int i = 0; i < 4; i++) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) a.info[6 + i] += (int64_t)((double)ms * 1e6);
        }
    }
    return 0;
}

// The call behind its argument checks; takes ix.mu (shared) for the whole call -- every sub-batch sees one state -- and ix.lex_mu.
int hybrid_batch(Index &ix, const BatchArgs &a, int64_t filter_len, uint64_t filter_epoch, const int64_t *also_ids, int64_t n_also) {
    const int k = a.k, nq = a.nq;
    std::shared_lock<std::shared_mutex> lk(ix.mu);
    if (int frc = filter_is_current(ix, a.row_filter, filter_len, filter_epoch, "ak_index_hybrid_search_batch")) return frc;
    const int64_t n = ix.n;
    if (n == 0) return 0;
    std::vector<int64_t> also;
    lex_also_slots(ix, also_ids, n_also, also);
    BatchArgs b = a;
    b.also = &also;
    // sub-batches: consecutive queries while they are <= 32 and their union fits the table; a query whose own terms do not fit
    // goes through the single-query passes (which take any number of terms)
    int cap = switches().lex_batch_terms.load(std::memory_order_relaxed);
    if (cap <= 0 || cap > LEX_BT_CAP) cap = LEX_BT_CAP;
    std::vector<SubBatch> subs;
    std::vector<int> alone;
    {
        std::map<uint32_t, uint32_t> uni;
        int first = 0, cnt = 0;
        auto close = [&](int next_first) {
            if (cnt > 0) {
                SubBatch sb;
                sb.first = first; sb.nq = cnt;
                for (auto &kv : uni) { sb.uterm.push_back(kv.first); sb.umask.push_back(kv.second); }
                subs.push_back(std::move(sb));
            }
            uni.clear(); cnt = 0; first = next_first;
        };
        for (int q = 0; q < nq; q++) {
            const std::vector<uint32_t> &t = (*a.uq)[q];
            if ((int)t.size() > cap) { close(q + 1); alone.push_back(q); continue; }
            size_t fresh = 0;
            for (uint32_t x : t) fresh += uni.count(x) ? 0 : 1;
            if (cnt == LEX_BQ || (int)(uni.size() + fresh) > cap) close(q);
            for (uint32_t x : t) uni[x] |= 1u << cnt;
            cnt++;
        }
        close(nq);
    }
    std::lock_guard<std::mutex> ql(ix.lex_mu);
    hipStream_t st;
    if (thread_stream(&st)) return -10;
    hipEvent_t *ev = lex_events(ix);
    int rc = 0;
    if (!subs.empty()) {
        int Qmax = 0;
        int64_t qterms = 0;
        for (const SubBatch &sb : subs) {
            Qmax = std::max(Qmax, sb.nq);
            int64_t s = 0;
            for (int q = 0; q < sb.nq; q++) s += (int64_t)(*a.uq)[(size_t)sb.first + q].size();
            qterms = std::max(qterms, s);
        }
        const size_t need = batch_plan(nullptr, n, Qmax, qterms, (int)also.size(), k, ix.dim, a.row_filter != nullptr).bytes;
        if (ix.ws_lex.reserve(need)) return -10;
        BatchPlan p = batch_plan((char *)ix.ws_lex.buf, n, Qmax, qterms, (int)also.size(), k, ix.dim, a.row_filter != nullptr);
        if (a.row_filter && hipMemcpyAsync(p.filter, a.row_filter, (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess) rc = -10;
        for (size_t i = 0; !rc && i < subs.size(); i++) rc = run_sub_batch(ix, b, subs[i], p, st, ev);
        if (rc) hipStreamSynchronize(st);          // nothing of a failed call may still be running on the workspace
        if (rc == -10) AK_FAIL(-10, std::string("ak_index_hybrid_search_batch: HIP error: ") + hipGetErrorString(hipGetLastError()));
        if (rc) return rc;
    }
    for (int q : alone) {       // after the sub-batches: the single-query passes lay the workspace out anew
        int64_t one[12];
        memset(one, 0, sizeof(one));
        const size_t o = (size_t)q * k;
        if ((rc = lex_hybrid_one(ix, a.queries + (size_t)q * ix.dim, (*a.uq)[q], a.k1, a.b, a.sign, a.w_s, a.w_b, also, a.row_filter, k,
                                 a.out_hit_ids + o, a.out_hit_comb + o, a.n_hit + q, a.out_scan_ids + o, a.out_scan_dist + o, a.n_scan + q, one)))
            return rc;
        a.info[0] = one[0]; a.info[1] = one[1]; a.info[2] += one[2]; a.info[3] += one[3]; a.info[4] += one[4]; a.info[5] = one[5];
        for (int i = 6; i < 10; i++) a.info[i] += one[i];
        a.info[10] += 1; a.info[11] += one[2] > 0 ? 1 : 0; a.info[12] += 1; a.info[14] += one[2]; a.info[15] += one[3];
    }
    return 0;
}

}  // namespace

// One group of same-keyed concurrent ak_index_hybrid_search calls (coalesce.h): a group of one runs the single-query call itself;
// a larger group is ONE batch call over the members' queries with their also lists united -- an extra row of U only changes the
// leg a row goes through, never its score.
void lex_hybrid_group(Index &ix, std::vector<HybridReq *> &g) {
    if (g.size() == 1) {
        HybridReq &r = *g[0];
        r.rc = lex_hybrid_single(ix, r);
        if (r.rc) r.err = ak_last_error();
        return;
    }
    const HybridReq &h = *g[0];
    const int nq = (int)g.size(), k = h.k, dim = ix.dim;
    std::vector<float> q((size_t)nq * dim);
    std::vector<std::vector<uint32_t>> uq((size_t)nq);
    std::vector<int64_t> also;
    int rc = 0;
    for (int i = 0; i < nq && !rc; i++) {
        memcpy(q.data() + (size_t)i * dim, g[i]->q, (size_t)dim * 4);
        rc = lex_unique_terms(g[i]->terms, g[i]->T, uq[i], "ak_index_hybrid_search");
        also.insert(also.end(), g[i]->also, g[i]->also + g[i]->n_also);
    }
    std::vector<int64_t> hi((size_t)nq * k, -1), si((size_t)nq * k, -1);
    std::vector<double> hc((size_t)nq * k, 0.0), sd((size_t)nq * k, 0.0);
    std::vector<int> nh((size_t)nq, 0), ns((size_t)nq, 0);
    int64_t info[16];
    memset(info, 0, sizeof(info));
    if (!rc) {
        BatchArgs a{q.data(), nq, &uq, h.k1, h.b, h.sign, h.w_s, h.w_b, nullptr, h.filter, k,
                    hi.data(), hc.data(), nh.data(), si.data(), sd.data(), ns.data(), info};
        rc = hybrid_batch(ix, a, h.flen, h.fepoch, also.data(), (int64_t)also.size());
    }
    const std::string err = rc ? std::string(ak_last_error()) : std::string();
    for (int i = 0; i < nq; i++) {
        HybridReq &r = *g[i];
        r.rc = rc;
        if (rc) { r.err = err; continue; }
        const size_t o = (size_t)i * k;
        memcpy(r.out_hit_ids, hi.data() + o, (size_t)nh[i] * 8);
        memcpy(r.out_hit_comb, hc.data() + o, (size_t)nh[i] * 8);
        memcpy(r.out_scan_ids, si.data() + o, (size_t)k * 8);
        memcpy(r.out_scan_dist, sd.data() + o, (size_t)k * 8);
        *r.n_hit = nh[i]; *r.n_scan = ns[i];
        if (r.out_info) {       // of the shared launch, not of this request alone
            for (int j = 0; j < 10; j++) r.out_info[j] = info[j];
            r.out_info[10] = nq; r.out_info[11] = 0;
        }
    }
}

}  // namespace ak

using namespace ak;

extern "C" {

int ak_index_hybrid_search_batch(ak_index_t h, const float *queries, int nq, const int64_t *term_offsets, const int32_t *terms, double k1,
                                 double b, double sign, double w_s, double w_b, const int64_t *also_ids, int64_t n_also,
                                 const uint8_t *row_filter, int64_t filter_len, uint64_t filter_epoch, int k, int64_t *out_hit_ids,
                                 double *out_hit_combined, int *n_hit, int64_t *out_scan_ids, double *out_scan_dist, int *n_scan,
                                 int64_t *out_info) {
    AK_BIND();
    if (!h) AK_FAIL(-1, "ak_index_hybrid_search_batch: NULL index");
    Index &ix = *(Index *)h;
    int64_t info[16];
    memset(info, 0, sizeof(info));
    if (out_info) memset(out_info, 0, sizeof(info));
    if (!queries || nq < 1 || !term_offsets || k <= 0 || k > 4096 || !out_hit_ids || !out_hit_combined || !n_hit || !out_scan_ids ||
        !out_scan_dist || !n_scan || n_also < 0 || n_also > (1 << 24) || (n_also > 0 && !also_ids) || term_offsets[0] != 0)
        AK_FAIL(-1, "ak_index_hybrid_search_batch: bad arguments");
    std::vector<std::vector<uint32_t>> uq((size_t)nq);
    for (int q = 0; q < nq; q++) {
        const int64_t lo = term_offsets[q], hi = term_offsets[q + 1];
        if (hi < lo || hi - lo > 0x7fffffff) AK_FAIL(-1, "ak_index_hybrid_search_batch: bad term_offsets");
        if (int rc = lex_unique_terms(terms ? terms + lo : nullptr, (int)(hi - lo), uq[q], "ak_index_hybrid_search_batch")) return rc;
        n_hit[q] = 0; n_scan[q] = 0;
    }
    RoctxRange range("ak_index_hybrid_search_batch");
    BatchArgs a{queries, nq, &uq, k1, b, sign, w_s, w_b, nullptr, row_filter, k,
                out_hit_ids, out_hit_combined, n_hit, out_scan_ids, out_scan_dist, n_scan, info};
    const int rc = hybrid_batch(ix, a, filter_len, filter_epoch, also_ids, n_also);
    if (!rc && out_info) memcpy(out_info, info, sizeof(info));
    return rc;
}

}  // extern "C"
