// mmr.hip -- max-marginal-relevance selection over the candidates of one search (ak_index_mmr_search, include/archi_knn.h).
// No counterpart in the reference's store: the method follows LangChain's VectorStore contract [upstream, not in tree]. Two
// kernels behind the candidate search:
//
//   k_mmr_gram<DT>   the float32 accumulator of exact_distance's chain for every candidate pair i < j of a query: the two STORED
//                    rows, element order, one rounding per multiply and per add, no contraction (exact_arith.h: the same load8 /
//                    exact_finish as the search's own distances).
//   k_mmr_select     one wave per query: finishes pairs to float64 on the fly and runs the greedy pick of the header's rule 3.
//
// k_mmr_gram is fed the way k_rerank_panel (exact.hip) is fed. The pair set of a query is the upper triangle of a
// fetch_k x fetch_k matrix, cut into 32 x 32 rank blocks (bi <= bj; 10 blocks at fetch_k = 128); one 256-thread workgroup per
// (block, query), so a single query with 128 candidates -- 8 128 chains of `dim` steps -- spreads over 10 CUs. The workgroup
// stages the 32 rows of rank block bi and the 32 of bj (the same rows twice on a diagonal block) panel by panel, 128 bytes of a row
// per panel, with coalesced 16-byte loads: 8 neighbouring lanes take the 128 contiguous bytes of one row, every thread two pieces
// (one of an A row, one of a B row), issued one panel ahead of the chains and parked in registers. Lane (ty, tx) = (tid / 16,
// tid % 16) owns the 2 x 2 pairs {ty, ty + 16} x {tx, tx + 16} of the block: four accumulators in registers across all panels,
// each walked in element order.
//
// LDS image and conflicts (MI355X: 64 banks of 4 bytes; a wave's ds_read_b128 is served in four groups of 16 lanes, and each of the
// four groups -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 -- holds ALL 16 values of lane % 16 = tx and two values
// of ty). Image row stride MG_STRIDE = 128 + 16 bytes = 36 dwords.
//   B rows (image rows 32 + tx, then 48 + tx): 16 lanes of a group read 16 different rows at dword offsets 36 tx mod 64 =
//     {0, 36, 8, 44, 16, 52, 24, 60, 32, 4, 40, 12, 48, 20, 56, 28}: 16 distinct multiples of 4, each read 4 dwords wide -> the 64
//     banks once each, conflict-free. (Owning columns {2 tx, 2 tx + 1} instead would put rows 72 dwords apart: tx and tx + 8 on
//     the same banks, 2-way. A 128-byte stride would put all 16 rows on banks 0-3.)
//   A rows (image rows ty, then ty + 16): a group reads two rows (16 lanes each the same address: broadcast), 36 dwords apart ->
//     banks 0-3 and 36-39, conflict-free.
//   An A read and a B read are separate instructions, so the two row sets never meet in one access.
//   Stores (ds_write_b128, groups of 8 contiguous lanes): the 8 lanes of a group write the 128 contiguous bytes of ONE image row ->
//     32 consecutive dwords, conflict-free.
// LDS footprint: two images (the loader writes panel p + 1 while the chains read panel p: one workgroup barrier per panel) of
// 64 rows x 144 B = 9 216 B each + 64 slot numbers = 18 688 B per workgroup. 160 KiB per CU / 18 688 B = 8 workgroups = 32 waves,
// the CU's wave limit (8 per SIMD) -- LDS does not cap occupancy; the register count (<= 64 VGPRs for 8 waves per SIMD) does, see
// DESIGN.md.
//
// Any dim the index accepts: dim % 8 == 0 (rows are then 16-byte aligned and a multiple of 16 bytes long) takes the 16-byte loads,
// the last panel may be partial; every other dim stages element by element with scalar loads, as exact_distance falls back. The
// chains read the image the same way on both paths. Any m from 0 to fetch_k: a rank >= m loads the row of rank 0 instead (never
// used), no slot number of an invalid rank is ever read, and blocks without a valid pair leave before the first barrier.
#include "exact_arith.h"
#include "index.h"

namespace ak {

#pragma clang fp contract(off)

constexpr int MG_THREADS = 256;
constexpr int MG_BLK = 32;                            // ranks per block side
constexpr int MG_ROWS = 2 * MG_BLK;                   // image rows: block bi's 32, then block bj's 32
constexpr int MG_ROWB = 128;                          // panel bytes per row: 64 elements (16-bit) / 32 (f32)
constexpr int MG_STRIDE = MG_ROWB + 16;               // + one chunk: see the conflict analysis above
constexpr int MG_IMAGE = MG_ROWS * MG_STRIDE;         // 9 216 B

__host__ __device__ inline int64_t mmr_tri(int i, int j, int fk) {      // i < j < fk
    return (int64_t)i * fk - (int64_t)i * (i + 1) / 2 + (j - i - 1);
}

template <int DT>
__device__ inline void mg_chains8(const typename Store<DT>::T *a0, const typename Store<DT>::T *a1, const typename Store<DT>::T *b0,
                                  const typename Store<DT>::T *b1, int i, float (&acc)[2][2]) {
    float va0[8], va1[8], vb0[8], vb1[8];
    load8<DT>(a0, i, va0);
    load8<DT>(a1, i, va1);
    load8<DT>(b0, i, vb0);
    load8<DT>(b1, i, vb1);
#pragma unroll
    for (int e = 0; e < 8; e++) {
        acc[0][0] = __fadd_rn(acc[0][0], __fmul_rn(va0[e], vb0[e]));
        acc[0][1] = __fadd_rn(acc[0][1], __fmul_rn(va0[e], vb1[e]));
        acc[1][0] = __fadd_rn(acc[1][0], __fmul_rn(va1[e], vb0[e]));
        acc[1][1] = __fadd_rn(acc[1][1], __fmul_rn(va1[e], vb1[e]));
    }
}

template <int DT>
__global__ __launch_bounds__(MG_THREADS) void k_mmr_gram(const typename Store<DT>::T *__restrict__ rows, int dim, int fk,
                                                         const int *__restrict__ slots, const int *__restrict__ cnt,
                                                         float *__restrict__ accs) {
    using S = Store<DT>;
    using T = typename S::T;
    constexpr int ES = (int)sizeof(T), PW = MG_ROWB / ES;                 // panel width in elements
    __shared__ __attribute__((aligned(16))) char s_img[2][MG_IMAGE];
    __shared__ int s_slot[MG_ROWS];
    const int qi = blockIdx.y, tid = threadIdx.x;
    int m = cnt[qi];
    m = m < fk ? m : fk;
    // blockIdx.x -> (bi, bj), bi <= bj, row-major over the upper triangle of the nb x nb block matrix
    const int nb = (fk + MG_BLK - 1) / MG_BLK;
    int bi = 0, left = blockIdx.x;
    while (left >= nb - bi) { left -= nb - bi; bi++; }
    const int bj = bi + left;
    // block-uniform exits, before any barrier: no column of the block is valid, or a diagonal block with a single valid rank
    if (m < 2 || bj * MG_BLK >= m || (bi == bj && m - bi * MG_BLK < 2)) return;
    if (tid < MG_ROWS) {
        const int rank = (tid < MG_BLK ? bi * MG_BLK : bj * MG_BLK - MG_BLK) + tid;
        s_slot[tid] = slots[(int64_t)qi * fk + (rank < m ? rank : 0)];     // rank 0 is valid (m >= 2); nothing is read at rank >= m
    }
    __syncthreads();
    const int tx = tid & 15, ty = tid >> 4;
    const bool vec = dim % 8 == 0;                                         // exact_distance's test; rows start on 16 bytes then
    const int npanels = (dim + PW - 1) / PW;
    // loader role (16-byte path): piece (tid % 8) of image rows tid / 8 (an A row) and 32 + tid / 8 (a B row)
    const int lrow = tid >> 3, piece = tid & 7;
    const char *ga = (const char *)rows + (int64_t)(uint32_t)s_slot[lrow] * dim * ES;
    const char *gb = (const char *)rows + (int64_t)(uint32_t)s_slot[MG_BLK + lrow] * dim * ES;
    uint4 pa = {0, 0, 0, 0}, pb = {0, 0, 0, 0};
    // the two pieces of panel P, in flight while the chains of panel P - 1 run. Pieces past the row's end (partial last panel)
    // re-read piece 0 of the panel: landed in the image, never read by a chain
#define MG_ISSUE(P)                                                                \
    do {                                                                           \
        const int nch_ = (dim - (P) * PW) * ES / 16;                               \
        const int off_ = (P) * MG_ROWB + (piece < nch_ ? piece : 0) * 16;          \
        pa = *(const uint4 *)(ga + off_);                                          \
        pb = *(const uint4 *)(gb + off_);                                          \
    } while (0)
    if (vec) MG_ISSUE(0);
    float acc[2][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
    for (int p = 0; p < npanels; p++) {
        char *img = s_img[p & 1];
        const int pe = dim - p * PW < PW ? dim - p * PW : PW;             // elements of this panel
        if (vec) {
            *(uint4 *)(img + lrow * MG_STRIDE + piece * 16) = pa;
            *(uint4 *)(img + (MG_BLK + lrow) * MG_STRIDE + piece * 16) = pb;
        } else {
            for (int idx = tid; idx < MG_ROWS * pe; idx += MG_THREADS) {
                const int ir = idx / pe, e = idx - ir * pe;
                ((T *)(img + ir * MG_STRIDE))[e] = rows[(int64_t)(uint32_t)s_slot[ir] * dim + p * PW + e];
            }
        }
        // one barrier per panel: this image was last read two panels ago, and every thread has passed the barrier of the panel
        // in between since
        __syncthreads();
        if (vec && p + 1 < npanels) MG_ISSUE(p + 1);
        const T *a0 = (const T *)(img + ty * MG_STRIDE), *a1 = (const T *)(img + (ty + 16) * MG_STRIDE);
        const T *b0 = (const T *)(img + (MG_BLK + tx) * MG_STRIDE), *b1 = (const T *)(img + (MG_BLK + 16 + tx) * MG_STRIDE);
        if (pe == PW) {
#pragma unroll
            for (int i = 0; i < PW; i += 8) mg_chains8<DT>(a0, a1, b0, b1, i, acc);
        } else {
            int i = 0;
            for (; i + 8 <= pe; i += 8) mg_chains8<DT>(a0, a1, b0, b1, i, acc);
            for (; i < pe; i++) {
                const float x0 = S::load(a0, i), x1 = S::load(a1, i), y0 = S::load(b0, i), y1 = S::load(b1, i);
                acc[0][0] = __fadd_rn(acc[0][0], __fmul_rn(x0, y0));
                acc[0][1] = __fadd_rn(acc[0][1], __fmul_rn(x0, y1));
                acc[1][0] = __fadd_rn(acc[1][0], __fmul_rn(x1, y0));
                acc[1][1] = __fadd_rn(acc[1][1], __fmul_rn(x1, y1));
            }
        }
    }
#undef MG_ISSUE
    float *out = accs + (int64_t)qi * ((int64_t)fk * (fk - 1) / 2);
#pragma unroll
    for (int ea = 0; ea < 2; ea++)
#pragma unroll
        for (int eb = 0; eb < 2; eb++) {
            const int i = bi * MG_BLK + ty + 16 * ea, j = bj * MG_BLK + tx + 16 * eb;
            if (i < j && j < m) out[mmr_tri(i, j, fk)] = acc[ea][eb];
        }
}

// One wave per query; lane l owns ranks l and l + 64. Everything a round needs of the pick (its slot's norm) travels by shuffle.
__global__ __launch_bounds__(WAVE) void k_mmr_select(const float *__restrict__ na, const int64_t *__restrict__ ids, int fk, int k,
                                                     double lam, const int *__restrict__ slots, const double *__restrict__ dq,
                                                     const int *__restrict__ cnt, const float *__restrict__ accs,
                                                     int64_t *__restrict__ oid, double *__restrict__ od, int *__restrict__ ork) {
    const int qi = blockIdx.x, lane = threadIdx.x;
    int m = cnt[qi];
    m = m < fk ? m : fk;
    const int picks = k < m ? k : m;
    const double oml = __dsub_rn(1.0, lam);
    const float *tri = accs + (int64_t)qi * ((int64_t)fk * (fk - 1) / 2);
    const double NEG_INF = -__builtin_inf();
    int slot[2];
    float nr[2];
    double d[2], sq[2], red[2];
    bool open[2];                                      // valid and not picked yet
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const int r = lane + 64 * e;
        open[e] = r < m;
        slot[e] = open[e] ? slots[(int64_t)qi * fk + r] : 0;
        nr[e] = open[e] ? na[(uint32_t)slot[e]] : 0.0f;
        d[e] = open[e] ? dq[(int64_t)qi * fk + r] : __builtin_nan("");
        sq[e] = __dsub_rn(1.0, d[e]);
        red[e] = NEG_INF;
    }
    int p = 0;
    for (int t = 0; t < picks; t++) {
        if (t > 0) {
            // argmax of score over the open ranks: strict >, the lowest rank wins a tie, a NaN never wins
            bool has = false;
            double bs = 0.0;
            int br = 0x7fffffff, lo = 0x7fffffff;     // lo: the lowest open rank, for the round in which every score is NaN
#pragma unroll
            for (int e = 0; e < 2; e++) {
                if (!open[e]) continue;
                const int r = lane + 64 * e;
                lo = r < lo ? r : lo;
                const double sc = __dsub_rn(__dmul_rn(lam, sq[e]), __dmul_rn(oml, red[e]));
                if (sc == sc && (!has || sc > bs)) { has = true; bs = sc; br = r; }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const int ohas = __shfl_xor((int)has, off), orr = __shfl_xor(br, off), olo = __shfl_xor(lo, off);
                const double os = __shfl_xor(bs, off);
                if (ohas && (!has || os > bs || (os == bs && orr < br))) { has = true; bs = os; br = orr; }
                lo = olo < lo ? olo : lo;
            }
            p = has ? br : lo;
        }
        const int pe = p >> 6, pl = p & 63;            // wave-uniform
        const int pslot = __shfl(pe ? slot[1] : slot[0], pl);
        const float pn = __shfl(pe ? nr[1] : nr[0], pl);
        const double pd = __shfl(pe ? d[1] : d[0], pl);
        if (lane == 0) {
            oid[(int64_t)qi * k + t] = ids[(uint32_t)pslot];
            od[(int64_t)qi * k + t] = pd;
            ork[(int64_t)qi * k + t] = p;
        }
        if (lane == pl) open[pe] = false;
#pragma unroll
        for (int e = 0; e < 2; e++) {
            if (!open[e]) continue;
            const int r = lane + 64 * e;
            const float a = tri[r < p ? mmr_tri(r, p, fk) : mmr_tri(p, r, fk)];
            const double s = __dsub_rn(1.0, exact_finish(a, AK_METRIC_COSINE, nr[e], pn));
            if (s > red[e]) red[e] = s;                // a NaN never updates
        }
    }
    for (int t = picks + lane; t < k; t += WAVE) {
        oid[(int64_t)qi * k + t] = -1;
        od[(int64_t)qi * k + t] = __builtin_nan("");
        ork[(int64_t)qi * k + t] = -1;
    }
}

#pragma clang fp contract(fast)

static inline size_t mmr_al(size_t x) { return (x + 255) & ~(size_t)255; }

MmrWs mmr_layout(void *base, int nq, int k, int fetch_k) {
    MmrWs w;
    char *p = (char *)base;
    size_t o = 0;
    w.slots = (int *)(p + o); o += mmr_al((size_t)nq * fetch_k * 4);
    w.acc = (float *)(p + o); o += mmr_al((size_t)nq * ((size_t)fetch_k * (fetch_k - 1) / 2) * 4 + 4);
    w.ids = (int64_t *)(p + o); o += mmr_al((size_t)nq * k * 8);
    w.dist = (double *)(p + o); o += mmr_al((size_t)nq * k * 8);
    w.rank = (int *)(p + o); o += mmr_al((size_t)nq * k * 4);
    w.bytes = o;
    return w;
}

// ak_index_profile: one event pair per kernel, appended to the index's list behind the scan's (ak_index_profile_read)
static int mmr_prof_pair(Index &ix, hipEvent_t *a, hipEvent_t *b) {
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

int mmr_run(Index &ix, int nq, int k, int fetch_k, double lambda_mult, const double *dq_dev, const int *cnt_dev, const MmrWs &w,
            hipStream_t st) {
    if (nq <= 0) return 0;
    if (k < 1 || fetch_k < k || fetch_k > MMR_MAX_FETCH) AK_FAIL(-1, "mmr: 1 <= k <= fetch_k <= 128");
    if (ix.metric != AK_METRIC_COSINE) AK_FAIL(-1, "mmr: cosine indexes only");
    hipEvent_t g0, g1, s0, s1;
    if (mmr_prof_pair(ix, &g0, &g1) || mmr_prof_pair(ix, &s0, &s1)) return -10;
    const int nb = (fetch_k + MG_BLK - 1) / MG_BLK, nblk = nb * (nb + 1) / 2;
    const int64_t tri = (int64_t)fetch_k * (fetch_k - 1) / 2;
    if (g0) AK_HIP(hipEventRecord(g0, st));
    if (fetch_k > 1)
        for (int q0 = 0; q0 < nq; q0 += 65535) {          // gridDim.y
            const int qc = nq - q0 < 65535 ? nq - q0 : 65535;
#define LAUNCH(DT)                                                                                                              \
    k_mmr_gram<DT><<<dim3(nblk, qc), MG_THREADS, 0, st>>>((const Store<DT>::T *)ix.rows, ix.dim, fetch_k,                          \
                                                           w.slots + (int64_t)q0 * fetch_k, cnt_dev + q0, w.acc + (int64_t)q0 * tri)
            if (ix.dtype == AK_DTYPE_F32) LAUNCH(AK_DTYPE_F32);
            else if (ix.dtype == AK_DTYPE_BF16) LAUNCH(AK_DTYPE_BF16);
            else LAUNCH(AK_DTYPE_F16);
#undef LAUNCH
            AK_HIP(hipGetLastError());
        }
    if (g1) AK_HIP(hipEventRecord(g1, st));
    if (s0) AK_HIP(hipEventRecord(s0, st));
    k_mmr_select<<<nq, WAVE, 0, st>>>(ix.na, ix.ids, fetch_k, k, lambda_mult, w.slots, dq_dev, cnt_dev, w.acc, w.ids, w.dist, w.rank);
    AK_HIP(hipGetLastError());
    if (s1) AK_HIP(hipEventRecord(s1, st));
    return 0;
}

}  // namespace ak
