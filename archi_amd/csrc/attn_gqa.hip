// attn_gqa.hip -- bidirectional grouped-query flash attention at head size 256 with an optional band (EmbeddingGemma, gemma.hip):
//   ctx[t][h * 256 + d] = sum_{s' visible} softmax_s'(q_h[s] . k_g[s']) v_g[s'][d],   g = h / (nq / nkv)
// key s' is visible to query s iff s' < len (the row's length) and, in a sliding layer with half-window w, |s - s'| <= w.
// q arrives pre-scaled by log2(e) * query_pre_attn_scalar^-0.5 (gemma.hip k_gm_qk_norm_rope), so the softmax runs in the base-2 domain.
//
// Layouts (k_gm_qk_norm_rope writes them): q [B][nq][S][256], k [B][nkv][S][256], v TRANSPOSED [B][nkv][256][S] with the keys of every
// 16-group in vt_pos order (what attn_long.hip takes); ctx [T][nq * 256] bf16 (the out-projection's A operand). Rows are right-padded;
// lens[b] is the row's length, clamped to [0, S] by the embedding kernel.
//
// Workgroup = (query block, kv head, sequence) and holds every query head of the group, as attn_causal.hip: wave v computes query head
// g = v % G of the group for the 32 query rows q0 = block * 32 R + 32 (v / G), R = 4 / G for G = 1, 2, 4 (four waves) and 1 for G = 3
// (three waves, 192 threads: the model's layout). Each 32-key block of K and V^T is staged ONCE for all G heads and R row blocks, through
// two LDS buffers as attn_long.hip: block kb + 1 is loaded into registers under block kb's MFMAs and written to the other buffer behind
// them (one barrier per block). Per wave and key block:
//   S^T = K Q^T    16 x v_mfma_f32_32x32x16_bf16: A = K (rows = keys, from LDS), B = Q^T (64 VGPRs held for the whole loop). Keys on M:
//                  a lane owns ONE query and 16 of the 32 keys (the other 16 in lane ^ 32): row max and sum take one cross-lane step.
//   mask           -inf on the keys past the row's length and outside the band, only in the blocks that straddle either edge
//   online softmax in base 2 (running max / sum; a block in which a query sees no key leaves them unchanged)
//   O^T += V^T P^T 16 MFMAs: A = V^T rows (d) from LDS, B = P^T straight from the S^T accumulators; the 256 x 32 O^T tile is 128 accumulators.
// A lane holds 64 (q) + 128 (O^T) + 16 (scores) + 32-48 (the block in flight) registers: one wave per SIMD (__launch_bounds__(256) gives
// the compiler the 512 unified registers of a lane).
// The band walk is k_attn_long<true>'s: a workgroup stages only the key blocks that intersect [q_begin - w, q_end - 1 + w] below the
// row's length, and a wave skips the blocks wholly outside the band of its own 32 queries. Query rows at or past the length get zero
// context rows; query blocks wholly past it are not computed.
// K tile [32 keys][256 d]: 512-byte rows, 16-byte chunk c of key r at c ^ (r & 7); V^T tile [256 d][32 keys]: 64-byte rows, chunk c of row
// d at c ^ ((d >> 1) & 3) (the XOR swizzles of attn_causal.hip). LDS per workgroup: 65 536 bytes (2 x 16 KB K, 2 x 16 KB V^T).
#include "encoder_kernels.h"
#include "mfma_tile.h"

namespace ak {
using namespace mt;

namespace {
constexpr int GA_HD = 256;
constexpr int GA_K_BYTES = 32 * GA_HD * 2, GA_V_BYTES = GA_HD * 64, GA_CHUNKS = 1024;      // 16-byte chunks of a K tile and of a V^T tile

template <int G, bool WIN>
__global__ __launch_bounds__(256) void k_attn_gqa(GqaAttnArgs a) {
    constexpr int R = G == 3 ? 1 : 4 / G, QR = 32 * R, NTHR = 64 * G * R, NCH = (GA_CHUNKS + NTHR - 1) / NTHR;
    __shared__ __attribute__((aligned(16))) char sK[2][GA_K_BYTES];
    __shared__ __attribute__((aligned(16))) char sV[2][GA_V_BYTES];
    const int kvh = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = wave % G, j = wave / G, h = kvh * G + g;
    const int S = a.S;
    const int len = min(max(a.lens[b], 0), S);
    const int q_begin = blockIdx.x * QR, q0 = q_begin + 32 * j;
    const int r = lane & 31, kh = lane >> 5;
    const int ldc = a.nq * GA_HD;
    const bool has_q = q0 < S;                                 // this wave's 32 rows exist (S % 32 == 0)
    const bool live = has_q && q0 < len;                       // ... and hold a valid query
    uint16_t *ctx_row = a.ctx + ((int64_t)b * S + (has_q ? q0 + r : 0)) * ldc + h * GA_HD;
    if (has_q && !live) {                                      // wholly past the length: zero rows
        for (int c = kh; c < GA_HD / 8; c += 2) *(uint4 *)(ctx_row + c * 8) = uint4{0, 0, 0, 0};
    }
    if (q_begin >= len) return;                                // (uniform over the workgroup: no barrier below is skipped by some waves only)
    int q_end = q_begin + QR;
    if (q_end > S) q_end = S;
    int kb_stop = (len + 31) / 32, kb_start = 0;
    if constexpr (WIN) {
        kb_start = max(q_begin - a.window, 0) / 32;            // q_begin < len: block q_begin / 32 is inside [kb_start, kb_stop)
        kb_stop = min(kb_stop, (q_end - 1 + a.window) / 32 + 1);
    }
    // staging: chunk i = tid + n NTHR of the K tile is (key i / 32, chunk i % 32), of the V^T tile (row d = i / 4, chunk i % 4)
    const uint16_t *kg = a.k + ((int64_t)b * a.nkv + kvh) * S * GA_HD;
    const uint16_t *vg = a.vt + ((int64_t)b * a.nkv + kvh) * GA_HD * S;
    // (scalars, not arrays: the compiler kept kreg[NCH] / vreg[NCH] in scratch)
    uint4 kr0, kr1, kr2, kr3, kr4, kr5, vr0, vr1, vr2, vr3, vr4, vr5;
    static_assert(NCH <= 6, "staging registers");
#define GA_LOAD1(n_, kr_, vr_, kb_)                                                                                 \
    if constexpr ((n_) < NCH) {                                                                                     \
        const int i = tid + (n_) * NTHR;                                                                            \
        if (GA_CHUNKS % NTHR == 0 || i < GA_CHUNKS) {                                                               \
            kr_ = *(const uint4 *)(kg + (int64_t)(kb_) * 32 * GA_HD + (int64_t)i * 8);                              \
            vr_ = *(const uint4 *)(vg + (int64_t)(i >> 2) * S + (kb_) * 32 + (i & 3) * 8);                          \
        }                                                                                                           \
    }
#define GA_STORE1(n_, kr_, vr_, buf_)                                                                               \
    if constexpr ((n_) < NCH) {                                                                                     \
        const int i = tid + (n_) * NTHR;                                                                            \
        if (GA_CHUNKS % NTHR == 0 || i < GA_CHUNKS) {                                                               \
            const int key = i >> 5, c = i & 31, d = i >> 2, vc = i & 3;                                             \
            *(uint4 *)(sK[buf_] + key * 512 + ((c ^ (key & 7)) << 4)) = kr_;                                        \
            *(uint4 *)(sV[buf_] + d * 64 + ((vc ^ ((d >> 1) & 3)) << 4)) = vr_;                                     \
        }                                                                                                           \
    }
#define GA_LOAD_BLOCK(kb_) GA_LOAD1(0, kr0, vr0, kb_) GA_LOAD1(1, kr1, vr1, kb_) GA_LOAD1(2, kr2, vr2, kb_) GA_LOAD1(3, kr3, vr3, kb_) \
    GA_LOAD1(4, kr4, vr4, kb_) GA_LOAD1(5, kr5, vr5, kb_)
#define GA_STORE_BLOCK(buf_) GA_STORE1(0, kr0, vr0, buf_) GA_STORE1(1, kr1, vr1, buf_) GA_STORE1(2, kr2, vr2, buf_) GA_STORE1(3, kr3, vr3, buf_) \
    GA_STORE1(4, kr4, vr4, buf_) GA_STORE1(5, kr5, vr5, buf_)
    GA_LOAD_BLOCK(kb_start)
    GA_STORE_BLOCK(kb_start & 1)                                // LDS buffers go by block parity

    // this lane's query: 16 chunks of 16 bytes (d = 16 c + 8 kh .. + 7), the B operand of every S^T MFMA
    uint4 qf[16];
    {
        const int qrow = live ? q0 + r : 0;
        const uint16_t *qp = a.q + (((int64_t)b * a.nq + h) * S + qrow) * GA_HD + kh * 8;
#pragma unroll
        for (int c = 0; c < 16; c++) qf[c] = *(const uint4 *)(qp + c * 16);
    }
    f32x16 o[8];
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    __syncthreads();
    for (int kb = kb_start; kb < kb_stop; kb++) {
        const int cur = kb & 1;
        const bool more = kb + 1 < kb_stop;
        if (more) { GA_LOAD_BLOCK(kb + 1) }                        // next block into registers: in flight under this block's MFMAs
        // the block against this wave's queries q0 .. q0 + 31 (wave-uniform): dk_hi / dk_lo = largest key - query / query - key
        const int dk_hi = kb * 32 + 31 - q0, dk_lo = q0 + 31 - kb * 32;
        const bool in_band = !WIN || (dk_hi - 62 <= a.window && dk_lo - 62 <= a.window);      // some (query, key) pair is visible
        if (live && in_band) {
            const char *k_t = sK[cur], *v_t = sV[cur];
            f32x16 s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 16; c++) {
                const uint4 ka = *(const uint4 *)(k_t + r * 512 + (((2 * c + kh) ^ (r & 7)) << 4));
                s = mfma_bf16(ka, qf[c], s);
            }
            // accumulator i: key kb * 32 + 8 (i / 4) + 4 kh + i % 4 of this lane's query
            const bool band_edge = WIN && (dk_hi > a.window || dk_lo > a.window);
            if (band_edge || kb * 32 + 32 > len) {             // an edge block: the band and the length, per (query r, key) pair
                const int key0 = kb * 32 + 4 * kh, qi = q0 + r;
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int key = key0 + 8 * (i >> 2) + (i & 3), dk = key - qi;
                    bool hide = key >= len;
                    if constexpr (WIN) hide = hide || dk > a.window || -dk > a.window;
                    if (hide) s[i] = -INFINITY;
                }
            }
            float mb = s[0];
#pragma unroll
            for (int i = 1; i < 16; i++) mb = fmaxf(mb, s[i]);
            mb = fmaxf(mb, __shfl_xor(mb, 32));
            const float mn = fmaxf(m, mb);
            const float mref = mn == -INFINITY ? 0.f : mn;     // no visible key seen yet: p = 0, nothing rescaled
            const float alpha = exp2f(m - mref);
            m = mn;
            float ps = 0.f;
#pragma unroll
            for (int i = 0; i < 16; i++) { s[i] = exp2f(s[i] - mref); ps += s[i]; }
            l = l * alpha + ps;
#pragma unroll
            for (int db = 0; db < 8; db++) o[db] = o[db] * alpha;
            // P^T as the B operand: k-step t takes accumulators 8 t .. 8 t + 7 (keys 16 t + 4 kh + {0-3, 8-11})
            uint4 pb[2];
#pragma unroll
            for (int t = 0; t < 2; t++)
                pb[t] = uint4{pack_bf16x2(s[8 * t + 0], s[8 * t + 1]), pack_bf16x2(s[8 * t + 2], s[8 * t + 3]),
                              pack_bf16x2(s[8 * t + 4], s[8 * t + 5]), pack_bf16x2(s[8 * t + 6], s[8 * t + 7])};
#pragma unroll
            for (int db = 0; db < 8; db++) {
                const int d = db * 32 + r;
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    const uint4 va = *(const uint4 *)(v_t + d * 64 + (((2 * t + kh) ^ ((d >> 1) & 3)) << 4));
                    o[db] = mfma_bf16(va, pb[t], o[db]);
                }
            }
        }
        if (more) { GA_STORE_BLOCK(cur ^ 1) }                      // the other buffer: its last readers passed the previous barrier
        __syncthreads();
    }
    if (!live) return;
    const float lt = l + __shfl_xor(l, 32);
    const float inv = lt > 0.f ? 1.0f / lt : 0.f;
    const bool qv = q0 + r < len;                              // a query row at or past the length: zeros, whatever its q row held
    auto fin = [&](float x) { return qv ? x * inv : 0.f; };
    // O^T accumulators: d = 32 db + 8 (i / 4) + 4 kh + i % 4 of this lane's query: four consecutive d per 8-byte store
#pragma unroll
    for (int db = 0; db < 8; db++)
#pragma unroll
        for (int gq = 0; gq < 4; gq++) {
            const int d = db * 32 + 8 * gq + 4 * kh;
            *(uint2 *)(ctx_row + d) = uint2{pack_bf16x2(fin(o[db][4 * gq + 0]), fin(o[db][4 * gq + 1])),
                                            pack_bf16x2(fin(o[db][4 * gq + 2]), fin(o[db][4 * gq + 3]))};
        }
}

#undef GA_LOAD_BLOCK
#undef GA_STORE_BLOCK
#undef GA_LOAD1
#undef GA_STORE1

template <int G>
int launch_g(const GqaAttnArgs &a, bool win, hipStream_t st) {
    constexpr int R = G == 3 ? 1 : 4 / G, QR = 32 * R;
    const dim3 grid((unsigned)((a.S + QR - 1) / QR), (unsigned)a.nkv, (unsigned)a.B);
    if (win) k_attn_gqa<G, true><<<grid, 64 * G * R, 0, st>>>(a);
    else k_attn_gqa<G, false><<<grid, 64 * G * R, 0, st>>>(a);
    AK_HIP(hipGetLastError());
    return 0;
}
}  // namespace

bool attn_gqa_supported(int nq, int nkv, int head_dim, int S) {
    if (head_dim != GA_HD || nq <= 0 || nkv <= 0 || nq % nkv) return false;
    const int G = nq / nkv;
    return G >= 1 && G <= 4 && S > 0 && S % 32 == 0 && S <= ATTN_GQA_MAX_S;
}

int launch_attn_gqa(const GqaAttnArgs &a0, int half_window, hipStream_t st) {
    GqaAttnArgs a = a0;
    if (!attn_gqa_supported(a.nq, a.nkv, GA_HD, a.S)) AK_FAIL(-1, "attn_gqa: unsupported head layout or sequence length");
    if (a.B <= 0 || a.B > 65535 || a.nkv > 65535) AK_FAIL(-1, "attn_gqa: at most 65535 rows and kv heads per launch");
    if (half_window < 0) AK_FAIL(-1, "attn_gqa: half_window must be >= 0 (0 = every key)");
    if (!a.q || !a.k || !a.vt || !a.lens || !a.ctx) AK_FAIL(-1, "attn_gqa: NULL argument");
    const bool win = half_window > 0 && half_window < a.S;     // a band as wide as the row hides nothing
    a.window = half_window;
    switch (a.nq / a.nkv) {
        case 1: return launch_g<1>(a, win, st);
        case 2: return launch_g<2>(a, win, st);
        case 3: return launch_g<3>(a, win, st);
        default: return launch_g<4>(a, win, st);
    }
}

}  // namespace ak
