// attn_gqa.hip -- bidirectional grouped-query flash attention at head size 256 with an optional band (EmbeddingGemma, gemma.hip):
//   ctx[t][h * 256 + d] = sum_{s' visible} softmax_s'(q_h[s] . k_g[s']) v_g[s'][d],   g = h / (nq / nkv)
// key s' is visible to query s iff s' < len (the row's length) and, in a sliding layer with half-window w, |s - s'| <= w.
// q arrives pre-scaled by log2(e) * query_pre_attn_scalar^-0.5 (gemma.hip k_gm_qk_norm_rope), so the softmax runs in the base-2 domain.
//
// Layouts (k_gm_qk_norm_rope writes them): q [B][nq][S][256], k [B][nkv][S][256], v TRANSPOSED [B][nkv][256][S] with the keys of every
// 16-group in vt_pos order (what attn_long.hip takes); ctx [T][nq * 256] bf16 (the out-projection's A operand). Rows are right-padded;
// lens[b] is the row's length, clamped to [0, S] by the embedding kernel.
//
// The per-key-block algorithm is flash_tile.h's (16 + 16 MFMAs per block; the 256 x 32 O^T tile is 128 accumulators); this file's own:
//
// Workgroup = (query block, kv head, sequence) and holds every query head of the group, as attn_causal.hip: wave v computes query head
// g = v % G of the group for the 32 query rows q0 = block * 32 R + 32 (v / G), R = rows_per_group(G): four waves for G = 1, 2, 4, three
// for G = 3 (192 threads: the model's layout).
// Staging: each 32-key block of K and V^T is staged ONCE for all G heads and R row blocks, through two LDS buffers as attn_long.hip: block
// kb + 1 is loaded into registers under block kb's MFMAs and written to the other buffer behind them (one barrier per block); up to six
// 16-byte chunks of each tile per thread, in named scalars.
// Mask: -inf on the keys past the row's length and outside the band, only in the blocks that straddle either edge; a block in which a
// query sees no key leaves its running max and sum unchanged (the guarded step). The band walk is k_attn_long<true>'s: a workgroup
// stages only the key blocks that intersect [q_begin - w, q_end - 1 + w] below the row's length, and a wave skips the blocks wholly
// outside the band of its own 32 queries. Query rows at or past the length get zero context rows; query blocks wholly past it are not
// computed.
// A lane holds 64 (q) + 128 (O^T) + 16 (scores) + 32-48 (the block in flight) registers: one wave per SIMD (__launch_bounds__(256) gives
// the compiler the 512 unified registers of a lane). LDS per workgroup: 65 536 bytes (2 x 16 KB K, 2 x 16 KB V^T).
#include "flash_tile.h"

namespace ak {
using namespace ft;

namespace {
constexpr int GA_HD = 256;
using Tile = FlashTile<GA_HD>;
constexpr int GA_CHUNKS = Tile::K_BYTES / 16;                 // 16-byte chunks of a K tile and of a V^T tile
static_assert(Tile::V_BYTES == Tile::K_BYTES, "one chunk count for both tiles");

template <int G, bool WIN>
__global__ __launch_bounds__(256) void k_attn_gqa(GqaAttnArgs a) {
    constexpr int R = rows_per_group(G), QR = 32 * R, NTHR = 64 * G * R, NCH = (GA_CHUNKS + NTHR - 1) / NTHR;
    __shared__ __attribute__((aligned(16))) char sK[2][Tile::K_BYTES];
    __shared__ __attribute__((aligned(16))) char sV[2][Tile::V_BYTES];
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
    if (has_q && !live) Tile::zero_row(ctx_row, kh);           // wholly past the length
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
            *(uint4 *)(sK[buf_] + Tile::k_off(i >> 5, i & 31)) = kr_;                                               \
            *(uint4 *)(sV[buf_] + Tile::v_off(i >> 2, i & 3)) = vr_;                                                \
        }                                                                                                           \
    }
#define GA_LOAD_BLOCK(kb_) GA_LOAD1(0, kr0, vr0, kb_) GA_LOAD1(1, kr1, vr1, kb_) GA_LOAD1(2, kr2, vr2, kb_) GA_LOAD1(3, kr3, vr3, kb_) \
    GA_LOAD1(4, kr4, vr4, kb_) GA_LOAD1(5, kr5, vr5, kb_)
#define GA_STORE_BLOCK(buf_) GA_STORE1(0, kr0, vr0, buf_) GA_STORE1(1, kr1, vr1, buf_) GA_STORE1(2, kr2, vr2, buf_) GA_STORE1(3, kr3, vr3, buf_) \
    GA_STORE1(4, kr4, vr4, buf_) GA_STORE1(5, kr5, vr5, buf_)
    GA_LOAD_BLOCK(kb_start)
    GA_STORE_BLOCK(kb_start & 1)                                // LDS buffers go by block parity

    uint4 qf[Tile::NC];
    Tile::load_q(qf, a.q + (((int64_t)b * a.nq + h) * S + (live ? q0 + r : 0)) * GA_HD, kh);
    f32x16 o[Tile::NDB];
#pragma unroll
    for (int i = 0; i < Tile::NDB; i++) o[i] = zero16();
    float m = -INFINITY, l = 0.f;
    __syncthreads();
    for (int kb = kb_start; kb < kb_stop; kb++) {
        const int cur = kb & 1;
        const bool more = kb + 1 < kb_stop;
        if (more) { GA_LOAD_BLOCK(kb + 1) }                        // next block into registers: in flight under this block's MFMAs
        const Band band = WIN ? band_of(kb, q0, a.window) : BAND_IN;       // the block against this wave's queries (wave-uniform)
        if (live && band != BAND_OUT) {
            f32x16 s = Tile::scores(sK[cur], qf, r, kh);
            if (band == BAND_EDGE || kb * 32 + 32 > len) {     // an edge block: the band and the length, per (query r, key) pair
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int key = kb * 32 + Tile::acc_row(i, kh);
                    bool hide = key >= len;
                    if constexpr (WIN) hide |= band_hides(key - (q0 + r), a.window);
                    if (hide) s[i] = -INFINITY;
                }
            }
            float alpha;
            s = Tile::softmax_step<true>(s, m, l, alpha);
            uint4 pb[2];
            Tile::pack_p(s, pb);
#pragma unroll
            for (int db = 0; db < Tile::NDB; db++) o[db] = Tile::pv(sV[cur], pb, o[db] * alpha, db, r, kh);    // (a rescale loop of its own spills at G = 3)
        }
        if (more) { GA_STORE_BLOCK(cur ^ 1) }                      // the other buffer: its last readers passed the previous barrier
        __syncthreads();
    }
    if (!live) return;
    const float lt = l + __shfl_xor(l, 32);
    const float inv = lt > 0.f ? 1.0f / lt : 0.f;
    const bool qv = q0 + r < len;                              // a query row at or past the length: zeros, whatever its q row held
#pragma unroll
    for (int db = 0; db < Tile::NDB; db++) Tile::store_ctx(ctx_row, o[db], db, kh, [&](float x) { return qv ? x * inv : 0.f; });
}

#undef GA_LOAD_BLOCK
#undef GA_STORE_BLOCK
#undef GA_LOAD1
#undef GA_STORE1

template <int G>
int launch_g(const GqaAttnArgs &a, bool win, hipStream_t st) {
    constexpr int R = rows_per_group(G), QR = 32 * R;
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
    return G * rows_per_group(G) <= 4 && S > 0 && S % 32 == 0 && S <= ATTN_GQA_MAX_S;
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
