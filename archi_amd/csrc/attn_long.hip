// attn_long.hip -- bidirectional flash attention of the BERT encoder for rows longer than 512 tokens (512 < S <= 8192, head size 64,
// bf16; XLM-RoBERTa / bge-m3 encoders given ak_encoder_set_positions_from_ids(max_seq > 512)):
//   ctx = softmax(q k^T / sqrt(64) + mask) v      per (sequence, head)
// The encoder's tiles with S <= 512 never come here (attention.hip). ModernBERT (mbert.hip) runs every tile, 32 <= S <= 8192, on this
// kernel through launch_attn_window: its global layers on the same instantiation, its sliding-window layers on k_attn_long<true> (below).
// q arrives pre-scaled by log2(e) / 8 from the QKV GEMM, so the softmax runs in
// the base-2 domain on v_exp_f32; v arrives transposed ([B][H][S], keys of every 16-group in vt_pos order) as attention.hip takes it.
//
// The per-key-block algorithm is flash_tile.h's; this file's own:
//
// Workgroup = (128-query block, head, sequence), four waves of 32 queries.
// Staging: the 32-key blocks of K and V^T stream through two LDS buffers: block kb + 1 is loaded into registers while block kb is
// computed, then written to the other buffer (one barrier per block); one 16-byte chunk of each tile per thread.
// Mask: the block's additive mask (0 / -inf from the int mask) is staged beside K and added to the scores: pad keys of the last block,
// and any hole of an explicit mask, are excluded; a block with no real key leaves the running max and sum unchanged (the guarded step).
// Key blocks wholly past the row's length (rowlen, k_positions) are not loaded; query blocks wholly past it write zero context rows.
// LDS per workgroup: 16 640 bytes (2 x 4 KB K, 2 x 4 KB V^T, 2 x 32 mask floats), both instantiations.
#include "flash_tile.h"

namespace ak {
using namespace ft;

namespace {
constexpr int AL_HD = 64, AL_QB = 128;
using Tile = FlashTile<AL_HD>;

// WIN (ModernBERT's sliding layers, a.window = half-window w >= 1): key k is visible to query q iff |q - k| <= w. The workgroup walks
// only the key blocks that intersect [q_begin - w, q_begin + 127 + w] (9 at most for w = 64); a wave skips the blocks that lie wholly
// outside the band of its own 32 queries and applies the band (-inf) only in the blocks that straddle its edge -- blocks wholly inside
// take the same instructions as WIN = false. WIN = false is the kernel as it was (every key block up to the row's length).
template <bool WIN>
__global__ __launch_bounds__(256) void k_attn_long(AttnArgs a) {
    __shared__ __attribute__((aligned(16))) char sK[2][Tile::K_BYTES];
    __shared__ __attribute__((aligned(16))) char sV[2][Tile::V_BYTES];
    __shared__ float sM[2][32];
    const int h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S, H = a.H;
    const int len = min(max(a.rowlen[b], 0), S);
    const int q_begin = blockIdx.x * AL_QB, q0 = q_begin + 32 * wave;
    const int r = lane & 31, kh = lane >> 5;
    const int64_t row0 = (int64_t)b * S;
    const bool has_q = q0 < S;                                 // this wave's 32 rows exist (S % 32 == 0)
    if (q_begin >= len) {                                      // wholly past the length (uniform): zero context rows
        if (has_q) Tile::zero_row(a.ctx + (row0 + q0 + r) * H + h * AL_HD, kh);
        return;
    }
    int kb_stop = (len + 31) / 32, kb_start = 0;
    if constexpr (WIN) {
        kb_start = max(q_begin - a.window, 0) / 32;            // q_begin < len: block q_begin / 32 is inside [kb_start, kb_stop)
        kb_stop = min(kb_stop, (q_begin + AL_QB - 1 + a.window) / 32 + 1);
    }
    // staging assignment: thread tid moves K chunk (key tid / 8, chunk tid % 8) and V^T chunk (row d = tid / 4, chunk tid % 4)
    const int k_key = tid >> 3, k_c = tid & 7, v_d = tid >> 2, v_c = tid & 3;
    const uint16_t *kg = a.k + row0 * H + (int64_t)h * a.qk_hs + (int64_t)k_key * a.qk_ld + k_c * 8;
    const int c0 = kb_start & 1;                               // LDS buffer of the first block (buffers go by block parity)
    const uint16_t *vg = a.vt + ((int64_t)b * H + h * AL_HD + v_d) * S + v_c * 8;
    const int k_dst = Tile::k_off(k_key, k_c), v_dst = Tile::v_off(v_d, v_c);
    uint4 kreg = *(const uint4 *)(kg + (int64_t)kb_start * 32 * a.qk_ld), vreg = *(const uint4 *)(vg + kb_start * 32);
    float mreg = tid < 32 ? (a.mask[row0 + kb_start * 32 + tid] ? 0.f : -INFINITY) : 0.f;
    *(uint4 *)(sK[c0] + k_dst) = kreg;
    *(uint4 *)(sV[c0] + v_dst) = vreg;
    if (tid < 32) sM[c0][tid] = mreg;

    uint4 qf[Tile::NC];
    Tile::load_q(qf, a.q + row0 * H + (int64_t)h * a.qk_hs + (int64_t)(has_q ? q0 + r : S - 1) * a.qk_ld, kh);
    f32x16 o[Tile::NDB];
#pragma unroll
    for (int i = 0; i < Tile::NDB; i++) o[i] = zero16();
    float m = -INFINITY, l = 0.f;
    __syncthreads();
    for (int kb = kb_start; kb < kb_stop; kb++) {
        const int cur = kb & 1;
        const bool more = kb + 1 < kb_stop;
        if (more) {                                            // next block into registers: in flight under this block's MFMAs
            kreg = *(const uint4 *)(kg + (int64_t)(kb + 1) * 32 * a.qk_ld);
            vreg = *(const uint4 *)(vg + (kb + 1) * 32);
            if (tid < 32) mreg = a.mask[row0 + (kb + 1) * 32 + tid] ? 0.f : -INFINITY;
        }
        const Band band = WIN ? band_of(kb, q0, a.window) : BAND_IN;       // the block against this wave's queries (wave-uniform)
        if (has_q && band != BAND_OUT) {
            f32x16 s = Tile::scores(sK[cur], qf, r, kh);
#pragma unroll
            for (int i = 0; i < 16; i++) s[i] += sM[cur][Tile::acc_row(i, kh)];
            if (WIN && band == BAND_EDGE) {                    // the band, per (query r, key) pair
                const int dq = kb * 32 - (q0 + r);             // key - query of the block's first key
#pragma unroll
                for (int i = 0; i < 16; i++)
                    if (band_hides(dq + Tile::acc_row(i, kh), a.window)) s[i] = -INFINITY;
            }
            float alpha;
            s = Tile::softmax_step<true>(s, m, l, alpha);
#pragma unroll
            for (int db = 0; db < Tile::NDB; db++) o[db] = o[db] * alpha;
            uint4 pb[2];
            Tile::pack_p(s, pb);
#pragma unroll
            for (int db = 0; db < Tile::NDB; db++) o[db] = Tile::pv(sV[cur], pb, o[db], db, r, kh);
        }
        if (more) {                                            // the other buffer: its last readers passed the previous barrier
            *(uint4 *)(sK[cur ^ 1] + k_dst) = kreg;
            *(uint4 *)(sV[cur ^ 1] + v_dst) = vreg;
            if (tid < 32) sM[cur ^ 1][tid] = mreg;
        }
        __syncthreads();
    }
    if (!has_q) return;
    const float lt = l + __shfl_xor(l, 32);
    const float inv = lt > 0.f ? 1.0f / lt : 0.f;
    uint16_t *crow = a.ctx + (row0 + q0 + r) * H + h * AL_HD;
#pragma unroll
    for (int db = 0; db < Tile::NDB; db++) Tile::store_ctx(crow, o[db], db, kh, [&](float x) { return x * inv; });
}
}  // namespace

// the same kernel for any S % 32 == 0 in [32, 8192] with an optional band (ModernBERT, mbert.hip): window < 0 or >= S: every key
int launch_attn_window(const AttnArgs &a0, int window, hipStream_t st) {
    AttnArgs a = a0;
    if (a.qk_ld == 0) { a.qk_ld = a.H; a.qk_hs = a.H / a.heads; }
    if (a.H != a.heads * AL_HD) AK_FAIL(-1, "attention (windowed): head size must be 64");
    if (a.S <= 0 || a.S % 32 || a.S > ATTN_LONG_MAX_S) AK_FAIL(-1, "attention (windowed): S must be a positive multiple of 32, <= 8192");
    if (!a.rowlen || !a.mask || a.rel) AK_FAIL(-1, "attention (windowed): needs the row lengths and the mask, no bias");
    const dim3 grid((unsigned)((a.S + AL_QB - 1) / AL_QB), (unsigned)a.heads, (unsigned)a.B);
    a.window = window;
    if (window >= 0 && window < a.S) k_attn_long<true><<<grid, 256, 0, st>>>(a);
    else k_attn_long<false><<<grid, 256, 0, st>>>(a);
    AK_HIP(hipGetLastError());
    return 0;
}

int launch_attn_long(const AttnArgs &a0, hipStream_t st) {
    AttnArgs a = a0;
    if (a.qk_ld == 0) { a.qk_ld = a.H; a.qk_hs = a.H / a.heads; }      // token-major q / k
    if (a.H != a.heads * AL_HD) AK_FAIL(-1, "attention (rows > 512 tokens): head size must be 64");
    if (a.S % 32 || a.S <= 512 || a.S > ATTN_LONG_MAX_S) AK_FAIL(-1, "attention (rows > 512 tokens): S must be a multiple of 32 in (512, 8192]");
    if (!a.rowlen || !a.mask || a.rel) AK_FAIL(-1, "attention (rows > 512 tokens): needs the row lengths and the mask, no bias");
    const dim3 grid((unsigned)((a.S + AL_QB - 1) / AL_QB), (unsigned)a.heads, (unsigned)a.B);
    k_attn_long<false><<<grid, 256, 0, st>>>(a);
    AK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ak
