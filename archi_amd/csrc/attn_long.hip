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
// LDS per workgroup: 16 640 bytes (2 x 4 KB K, 2 x 4 KB V^T, 2 x 32 mask floats), every instantiation; k_attn_long_relbias (T5's
// relative bias, below) adds the head's 2 D + 1 + 128 table floats as dynamic LDS (1540 bytes at D = 128).
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
//
// BIAS (T5, t5.hip: launch_attn_relbias; WIN = false only): the scores get tab[clamp(key - query, -D, D) + D] of the workgroup's head
// (a.rbias, D = a.rbias_D >= 1; base-2 domain like q) in float32 before the mask. The head's 2 D + 1 floats are staged into LDS once,
// with RB_PAD copies of the first entry in front and of the last entry behind: sB[j] = tab[clamp(j - RB_PAD, 0, 2 D)].
// Per key block a lane forms ONE table index, that of the block's first key against its query, clamps it into [0, 2 D + RB_PAD]
// and reads its 16 accumulators' entries at constant offsets from it (one address register; the 32 lanes of a half read
// consecutive dwords). A pair within RB_PAD - 1 of [-D, D] finds its clamp in the padding; a lane whose whole block lies further
// out reads 32 copies of the end entry, which is what the clamp gives each of its pairs -- a block wholly at or beyond -D or +D
// ("far") so adds the constant tab[0] / tab[2 D] with the instructions of every other block. (Classifying the blocks wave-uniformly
// and adding that constant from a register on a branch of its own was measured first: 138 VGPRs against 117, two waves per SIMD
// against three, 1.36x / 1.40x the un-biased launch at 128 x 512 / 8 x 8192 against 1.05x / 1.06x: docs/EXPERIMENTS.md.)
// BIAS = false is the kernel as it was.
constexpr int RB_PAD = 64;
__device__ inline float *rbias_lds() {
    extern __shared__ float s_rbias[];
    return s_rbias;
}

// The kernel text is attn_long_body.h, compiled once per kernel (as attn_causal_body.h is): k_attn_long<WIN> keeps its one template
// parameter -- other tests hold these two instantiations to their register counts by mangled name, and a second parameter would
// make every such name match twice -- and T5's biased walk is a kernel of its own name over the same text.
template <bool WIN>
__global__ __launch_bounds__(256) void k_attn_long(AttnArgs a) {
    constexpr bool BIAS = false;
#include "attn_long_body.h"
}
__global__ __launch_bounds__(256) void k_attn_long_relbias(AttnArgs a) {
    constexpr bool WIN = false, BIAS = true;
#include "attn_long_body.h"
}
}  // namespace

// the same kernel for any S % 32 == 0 in [32, 8192] with an optional band (ModernBERT, mbert.hip): window < 0 or >= S: every key
int launch_attn_window(const AttnArgs &a0, int window, hipStream_t st) {
    AttnArgs a = a0;
    if (a.qk_ld == 0) { a.qk_ld = a.H; a.qk_hs = a.H / a.heads; }
    if (a.H != a.heads * AL_HD) AK_FAIL(-1, "attention (windowed): head size must be 64");
    if (a.S <= 0 || a.S % 32 || a.S > ATTN_LONG_MAX_S) AK_FAIL(-1, "attention (windowed): S must be a positive multiple of 32, <= 8192");
    if (!a.rowlen || !a.mask || a.rel || a.rbias) AK_FAIL(-1, "attention (windowed): needs the row lengths and the mask, no bias");
    const dim3 grid((unsigned)((a.S + AL_QB - 1) / AL_QB), (unsigned)a.heads, (unsigned)a.B);
    a.window = window;
    if (window >= 0 && window < a.S) k_attn_long<true><<<grid, 256, 0, st>>>(a);
    else k_attn_long<false><<<grid, 256, 0, st>>>(a);
    AK_HIP(hipGetLastError());
    return 0;
}

// the same kernel, every key, with the clamped relative bias (T5, t5.hip): a.rbias [heads][2 D + 1], D = a.rbias_D
int launch_attn_relbias(const AttnArgs &a0, hipStream_t st) {
    AttnArgs a = a0;
    if (a.qk_ld == 0) { a.qk_ld = a.H; a.qk_hs = a.H / a.heads; }
    if (a.H != a.heads * AL_HD) AK_FAIL(-1, "attention (relative bias): head size must be 64");
    if (a.S <= 0 || a.S % 32 || a.S > ATTN_LONG_MAX_S) AK_FAIL(-1, "attention (relative bias): S must be a positive multiple of 32, <= 8192");
    if (!a.rowlen || !a.mask || a.rel) AK_FAIL(-1, "attention (relative bias): needs the row lengths and the mask, no S <= 512 bias row");
    if (!a.rbias || a.rbias_D < 1 || a.rbias_D > ATTN_RELBIAS_MAX_D) AK_FAIL(-1, "attention (relative bias): needs the table and 1 <= D <= 4096");
    const dim3 grid((unsigned)((a.S + AL_QB - 1) / AL_QB), (unsigned)a.heads, (unsigned)a.B);
    a.window = -1;
    k_attn_long_relbias<<<grid, 256, (size_t)(2 * a.rbias_D + 1 + 2 * RB_PAD) * sizeof(float), st>>>(a);
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
