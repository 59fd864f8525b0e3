// attn_causal.hip -- causal grouped-query flash attention at head dim 128 (the decoder's attention, decoder128.hip):
//   ctx[t][h * 128 + d] = sum_{s' <= s} softmax_s'(q_h[s] . k_g[s']) v_g[s'][d],   g = h / (nq / nkv)
// q arrives pre-scaled by log2(e) / sqrt(128) (decoder128.hip k_dec_qk_rope). The per-key-block algorithm is flash_tile.h's; this file's own:
//
// Layouts (decoder128.hip writes them): q [B][nq][S][128], k and v [B][nkv][S][128] bf16; ctx [T][nq * 128] bf16 (the out-projection's
// A operand). Rows are right-padded; lens[b] is the row's length, clamped to [0, S] by the embedding kernel.
//
// Workgroup = (query block, kv head, sequence) and holds every query head of the group: wave w computes query head g = w % G of the
// group for the 32 query rows q0 = (block) * QR + 32 (w / G), QR = 32 R, R = rows_per_group(G): four waves per workgroup for G = 1, 2, 4,
// three for G = 3 (G <= 4: 256 threads, so that the compiler may give a lane the registers the kernel needs -- at 1024 threads it spilled 34).
// Staging: each 32-key block of K and V is staged into ONE LDS buffer inside the loop, once for all G heads and R row blocks; V arrives
// key-major and is transposed on the way (a 2-byte scatter into the V^T tile).
// Mask: key blocks above a wave's diagonal are not computed (the workgroup stages up to its last wave's diagonal); inside the diagonal
// block keys past the query are masked. The first block always holds a visible key (key 0), so the softmax step runs without its -inf
// guard. Query blocks wholly past the row's length are not computed: their context rows are zero (finite, and nothing valid reads
// them: a valid query never sees a pad key under the causal mask).
// BAND (k_attn_causal_band: Mistral's sliding window, decoder128.hip; CausalAttnArgs::window = w): key <= query and query - key <= w - 1, flash_tile.h's band of
// half-width w - 1 under the diagonal. The workgroup stages from the block of its first wave's lowest visible key (at S = 8192,
// w = 4096 three quarters of the plain walk's blocks); a wave skips the blocks its band does not reach (BAND_OUT). The first block a
// wave computes may hold no visible key for its later queries, so this kernel runs the guarded softmax step; every query sees
// itself, so no row sum is zero at the end. It also stores zeros for the queries at or past the length inside a live row block.
// BIDIR (k_attn_bidir: the Mistral / Llama embedders trained without the causal mask; CausalAttnArgs::bidirectional): every key below the
// row's length for every query below it. The workgroup walks the blocks that hold such a key and no others; inside the last partial
// block the keys at or past the length are masked (the causal mask hid them for free). Key 0 is below the length of a live row, so the
// step needs no guard. Rows at or past the length are stored as zeros.
// SPLIT (k_attn_causal_gs, k_attn_bidir_gs; launch_attn_causal_split: Qwen2's 5 to 8 query heads per kv head): the same wave, one
// 32-row query block per workgroup, the group's heads in two workgroups of 3 or 4 waves (attn_causal_body.h says how).
#include "flash_tile.h"

namespace ak {
using namespace ft;

namespace {
constexpr int CA_HD = 128;
using Tile = FlashTile<CA_HD>;

// k_attn_causal (Qwen3; Mistral / Llama without a window), k_attn_causal_band and k_attn_bidir: one text, attn_causal_body.h
#define AK_CAUSAL_KERNEL k_attn_causal
#define AK_CAUSAL_VIS 0
#include "attn_causal_body.h"
#undef AK_CAUSAL_KERNEL
#undef AK_CAUSAL_VIS
#define AK_CAUSAL_KERNEL k_attn_causal_band
#define AK_CAUSAL_VIS 1
#include "attn_causal_body.h"
#undef AK_CAUSAL_KERNEL
#undef AK_CAUSAL_VIS
#define AK_CAUSAL_KERNEL k_attn_bidir
#define AK_CAUSAL_VIS 2
#include "attn_causal_body.h"
#undef AK_CAUSAL_KERNEL
#undef AK_CAUSAL_VIS
// the kv group split over workgroups (5 to 8 query heads per kv head: Qwen2), causal and bidirectional; no banded variant
#define AK_CAUSAL_SPLIT 1
#define AK_CAUSAL_KERNEL k_attn_causal_gs
#define AK_CAUSAL_VIS 0
#include "attn_causal_body.h"
#undef AK_CAUSAL_KERNEL
#undef AK_CAUSAL_VIS
#define AK_CAUSAL_KERNEL k_attn_bidir_gs
#define AK_CAUSAL_VIS 2
#include "attn_causal_body.h"
#undef AK_CAUSAL_KERNEL
#undef AK_CAUSAL_VIS
#undef AK_CAUSAL_SPLIT
}  // namespace

bool attn_causal_supported(int nq, int nkv, int head_dim, int S) {
    if (head_dim != CA_HD || nkv <= 0 || nq % nkv) return false;
    const int G = nq / nkv, R = rows_per_group(G);
    return G * R <= 4 && S % 32 == 0 && S > 0 && S <= 8192;
}

int launch_attn_causal(const CausalAttnArgs &a, hipStream_t st) {
    if (!attn_causal_supported(a.nq, a.nkv, CA_HD, a.S)) AK_FAIL(-1, "attn_causal: unsupported head layout or sequence length");
    const int G = a.nq / a.nkv, R = rows_per_group(G), QR = 32 * R;
    const dim3 grid((a.S + QR - 1) / QR, a.nkv, a.B);
    if (a.window < 0) AK_FAIL(-1, "attn_causal: window must be >= 0");
    if (a.bidirectional) k_attn_bidir<<<grid, 64 * G * R, 0, st>>>(a);        // ignores the window
    else if (a.window > 0) k_attn_causal_band<<<grid, 64 * G * R, 0, st>>>(a);      // (a window >= S hides nothing; the rows past a length are still zeroed)
    else k_attn_causal<<<grid, 64 * G * R, 0, st>>>(a);
    AK_HIP(hipGetLastError());
    return 0;
}

// 5 to 8 query heads per kv head (Qwen2-1.5B: 6, Qwen2-7B: 7, Qwen2.5-3B: 8, Qwen2.5-14B: 5): the group in P = ceil(G / 4) workgroups of
// GP = ceil(G / P) waves (3 + 2, 3 + 3, 4 + 3, 4 + 4 heads), grid (S / 32, nkv * P, B); each workgroup stages the K / V blocks it walks
// once for its 3 or 4 heads
bool attn_causal_split_supported(int nq, int nkv, int head_dim, int S) {
    if (head_dim != CA_HD || nkv <= 0 || nq <= 0 || nq % nkv) return false;
    const int G = nq / nkv;
    return G >= 5 && G <= 8 && S % 32 == 0 && S > 0 && S <= 8192;
}

int launch_attn_causal_split(const CausalAttnArgs &a, hipStream_t st) {
    if (!attn_causal_split_supported(a.nq, a.nkv, CA_HD, a.S))
        AK_FAIL(-1, "attn_causal_split: 5 to 8 query heads per kv head, S a multiple of 32 up to 8192");
    if (a.window != 0) AK_FAIL(-1, "attn_causal_split: no sliding window (window must be 0)");
    if (a.B <= 0 || a.B > 65535) AK_FAIL(-1, "attn_causal_split: 1 to 65535 rows");
    const int G = a.nq / a.nkv, P = (G + 3) / 4, GP = (G + P - 1) / P;
    const dim3 grid(a.S / 32, a.nkv * P, a.B);
    if (a.bidirectional) k_attn_bidir_gs<<<grid, 64 * GP, 0, st>>>(a);
    else k_attn_causal_gs<<<grid, 64 * GP, 0, st>>>(a);
    AK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ak
