// flash_tile.h -- the flash-attention tile shared by attn_causal.hip (head size 128), attn_long.hip (64) and attn_gqa.hip (256): the one
// place that knows the fragment format. A wave owns 32 queries and walks 32-key blocks of K and V^T staged in LDS. Per key block:
//   S^T = K Q^T    HD / 16 x v_mfma_f32_32x32x16_bf16: A = K (rows = keys, from LDS), B = Q^T (columns = queries, HD / 4 VGPRs held for the
//                  whole walk). Keys on M: a lane owns ONE query column and 16 of the 32 keys (acc_row); the other 16 are in lane ^ 32, so
//                  the row max and the row sum take one cross-lane step each.
//   mask           the caller's own: -inf on the score accumulators it hides (an int mask, the causal diagonal, a length, a band)
//   online softmax in base 2 on v_exp_f32 (q arrives pre-scaled by log2(e) x the model's scale): running max m and sum l per lane
//   O^T += V^T P^T HD / 16 MFMAs: A = V^T (rows = d, the keys of each 16-group in vt_pos order), B = P^T straight from the S^T accumulators
//                  (the lane's 16 keys are exactly the two k-steps' B operands in vt_pos order).
// K tile [32 keys][HD]: 2 HD-byte rows, 16-byte chunk c of key r stored at chunk c ^ (r & 7) (the 8 lanes of a ds_read_b128 phase read 8
// keys' same chunk: 8 distinct bank groups). V^T tile [HD d][32 keys]: 64-byte rows, chunk c of row d at c ^ ((d >> 1) & 3).
// r = lane & 31 (the query, the K row, the V^T row within a d-block), kh = lane >> 5 throughout.
// The O^T accumulators travel BY VALUE, one f32x16 per call (o[db] = pv(.., o[db], ..)): a helper that took the array by reference put
// k_attn_gqa<3, *> into scratch (docs/EXPERIMENTS.md).
#pragma once
#include "encoder_kernels.h"
#include "mfma_tile.h"

namespace ak {
namespace ft {
using namespace mt;

// 32-query row blocks per workgroup of the grouped-query kernels (attn_causal.hip, attn_gqa.hip) at G query heads per kv head: G R <= 4 waves
constexpr int rows_per_group(int G) { return G >= 4 ? 1 : 4 / G; }

// A 32-key block against a wave's queries q0 .. q0 + 31 under the band |query - key| <= w (wave-uniform)
enum Band { BAND_OUT, BAND_IN, BAND_EDGE };                    // no visible pair: skip / every pair visible / the band per pair (band_hides)
__device__ inline Band band_of(int kb, int q0, int w) {
    const int dk_hi = kb * 32 + 31 - q0, dk_lo = q0 + 31 - kb * 32;      // largest key - query / query - key
    if (dk_hi - 62 > w || dk_lo - 62 > w) return BAND_OUT;
    return dk_hi > w || dk_lo > w ? BAND_EDGE : BAND_IN;
}
__device__ inline bool band_hides(int dk, int w) { return (dk > w) | (-dk > w); }      // dk = key - query (|: no branch per accumulator)

__device__ inline f32x16 zero16() { return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; }

template <int HD>
struct FlashTile {
    static_assert(HD == 64 || HD == 128 || HD == 256, "head size");
    static constexpr int K_ROW = 2 * HD, K_BYTES = 32 * K_ROW, V_BYTES = HD * 64;
    static constexpr int NC = HD / 16, NDB = HD / 32;          // q chunks = MFMAs per product, 32-row d-blocks of O^T

    // byte offsets of 16-byte chunk c of key r in a K tile, of chunk c of row d in a V^T tile
    static __device__ int k_off(int r, int c) { return r * K_ROW + ((c ^ (r & 7)) << 4); }
    static __device__ int v_off(int d, int c) { return d * 64 + ((c ^ ((d >> 1) & 3)) << 4); }
    // accumulator i of lane half kh: row (key of S^T, d of O^T) within the 32-row block
    static __device__ int acc_row(int i, int kh) { return 8 * (i >> 2) + 4 * kh + (i & 3); }

    // this lane's query: NC chunks of 16 bytes (d = 16 c + 8 kh .. + 7), the B operand of every S^T MFMA. qrow: the lane's q row.
    static __device__ void load_q(uint4 (&qf)[NC], const uint16_t *qrow, int kh) {
#pragma unroll
        for (int c = 0; c < NC; c++) qf[c] = *(const uint4 *)(qrow + kh * 8 + c * 16);
    }
    // S^T block from K tile k_t: accumulator i = key acc_row(i, kh) of the block against this lane's query
    static __device__ f32x16 scores(const char *k_t, const uint4 (&qf)[NC], int r, int kh) {
        f32x16 s = zero16();
#pragma unroll
        for (int c = 0; c < NC; c++) s = mfma_bf16(*(const uint4 *)(k_t + k_off(r, 2 * c + kh)), qf[c], s);
        return s;
    }
    // One online-softmax step over the masked scores: updates m and l, sets alpha (the factor the caller rescales O^T by) and returns
    // the probabilities. GUARD: a lane may have seen no visible key yet (mn == -inf): then p = 0 and nothing is rescaled. Without it
    // the caller promises a visible key in the first block.
    template <bool GUARD>
    static __device__ f32x16 softmax_step(f32x16 s, float &m, float &l, float &alpha) {
        float mb = s[0];
#pragma unroll
        for (int i = 1; i < 16; i++) mb = fmaxf(mb, s[i]);
        mb = fmaxf(mb, __shfl_xor(mb, 32));
        const float mn = fmaxf(m, mb);
        const float mref = GUARD && mn == -INFINITY ? 0.f : mn;
        alpha = exp2f(m - mref);
        m = mn;
        float ps = 0.f;
#pragma unroll
        for (int i = 0; i < 16; i++) { s[i] = exp2f(s[i] - mref); ps += s[i]; }
        l = l * alpha + ps;
        return s;
    }
    // P^T as the B operand: k-step t takes accumulators 8 t .. 8 t + 7 (keys 16 t + 4 kh + {0-3, 8-11})
    static __device__ void pack_p(f32x16 p, uint4 (&pb)[2]) {
#pragma unroll
        for (int t = 0; t < 2; t++)
            pb[t] = uint4{pack_bf16x2(p[8 * t + 0], p[8 * t + 1]), pack_bf16x2(p[8 * t + 2], p[8 * t + 3]),
                          pack_bf16x2(p[8 * t + 4], p[8 * t + 5]), pack_bf16x2(p[8 * t + 6], p[8 * t + 7])};
    }
    // d-block db of O^T += V^T P^T from V^T tile v_t: two k-steps
    static __device__ f32x16 pv(const char *v_t, const uint4 (&pb)[2], f32x16 o, int db, int r, int kh) {
#pragma unroll
        for (int t = 0; t < 2; t++) o = mfma_bf16(*(const uint4 *)(v_t + v_off(db * 32 + r, 2 * t + kh)), pb[t], o);
        return o;
    }
    // d-block db of the lane's context row: d = 32 db + acc_row(i, kh), four consecutive d per 8-byte store; fin finishes one value
    template <class F>
    static __device__ void store_ctx(uint16_t *ctx_row, f32x16 o, int db, int kh, F fin) {
#pragma unroll
        for (int gq = 0; gq < 4; gq++)
            *(uint2 *)(ctx_row + db * 32 + acc_row(4 * gq, kh)) = uint2{pack_bf16x2(fin(o[4 * gq + 0]), fin(o[4 * gq + 1])),
                                                                        pack_bf16x2(fin(o[4 * gq + 2]), fin(o[4 * gq + 3]))};
    }
    // a context row past the length: zeros, half a row per lane of the pair (r, r + 32)
    static __device__ void zero_row(uint16_t *ctx_row, int kh) {
        for (int c = kh; c < HD / 8; c += 2) *(uint4 *)(ctx_row + c * 8) = uint4{0, 0, 0, 0};
    }
};

}  // namespace ft
}  // namespace ak
