// mbert.hip -- the ModernBERT encoder forward pass (nomic-ai/modernbert-embed-base, Alibaba-NLP/gte-modernbert-base,
// lightonai/modernbert-embed-large) behind ak_mbert_*: orchestration and the small kernels. As HF ModernBertModel:
//   x = LayerNorm(tok_embeddings[id]; w)               k_mb_embed (float32 x, bf16 h = x: attn_norm of layer 0 is the identity)
// per layer (pre-norm, no bias anywhere, LayerNorms with a weight only):
//   q | k | v = h Wqkv^T                               k_gemm MODE 0 (gemm.hip): q pre-scaled by log2(e) / 8, k as [T][H], V transposed
//   q, k = RoPE(q), RoPE(k)                            k_mb_rope, in place: rotate_half at head size 64, the table of the layer's type
//                                                      (global theta / local theta)
//   a = softmax(q k^T + band + pad mask) v             k_attn_long<WIN> (attn_long.hip): WIN = true with the half-window in a sliding layer
//   x += a Wo^T; h = LayerNorm(x; mlp_norm)            k_gemm MODE 2 (float32 out) + k_mb_add_ln
//   f = gelu(h Wi_a^T) (h Wi_g^T)                      k_gemm MODE 8 (GeGLU epilogue; the halves of Wi interleaved at create, and padded
//                                                      with zero rows to 2 I % 256 == 0 -- large: 5248 -> 5376 -- for the wide tile:
//                                                      padded_intermediate, stack.h)
//   x += f Wo^T; h = LayerNorm(x; next attn_norm)      k_gemm MODE 2 + k_mb_add_ln
// then final_norm per token, mean / cls pooling over the valid tokens and L2 normalisation in float32 (k_mb_pool_part, k_mb_pool_fin).
// The residual stream x is float32 throughout; GEMM operands are bf16. Token counts are padded to the GEMM tile (256) as in decoder128.hip.
// Here: the config struct's own checks, the layer struct, the order of a layer (block, join, block, join) and the family's kernels: the
// embedding, the join k_mb_add_ln (x32 keeps the SUM), k_mb_rope, the per-token transform of the pool. stack.h holds the token-slot
// prologue, the LayerNorm of a row in registers, both pooling bodies and the NJ dispatch; enc64.h (shared with nomic.hip) the handle's
// workspace, the common create steps, the attention and FFN blocks and the body of ak_mbert_forward_lens.
// LDS per workgroup: k_mb_embed / k_mb_add_ln / k_mb_rope none; k_mb_pool_part 4 * H * 4 bytes (dynamic: 12 KB at H = 768, 16 KB at
// 1024); k_mb_pool_fin 16 bytes; the GEMMs and the attention kernel as their files state.
#include "enc64.h"

namespace ak {

namespace {
constexpr int MB_HD = Enc64::HD;

// LayerNorm statistics of one float32 row held in memory (H % 4 == 0), by one wave: mean, then the variance about it (two passes,
// as torch's float32 kernel -- not E[x^2] - mean^2)
__device__ inline void mb_row_stats(const float *__restrict__ xr, int H, int lane, float eps, float &mean, float &rstd) {
    float s = 0.f;
    for (int c = lane * 4; c < H; c += 256) s += row_sum4(*(const float4 *)(xr + c));
    mean = wave_sum(s) / (float)H;
    float q = 0.f;
    for (int c = lane * 4; c < H; c += 256) q += row_sq4(*(const float4 *)(xr + c), mean);
    rstd = rsqrtf(wave_sum(q) / (float)H + eps);
}

// one wave per token slot t < B * S: ids past the row's length read as 0; x32 = LayerNorm(tok_embeddings[id]; w), h16 = bf16(x32).
// Also the int key mask (slot < length) the attention kernel stages, and per row the clamped length.
__global__ __launch_bounds__(256) void k_mb_embed(const int *__restrict__ ids, int ld_ids, const int *__restrict__ lens, int lens_stride, int B, int S,
                                                  int H, int vocab, const uint16_t *__restrict__ emb, const float *__restrict__ w, float eps,
                                                  float *__restrict__ x32, uint16_t *__restrict__ h16, int *__restrict__ mask, int *__restrict__ lens_out) {
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= (int64_t)B * S) return;
    const int id = token_slot<true>(ids, ld_ids, lens, lens_stride, S, vocab, t, lane, mask, lens_out);
    const uint16_t *e = emb + (int64_t)id * H;
    float *xr = x32 + t * H;
    for (int c = lane * 4; c < H; c += 256) *(float4 *)(xr + c) = load_bf16x4(e + c);
    float mean, rstd;
    mb_row_stats(xr, H, lane, eps, mean, rstd);                // (a lane re-reads only what it wrote itself)
    for (int c = lane * 4; c < H; c += 256) {
        const float4 f = *(const float4 *)(xr + c), g = *(const float4 *)(w + c);
        const float4 y = {(f.x - mean) * rstd * g.x, (f.y - mean) * rstd * g.y, (f.z - mean) * rstd * g.z, (f.w - mean) * rstd * g.w};
        *(float4 *)(xr + c) = y;
        store_bf16x4(h16 + t * H + c, y.x, y.y, y.z, y.w);
    }
}

// one wave per token t < T: x32 += y32 (the sub-layer's float32 GEMM output), then h16 = LayerNorm(x32; w) (w == NULL: the add only).
// The LayerNorm twin of k_dec_add_rmsnorm. The row stays in registers between the add, the two reductions and the store (NJ float4 per
// lane, NJ = ceil(H / 256)): one pass over memory. The statistics: row_ln_stats (stack.h), as mb_row_stats.
template <int NJ>
__global__ __launch_bounds__(256) void k_mb_add_ln(float *__restrict__ x32, const float *__restrict__ y32, int64_t T, int H, const float *__restrict__ w,
                                                   float eps, uint16_t *__restrict__ h16) {
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= T) return;
    float4 f[NJ];
    const float s = row_load_sum<true>(x32 + t * H, y32 + t * H, H, lane, f);
    if (!w) return;
    float mean, rstd;
    row_ln_stats(f, s, H, lane, eps, mean, rstd);
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int c = lane * 4 + j * 256;
        if (c < H) {
            const float4 g = *(const float4 *)(w + c);
            *(uint2 *)(h16 + t * H + c) = uint2{mt::pack_bf16x2((f[j].x - mean) * rstd * g.x, (f[j].y - mean) * rstd * g.y),
                                                mt::pack_bf16x2((f[j].z - mean) * rstd * g.z, (f[j].w - mean) * rstd * g.w)};
        }
    }
}

// RoPE in place on the q and k rows the QKV GEMM wrote ([T][H] bf16 each, q already scaled: the rotation is linear). One thread per
// (token, q | k, head, 8-element chunk c < 4): it takes elements 8 c .. 8 c + 7 and their rotate_half partners 32 + 8 c .. of one head,
// 16 bytes each: x' = x cos + rot(x) sin, rot(x)[d] = -x[d + 32], rot(x)[d + 32] = x[d], at position t % S. rc / rs: the layer's
// table [n_pos][32].
__global__ __launch_bounds__(256) void k_mb_rope(uint16_t *__restrict__ q, uint16_t *__restrict__ k, int64_t T, int S, int H, const float *__restrict__ rc,
                                                 const float *__restrict__ rs) {
    const int per_tok = H / 8;                                 // 2 (q | k) x heads x 4 chunks
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t t = idx / per_tok;
    if (t >= T) return;
    const int rem = (int)(idx - t * per_tok), c = rem & 3, hs = rem >> 2, heads = H / MB_HD;
    const int sq = (int)(t % S);
    uint16_t *row = (hs < heads ? q + t * H + hs * MB_HD : k + t * H + (hs - heads) * MB_HD) + c * 8;
    const uint4 a = *(const uint4 *)row, b = *(const uint4 *)(row + 32);
    const float4 c0 = *(const float4 *)(rc + (int64_t)sq * 32 + c * 8), c1 = *(const float4 *)(rc + (int64_t)sq * 32 + c * 8 + 4);
    const float4 s0 = *(const float4 *)(rs + (int64_t)sq * 32 + c * 8), s1 = *(const float4 *)(rs + (int64_t)sq * 32 + c * 8 + 4);
    const float cs[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w}, sn[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
    uint32_t ao[4], bo[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float x0l = bf16_to_f32((uint16_t)aw[i]), x0h = bf16_to_f32((uint16_t)(aw[i] >> 16));
        const float x1l = bf16_to_f32((uint16_t)bw[i]), x1h = bf16_to_f32((uint16_t)(bw[i] >> 16));
        ao[i] = (uint32_t)f32_to_bf16(x0l * cs[2 * i] - x1l * sn[2 * i]) | ((uint32_t)f32_to_bf16(x0h * cs[2 * i + 1] - x1h * sn[2 * i + 1]) << 16);
        bo[i] = (uint32_t)f32_to_bf16(x1l * cs[2 * i] + x0l * sn[2 * i]) | ((uint32_t)f32_to_bf16(x1h * cs[2 * i + 1] + x0h * sn[2 * i + 1]) << 16);
    }
    *(uint4 *)row = uint4{ao[0], ao[1], ao[2], ao[3]};
    *(uint4 *)(row + 32) = uint4{bo[0], bo[1], bo[2], bo[3]};
}

// Pooling, stage 1 (pool_part of stack.h) over the pooled tokens of a row -- mean: its length; cls: token 0 --, the per-token transform
// y_t = (x_t - mean_t) rstd_t: the final LayerNorm without its weight.
struct MbFinalNorm {
    float eps; int pooling;
    struct Token {
        float mean, rstd;
        __device__ float apply(float x) const { return (x - mean) * rstd; }
    };
    __device__ int count(int len) const { return pooled_count(len, pooling); }
    __device__ Token begin(const float *xr, int H, int lane) const {
        Token t;
        mb_row_stats(xr, H, lane, eps, t.mean, t.rstd);
        return t;
    }
};
__global__ __launch_bounds__(256) void k_mb_pool_part(const float *__restrict__ x32, const int *__restrict__ lens, int S, int H, float eps, int pooling,
                                                      float *__restrict__ part) {
    pool_part(x32, lens, S, H, MbFinalNorm{eps, pooling}, part);
}

// Pooling, stage 2 (pool_fin of stack.h) with the final LayerNorm's weight: sum * w / n, then the L2 normalisation
__global__ __launch_bounds__(256) void k_mb_pool_fin(const float *__restrict__ part, int nch, const int *__restrict__ lens, int H, const float *__restrict__ w,
                                                     int pooling, int normalise, float *__restrict__ out) {
    pool_fin<true>(part, nch, lens, H, w, pooling, normalise, out);
}

}  // namespace

// ---- launches: the one place each kernel's grid is spelled (the forward pass below and the single-launch tests call these) ----
int launch_mb_embed(const int *ids, int ld_ids, const int *lens, int lens_stride, int B, int S, int H, int vocab, const uint16_t *emb, const float *w,
                    float eps, float *x32, uint16_t *h16, int *mask, int *lens_out, hipStream_t st) {
    const unsigned rows4 = (unsigned)(((int64_t)B * S + 3) / 4);
    k_mb_embed<<<rows4, 256, 0, st>>>(ids, ld_ids, lens, lens_stride, B, S, H, vocab, emb, w, eps, x32, h16, mask, lens_out);
    AK_HIP(hipGetLastError());
    return 0;
}

int launch_mb_add_ln(float *x32, const float *y32, int64_t T, int H, const float *w, float eps, uint16_t *h16, hipStream_t st) {
    const unsigned rows4 = (unsigned)((T + 3) / 4);
    dispatch_nj(H, [&](auto nj) { k_mb_add_ln<decltype(nj)::value><<<rows4, 256, 0, st>>>(x32, y32, T, H, w, eps, h16); });
    AK_HIP(hipGetLastError());
    return 0;
}

int launch_mb_rope(uint16_t *q, uint16_t *k, int64_t T, int S, int H, const float *rc, const float *rs, hipStream_t st) {
    k_mb_rope<<<(unsigned)((T * (H / 8) + 255) / 256), 256, 0, st>>>(q, k, T, S, H, rc, rs);
    AK_HIP(hipGetLastError());
    return 0;
}

// both pooling stages: part [B][ceil(S / 64)][H] floats of workspace
int launch_mb_pool(const float *x32, const int *lens, int B, int S, int H, float eps, const float *w, int pooling, int normalise, float *part,
                   float *out, hipStream_t st) {
    return launch_pool_stages(
        B, S, H, [&](dim3 grid, size_t lds) { k_mb_pool_part<<<grid, 256, lds, st>>>(x32, lens, S, H, eps, pooling, part); },
        [&](int nch) { k_mb_pool_fin<<<B, 256, 0, st>>>(part, nch, lens, H, w, pooling, normalise, out); });
}

namespace {
// Wi [2 I][H] -> rows interleaved: row 2 j = Wi row j (GELU input), row 2 j + 1 = Wi row I + j (gate): gemm.hip MODE 8
struct MbLayer {
    const uint16_t *wqkv, *wo, *wi, *wo2;      // wi (interleaved) is owned, wo2 too when the intermediate size is padded
    const float *attn_norm, *mlp_norm;         // attn_norm of layer 0: not read
    bool global;
};
struct MBert : Enc64 {
    AkModernBertConfig cfg;
    const uint16_t *emb = nullptr; const float *emb_norm = nullptr, *final_norm = nullptr;
    std::vector<MbLayer> layers;
    float *rope_c[2] = {nullptr, nullptr}, *rope_s[2] = {nullptr, nullptr};      // [0] local theta, [1] global theta

    int forward(const int32_t *ids, int ld_ids, const int32_t *lens_in, int lens_stride, int B, int S, int pooling, int normalise, float *out,
                hipStream_t st) {
        const float eps = cfg.norm_eps;
        const int64_t T = (int64_t)B * S, tpad = (T + 255) / 256 * 256;
        if (reserve(tpad, B)) return -10;
        if (launch_mb_embed(ids, ld_ids, lens_in, lens_stride, B, S, H, cfg.vocab_size, emb, emb_norm, eps, x32, h16, mask, lens, st)) return -10;
        for (size_t l = 0; l < layers.size(); l++) {
            const MbLayer &ly = layers[l];
            const int tb = ly.global ? 1 : 0;
            // x += attention(h) Wo^T; h = LayerNorm(x; mlp_norm)
            if (attention_block(tpad, B, S, ly.wqkv, ly.wo, rope_c[tb], rope_s[tb], ly.global ? -1 : cfg.half_window, st)) return -10;
            if (launch_mb_add_ln(x32, y32, T, H, ly.mlp_norm, eps, h16, st)) return -10;
            // x += (gelu(h Wi_a^T) (h Wi_g^T)) Wo^T; h = LayerNorm(x; next layer's attn_norm) (after the last layer: the add only, the
            // pool applies final_norm)
            if (ffn_block(8, tpad, ly.wi, ly.wo2, st)) return -10;
            const float *wn = l + 1 < layers.size() ? layers[l + 1].attn_norm : nullptr;
            if (launch_mb_add_ln(x32, y32, T, H, wn, eps, h16, st)) return -10;
        }
        return launch_mb_pool(x32, lens, B, S, H, eps, final_norm, pooling, normalise, part, out, st) ? -10 : 0;
    }
};
}  // namespace

}  // namespace ak

using namespace ak;

extern "C" int ak_mbert_destroy(ak_mbert_t h) { return stack_destroy<MBert>(h); }

extern "C" int ak_mbert_create(const AkModernBertConfig *cfg, const void *const *w, int n_weights, ak_mbert_t *out) {
    AK_BIND();
    if (!cfg || !w || !out) AK_FAIL(-1, "ak_mbert_create: NULL argument");
    *out = nullptr;
    const AkModernBertConfig c = *cfg;
    const int H = c.hidden, I = c.intermediate, L = c.layers;
    if (Enc64::check_sizes("ak_mbert_create", H, I, c.heads, L, c.vocab_size, c.max_position, true)) return -1;
    if (c.half_window < 1) AK_FAIL(-1, "ak_mbert_create: half_window must be >= 1");
    if (!(c.norm_eps > 0.f) || !(c.global_rope_theta > 0.f) || !(c.local_rope_theta > 0.f)) AK_FAIL(-1, "ak_mbert_create: norm_eps and the rope thetas must be positive");
    if (n_weights != 3 + 6 * L) AK_FAIL(-1, "ak_mbert_create: expected 3 + 6 * layers weight pointers");
    for (int i = 0; i < n_weights; i++)
        if (!w[i]) AK_FAIL(-1, "ak_mbert_create: NULL weight pointer");
    MBert *d = new MBert();
    d->cfg = c;
    d->emb = (const uint16_t *)w[0];
    d->emb_norm = (const float *)w[1];
    d->final_norm = (const float *)w[2];
    auto fail = [&](const char *what) { return enc64_create_failed(d, "ak_mbert_create", what); };
    if (const char *what = d->init(H, c.heads, I, c.max_position)) return fail(what);
    for (int tb = 0; tb < 2; tb++)
        if (!d->rope_table(tb ? c.global_rope_theta : c.local_rope_theta, &d->rope_c[tb], &d->rope_s[tb])) return fail("rotary table upload failed");
    for (int l = 0; l < L; l++) {
        const void *const *p = w + 3 + 6 * l;      // attn_norm wqkv wo mlp_norm wi mlp_wo
        MbLayer ly{};
        if (const char *what = d->prepare_gated(p[4], (const uint16_t *)p[4] + (size_t)I * H, I, p[5], &ly.wi, &ly.wo2)) return fail(what);
        ly.attn_norm = (const float *)p[0]; ly.wqkv = (const uint16_t *)p[1]; ly.wo = (const uint16_t *)p[2];
        ly.mlp_norm = (const float *)p[3];
        ly.global = c.layer_global[l] != 0;
        d->layers.push_back(ly);
    }
    if (hipDeviceSynchronize() != hipSuccess) return fail("weight preparation failed");
    *out = d;
    return 0;
}

extern "C" int ak_mbert_forward_lens(ak_mbert_t h, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S, int pooling,
                                     int normalise, float *out, void *stream) {
    return enc64_forward_lens<MBert>("ak_mbert_forward_lens", h, ids, ld_ids, lens, lens_stride, B, S, pooling, normalise, out, stream);
}
