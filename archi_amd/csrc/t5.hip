// t5.hip -- the T5 encoder forward pass (sentence-transformers/gtr-t5-base / -large, sentence-t5-base / -large, the GTR-initialised
// instructor models as plain sentence-transformers directories) behind ak_t5_*: orchestration and the small kernels. As HF
// T5EncoderModel (no bias in any Linear, no embedding scale, no position table, T5LayerNorm = RMSNorm without a mean):
//   x = shared[id]; h = bf16(RMSNorm(x; block 0's ln0))   k_t5_embed (float32 x)
// per layer (pre-norm):
//   q | k | v = h [Wq; Wk; Wv]^T                       k_gemm MODE 0 (gemm.hip): q scaled by log2(e) ALONE -- T5 does not scale its
//                                                      scores --, k as [T][H], V transposed
//   a = softmax(q k^T + bias(key - query) + pad mask) v   k_attn_long_relbias (attn_long.hip): position enters here only, as the
//                                                      learned per-head bias of the T5 bucket of key - query. The bidirectional bucket
//                                                      saturates at relative_attention_max_distance D, so the bias is a function of
//                                                      clamp(key - query, -D, D): ONE table [heads][2 D + 1] for all layers (block 0's
//                                                      weight), built and scaled by log2(e) by the binding (archi_amd/t5.py)
//   x += a Wo^T; h = bf16(RMSNorm(x; ln1))             k_gemm MODE 2 (float32 out) + k_dec_add_rmsnorm (decoder128.hip)
//   f = relu(h Wi^T)                                   k_gemm MODE 10 (T5 v1.0: feed_forward_proj relu), or
//   f = gelu_new(h Wi0^T) (h Wi1^T)                    k_gemm MODE 9 (T5 v1.1: gated-gelu; Wi0 / Wi1 rows interleaved at create)
//   x += f Wo_ff^T; h = bf16(RMSNorm(x; next ln0))     k_gemm MODE 2 + k_dec_add_rmsnorm (after the last layer: the add alone)
// then the final_layer_norm per token, mean / cls pooling over the valid tokens (k_t5_pool_part / _fin on stack.h's pool bodies: the
// norm per token BEFORE the mean, its weight after it), the 0 - 2 Dense matrices of the sentence-transformers tail in float32
// (k_gm_dense, gemma.hip) and the L2 normalisation (k_gm_l2). The residual stream x is float32 throughout; GEMM operands are bf16.
// Token counts are padded to the GEMM tile (256) as in mbert.hip. enc64.h holds the workspace, both blocks and the body of
// ak_t5_forward_lens. Nothing here reads the environment.
// LDS per workgroup: k_t5_embed none; k_t5_pool_part 4 * H * 4 bytes (dynamic: 12 KB at H = 768); k_t5_pool_fin 16 bytes.
#include <algorithm>

#include "enc64.h"

namespace ak {

namespace {
constexpr int T5_MAX_DENSE = 4096;
constexpr float LOG2E = 1.4426950408889634f;

// one wave per token slot t < B * S: ids past the row's length read as 0; x32 = shared[id] (float32 of the bf16 row), h16 =
// bf16(RMSNorm(x32) * w). Also the int key mask (slot < length) the attention kernel stages, and per row the clamped length.
__global__ __launch_bounds__(256) void k_t5_embed(const int *__restrict__ ids, int ld_ids, const int *__restrict__ lens, int lens_stride, int B, int S,
                                                  int H, int vocab, const uint16_t *__restrict__ emb, const float *__restrict__ w, float eps,
                                                  float *__restrict__ x32, uint16_t *__restrict__ h16, int *__restrict__ mask,
                                                  int *__restrict__ lens_out) {
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= (int64_t)B * S) return;
    const int id = token_slot<true>(ids, ld_ids, lens, lens_stride, S, vocab, t, lane, mask, lens_out);
    const uint16_t *e = emb + (int64_t)id * H;
    float *xr = x32 + t * H;
    float ss = 0.f;
    for (int c = lane * 4; c < H; c += 256) {
        const float4 f = load_bf16x4(e + c);
        *(float4 *)(xr + c) = f;
        ss += f.x * f.x + f.y * f.y + f.z * f.z + f.w * f.w;
    }
    const float rs = rsqrtf(wave_sum(ss) / (float)H + eps);
    for (int c = lane * 4; c < H; c += 256) {
        const float4 f = *(const float4 *)(xr + c), g = *(const float4 *)(w + c);
        store_bf16x4(h16 + t * H + c, f.x * rs * g.x, f.y * rs * g.y, f.z * rs * g.z, f.w * rs * g.w);
    }
}

// Pooling, stage 1 (pool_part of stack.h) over the pooled tokens of a row -- mean: its length; cls: token 0 --, the per-token
// transform y_t = x_t rs_t, rs_t = 1 / sqrt(mean x_t^2 + eps): the final_layer_norm without its weight, per token, BEFORE the mean.
struct T5FinalNorm {
    float eps;
    int pooling;
    struct Token {
        float rs;
        __device__ float apply(float x) const { return x * rs; }
    };
    __device__ int count(int len) const { return pooled_count(len, pooling); }
    __device__ Token begin(const float *xr, int H, int lane) const {
        float ss = 0.f;
        for (int c = lane * 4; c < H; c += 256) {
            const float4 f = *(const float4 *)(xr + c);
            ss += f.x * f.x + f.y * f.y + f.z * f.z + f.w * f.w;
        }
        return Token{rsqrtf(wave_sum(ss) / (float)H + eps)};
    }
};
__global__ __launch_bounds__(256) void k_t5_pool_part(const float *__restrict__ x32, const int *__restrict__ lens, int S, int H, float eps, int pooling,
                                                      float *__restrict__ part) {
    pool_part(x32, lens, S, H, T5FinalNorm{eps, pooling}, part);
}

// Pooling, stage 2 (pool_fin of stack.h): the chunk sums times the final norm's weight, / n; not normalised (the Dense head follows)
__global__ __launch_bounds__(256) void k_t5_pool_fin(const float *__restrict__ part, int nch, const int *__restrict__ lens, int H,
                                                     const float *__restrict__ w, int pooling, float *__restrict__ pooled) {
    pool_fin<true>(part, nch, lens, H, w, pooling, 0, pooled);
}
}  // namespace

// ---- launches: the one place each kernel's grid is spelled ----
int launch_t5_embed(const int *ids, int ld_ids, const int *lens, int lens_stride, int B, int S, int H, int vocab, const uint16_t *emb, const float *w,
                    float eps, float *x32, uint16_t *h16, int *mask, int *lens_out, hipStream_t st) {
    const unsigned rows4 = (unsigned)(((int64_t)B * S + 3) / 4);
    k_t5_embed<<<rows4, 256, 0, st>>>(ids, ld_ids, lens, lens_stride, B, S, H, vocab, emb, w, eps, x32, h16, mask, lens_out);
    AK_HIP(hipGetLastError());
    return 0;
}

// both pooling stages: part [B][ceil(S / 64)][H] floats of workspace -> pooled [B][H]
int launch_t5_pool(const float *x32, const int *lens, int B, int S, int H, const float *w, float eps, int pooling, float *part, float *pooled,
                   hipStream_t st) {
    return launch_pool_stages(
        B, S, H, [&](dim3 grid, size_t lds) { k_t5_pool_part<<<grid, 256, lds, st>>>(x32, lens, S, H, eps, pooling, part); },
        [&](int nch) { k_t5_pool_fin<<<B, 256, 0, st>>>(part, nch, lens, H, w, pooling, pooled); });
}

namespace {
struct T5Layer {
    const uint16_t *wqkv, *wo, *wi, *wo_ff;    // wqkv (concatenated) is owned; wi (interleaved when gated) and wo_ff too when they are padded
    const float *ln0, *ln1;
};
struct T5 : Enc64 {
    AkT5Config cfg;
    const uint16_t *emb = nullptr;
    const float *rbias = nullptr, *final_norm = nullptr;
    std::vector<T5Layer> layers;
    const float *dense[2] = {nullptr, nullptr};
    int dense_in[2] = {0, 0}, out_dim = 0;
    float *pool_a = nullptr, *pool_b = nullptr;

    int forward(const int32_t *ids, int ld_ids, const int32_t *lens_in, int lens_stride, int B, int S, int pooling, int normalise, float *out,
                hipStream_t st) {
        const float eps = cfg.ln_eps;
        const int64_t T = (int64_t)B * S, tpad = (T + 255) / 256 * 256;
        if (reserve(tpad, B)) return -10;
        if (launch_t5_embed(ids, ld_ids, lens_in, lens_stride, B, S, H, cfg.vocab_size, emb, layers[0].ln0, eps, x32, h16, mask, lens, st)) return -10;
        for (size_t l = 0; l < layers.size(); l++) {
            const T5Layer &ly = layers[l];
            // x += attention(h) Wo^T; h = RMSNorm(x; ln1)
            if (attention_block_relbias(tpad, B, S, ly.wqkv, ly.wo, LOG2E, rbias, cfg.max_distance, st)) return -10;
            if (launch_dec_add_rmsnorm(x32, y32, T, H, ly.ln1, eps, h16, st)) return -10;
            // x += FFN(h); h = RMSNorm(x; the next layer's ln0) (after the last layer: the add alone, the pool norms each token)
            if (cfg.gated ? ffn_block(9, tpad, ly.wi, ly.wo_ff, st) : ffn_block_plain(10, tpad, ly.wi, ly.wo_ff, st)) return -10;
            if (launch_dec_add_rmsnorm(x32, y32, T, H, l + 1 < layers.size() ? layers[l + 1].ln0 : nullptr, eps, h16, st)) return -10;
        }
        if (launch_t5_pool(x32, lens, B, S, H, final_norm, eps, pooling, part, pool_a, st)) return -10;
        float *cur = pool_a, *nxt = pool_b;
        for (int i = 0; i < cfg.n_dense; i++) {
            if (launch_gm_dense(cur, dense[i], B, cfg.dense_out[i], dense_in[i], nxt, st)) return -10;
            std::swap(cur, nxt);
        }
        return launch_gm_l2(cur, B, out_dim, normalise, out, st) ? -10 : 0;
    }
};
}  // namespace

}  // namespace ak

using namespace ak;

extern "C" int ak_t5_destroy(ak_t5_t h) { return stack_destroy<T5>(h); }

extern "C" int ak_t5_create(const AkT5Config *cfg, const void *const *w, int n_weights, ak_t5_t *out) {
    AK_BIND();
    if (!cfg || !w || !out) AK_FAIL(-1, "ak_t5_create: NULL argument");
    *out = nullptr;
    const AkT5Config c = *cfg;
    const int H = c.hidden, I = c.d_ff, L = c.layers;
    if (L <= 0 || c.vocab_size <= 0 || c.heads <= 0 || H <= 0 || I <= 0 || c.head_dim <= 0) AK_FAIL(-1, "ak_t5_create: sizes must be positive");
    if (L > AK_MBERT_MAX_LAYERS) AK_FAIL(-1, "ak_t5_create: more than AK_MBERT_MAX_LAYERS layers");
    if (c.head_dim != Enc64::HD) AK_FAIL(-1, "ak_t5_create: head size (head_dim) must be 64");
    if (c.heads * Enc64::HD != H) AK_FAIL(-1, "ak_t5_create: heads * 64 must equal hidden (the inner attention width is the model width)");
    if (H % 128 || H > Enc64::MAX_H) AK_FAIL(-1, "ak_t5_create: hidden must be a multiple of 128, <= 1024");
    if (I % 64) AK_FAIL(-1, "ak_t5_create: d_ff must be a multiple of 64");
    if (c.max_distance < 1 || c.max_distance > ATTN_RELBIAS_MAX_D) AK_FAIL(-1, "ak_t5_create: max_distance must be in [1, 4096]");
    if (!(c.ln_eps > 0.f)) AK_FAIL(-1, "ak_t5_create: ln_eps must be positive");
    if (c.gated != 0 && c.gated != 1) AK_FAIL(-1, "ak_t5_create: gated must be 0 (relu) or 1 (gated-gelu)");
    if (c.n_dense < 0 || c.n_dense > 2) AK_FAIL(-1, "ak_t5_create: n_dense must be 0, 1 or 2");
    for (int i = 0; i < c.n_dense; i++)
        if (c.dense_out[i] <= 0 || c.dense_out[i] > T5_MAX_DENSE || c.dense_out[i] % 4) AK_FAIL(-1, "ak_t5_create: dense_out must be a multiple of 4 in (0, 4096]");
    const int per = 8 + c.gated;
    if (n_weights != 3 + per * L + c.n_dense) AK_FAIL(-1, "ak_t5_create: expected 3 + (8 + gated) * layers + n_dense weight pointers");
    for (int i = 0; i < n_weights; i++)
        if (!w[i]) AK_FAIL(-1, "ak_t5_create: NULL weight pointer");
    T5 *d = new T5();
    d->cfg = c;
    d->emb = (const uint16_t *)w[0];
    d->rbias = (const float *)w[1];
    d->final_norm = (const float *)w[2];
    auto fail = [&](const char *what) { return enc64_create_failed(d, "ak_t5_create", what); };
    if (const char *what = d->init(H, c.heads, I, Enc64::MAX_S)) return fail(what);
    for (int l = 0; l < L; l++) {
        const void *const *p = w + 3 + per * l;        // ln0 wq wk wv wo ln1, then wi wo_ff (relu) or wi_0 wi_1 wo_ff (gated-gelu)
        T5Layer ly{};
        uint16_t *wqkv = d->dev_as<uint16_t>((size_t)3 * H * H);
        if (!wqkv) return fail("hipMalloc failed");
        if (!d->concat_rows(wqkv, H, {{p[1], (size_t)H}, {p[2], (size_t)H}, {p[3], (size_t)H}})) return fail("QKV concatenation failed");
        // gated: row 2 j = wi_0 row j (the GELU input), row 2 j + 1 = wi_1 row j (the linear gate): MODE 9's layout
        if (const char *what = c.gated ? d->prepare_gated(p[6], p[7], I, p[8], &ly.wi, &ly.wo_ff) : d->prepare_plain(p[6], I, p[7], &ly.wi, &ly.wo_ff))
            return fail(what);
        ly.wqkv = wqkv; ly.ln0 = (const float *)p[0]; ly.wo = (const uint16_t *)p[4]; ly.ln1 = (const float *)p[5];
        d->layers.push_back(ly);
    }
    int din = H;
    for (int i = 0; i < c.n_dense; i++) {
        d->dense[i] = (const float *)w[3 + per * L + i];
        d->dense_in[i] = din;
        din = c.dense_out[i];
    }
    d->out_dim = din;
    const size_t pw = (size_t)std::max(H, std::max(c.n_dense > 0 ? c.dense_out[0] : 0, c.n_dense > 1 ? c.dense_out[1] : 0)) * 4;      // widest pooled row
    d->buffer(&d->pool_a, 0, pw); d->buffer(&d->pool_b, 0, pw);
    if (hipDeviceSynchronize() != hipSuccess) return fail("weight preparation failed");
    *out = d;
    return 0;
}

extern "C" int ak_t5_forward_lens(ak_t5_t h, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S, int pooling,
                                  int normalise, float *out, void *stream) {
    return enc64_forward_lens<T5>("ak_t5_forward_lens", h, ids, ld_ids, lens, lens_stride, B, S, pooling, normalise, out, stream);
}
