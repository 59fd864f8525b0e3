// decoder128.hip -- the head-128 decoder stack: the forward pass of the Qwen3 (ak_decoder_*, decoder.hip), Mistral / Llama (ak_llama_*,
// llama.hip) and Qwen2 (ak_qwen2_*, qwen2.hip) embedders. The three are one architecture; LlFeatures (decoder128.h) names what a
// family adds. Per layer, as HF Qwen3Model / MistralModel / LlamaModel / Qwen2Model:
//   h = RMSNorm(x; ln_in)                         k_dec_embed (layer 0) / k_dec_add_rmsnorm
//   q | k | v = h [Wq; Wk; Wv]^T (+ [bq; bk; bv]) k_gemm MODE 3 (gemm.hip), one launch over the matrices concatenated at create; qkv_bias
//                                                 (Qwen2): the three biases concatenated in the same row order are the GEMM's bias, added
//                                                 in float32 before the bf16 store
//   q, k = RoPE(q | k)                            k_ll_rope: rotate_half RoPE at head size 128; qk_norm (Qwen3) k_dec_qk_rope: RMSNorm
//                                                 over each head (q_norm / k_norm) first; q scaled by log2(e) / sqrt(128); v copied
//   a = GQA softmax(q k^T + mask) v               attn_causal.hip: causal; with sliding_window = w > 0 key <= query and query - key <= w - 1
//                                                 (HF's sliding_window_overlay); bidirectional (cfg.bidirectional): every key below the
//                                                 length; split_attn (Qwen2 at 5 to 8 query heads per kv head): launch_attn_causal_split
//   x = x + a Wo^T                                k_gemm MODE 2 (fp32 out) + k_dec_add_rmsnorm (x += y; h = RMSNorm(x; ln_post))
//   x = x + (silu(h Wg^T) (h Wu^T)) Wd^T          k_gemm MODE 7 (SwiGLU epilogue, gate / up rows interleaved at create), MODE 2, add;
//                                                 unfused_swiglu (Qwen3's A/B switch): k_gemm MODE 3 2I wide + k_dec_swiglu
// then the final norm on each row's last valid token and L2 normalisation (k_dec_pool): sentence-transformers' lasttoken Pooling
// + Normalize; or (AK_POOL_MEAN, Llama and Qwen2) the mean over the valid tokens of the final norm per token, k_ll_pool_part / _fin on
// stack.h's pool body. The residual stream x is float32 throughout; GEMM operands are bf16. The rotary table comes from rope_theta (HF's
// default rotary embedding) or from inverse frequencies the caller hands over (ll_set_rope_inv_freq: rope_type llama3).
// Here: the family's kernels and their launches (launch_dec_embed, launch_dec_add_rmsnorm and launch_dec_pool also serve t5.hip), the
// config check, create and the layer loop. The plumbing shared with mbert.hip and gemma.hip is stack.h / stack.hip: the token-slot
// prologue and the row helpers, the L2 tail, the workspace, the weight preparation at create, the rotary tables, the GemmArgs.
#include <algorithm>
#include <cmath>

#include "decoder128.h"

namespace ak {

// ---- kernels ------------------------------------------------------------------------------------------------------------
// one wave per token slot t < B * S: ids past the row's length read as 0; x32 = embed_tokens[id] (float32 of the bf16 row),
// h16 = RMSNorm(x) * ln_in of layer 0. The wave of a row's slot 0 stores the clamped length (attention and pooling read it).
__global__ __launch_bounds__(256) void k_dec_embed(const int *__restrict__ ids, int ld_ids, const int *__restrict__ lens, int lens_stride, int B, int S,
                                                   int H, int vocab, const uint16_t *__restrict__ emb, const float *__restrict__ w, float eps,
                                                   float *__restrict__ x32, uint16_t *__restrict__ h16, int *__restrict__ lens_out) {
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= (int64_t)B * S) return;
    const int id = token_slot<false>(ids, ld_ids, lens, lens_stride, S, vocab, t, lane, nullptr, lens_out);
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

// one wave per token t < T: x32 += y32 (the sub-layer's float32 GEMM output), then h16 = RMSNorm(x32) * w (w == NULL: the add only)
__global__ __launch_bounds__(256) void k_dec_add_rmsnorm(float *__restrict__ x32, const float *__restrict__ y32, int64_t T, int H,
                                                         const float *__restrict__ w, float eps, uint16_t *__restrict__ h16) {
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= T) return;
    float *xr = x32 + t * H;
    const float *yr = y32 + t * H;
    float ss = 0.f;
    for (int c = lane * 4; c < H; c += 256) {
        float4 f = *(const float4 *)(xr + c);
        const float4 y = *(const float4 *)(yr + c);
        f.x += y.x; f.y += y.y; f.z += y.z; f.w += y.w;
        *(float4 *)(xr + c) = f;
        ss += f.x * f.x + f.y * f.y + f.z * f.z + f.w * f.w;
    }
    if (!w) return;
    const float rs = rsqrtf(wave_sum(ss) / (float)H + eps);
    for (int c = lane * 4; c < H; c += 256) {
        const float4 f = *(const float4 *)(xr + c), g = *(const float4 *)(w + c);
        store_bf16x4(h16 + t * H + c, f.x * rs * g.x, f.y * rs * g.y, f.z * rs * g.z, f.w * rs * g.w);
    }
}

// one workgroup (4 waves) per token t < B * S; a wave takes one head slot of the QKV row at a time (nq query heads, nkv key heads,
// nkv value heads), a lane the pair (d, d + 64) that rotate_half couples: q and k get -- NORM: RMSNorm over the head (q_norm / k_norm),
// then -- RoPE at position t % S: x'[d] = x[d] cos - x[d + 64] sin, x'[d + 64] = x[d + 64] cos + x[d] sin; q then the scale
// log2(e) / sqrt(128); v is copied. Out: q [B][nq][S][128], k / v [B][nkv][S][128].
template <bool NORM>
__device__ inline void rope_body(const uint16_t *__restrict__ qkv, int S, int nq, int nkv, const float *__restrict__ qn, const float *__restrict__ kn,
                                 float eps, const float *__restrict__ rc, const float *__restrict__ rsn, float qscale, uint16_t *__restrict__ q,
                                 uint16_t *__restrict__ k, uint16_t *__restrict__ v) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = (int)(t / S), sq = (int)(t - (int64_t)b * S);
    const int slots = nq + 2 * nkv;
    const uint16_t *row = qkv + t * (int64_t)slots * LL_HD;
    const float c = rc[(int64_t)sq * 64 + lane], sn = rsn[(int64_t)sq * 64 + lane];
    for (int hs = wave; hs < slots; hs += 4) {
        const float x0 = bf16_to_f32(row[hs * LL_HD + lane]), x1 = bf16_to_f32(row[hs * LL_HD + 64 + lane]);
        uint16_t *dst;
        float o0 = x0, o1 = x1;
        if (hs < nq + nkv) {
            const bool isq = hs < nq;
            float y0 = x0, y1 = x1;
            if constexpr (NORM) {
                const float *wn = isq ? qn : kn;
                const float rs = rsqrtf(wave_sum(x0 * x0 + x1 * x1) * (1.0f / LL_HD) + eps);
                y0 = x0 * rs * wn[lane]; y1 = x1 * rs * wn[64 + lane];
            }
            o0 = y0 * c - y1 * sn;
            o1 = y1 * c + y0 * sn;
            if (isq) { o0 *= qscale; o1 *= qscale; dst = q + (((int64_t)b * nq + hs) * S + sq) * LL_HD; }
            else dst = k + (((int64_t)b * nkv + (hs - nq)) * S + sq) * LL_HD;
        } else {
            dst = v + (((int64_t)b * nkv + (hs - nq - nkv)) * S + sq) * LL_HD;
        }
        dst[lane] = f32_to_bf16(o0);
        dst[64 + lane] = f32_to_bf16(o1);
    }
}
__global__ __launch_bounds__(256) void k_dec_qk_rope(const uint16_t *__restrict__ qkv, int S, int nq, int nkv, const float *__restrict__ qn,
                                                     const float *__restrict__ kn, float eps, const float *__restrict__ rc, const float *__restrict__ rsn,
                                                     float qscale, uint16_t *__restrict__ q, uint16_t *__restrict__ k, uint16_t *__restrict__ v) {
    rope_body<true>(qkv, S, nq, nkv, qn, kn, eps, rc, rsn, qscale, q, k, v);
}
__global__ __launch_bounds__(256) void k_ll_rope(const uint16_t *__restrict__ qkv, int S, int nq, int nkv, const float *__restrict__ rc,
                                                 const float *__restrict__ rsn, float qscale, uint16_t *__restrict__ q, uint16_t *__restrict__ k,
                                                 uint16_t *__restrict__ v) {
    rope_body<false>(qkv, S, nq, nkv, nullptr, nullptr, 0.f, rc, rsn, qscale, q, k, v);
}

// one workgroup per row b: the final norm of the row's last valid token (b * S + len - 1), then L2 normalisation (normalise != 0);
// a row of length 0 embeds to zeros
__global__ __launch_bounds__(256) void k_dec_pool(const float *__restrict__ x32, const int *__restrict__ lens, int S, int H, const float *__restrict__ w,
                                                  float eps, int normalise, float *__restrict__ out) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = lens[b];
    float *o = out + (int64_t)b * H;
    if (len <= 0) {
        for (int c = tid; c < H; c += 256) o[c] = 0.f;
        return;
    }
    const float *xr = x32 + ((int64_t)b * S + len - 1) * H;
    float ss = 0.f;
    for (int c = tid; c < H; c += 256) ss += xr[c] * xr[c];
    ss = wave_sum(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    const float rs = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)H + eps);
    float s2 = 0.f;
    for (int c = tid; c < H; c += 256) { const float y = xr[c] * rs * w[c]; s2 += y * y; }
    const float sc = block_l2_scale(s2, lane, wave, normalise);
    for (int c = tid; c < H; c += 256) o[c] = xr[c] * rs * w[c] * sc;
}

// the un-fused SwiGLU (A/B baseline of k_gemm MODE 7; AK_DEC_SWIGLU=unfused): gu [T][2 I] bf16 rows in the interleaved order
// (g_j, u_j) -> f [T][I] = silu(g) u
__global__ __launch_bounds__(256) void k_dec_swiglu(const uint16_t *__restrict__ gu, int64_t n, uint16_t *__restrict__ f) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = ((const uint32_t *)gu)[i];
    const float g = bf16_to_f32((uint16_t)p), u = bf16_to_f32((uint16_t)(p >> 16));
    f[i] = f32_to_bf16(g * u / (1.0f + __expf(-g)));
}

namespace {
// Mean pooling, stage 1 (pool_part of stack.h, in column slices of 1024 features: hidden is 4096) over the tokens below the row's length,
// the per-token transform y_t = x_t rs_t, rs_t = 1 / sqrt(mean x_t^2 + eps): the final RMSNorm without its weight, per token, BEFORE the mean.
struct LlFinalNorm {
    float eps;
    struct Token {
        float rs;
        __device__ float apply(float x) const { return x * rs; }
    };
    __device__ int count(int len) const { return len <= 0 ? 0 : len; }
    __device__ Token begin(const float *xr, int H, int lane) const {
        float ss = 0.f;
        for (int c = lane * 4; c < H; c += 256) {
            const float4 f = *(const float4 *)(xr + c);
            ss += f.x * f.x + f.y * f.y + f.z * f.z + f.w * f.w;
        }
        return Token{rsqrtf(wave_sum(ss) / (float)H + eps)};
    }
};
__global__ __launch_bounds__(256) void k_ll_pool_part(const float *__restrict__ x32, const int *__restrict__ lens, int S, int H, float eps,
                                                      float *__restrict__ part) {
    pool_part(x32, lens, S, H, LlFinalNorm{eps}, part);
}

// Mean pooling, stage 2: pool_fin<true> of stack.h restated for rows wider than a workgroup holds in registers (one workgroup per row b,
// any H): the chunk sums added in chunk order, * w[c] / n, written, then scaled in place by the L2 tail. A row of length 0 embeds to zeros.
__global__ __launch_bounds__(256) void k_ll_pool_fin(const float *__restrict__ part, int nch, const int *__restrict__ lens, int H,
                                                     const float *__restrict__ w, int normalise, float *__restrict__ out) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lens[b];
    float *o = out + (int64_t)b * H;
    if (n <= 0) {
        for (int c = tid; c < H; c += 256) o[c] = 0.f;
        return;
    }
    const int used = (n + POOL_CHUNK - 1) / POOL_CHUNK;
    const float inv_n = 1.0f / (float)n;
    float s2 = 0.f;
    for (int c = tid; c < H; c += 256) {
        float y = 0.f;
        for (int ck = 0; ck < used; ck++) y += part[((int64_t)b * nch + ck) * H + c];
        y = y * w[c] * inv_n;
        o[c] = y;
        s2 += y * y;
    }
    const float sc = block_l2_scale(s2, lane, wave, normalise);
    for (int c = tid; c < H; c += 256) o[c] = o[c] * sc;      // (a thread rescales what it wrote itself)
}
}  // namespace

// ---- launches: the one place each kernel's grid is spelled (the forward pass below and the single-launch tests call these) ----
int launch_dec_embed(const int *ids, int ld_ids, const int *lens, int lens_stride, int B, int S, int H, int vocab, const uint16_t *emb, const float *w,
                     float eps, float *x32, uint16_t *h16, int *lens_out, hipStream_t st) {
    const unsigned rows4 = (unsigned)(((int64_t)B * S + 3) / 4);
    k_dec_embed<<<rows4, 256, 0, st>>>(ids, ld_ids, lens, lens_stride, B, S, H, vocab, emb, w, eps, x32, h16, lens_out);
    AK_HIP(hipGetLastError());
    return 0;
}

int launch_dec_add_rmsnorm(float *x32, const float *y32, int64_t T, int H, const float *w, float eps, uint16_t *h16, hipStream_t st) {
    const unsigned rows4 = (unsigned)((T + 3) / 4);
    k_dec_add_rmsnorm<<<rows4, 256, 0, st>>>(x32, y32, T, H, w, eps, h16);
    AK_HIP(hipGetLastError());
    return 0;
}

// qn != NULL: k_dec_qk_rope with the head norms qn / kn, else k_ll_rope
static int launch_rope(const uint16_t *qkv, int B, int S, int nq, int nkv, const float *qn, const float *kn, float eps, const float *rc,
                       const float *rs, float qscale, uint16_t *q, uint16_t *k, uint16_t *v, hipStream_t st) {
    const int64_t T = (int64_t)B * S;
    if (B <= 0 || S <= 0 || nq <= 0 || nkv <= 0 || T > 0x7fffffff) AK_FAIL(-1, "rope: bad shape");
    if (qn) k_dec_qk_rope<<<(unsigned)T, 256, 0, st>>>(qkv, S, nq, nkv, qn, kn, eps, rc, rs, qscale, q, k, v);
    else k_ll_rope<<<(unsigned)T, 256, 0, st>>>(qkv, S, nq, nkv, rc, rs, qscale, q, k, v);
    AK_HIP(hipGetLastError());
    return 0;
}
int launch_dec_qk_rope(const uint16_t *qkv, int B, int S, int nq, int nkv, const float *qn, const float *kn, float eps, const float *rc,
                       const float *rs, float qscale, uint16_t *q, uint16_t *k, uint16_t *v, hipStream_t st) {
    if (!qn || !kn) AK_FAIL(-1, "dec_qk_rope: NULL head norm");
    return launch_rope(qkv, B, S, nq, nkv, qn, kn, eps, rc, rs, qscale, q, k, v, st);
}
int launch_ll_rope(const uint16_t *qkv, int B, int S, int nq, int nkv, const float *rc, const float *rs, float qscale, uint16_t *q, uint16_t *k,
                   uint16_t *v, hipStream_t st) {
    return launch_rope(qkv, B, S, nq, nkv, nullptr, nullptr, 0.f, rc, rs, qscale, q, k, v, st);
}

int launch_dec_pool(const float *x32, const int *lens, int B, int S, int H, const float *w, float eps, int normalise, float *out, hipStream_t st) {
    k_dec_pool<<<B, 256, 0, st>>>(x32, lens, S, H, w, eps, normalise, out);
    AK_HIP(hipGetLastError());
    return 0;
}

int launch_ll_pool(const float *x32, const int *lens, int B, int S, int H, const float *w, float eps, int normalise, float *part, float *out,
                   hipStream_t st) {
    if (B <= 0 || B > 65535 || S <= 0 || H <= 0 || H % 128) AK_FAIL(-1, "ll_pool: bad shape");
    const int nch = (S + POOL_CHUNK - 1) / POOL_CHUNK, nz = (H + POOL_MAX_H - 1) / POOL_MAX_H, wmax = H < POOL_MAX_H ? H : POOL_MAX_H;
    k_ll_pool_part<<<dim3((unsigned)nch, (unsigned)B, (unsigned)nz), 256, (size_t)4 * wmax * 4, st>>>(x32, lens, S, H, eps, part);
    AK_HIP(hipGetLastError());
    k_ll_pool_fin<<<B, 256, 0, st>>>(part, nch, lens, H, w, normalise, out);
    AK_HIP(hipGetLastError());
    return 0;
}

// ---- the layer loop ----------------------------------------------------------------------------------------------------------
static int ll_forward_locked(Llama &d, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S, int pooling, int normalise, float *out,
                      hipStream_t st) {
    const AkLlamaConfig &c = d.cfg;
    const int H = c.hidden, I = c.intermediate, nq = c.q_heads, nkv = c.kv_heads, nqkv = (nq + 2 * nkv) * LL_HD;
    const int64_t T = (int64_t)B * S, tpad = (T + 255) / 256 * 256;
    if (d.reserve(tpad, B)) return -10;
    const float qscale = 1.4426950408889634f / sqrtf((float)LL_HD);
    if (launch_dec_embed(ids, ld_ids, lens, lens_stride, B, S, H, c.vocab_size, d.emb, d.layers[0].ln_in, c.rms_eps, d.x32, d.h16, d.lens, st)) return -10;
    for (size_t l = 0; l < d.layers.size(); l++) {
        const LlLayer &ly = d.layers[l];
        // q | k | v (+ the layer's q | k | v bias in float32 before the bf16 store: Qwen2)
        GemmArgs gq = d.gemm_bf16(tpad, d.h16, ly.wqkv, nqkv, H, d.qkv);
        if (ly.bqkv) gq.bias = ly.bqkv;
        if (launch_gemm(3, gq, st)) return -10;
        if (launch_rope(d.qkv, B, S, nq, nkv, ly.qn, ly.kn, c.rms_eps, d.rope_c, d.rope_s, qscale, d.q, d.k, d.v, st)) return -10;
        CausalAttnArgs aa{d.q, d.k, d.v, d.lens, d.ctx, B, S, nq, nkv};
        aa.window = c.sliding_window;
        aa.bidirectional = c.bidirectional;
        if (d.feat.split_attn ? launch_attn_causal_split(aa, st) : launch_attn_causal(aa, st)) return -10;
        // x += ctx Wo^T; h = RMSNorm(x; ln_post)
        if (launch_gemm(2, d.gemm_f32(tpad, d.ctx, ly.wo, H, nq * LL_HD, d.y32), st)) return -10;
        if (launch_dec_add_rmsnorm(d.x32, d.y32, T, H, ly.ln_post, c.rms_eps, d.h16, st)) return -10;
        // f = silu(h Wg^T) (h Wu^T)
        if (d.feat.unfused_swiglu) {
            uint16_t *gu = d.f + tpad * I;                      // the 2I-wide product behind f (create registered f 3 I wide)
            if (launch_gemm(3, d.gemm_bf16(tpad, d.h16, ly.wgu, 2 * I, H, gu), st)) return -10;
            const int64_t n = tpad * I;
            k_dec_swiglu<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(gu, n, d.f);
            AK_HIP(hipGetLastError());
        } else if (launch_gemm(7, d.gemm_gated(tpad, d.h16, ly.wgu, I, H, d.f), st)) {
            return -10;
        }
        // x += f Wd^T; h = RMSNorm(x; next layer's ln_in) (after the last layer: the add only, the pool applies the final norm)
        if (launch_gemm(2, d.gemm_f32(tpad, d.f, ly.wd, H, I, d.y32), st)) return -10;
        const float *wn = l + 1 < d.layers.size() ? d.layers[l + 1].ln_in : nullptr;
        if (launch_dec_add_rmsnorm(d.x32, d.y32, T, H, wn, c.rms_eps, d.h16, st)) return -10;
    }
    if (pooling == AK_POOL_MEAN) return launch_ll_pool(d.x32, d.lens, B, S, H, d.norm, c.rms_eps, normalise, d.part, out, st) ? -10 : 0;
    return launch_dec_pool(d.x32, d.lens, B, S, H, d.norm, c.rms_eps, normalise, out, st) ? -10 : 0;
}

// ---- create ------------------------------------------------------------------------------------------------------------------
int ll_check_config(const char *fn, const AkLlamaConfig &c, const LlFeatures &feat, int max_group, const void *const *w, int n_weights) {
    const std::string f = std::string(fn) + ": ";
    const int H = c.hidden, I = c.intermediate, L = c.layers, nq = c.q_heads, nkv = c.kv_heads;
    if (L <= 0 || c.vocab_size <= 0 || nq <= 0 || nkv <= 0 || H <= 0 || I <= 0 || c.max_position <= 0) AK_FAIL(-1, f + "sizes must be positive");
    if (c.head_dim != LL_HD) AK_FAIL(-1, f + "head_dim must be 128");
    if (nq % nkv) AK_FAIL(-1, f + "q_heads must be a multiple of kv_heads");
    if (!attn_causal_supported(nq, nkv, c.head_dim, 32) && !(max_group > 4 && attn_causal_split_supported(nq, nkv, c.head_dim, 32)))
        AK_FAIL(-1, f + "q_heads / kv_heads: more than " + std::to_string(max_group) + " query heads per kv head");
    if (H % 128 || I % 64) AK_FAIL(-1, f + "hidden must be a multiple of 128, intermediate a multiple of 64");
    if (c.sliding_window < 0) AK_FAIL(-1, f + "sliding_window must be >= 0 (0 = none)");
    if (c.bidirectional != 0 && c.bidirectional != 1) AK_FAIL(-1, f + "bidirectional must be 0 or 1");
    if (!(c.rms_eps > 0.f) || !(c.rope_theta > 0.f)) AK_FAIL(-1, f + "rms_eps and rope_theta must be positive");
    if (n_weights != 2 + feat.per_layer() * L) AK_FAIL(-1, f + "expected 2 + " + std::to_string(feat.per_layer()) + " * layers weight pointers");
    for (int i = 0; i < n_weights; i++)
        if (!w[i]) AK_FAIL(-1, f + "NULL weight pointer");
    return 0;
}

int ll_create(const char *fn, const AkLlamaConfig &c, const void *const *w, const LlFeatures &feat, void **out) {
    const std::string f = std::string(fn) + ": ";
    const int H = c.hidden, I = c.intermediate, L = c.layers, nq = c.q_heads, nkv = c.kv_heads;
    Llama *d = new Llama();
    d->cfg = c;
    d->feat = feat;
    d->emb = (const uint16_t *)w[0];
    d->norm = (const float *)w[1];
    auto fail = [&](const char *what) { set_error(f + what); stack_destroy<Llama>(d); return -10; };
    const size_t qrows = (size_t)nq * LL_HD, kvrows = (size_t)nkv * LL_HD, nqkv = qrows + 2 * kvrows;
    d->zero_bias = d->dev_as<float>(std::max<size_t>({nqkv, (size_t)2 * I, (size_t)H}), true);
    if (!d->zero_bias) return fail("hipMalloc failed");
    // RoPE table, positions 0 .. min(max_position, 8192) - 1
    d->n_pos = c.max_position < LL_MAX_S ? c.max_position : LL_MAX_S;
    if (!d->rope_tables(c.rope_theta, LL_HD, &d->rope_c, &d->rope_s)) return fail("RoPE table upload failed");
    for (int l = 0; l < L; l++) {
        const void *const *p = w + 2 + feat.per_layer() * l;      // wq wk wv [bq bk bv] [q_norm k_norm] wo ln_in ln_post w_gate w_up w_down
        LlLayer ly{};
        uint16_t *wqkv = d->dev_as<uint16_t>(nqkv * H), *wgu = d->dev_as<uint16_t>((size_t)2 * I * H);
        if (!wqkv || !wgu) return fail("hipMalloc failed");
        if (!d->concat_rows(wqkv, H, {{p[0], qrows}, {p[1], kvrows}, {p[2], kvrows}})) return fail("QKV concatenation failed");
        p += 3;
        if (feat.qkv_bias) {                                // bq | bk | bv in the row order of wqkv
            float *b = d->dev_as<float>(nqkv);
            if (!b) return fail("hipMalloc failed");
            if (hipMemcpyAsync(b, p[0], qrows * 4, hipMemcpyDeviceToDevice, 0) != hipSuccess ||
                hipMemcpyAsync(b + qrows, p[1], kvrows * 4, hipMemcpyDeviceToDevice, 0) != hipSuccess ||
                hipMemcpyAsync(b + qrows + kvrows, p[2], kvrows * 4, hipMemcpyDeviceToDevice, 0) != hipSuccess)
                return fail("QKV bias concatenation failed");
            ly.bqkv = b;
            p += 3;
        }
        if (feat.qk_norm) {
            ly.qn = (const float *)p[0]; ly.kn = (const float *)p[1];
            p += 2;
        }
        if (!d->interleave_rows(wgu, p[3], p[4], I, H)) return fail("gate / up interleave failed");      // gemm.hip MODE 7
        ly.wqkv = wqkv; ly.wgu = wgu;
        ly.wo = (const uint16_t *)p[0];
        ly.ln_in = (const float *)p[1]; ly.ln_post = (const float *)p[2];
        ly.wd = (const uint16_t *)p[5];
        d->layers.push_back(ly);
    }
    const size_t fcols = feat.unfused_swiglu ? 3 * I : I;       // un-fused A/B: the 2I-wide product behind f
    d->buffer(&d->x32, (size_t)H * 4); d->buffer(&d->y32, (size_t)H * 4); d->buffer(&d->h16, (size_t)H * 2);
    d->buffer(&d->qkv, nqkv * 2); d->buffer(&d->q, qrows * 2); d->buffer(&d->k, kvrows * 2); d->buffer(&d->v, kvrows * 2);
    d->buffer(&d->ctx, qrows * 2); d->buffer(&d->f, fcols * 2); d->buffer(&d->lens, 0, 4);
    if (feat.mean_pool) d->buffer(&d->part, (size_t)H * 4 / POOL_CHUNK, (size_t)H * 4);      // B ceil(S / 64) <= T / 64 + B rows of H floats
    if (hipDeviceSynchronize() != hipSuccess) return fail("weight preparation failed");
    *out = d;
    return 0;
}

int ll_set_rope_inv_freq(const char *fn, void *h, const float *inv_freq) {
    if (!h || !inv_freq) AK_FAIL(-1, std::string(fn) + ": NULL argument");
    Llama &d = *(Llama *)h;
    std::lock_guard<std::mutex> lk(d.mu);
    AK_HIP(hipDeviceSynchronize());                            // no forward of this handle reads the table while it changes
    return d.rope_tables_set_inv(inv_freq, LL_HD / 2, d.rope_c, d.rope_s) ? -10 : 0;
}

int ll_forward_lens(const char *fn, void *h, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S, int pooling,
                    int normalise, float *out, void *stream) {
    if (!h) AK_FAIL(-1, std::string(fn) + ": NULL handle");
    RoctxRange range(fn);
    Llama &d = *(Llama *)h;
    if (B <= 0) return 0;
    // at most 65535 rows: the attention launch indexes the batch row with blockIdx.z
    const bool pool_ok = pooling == AK_POOL_LAST || (pooling == AK_POOL_MEAN && d.feat.mean_pool);      // (no mean_pool: no `part`)
    if (check_forward_lens(fn, ids, lens, out, ld_ids, lens_stride, B, S, LL_MAX_S, d.n_pos,
                           pool_ok ? nullptr : "pooling must be AK_POOL_LAST or AK_POOL_MEAN", 65535))
        return -1;
    std::lock_guard<std::mutex> lk(d.mu);
    return ll_forward_locked(d, ids, ld_ids, lens, lens_stride, B, S, pooling, normalise, out, (hipStream_t)stream);
}

}  // namespace ak
