// decoder.hip -- the Qwen3 causal decoder forward pass (Qwen3-Embedding-0.6B / 4B / 8B) behind ak_decoder_*: orchestration and the
// small kernels. Per layer, as HF Qwen3Model:
//   h = RMSNorm(x; ln_in)                         k_dec_embed (layer 0) / k_dec_add_rmsnorm
//   q | k | v = h [Wq; Wk; Wv]^T                  k_gemm MODE 3 (gemm.hip), one launch over the matrices concatenated at create
//   q, k = RoPE(RMSNorm_head(q | k))              k_dec_qk_rope: per-head RMSNorm over 128, rotate_half RoPE; q scaled by log2(e) / sqrt(128)
//   a = causal GQA softmax(q k^T) v               k_attn_causal (attn_causal.hip)
//   x = x + a Wo^T                                k_gemm MODE 2 (fp32 out) + k_dec_add_rmsnorm (x += y; h = RMSNorm(x; ln_post))
//   x = x + (silu(h Wg^T) (h Wu^T)) Wd^T          k_gemm MODE 7 (SwiGLU epilogue, gate / up rows interleaved at create), MODE 2, add
// then the final norm on each row's last valid token and L2 normalisation (k_dec_pool): sentence-transformers' lasttoken Pooling
// + Normalize. The residual stream x is float32 throughout, like the reference's CPU path; GEMM operands are bf16.
#include <cmath>
#include <mutex>
#include <vector>

#include "encoder_kernels.h"
#include "mfma_tile.h"
#include "switches.h"

namespace ak {

constexpr int DEC_HD = 128, DEC_MAX_S = 8192;

// ---- RoPE table (host): HF's default rotary embedding in float32 --------------------------------------------------------
// inv_freq[i] = 1 / theta^(2 i / hd) (the exponent 2 i / hd is exact in float32; the power is rounded once from double),
// angle = float(pos) * inv_freq[i] (one float32 product, as HF's float32 matmul of a 1-deep product), cos / sin rounded once from
// double. Table rows [n_pos][hd / 2]: HF's cos / sin are these rows twice (cat(freqs, freqs)).
// the second half of the routine on given inverse frequencies (ak_decoder_rope_table_inv: a caller that holds HF's own buffer)
static void rope_table_from_inv(const float *inv, int half, int n_pos, float *c, float *s) {
    for (int p = 0; p < n_pos; p++)
        for (int i = 0; i < half; i++) {
            const float ang = (float)p * inv[i];
            c[(size_t)p * half + i] = (float)std::cos((double)ang);
            s[(size_t)p * half + i] = (float)std::sin((double)ang);
        }
}
static void rope_table_host(float theta, int hd, int n_pos, float *c, float *s) {
    const int half = hd / 2;
    std::vector<float> inv(half);
    for (int i = 0; i < half; i++) {
        const float e = (float)(2 * i) / (float)hd;
        inv[i] = 1.0f / (float)std::pow((double)theta, (double)e);
    }
    rope_table_from_inv(inv.data(), half, n_pos, c, s);
}

// ---- kernels ------------------------------------------------------------------------------------------------------------
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// one wave per token slot t < B * S: ids past the row's length read as 0; x32 = embed_tokens[id] (float32 of the bf16 row),
// h16 = RMSNorm(x) * ln_in of layer 0. The wave of a row's slot 0 stores the clamped length (attention and pooling read it).
__global__ __launch_bounds__(256) void k_dec_embed(const int *__restrict__ ids, int ld_ids, const int *__restrict__ lens, int lens_stride, int B, int S,
                                                   int H, int vocab, const uint16_t *__restrict__ emb, const float *__restrict__ w, float eps,
                                                   float *__restrict__ x32, uint16_t *__restrict__ h16, int *__restrict__ lens_out) {
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= (int64_t)B * S) return;
    const int b = (int)(t / S), sq = (int)(t - (int64_t)b * S);
    int len = lens[(int64_t)b * lens_stride];
    len = len < 0 ? 0 : (len > S ? S : len);
    if (sq == 0 && lane == 0) lens_out[b] = len;
    int id = sq < len ? ids[(int64_t)b * ld_ids + sq] : 0;
    if (id < 0 || id >= vocab) id = 0;                         // (the tokenizer's ids are in range; a stray id must not read out of bounds)
    const uint16_t *e = emb + (int64_t)id * H;
    float *xr = x32 + t * H;
    float ss = 0.f;
    for (int c = lane * 4; c < H; c += 256) {
        const uint2 v = *(const uint2 *)(e + c);
        const float4 f = {bf16_to_f32((uint16_t)v.x), bf16_to_f32((uint16_t)(v.x >> 16)), bf16_to_f32((uint16_t)v.y), bf16_to_f32((uint16_t)(v.y >> 16))};
        *(float4 *)(xr + c) = f;
        ss += f.x * f.x + f.y * f.y + f.z * f.z + f.w * f.w;
    }
    const float rs = rsqrtf(wave_sum(ss) / (float)H + eps);
    for (int c = lane * 4; c < H; c += 256) {
        const float4 f = *(const float4 *)(xr + c), g = *(const float4 *)(w + c);
        *(uint2 *)(h16 + t * H + c) = uint2{mt::pack_bf16x2(f.x * rs * g.x, f.y * rs * g.y), mt::pack_bf16x2(f.z * rs * g.z, f.w * rs * g.w)};
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
        *(uint2 *)(h16 + t * H + c) = uint2{mt::pack_bf16x2(f.x * rs * g.x, f.y * rs * g.y), mt::pack_bf16x2(f.z * rs * g.z, f.w * rs * g.w)};
    }
}

// one workgroup (4 waves) per token t < B * S; a wave takes one head slot of the QKV row at a time (nq query heads, nkv key heads,
// nkv value heads), a lane the pair (d, d + 64) that rotate_half couples: q and k get RMSNorm over the head (q_norm / k_norm) and
// RoPE at position t % S, q the scale log2(e) / sqrt(128); v is copied. Out: q [B][nq][S][128], k / v [B][nkv][S][128].
__global__ __launch_bounds__(256) void k_dec_qk_rope(const uint16_t *__restrict__ qkv, int S, int nq, int nkv, const float *__restrict__ qn,
                                                     const float *__restrict__ kn, float eps, const float *__restrict__ rc, const float *__restrict__ rsn,
                                                     float qscale, uint16_t *__restrict__ q, uint16_t *__restrict__ k, uint16_t *__restrict__ v) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = (int)(t / S), sq = (int)(t - (int64_t)b * S);
    const int slots = nq + 2 * nkv;
    const uint16_t *row = qkv + t * (int64_t)slots * DEC_HD;
    const float c = rc[(int64_t)sq * 64 + lane], sn = rsn[(int64_t)sq * 64 + lane];
    for (int hs = wave; hs < slots; hs += 4) {
        const float x0 = bf16_to_f32(row[hs * DEC_HD + lane]), x1 = bf16_to_f32(row[hs * DEC_HD + 64 + lane]);
        uint16_t *dst;
        float o0 = x0, o1 = x1;
        if (hs < nq + nkv) {
            const bool isq = hs < nq;
            const float *wn = isq ? qn : kn;
            const float rs = rsqrtf(wave_sum(x0 * x0 + x1 * x1) * (1.0f / DEC_HD) + eps);
            const float y0 = x0 * rs * wn[lane], y1 = x1 * rs * wn[64 + lane];
            o0 = y0 * c - y1 * sn;
            o1 = y1 * c + y0 * sn;
            if (isq) { o0 *= qscale; o1 *= qscale; dst = q + (((int64_t)b * nq + hs) * S + sq) * DEC_HD; }
            else dst = k + (((int64_t)b * nkv + (hs - nq)) * S + sq) * DEC_HD;
        } else {
            dst = v + (((int64_t)b * nkv + (hs - nq - nkv)) * S + sq) * DEC_HD;
        }
        dst[lane] = f32_to_bf16(o0);
        dst[64 + lane] = f32_to_bf16(o1);
    }
}

// one workgroup per row b: the final norm of the row's last valid token (b * S + len - 1), then L2 normalisation (normalise != 0);
// a row of length 0 embeds to zeros
__global__ __launch_bounds__(256) void k_dec_pool(const float *__restrict__ x32, const int *__restrict__ lens, int S, int H, const float *__restrict__ w,
                                                  float eps, int normalise, float *__restrict__ out) {
    __shared__ float red[2][4];
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
    if (lane == 0) red[0][wave] = ss;
    __syncthreads();
    const float rs = rsqrtf((red[0][0] + red[0][1] + red[0][2] + red[0][3]) / (float)H + eps);
    float s2 = 0.f;
    for (int c = tid; c < H; c += 256) { const float y = xr[c] * rs * w[c]; s2 += y * y; }
    s2 = wave_sum(s2);
    if (lane == 0) red[1][wave] = s2;
    __syncthreads();
    const float nrm = sqrtf(red[1][0] + red[1][1] + red[1][2] + red[1][3]);
    const float sc = normalise ? 1.0f / fmaxf(nrm, 1e-12f) : 1.0f;      // torch.nn.functional.normalize's eps
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

// ---- handle ----------------------------------------------------------------------------------------------------------------
struct DecLayer {
    const uint16_t *wqkv, *wo, *wgu, *wd;      // wqkv [(nq + 2 nkv) 128][H] and wgu [2 I][H] (interleaved) are owned
    const float *qn, *kn, *ln_in, *ln_post;
};
struct Decoder {
    AkDecoderConfig cfg;
    const uint16_t *emb = nullptr; const float *norm = nullptr;
    std::vector<DecLayer> layers;
    std::vector<void *> owned;
    float *zero_bias = nullptr, *rope_c = nullptr, *rope_s = nullptr;
    int n_pos = 0;
    int64_t cap = 0; int cap_B = 0;
    float *x32 = nullptr, *y32 = nullptr;
    uint16_t *h16 = nullptr, *qkv = nullptr, *q = nullptr, *k = nullptr, *v = nullptr, *ctx = nullptr, *f = nullptr;
    int *lens = nullptr;
    std::mutex mu;
};

static void dec_free_ws(Decoder &d) {
    void *p[] = {d.x32, d.y32, d.h16, d.qkv, d.q, d.k, d.v, d.ctx, d.f, d.lens};
    for (void *x : p) if (x) hipFree(x);
    d.x32 = d.y32 = nullptr; d.h16 = d.qkv = d.q = d.k = d.v = d.ctx = d.f = nullptr; d.lens = nullptr;
    d.cap = 0; d.cap_B = 0;
}

static bool swiglu_unfused() {
    static const bool u = env_get("AK_DEC_SWIGLU") && std::string(env_get("AK_DEC_SWIGLU")) == "unfused";
    return u;
}

// workspace for tpad token rows (a multiple of 256) and B rows; zeroed when (re)allocated, so rows that no kernel writes (GEMM
// padding rows past B * S) stay finite
static int dec_reserve(Decoder &d, int64_t tpad, int B) {
    if (tpad <= d.cap && B <= d.cap_B) return 0;
    if (tpad < d.cap) tpad = d.cap;
    if (B < d.cap_B) B = d.cap_B;
    dec_free_ws(d);
    const int64_t H = d.cfg.hidden, I = d.cfg.intermediate, nq = d.cfg.q_heads, nkv = d.cfg.kv_heads;
    const int64_t nqkv = (nq + 2 * nkv) * DEC_HD;
    const int64_t fcols = swiglu_unfused() ? 3 * I : I;          // un-fused A/B: the 2I-wide product behind f
    struct { void **p; size_t bytes; } bufs[] = {
        {(void **)&d.x32, (size_t)(tpad * H * 4)}, {(void **)&d.y32, (size_t)(tpad * H * 4)}, {(void **)&d.h16, (size_t)(tpad * H * 2)},
        {(void **)&d.qkv, (size_t)(tpad * nqkv * 2)}, {(void **)&d.q, (size_t)(tpad * nq * DEC_HD * 2)},
        {(void **)&d.k, (size_t)(tpad * nkv * DEC_HD * 2)}, {(void **)&d.v, (size_t)(tpad * nkv * DEC_HD * 2)},
        {(void **)&d.ctx, (size_t)(tpad * nq * DEC_HD * 2)}, {(void **)&d.f, (size_t)(tpad * fcols * 2)}, {(void **)&d.lens, (size_t)B * 4},
    };
    for (auto &bf : bufs) {
        AK_HIP(hipMalloc(bf.p, bf.bytes));
        AK_HIP(hipMemset(*bf.p, 0, bf.bytes));
    }
    d.cap = tpad; d.cap_B = B;
    return 0;
}

static int dec_forward_locked(Decoder &d, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S, int normalise,
                              float *out, hipStream_t st) {
    const AkDecoderConfig &c = d.cfg;
    const int H = c.hidden, I = c.intermediate, nq = c.q_heads, nkv = c.kv_heads, nqkv = (nq + 2 * nkv) * DEC_HD;
    const int64_t T = (int64_t)B * S, tpad = (T + 255) / 256 * 256;
    if (dec_reserve(d, tpad, B)) return -10;
    const unsigned rows4 = (unsigned)((T + 3) / 4);
    const float qscale = 1.4426950408889634f / sqrtf((float)DEC_HD);
    const bool unfused = swiglu_unfused();
    k_dec_embed<<<rows4, 256, 0, st>>>(ids, ld_ids, lens, lens_stride, B, S, H, c.vocab_size, d.emb, d.layers[0].ln_in, c.rms_eps, d.x32, d.h16, d.lens);
    AK_HIP(hipGetLastError());
    for (size_t l = 0; l < d.layers.size(); l++) {
        const DecLayer &ly = d.layers[l];
        GemmArgs g{};
        g.bias = d.zero_bias; g.T = (int)tpad;
        // q | k | v
        g.X = d.h16; g.W = ly.wqkv; g.N = nqkv; g.K = H; g.out_bf16 = d.qkv; g.ldo = nqkv;
        if (launch_gemm(3, g, st)) return -10;
        k_dec_qk_rope<<<(unsigned)T, 256, 0, st>>>(d.qkv, S, nq, nkv, ly.qn, ly.kn, c.rms_eps, d.rope_c, d.rope_s, qscale, d.q, d.k, d.v);
        AK_HIP(hipGetLastError());
        CausalAttnArgs aa{d.q, d.k, d.v, d.lens, d.ctx, B, S, nq, nkv};
        if (launch_attn_causal(aa, st)) return -10;
        // x += ctx Wo^T; h = RMSNorm(x; ln_post)
        g = GemmArgs{}; g.bias = d.zero_bias; g.T = (int)tpad;
        g.X = d.ctx; g.W = ly.wo; g.N = H; g.K = nq * DEC_HD; g.out_f32 = d.y32;
        if (launch_gemm(2, g, st)) return -10;
        k_dec_add_rmsnorm<<<rows4, 256, 0, st>>>(d.x32, d.y32, T, H, ly.ln_post, c.rms_eps, d.h16);
        AK_HIP(hipGetLastError());
        // f = silu(h Wg^T) (h Wu^T)
        g = GemmArgs{}; g.bias = d.zero_bias; g.T = (int)tpad;
        g.X = d.h16; g.W = ly.wgu; g.N = 2 * I; g.K = H;
        if (unfused) {
            uint16_t *gu = d.f + tpad * I;
            g.out_bf16 = gu; g.ldo = 2 * I;
            if (launch_gemm(3, g, st)) return -10;
            const int64_t n = tpad * I;
            k_dec_swiglu<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(gu, n, d.f);
            AK_HIP(hipGetLastError());
        } else {
            g.out_bf16 = d.f; g.ldo = I;
            if (launch_gemm(7, g, st)) return -10;
        }
        // x += f Wd^T; h = RMSNorm(x; next layer's ln_in) (after the last layer: the add only, the pool applies the final norm)
        g = GemmArgs{}; g.bias = d.zero_bias; g.T = (int)tpad;
        g.X = d.f; g.W = ly.wd; g.N = H; g.K = I; g.out_f32 = d.y32;
        if (launch_gemm(2, g, st)) return -10;
        const float *wn = l + 1 < d.layers.size() ? d.layers[l + 1].ln_in : nullptr;
        k_dec_add_rmsnorm<<<rows4, 256, 0, st>>>(d.x32, d.y32, T, H, wn, c.rms_eps, d.h16);
        AK_HIP(hipGetLastError());
    }
    k_dec_pool<<<B, 256, 0, st>>>(d.x32, d.lens, S, H, d.norm, c.rms_eps, normalise, out);
    AK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ak

using namespace ak;

extern "C" int ak_decoder_rope_table(float theta, int head_dim, int n_pos, float *cos_out, float *sin_out) {
    if (!cos_out || !sin_out || head_dim <= 0 || head_dim % 2 || n_pos < 0 || !(theta > 0.f))
        AK_FAIL(-1, "ak_decoder_rope_table: bad arguments");
    rope_table_host(theta, head_dim, n_pos, cos_out, sin_out);
    return 0;
}

extern "C" int ak_decoder_rope_table_inv(const float *inv_freq, int half, int n_pos, float *cos_out, float *sin_out) {
    if (!inv_freq || !cos_out || !sin_out || half <= 0 || n_pos < 0) AK_FAIL(-1, "ak_decoder_rope_table_inv: bad arguments");
    rope_table_from_inv(inv_freq, half, n_pos, cos_out, sin_out);
    return 0;
}

extern "C" int ak_decoder_destroy(ak_decoder_t h) {
    AK_BIND();
    if (!h) return 0;
    Decoder *d = (Decoder *)h;
    hipDeviceSynchronize();
    dec_free_ws(*d);
    for (void *p : d->owned) hipFree(p);
    delete d;
    return 0;
}

extern "C" int ak_decoder_create(const AkDecoderConfig *cfg, const void *const *w, int n_weights, ak_decoder_t *out) {
    AK_BIND();
    if (!cfg || !w || !out) AK_FAIL(-1, "ak_decoder_create: NULL argument");
    *out = nullptr;
    const AkDecoderConfig c = *cfg;
    const int H = c.hidden, I = c.intermediate, L = c.layers, nq = c.q_heads, nkv = c.kv_heads;
    if (L <= 0 || c.vocab_size <= 0 || nq <= 0 || nkv <= 0 || c.max_position <= 0) AK_FAIL(-1, "ak_decoder_create: sizes must be positive");
    if (c.head_dim != DEC_HD) AK_FAIL(-1, "ak_decoder_create: head_dim must be 128");
    if (nq % nkv) AK_FAIL(-1, "ak_decoder_create: q_heads must be a multiple of kv_heads");
    if (!attn_causal_supported(nq, nkv, c.head_dim, 32)) AK_FAIL(-1, "ak_decoder_create: more than 4 query heads per kv head");
    if (H % 128 || I % 64) AK_FAIL(-1, "ak_decoder_create: hidden must be a multiple of 128, intermediate a multiple of 64");
    if (!(c.rms_eps > 0.f) || !(c.rope_theta > 0.f)) AK_FAIL(-1, "ak_decoder_create: rms_eps and rope_theta must be positive");
    if (n_weights != 2 + 11 * L) AK_FAIL(-1, "ak_decoder_create: expected 2 + 11 * layers weight pointers");
    for (int i = 0; i < n_weights; i++)
        if (!w[i]) AK_FAIL(-1, "ak_decoder_create: NULL weight pointer");
    Decoder *d = new Decoder();
    d->cfg = c;
    d->emb = (const uint16_t *)w[0];
    d->norm = (const float *)w[1];
    auto fail = [&](const char *what) { set_error(what); ak_decoder_destroy(d); return -10; };
    auto dev = [&](size_t bytes) -> void * {
        void *p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
        d->owned.push_back(p);
        return p;
    };
    const size_t qrows = (size_t)nq * DEC_HD, kvrows = (size_t)nkv * DEC_HD;
    const size_t zb = std::max<size_t>({qrows + 2 * kvrows, (size_t)2 * I, (size_t)H});
    d->zero_bias = (float *)dev(zb * 4);
    if (!d->zero_bias || hipMemset(d->zero_bias, 0, zb * 4) != hipSuccess) return fail("ak_decoder_create: hipMalloc failed");
    // RoPE table, positions 0 .. min(max_position, 8192) - 1
    d->n_pos = c.max_position < DEC_MAX_S ? c.max_position : DEC_MAX_S;
    {
        std::vector<float> hc((size_t)d->n_pos * 64), hs((size_t)d->n_pos * 64);
        rope_table_host(c.rope_theta, DEC_HD, d->n_pos, hc.data(), hs.data());
        d->rope_c = (float *)dev(hc.size() * 4);
        d->rope_s = (float *)dev(hs.size() * 4);
        if (!d->rope_c || !d->rope_s || hipMemcpy(d->rope_c, hc.data(), hc.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d->rope_s, hs.data(), hs.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            return fail("ak_decoder_create: RoPE table upload failed");
    }
    for (int l = 0; l < L; l++) {
        const void *const *p = w + 2 + 11 * l;      // wq wk wv q_norm k_norm wo ln_in ln_post w_gate w_up w_down
        DecLayer ly{};
        uint16_t *wqkv = (uint16_t *)dev((qrows + 2 * kvrows) * H * 2);
        uint16_t *wgu = (uint16_t *)dev((size_t)2 * I * H * 2);
        if (!wqkv || !wgu) return fail("ak_decoder_create: hipMalloc failed");
        if (hipMemcpy(wqkv, p[0], qrows * H * 2, hipMemcpyDeviceToDevice) != hipSuccess ||
            hipMemcpy(wqkv + qrows * H, p[1], kvrows * H * 2, hipMemcpyDeviceToDevice) != hipSuccess ||
            hipMemcpy(wqkv + (qrows + kvrows) * H, p[2], kvrows * H * 2, hipMemcpyDeviceToDevice) != hipSuccess)
            return fail("ak_decoder_create: QKV concatenation failed");
        // gate / up rows interleaved: row 2 j = gate j, row 2 j + 1 = up j (gemm.hip MODE 7)
        if (hipMemcpy2D(wgu, (size_t)4 * H, p[8], (size_t)2 * H, (size_t)2 * H, I, hipMemcpyDeviceToDevice) != hipSuccess ||
            hipMemcpy2D(wgu + H, (size_t)4 * H, p[9], (size_t)2 * H, (size_t)2 * H, I, hipMemcpyDeviceToDevice) != hipSuccess)
            return fail("ak_decoder_create: gate / up interleave failed");
        ly.wqkv = wqkv; ly.wgu = wgu;
        ly.qn = (const float *)p[3]; ly.kn = (const float *)p[4];
        ly.wo = (const uint16_t *)p[5];
        ly.ln_in = (const float *)p[6]; ly.ln_post = (const float *)p[7];
        ly.wd = (const uint16_t *)p[10];
        d->layers.push_back(ly);
    }
    if (hipDeviceSynchronize() != hipSuccess) return fail("ak_decoder_create: weight preparation failed");
    *out = d;
    return 0;
}

extern "C" int ak_decoder_forward_lens(ak_decoder_t h, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S,
                                       int normalise, float *out, void *stream) {
    AK_BIND();
    if (!h) AK_FAIL(-1, "ak_decoder_forward_lens: NULL decoder");
    RoctxRange range("ak_decoder_forward_lens");
    Decoder &d = *(Decoder *)h;
    if (B <= 0) return 0;
    if (!ids || !lens || !out || ld_ids < S || lens_stride < 1) AK_FAIL(-1, "ak_decoder_forward_lens: bad arguments");
    if (S <= 0 || S % 32 || S > DEC_MAX_S) AK_FAIL(-1, "ak_decoder_forward_lens: S must be a positive multiple of 32, <= 8192");
    if (S > d.n_pos) AK_FAIL(-1, "ak_decoder_forward_lens: S exceeds max_position");
    std::lock_guard<std::mutex> lk(d.mu);
    return dec_forward_locked(d, ids, ld_ids, lens, lens_stride, B, S, normalise, out, (hipStream_t)stream);
}
