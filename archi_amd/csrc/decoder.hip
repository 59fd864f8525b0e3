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
// Here: the config checks, the layer struct, the layer loop and the family's own kernels. The plumbing shared with mbert.hip and gemma.hip
// is stack.h / stack.hip: the token-slot prologue and the row helpers of k_dec_embed / k_dec_add_rmsnorm, the L2 tail of k_dec_pool, the
// workspace, the weight preparation at create, the rotary tables (ak_decoder_rope_table* are thin wrappers), the GemmArgs of the launches.
#include <cmath>
#include <string>

#include "stack.h"
#include "switches.h"

namespace ak {

constexpr int DEC_HD = 128, DEC_MAX_S = 8192;

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

int launch_dec_qk_rope(const uint16_t *qkv, int B, int S, int nq, int nkv, const float *qn, const float *kn, float eps, const float *rc,
                       const float *rs, float qscale, uint16_t *q, uint16_t *k, uint16_t *v, hipStream_t st) {
    const int64_t T = (int64_t)B * S;
    k_dec_qk_rope<<<(unsigned)T, 256, 0, st>>>(qkv, S, nq, nkv, qn, kn, eps, rc, rs, qscale, q, k, v);
    AK_HIP(hipGetLastError());
    return 0;
}

int launch_dec_pool(const float *x32, const int *lens, int B, int S, int H, const float *w, float eps, int normalise, float *out, hipStream_t st) {
    k_dec_pool<<<B, 256, 0, st>>>(x32, lens, S, H, w, eps, normalise, out);
    AK_HIP(hipGetLastError());
    return 0;
}

// ---- handle ----------------------------------------------------------------------------------------------------------------
struct DecLayer {
    const uint16_t *wqkv, *wo, *wgu, *wd;      // wqkv [(nq + 2 nkv) 128][H] and wgu [2 I][H] (interleaved) are owned
    const float *qn, *kn, *ln_in, *ln_post;
};
struct Decoder : Stack {
    AkDecoderConfig cfg;
    const uint16_t *emb = nullptr; const float *norm = nullptr;
    std::vector<DecLayer> layers;
    float *rope_c = nullptr, *rope_s = nullptr;
    float *x32 = nullptr, *y32 = nullptr;
    uint16_t *h16 = nullptr, *qkv = nullptr, *q = nullptr, *k = nullptr, *v = nullptr, *ctx = nullptr, *f = nullptr;
    int *lens = nullptr;
};

static bool swiglu_unfused() {
    static const bool u = env_get("AK_DEC_SWIGLU") && std::string(env_get("AK_DEC_SWIGLU")) == "unfused";
    return u;
}

static int dec_forward_locked(Decoder &d, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S, int normalise,
                              float *out, hipStream_t st) {
    const AkDecoderConfig &c = d.cfg;
    const int H = c.hidden, I = c.intermediate, nq = c.q_heads, nkv = c.kv_heads, nqkv = (nq + 2 * nkv) * DEC_HD;
    const int64_t T = (int64_t)B * S, tpad = (T + 255) / 256 * 256;
    if (d.reserve(tpad, B)) return -10;
    const float qscale = 1.4426950408889634f / sqrtf((float)DEC_HD);
    if (launch_dec_embed(ids, ld_ids, lens, lens_stride, B, S, H, c.vocab_size, d.emb, d.layers[0].ln_in, c.rms_eps, d.x32, d.h16, d.lens, st)) return -10;
    for (size_t l = 0; l < d.layers.size(); l++) {
        const DecLayer &ly = d.layers[l];
        // q | k | v
        if (launch_gemm(3, d.gemm_bf16(tpad, d.h16, ly.wqkv, nqkv, H, d.qkv), st)) return -10;
        if (launch_dec_qk_rope(d.qkv, B, S, nq, nkv, ly.qn, ly.kn, c.rms_eps, d.rope_c, d.rope_s, qscale, d.q, d.k, d.v, st)) return -10;
        CausalAttnArgs aa{d.q, d.k, d.v, d.lens, d.ctx, B, S, nq, nkv};
        if (launch_attn_causal(aa, st)) return -10;
        // x += ctx Wo^T; h = RMSNorm(x; ln_post)
        if (launch_gemm(2, d.gemm_f32(tpad, d.ctx, ly.wo, H, nq * DEC_HD, d.y32), st)) return -10;
        if (launch_dec_add_rmsnorm(d.x32, d.y32, T, H, ly.ln_post, c.rms_eps, d.h16, st)) return -10;
        // f = silu(h Wg^T) (h Wu^T)
        if (swiglu_unfused()) {
            uint16_t *gu = d.f + tpad * I;
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
    return launch_dec_pool(d.x32, d.lens, B, S, H, d.norm, c.rms_eps, normalise, out, st) ? -10 : 0;
}

}  // namespace ak

using namespace ak;

// the rotary table routines of stack.hip, for callers that hold HF's own buffers (host only)
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

extern "C" int ak_decoder_destroy(ak_decoder_t h) { return stack_destroy<Decoder>(h); }

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
    const size_t qrows = (size_t)nq * DEC_HD, kvrows = (size_t)nkv * DEC_HD, nqkv = qrows + 2 * kvrows;
    d->zero_bias = d->dev_as<float>(std::max<size_t>({nqkv, (size_t)2 * I, (size_t)H}), true);
    if (!d->zero_bias) return fail("ak_decoder_create: hipMalloc failed");
    // RoPE table, positions 0 .. min(max_position, 8192) - 1
    d->n_pos = c.max_position < DEC_MAX_S ? c.max_position : DEC_MAX_S;
    if (!d->rope_tables(c.rope_theta, DEC_HD, &d->rope_c, &d->rope_s)) return fail("ak_decoder_create: RoPE table upload failed");
    for (int l = 0; l < L; l++) {
        const void *const *p = w + 2 + 11 * l;      // wq wk wv q_norm k_norm wo ln_in ln_post w_gate w_up w_down
        DecLayer ly{};
        uint16_t *wqkv = d->dev_as<uint16_t>(nqkv * H), *wgu = d->dev_as<uint16_t>((size_t)2 * I * H);
        if (!wqkv || !wgu) return fail("ak_decoder_create: hipMalloc failed");
        if (!d->concat_rows(wqkv, H, {{p[0], qrows}, {p[1], kvrows}, {p[2], kvrows}})) return fail("ak_decoder_create: QKV concatenation failed");
        if (!d->interleave_rows(wgu, p[8], p[9], I, H)) return fail("ak_decoder_create: gate / up interleave failed");      // gemm.hip MODE 7
        ly.wqkv = wqkv; ly.wgu = wgu;
        ly.qn = (const float *)p[3]; ly.kn = (const float *)p[4];
        ly.wo = (const uint16_t *)p[5];
        ly.ln_in = (const float *)p[6]; ly.ln_post = (const float *)p[7];
        ly.wd = (const uint16_t *)p[10];
        d->layers.push_back(ly);
    }
    const size_t fcols = swiglu_unfused() ? 3 * I : I;          // un-fused A/B: the 2I-wide product behind f
    d->buffer(&d->x32, (size_t)H * 4); d->buffer(&d->y32, (size_t)H * 4); d->buffer(&d->h16, (size_t)H * 2);
    d->buffer(&d->qkv, nqkv * 2); d->buffer(&d->q, qrows * 2); d->buffer(&d->k, kvrows * 2); d->buffer(&d->v, kvrows * 2);
    d->buffer(&d->ctx, qrows * 2); d->buffer(&d->f, fcols * 2); d->buffer(&d->lens, 0, 4);
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
    // at most 65535 rows: the attention launch indexes the batch row with blockIdx.z
    if (check_forward_lens("ak_decoder_forward_lens", ids, lens, out, ld_ids, lens_stride, B, S, DEC_MAX_S, d.n_pos, nullptr, 65535)) return -1;
    std::lock_guard<std::mutex> lk(d.mu);
    return dec_forward_locked(d, ids, ld_ids, lens, lens_stride, B, S, normalise, out, (hipStream_t)stream);
}
