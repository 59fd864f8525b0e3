// llama.hip -- the Mistral / Llama decoder forward pass (intfloat/e5-mistral-7b-instruct, Salesforce/SFR-Embedding-Mistral,
// Linq-AI-Research/Linq-Embed-Mistral, the Llama-3.1-8B based embedders) behind ak_llama_*: orchestration and the family's own kernel.
// Per layer, as HF MistralModel / LlamaModel:
//   h = RMSNorm(x; ln_in)                         k_dec_embed (layer 0) / k_dec_add_rmsnorm (decoder.hip)
//   q | k | v = h [Wq; Wk; Wv]^T                  k_gemm MODE 3 (gemm.hip), one launch over the matrices concatenated at create
//   q, k = RoPE(q | k)                            k_ll_rope: rotate_half RoPE at head size 128, NO per-head norm (Qwen3's k_dec_qk_rope
//                                                 always normalises); q scaled by log2(e) / sqrt(128); v copied
//   a = GQA softmax(q k^T + mask) v               attn_causal.hip: causal; with sliding_window = w > 0 key <= query and query - key <= w - 1
//                                                 (HF's sliding_window_overlay); bidirectional (cfg.bidirectional): every key below the length
//   x = x + a Wo^T                                k_gemm MODE 2 (fp32 out) + k_dec_add_rmsnorm (x += y; h = RMSNorm(x; ln_post))
//   x = x + (silu(h Wg^T) (h Wu^T)) Wd^T          k_gemm MODE 7 (SwiGLU epilogue, gate / up rows interleaved at create), MODE 2, add
// then the final norm on each row's last valid token and L2 normalisation (k_dec_pool): sentence-transformers' lasttoken Pooling
// + Normalize; or (AK_POOL_MEAN) the mean over the valid tokens of the final norm per token, k_ll_pool_part / _fin on stack.h's pool body.
// The residual stream x is float32 throughout; GEMM operands are bf16. The rotary table comes from rope_theta (HF's default
// rotary embedding) or from inverse frequencies the caller hands over (ak_llama_set_rope_inv_freq: rope_type llama3).
// Here: ak_llama_*'s config checks, the layer loop (llama_impl.h: qwen2.hip builds its handle on it, with q / k / v biases and the split
// attention launch) and k_ll_rope. Everything else is stack.h / stack.hip and the launches
// decoder.hip spells (launch_dec_embed, launch_dec_add_rmsnorm, launch_dec_pool).
#include <algorithm>
#include <cmath>

#include "llama_impl.h"

namespace ak {

namespace {
// one workgroup (4 waves) per token t < B * S; a wave takes one head slot of the QKV row at a time (nq query heads, nkv key heads,
// nkv value heads), a lane the pair (d, d + 64) that rotate_half couples: q and k get RoPE at position t % S --
// x'[d] = x[d] cos - x[d + 64] sin, x'[d + 64] = x[d + 64] cos + x[d] sin --, q then the scale log2(e) / sqrt(128); v is copied.
// Out: q [B][nq][S][128], k / v [B][nkv][S][128].
__global__ __launch_bounds__(256) void k_ll_rope(const uint16_t *__restrict__ qkv, int S, int nq, int nkv, const float *__restrict__ rc,
                                                 const float *__restrict__ rsn, float qscale, uint16_t *__restrict__ q, uint16_t *__restrict__ k,
                                                 uint16_t *__restrict__ v) {
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
            o0 = x0 * c - x1 * sn;
            o1 = x1 * c + x0 * sn;
            if (isq) { o0 *= qscale; o1 *= qscale; dst = q + (((int64_t)b * nq + hs) * S + sq) * LL_HD; }
            else dst = k + (((int64_t)b * nkv + (hs - nq)) * S + sq) * LL_HD;
        } else {
            dst = v + (((int64_t)b * nkv + (hs - nq - nkv)) * S + sq) * LL_HD;
        }
        dst[lane] = f32_to_bf16(o0);
        dst[64 + lane] = f32_to_bf16(o1);
    }
}

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

// ---- launch: the one place the kernel's grid is spelled (the forward pass below and the single-launch test call it) ----
int launch_ll_rope(const uint16_t *qkv, int B, int S, int nq, int nkv, const float *rc, const float *rs, float qscale, uint16_t *q, uint16_t *k,
                   uint16_t *v, hipStream_t st) {
    const int64_t T = (int64_t)B * S;
    if (B <= 0 || S <= 0 || nq <= 0 || nkv <= 0 || T > 0x7fffffff) AK_FAIL(-1, "ll_rope: bad shape");
    k_ll_rope<<<(unsigned)T, 256, 0, st>>>(qkv, S, nq, nkv, rc, rs, qscale, q, k, v);
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
        if (launch_ll_rope(d.qkv, B, S, nq, nkv, d.rope_c, d.rope_s, qscale, d.q, d.k, d.v, st)) return -10;
        CausalAttnArgs aa{d.q, d.k, d.v, d.lens, d.ctx, B, S, nq, nkv};
        aa.window = c.sliding_window;
        aa.bidirectional = c.bidirectional;
        if (d.split_attn ? launch_attn_causal_split(aa, st) : launch_attn_causal(aa, st)) return -10;
        // x += ctx Wo^T; h = RMSNorm(x; ln_post)
        if (launch_gemm(2, d.gemm_f32(tpad, d.ctx, ly.wo, H, nq * LL_HD, d.y32), st)) return -10;
        if (launch_dec_add_rmsnorm(d.x32, d.y32, T, H, ly.ln_post, c.rms_eps, d.h16, st)) return -10;
        // f = silu(h Wg^T) (h Wu^T)
        if (launch_gemm(7, d.gemm_gated(tpad, d.h16, ly.wgu, I, H, d.f), st)) return -10;
        // x += f Wd^T; h = RMSNorm(x; next layer's ln_in) (after the last layer: the add only, the pool applies the final norm)
        if (launch_gemm(2, d.gemm_f32(tpad, d.f, ly.wd, H, I, d.y32), st)) return -10;
        const float *wn = l + 1 < d.layers.size() ? d.layers[l + 1].ln_in : nullptr;
        if (launch_dec_add_rmsnorm(d.x32, d.y32, T, H, wn, c.rms_eps, d.h16, st)) return -10;
    }
    if (pooling == AK_POOL_MEAN) return launch_ll_pool(d.x32, d.lens, B, S, H, d.norm, c.rms_eps, normalise, d.part, out, st) ? -10 : 0;
    return launch_dec_pool(d.x32, d.lens, B, S, H, d.norm, c.rms_eps, normalise, out, st) ? -10 : 0;
}

// The handle of a checked config (the caller's create has refused what it refuses; n_weights = 2 + (qkv_bias ? 12 : 9) * layers):
// the concatenated / interleaved matrices, the rotary table, the workspace
int ll_create(const char *fn, const AkLlamaConfig &c, const void *const *w, bool qkv_bias, bool split_attn, void **out) {
    const std::string f = std::string(fn) + ": ";
    const int H = c.hidden, I = c.intermediate, L = c.layers, nq = c.q_heads, nkv = c.kv_heads;
    Llama *d = new Llama();
    d->cfg = c;
    d->split_attn = split_attn;
    d->emb = (const uint16_t *)w[0];
    d->norm = (const float *)w[1];
    auto fail = [&](const char *what) { set_error(f + what); stack_destroy<Llama>(d); return -10; };
    const size_t qrows = (size_t)nq * LL_HD, kvrows = (size_t)nkv * LL_HD, nqkv = qrows + 2 * kvrows;
    d->zero_bias = d->dev_as<float>(std::max<size_t>({nqkv, (size_t)2 * I, (size_t)H}), true);
    if (!d->zero_bias) return fail("hipMalloc failed");
    // RoPE table, positions 0 .. min(max_position, 8192) - 1
    d->n_pos = c.max_position < LL_MAX_S ? c.max_position : LL_MAX_S;
    if (!d->rope_tables(c.rope_theta, LL_HD, &d->rope_c, &d->rope_s)) return fail("RoPE table upload failed");
    const int per_layer = qkv_bias ? 12 : 9, o = qkv_bias ? 3 : 0;
    for (int l = 0; l < L; l++) {
        const void *const *p = w + 2 + per_layer * l;       // wq wk wv [bq bk bv] wo ln_in ln_post w_gate w_up w_down
        LlLayer ly{};
        uint16_t *wqkv = d->dev_as<uint16_t>(nqkv * H), *wgu = d->dev_as<uint16_t>((size_t)2 * I * H);
        if (!wqkv || !wgu) return fail("hipMalloc failed");
        if (!d->concat_rows(wqkv, H, {{p[0], qrows}, {p[1], kvrows}, {p[2], kvrows}})) return fail("QKV concatenation failed");
        if (qkv_bias) {                                     // bq | bk | bv in the row order of wqkv
            float *b = d->dev_as<float>(nqkv);
            if (!b) return fail("hipMalloc failed");
            if (hipMemcpyAsync(b, p[3], qrows * 4, hipMemcpyDeviceToDevice, 0) != hipSuccess ||
                hipMemcpyAsync(b + qrows, p[4], kvrows * 4, hipMemcpyDeviceToDevice, 0) != hipSuccess ||
                hipMemcpyAsync(b + qrows + kvrows, p[5], kvrows * 4, hipMemcpyDeviceToDevice, 0) != hipSuccess)
                return fail("QKV bias concatenation failed");
            ly.bqkv = b;
        }
        if (!d->interleave_rows(wgu, p[o + 6], p[o + 7], I, H)) return fail("gate / up interleave failed");      // gemm.hip MODE 7
        ly.wqkv = wqkv; ly.wgu = wgu;
        ly.wo = (const uint16_t *)p[o + 3];
        ly.ln_in = (const float *)p[o + 4]; ly.ln_post = (const float *)p[o + 5];
        ly.wd = (const uint16_t *)p[o + 8];
        d->layers.push_back(ly);
    }
    d->buffer(&d->x32, (size_t)H * 4); d->buffer(&d->y32, (size_t)H * 4); d->buffer(&d->h16, (size_t)H * 2);
    d->buffer(&d->qkv, nqkv * 2); d->buffer(&d->q, qrows * 2); d->buffer(&d->k, kvrows * 2); d->buffer(&d->v, kvrows * 2);
    d->buffer(&d->ctx, qrows * 2); d->buffer(&d->f, (size_t)I * 2); d->buffer(&d->lens, 0, 4);
    d->buffer(&d->part, (size_t)H * 4 / POOL_CHUNK, (size_t)H * 4);      // B ceil(S / 64) <= T / 64 + B rows of H floats
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
    if (check_forward_lens(fn, ids, lens, out, ld_ids, lens_stride, B, S, LL_MAX_S, d.n_pos,
                           pooling == AK_POOL_LAST || pooling == AK_POOL_MEAN ? nullptr : "pooling must be AK_POOL_LAST or AK_POOL_MEAN", 65535))
        return -1;
    std::lock_guard<std::mutex> lk(d.mu);
    return ll_forward_locked(d, ids, ld_ids, lens, lens_stride, B, S, pooling, normalise, out, (hipStream_t)stream);
}

}  // namespace ak

using namespace ak;

extern "C" int ak_llama_destroy(ak_llama_t h) { return stack_destroy<Llama>(h); }

extern "C" int ak_llama_create(const AkLlamaConfig *cfg, const void *const *w, int n_weights, ak_llama_t *out) {
    AK_BIND();
    if (!cfg || !w || !out) AK_FAIL(-1, "ak_llama_create: NULL argument");
    *out = nullptr;
    const AkLlamaConfig c = *cfg;
    const int H = c.hidden, I = c.intermediate, L = c.layers, nq = c.q_heads, nkv = c.kv_heads;
    if (L <= 0 || c.vocab_size <= 0 || nq <= 0 || nkv <= 0 || H <= 0 || I <= 0 || c.max_position <= 0) AK_FAIL(-1, "ak_llama_create: sizes must be positive");
    if (c.head_dim != LL_HD) AK_FAIL(-1, "ak_llama_create: head_dim must be 128");
    if (nq % nkv) AK_FAIL(-1, "ak_llama_create: q_heads must be a multiple of kv_heads");
    if (!attn_causal_supported(nq, nkv, c.head_dim, 32)) AK_FAIL(-1, "ak_llama_create: q_heads / kv_heads: more than 4 query heads per kv head");
    if (H % 128 || I % 64) AK_FAIL(-1, "ak_llama_create: hidden must be a multiple of 128, intermediate a multiple of 64");
    if (c.sliding_window < 0) AK_FAIL(-1, "ak_llama_create: sliding_window must be >= 0 (0 = none)");
    if (c.bidirectional != 0 && c.bidirectional != 1) AK_FAIL(-1, "ak_llama_create: bidirectional must be 0 or 1");
    if (!(c.rms_eps > 0.f) || !(c.rope_theta > 0.f)) AK_FAIL(-1, "ak_llama_create: rms_eps and rope_theta must be positive");
    if (n_weights != 2 + 9 * L) AK_FAIL(-1, "ak_llama_create: expected 2 + 9 * layers weight pointers");
    for (int i = 0; i < n_weights; i++)
        if (!w[i]) AK_FAIL(-1, "ak_llama_create: NULL weight pointer");
    return ll_create("ak_llama_create", c, w, false, false, out);
}

extern "C" int ak_llama_set_rope_inv_freq(ak_llama_t h, const float *inv_freq) {
    AK_BIND();
    return ll_set_rope_inv_freq("ak_llama_set_rope_inv_freq", h, inv_freq);
}

extern "C" int ak_llama_forward_lens(ak_llama_t h, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S, int pooling,
                                     int normalise, float *out, void *stream) {
    AK_BIND();
    return ll_forward_lens("ak_llama_forward_lens", h, ids, ld_ids, lens, lens_stride, B, S, pooling, normalise, out, stream);
}
