// nomic.hip -- the NomicBERT encoder forward pass (nomic-ai/nomic-embed-text-v1 / -v1.5 / -v1-unsupervised,
// Snowflake/snowflake-arctic-embed-m-long) behind ak_nomic_*: orchestration and the small kernels. As HF NomicBertModel:
//   x = LayerNorm(word_emb[id] + type_emb[0]; g, b)    k_nb_embed (float32 x, bf16 h = x); no position table
// per layer (POST-norm: the residual stream is the LayerNorm output; no bias in any Linear, LayerNorms with weight and bias):
//   q | k | v = h [Wq; Wk; Wv]^T                       k_gemm MODE 0 (gemm.hip): q pre-scaled by log2(e) / 8, k as [T][H], V transposed
//   q, k = RoPE(q), RoPE(k)                            k_mb_rope (mbert.hip), in place: rotate_half at head size 64, one table
//   a = softmax(q k^T + pad mask) v                    k_attn_long<false> (attn_long.hip) at every S, with the row lengths
//   x = LayerNorm(x + a Wo^T; ln1); h = bf16(x)        k_gemm MODE 2 (float32 out) + k_nb_add_ln
//   f = silu(h Wgate^T) (h Wup^T)                      k_gemm MODE 7 (SwiGLU epilogue; gate / up rows interleaved at create and padded
//                                                      with zero rows to 2 I % 256 == 0 for the wide tile: padded_intermediate, stack.h)
//   x = LayerNorm(x + f Wdown^T; ln2); h = bf16(x)     k_gemm MODE 2 + k_nb_add_ln
// then mean / cls pooling over the valid tokens of x (no final norm) and L2 normalisation in float32 (k_nb_pool_part, k_nb_pool_fin).
// The residual stream x is float32 throughout; GEMM operands are bf16. Token counts are padded to the GEMM tile (256) as in mbert.hip.
// What differs from mbert.hip's k_mb_add_ln is the post-norm: the NORMALISED row goes back to x32 (there: the sum), and the
// LayerNorms carry a bias. The plumbing is stack.h / stack.hip. Nothing here reads the environment.
// LDS per workgroup: k_nb_embed / k_nb_add_ln none; k_nb_pool_part 4 * H * 4 bytes (dynamic: 12 KB at H = 768); k_nb_pool_fin 16 bytes.
#include <algorithm>
#include <cmath>

#include "stack.h"

namespace ak {

namespace {
constexpr int NB_HD = 64, NB_MAX_S = ATTN_LONG_MAX_S, NB_MAX_H = POOL_MAX_H;

// The tail both row kernels share, one wave per row held in registers (NJ float4 per lane, feature c = 4 lane + 256 j; lanes at or
// past H hold zeros and store nothing): s = the lane's share of the row's sum. Mean, then the variance about it (two passes, as
// torch's float32 kernel and mb_row_stats -- not E[x^2] - mean^2); x32 row = (f - mean) rstd g + b in float32, h16 row = bf16 of it.
template <int NJ>
__device__ inline void nb_ln_store(float4 (&f)[NJ], float s, int H, int lane, const float *__restrict__ g, const float *__restrict__ b, float eps,
                                   float *__restrict__ xr, uint16_t *__restrict__ hr) {
    const float mean = wave_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; j++)
        if (lane * 4 + j * 256 < H) {
            const float a = f[j].x - mean, bb = f[j].y - mean, cc = f[j].z - mean, d = f[j].w - mean;
            q += (a * a + bb * bb) + (cc * cc + d * d);
        }
    const float rstd = rsqrtf(wave_sum(q) / (float)H + eps);
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int c = lane * 4 + j * 256;
        if (c < H) {
            const float4 gw = *(const float4 *)(g + c), bw = *(const float4 *)(b + c);
            const float4 y = {(f[j].x - mean) * rstd * gw.x + bw.x, (f[j].y - mean) * rstd * gw.y + bw.y, (f[j].z - mean) * rstd * gw.z + bw.z,
                              (f[j].w - mean) * rstd * gw.w + bw.w};
            *(float4 *)(xr + c) = y;
            store_bf16x4(hr + c, y.x, y.y, y.z, y.w);
        }
    }
}

// one wave per token slot t < B * S: ids past the row's length read as 0; x32 = LayerNorm(word[id] + type[0]; g, b), h16 = bf16(x32).
// Also the int key mask (slot < length) the attention kernel stages, and per row the clamped length.
template <int NJ>
__global__ __launch_bounds__(256) void k_nb_embed(const int *__restrict__ ids, int ld_ids, const int *__restrict__ lens, int lens_stride, int B, int S,
                                                  int H, int vocab, const uint16_t *__restrict__ word, const float *__restrict__ type0,
                                                  const float *__restrict__ g, const float *__restrict__ b, float eps, float *__restrict__ x32,
                                                  uint16_t *__restrict__ h16, int *__restrict__ mask, int *__restrict__ lens_out) {
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= (int64_t)B * S) return;
    const int id = token_slot<true>(ids, ld_ids, lens, lens_stride, S, vocab, t, lane, mask, lens_out);
    const uint16_t *e = word + (int64_t)id * H;
    float4 f[NJ];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int c = lane * 4 + j * 256;
        f[j] = float4{0.f, 0.f, 0.f, 0.f};
        if (c < H) {
            f[j] = load_bf16x4(e + c);
            const float4 ty = *(const float4 *)(type0 + c);
            f[j].x += ty.x; f[j].y += ty.y; f[j].z += ty.z; f[j].w += ty.w;
            s += (f[j].x + f[j].y) + (f[j].z + f[j].w);
        }
    }
    nb_ln_store<NJ>(f, s, H, lane, g, b, eps, x32 + t * H, h16 + t * H);
}

// one wave per token t < T: x32 = LayerNorm(x32 + y32; g, b) (y32 the sub-layer's float32 GEMM output), h16 = bf16(x32). The row
// stays in registers between the add, the two reductions and the stores: one pass over memory.
template <int NJ>
__global__ __launch_bounds__(256) void k_nb_add_ln(float *__restrict__ x32, const float *__restrict__ y32, int64_t T, int H, const float *__restrict__ g,
                                                   const float *__restrict__ b, float eps, uint16_t *__restrict__ h16) {
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= T) return;
    float *xr = x32 + t * H;
    const float *yr = y32 + t * H;
    float4 f[NJ];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int c = lane * 4 + j * 256;
        f[j] = float4{0.f, 0.f, 0.f, 0.f};
        if (c < H) {
            f[j] = *(const float4 *)(xr + c);
            const float4 y = *(const float4 *)(yr + c);
            f[j].x += y.x; f[j].y += y.y; f[j].z += y.z; f[j].w += y.w;
            s += (f[j].x + f[j].y) + (f[j].z + f[j].w);
        }
    }
    nb_ln_store<NJ>(f, s, H, lane, g, b, eps, xr, h16 + t * H);
}

// Pooling, stage 1 (pool_part of stack.h) over the pooled tokens of a row -- mean: its length; cls: token 0 --, the per-token
// transform the identity: the model has no final norm.
struct NbIdentity {
    int pooling;
    struct Token {
        __device__ float apply(float x) const { return x; }
    };
    __device__ int count(int len) const { return len <= 0 ? 0 : (pooling == AK_POOL_CLS ? 1 : len); }
    __device__ Token begin(const float *, int, int) const { return Token{}; }
};
__global__ __launch_bounds__(256) void k_nb_pool_part(const float *__restrict__ x32, const int *__restrict__ lens, int S, int H, int pooling,
                                                      float *__restrict__ part) {
    pool_part(x32, lens, S, H, NbIdentity{pooling}, part);
}

// Pooling, stage 2. One workgroup per row b: the chunk sums added in chunk order, / n, then the L2 normalisation. A row of length 0
// embeds to zeros.
__global__ __launch_bounds__(256) void k_nb_pool_fin(const float *__restrict__ part, int nch, const int *__restrict__ lens, int H, int pooling,
                                                     int normalise, float *__restrict__ out) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = lens[b];
    float *o = out + (int64_t)b * H;
    if (len <= 0) {
        for (int c = tid; c < H; c += 256) o[c] = 0.f;
        return;
    }
    const int n = pooling == AK_POOL_CLS ? 1 : len, used = (n + POOL_CHUNK - 1) / POOL_CHUNK;
    const float inv_n = 1.0f / (float)n;
    float y[NB_MAX_H / 256];
    float s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NB_MAX_H / 256; j++) {
        const int c = tid + j * 256;
        y[j] = 0.f;
        if (c < H) {
            for (int ck = 0; ck < used; ck++) y[j] += part[((int64_t)b * nch + ck) * H + c];
            y[j] = y[j] * inv_n;
            s2 += y[j] * y[j];
        }
    }
    const float sc = block_l2_scale(s2, lane, wave, normalise);
#pragma unroll
    for (int j = 0; j < NB_MAX_H / 256; j++) {
        const int c = tid + j * 256;
        if (c < H) o[c] = y[j] * sc;
    }
}

}  // namespace

// ---- launches: the one place each kernel's grid is spelled (the forward pass below and the single-launch tests call these) ----
int launch_nb_embed(const int *ids, int ld_ids, const int *lens, int lens_stride, int B, int S, int H, int vocab, const uint16_t *word,
                    const float *type0, const float *g, const float *b, float eps, float *x32, uint16_t *h16, int *mask, int *lens_out, hipStream_t st) {
    const unsigned rows4 = (unsigned)(((int64_t)B * S + 3) / 4);
    dispatch_nj(H, [&](auto nj) {
        k_nb_embed<decltype(nj)::value><<<rows4, 256, 0, st>>>(ids, ld_ids, lens, lens_stride, B, S, H, vocab, word, type0, g, b, eps, x32, h16, mask,
                                                               lens_out);
    });
    AK_HIP(hipGetLastError());
    return 0;
}

int launch_nb_add_ln(float *x32, const float *y32, int64_t T, int H, const float *g, const float *b, float eps, uint16_t *h16, hipStream_t st) {
    const unsigned rows4 = (unsigned)((T + 3) / 4);
    dispatch_nj(H, [&](auto nj) { k_nb_add_ln<decltype(nj)::value><<<rows4, 256, 0, st>>>(x32, y32, T, H, g, b, eps, h16); });
    AK_HIP(hipGetLastError());
    return 0;
}

// both pooling stages: part [B][ceil(S / 64)][H] floats of workspace
int launch_nb_pool(const float *x32, const int *lens, int B, int S, int H, int pooling, int normalise, float *part, float *out, hipStream_t st) {
    const int nch = (S + POOL_CHUNK - 1) / POOL_CHUNK;
    k_nb_pool_part<<<dim3((unsigned)nch, (unsigned)B), 256, (size_t)4 * H * 4, st>>>(x32, lens, S, H, pooling, part);
    AK_HIP(hipGetLastError());
    k_nb_pool_fin<<<B, 256, 0, st>>>(part, nch, lens, H, pooling, normalise, out);
    AK_HIP(hipGetLastError());
    return 0;
}

namespace {
struct NbLayer {
    const uint16_t *wqkv, *wo, *wgu, *wdown;   // wqkv (concatenated) and wgu (gate / up interleaved) are owned, wdown too when I is padded
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
};
struct Nomic : Stack {
    AkNomicBertConfig cfg;
    const uint16_t *word = nullptr; const float *type0 = nullptr, *emb_g = nullptr, *emb_b = nullptr;
    std::vector<NbLayer> layers;
    float *rope_c = nullptr, *rope_s = nullptr;
    int Ip = 0;                                // intermediate size as the GEMMs see it (padded_intermediate)
    float *x32 = nullptr, *y32 = nullptr;
    uint16_t *h16 = nullptr, *q = nullptr, *k = nullptr, *vt = nullptr, *ctx = nullptr, *f = nullptr;
    float *part = nullptr;                     // pooling: chunk sums [B][ceil(S / 64)][H]
    int *mask = nullptr, *lens = nullptr;
};

int nb_forward_locked(Nomic &d, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S, int pooling, int normalise,
                      float *out, hipStream_t st) {
    const AkNomicBertConfig &c = d.cfg;
    const int H = c.hidden, I = d.Ip, heads = c.heads;
    const int64_t T = (int64_t)B * S, tpad = (T + 255) / 256 * 256;
    if (d.reserve(tpad, B)) return -10;
    if (launch_nb_embed(ids, ld_ids, lens, lens_stride, B, S, H, c.vocab_size, d.word, d.type0, d.emb_g, d.emb_b, c.ln_eps, d.x32, d.h16, d.mask,
                        d.lens, st))
        return -10;
    for (const NbLayer &ly : d.layers) {
        // q (scaled) | k | V^T
        GemmArgs g = d.gemm(tpad, d.h16, ly.wqkv, 3 * H, H);
        g.q = d.q; g.k = d.k; g.vt = d.vt; g.H = H; g.S = S; g.qscale = 1.4426950408889634f / sqrtf((float)NB_HD);
        g.ldo = (int)T;                                        // MODE 0: number of real tokens (rows beyond it have no V^T slot)
        if (launch_gemm(0, g, st)) return -10;
        if (launch_mb_rope(d.q, d.k, T, S, H, d.rope_c, d.rope_s, st)) return -10;
        AttnArgs a{d.q, d.k, d.vt, d.mask, d.ctx, B, S, H, heads, nullptr, nullptr, 0, 0, nullptr, d.lens};
        if (launch_attn_window(a, -1, st)) return -10;
        // x = LayerNorm(x + ctx Wo^T; ln1)
        if (launch_gemm(2, d.gemm_f32(tpad, d.ctx, ly.wo, H, H, d.y32), st)) return -10;
        if (launch_nb_add_ln(d.x32, d.y32, T, H, ly.ln1_g, ly.ln1_b, c.ln_eps, d.h16, st)) return -10;
        // f = silu(h Wgate^T) (h Wup^T)
        if (launch_gemm(7, d.gemm_gated(tpad, d.h16, ly.wgu, I, H, d.f), st)) return -10;
        // x = LayerNorm(x + f Wdown^T; ln2)
        if (launch_gemm(2, d.gemm_f32(tpad, d.f, ly.wdown, H, I, d.y32), st)) return -10;
        if (launch_nb_add_ln(d.x32, d.y32, T, H, ly.ln2_g, ly.ln2_b, c.ln_eps, d.h16, st)) return -10;
    }
    return launch_nb_pool(d.x32, d.lens, B, S, H, pooling, normalise, d.part, out, st) ? -10 : 0;
}
}  // namespace

}  // namespace ak

using namespace ak;

extern "C" int ak_nomic_destroy(ak_nomic_t h) { return stack_destroy<Nomic>(h); }

extern "C" int ak_nomic_create(const AkNomicBertConfig *cfg, const void *const *w, int n_weights, ak_nomic_t *out) {
    AK_BIND();
    if (!cfg || !w || !out) AK_FAIL(-1, "ak_nomic_create: NULL argument");
    *out = nullptr;
    const AkNomicBertConfig c = *cfg;
    const int H = c.hidden, I = c.intermediate, L = c.layers;
    if (L <= 0 || c.vocab_size <= 0 || c.heads <= 0 || H <= 0 || I <= 0 || c.type_vocab <= 0 || c.max_position <= 0)
        AK_FAIL(-1, "ak_nomic_create: sizes must be positive");
    if (L > AK_MBERT_MAX_LAYERS) AK_FAIL(-1, "ak_nomic_create: more than AK_MBERT_MAX_LAYERS layers");
    if (H != c.heads * NB_HD) AK_FAIL(-1, "ak_nomic_create: head size (hidden / heads) must be 64");
    if (H % 128 || H > NB_MAX_H || I % 64) AK_FAIL(-1, "ak_nomic_create: hidden must be a multiple of 128 (<= 1024), intermediate a multiple of 64");
    if (!(c.ln_eps > 0.f) || !(c.rope_theta > 0.f)) AK_FAIL(-1, "ak_nomic_create: ln_eps and rope_theta must be positive");
    if (n_weights != 4 + 11 * L) AK_FAIL(-1, "ak_nomic_create: expected 4 + 11 * layers weight pointers");
    for (int i = 0; i < n_weights; i++)
        if (!w[i]) AK_FAIL(-1, "ak_nomic_create: NULL weight pointer");
    Nomic *d = new Nomic();
    d->cfg = c;
    d->word = (const uint16_t *)w[0];
    d->type0 = (const float *)w[1];            // row 0 of [type_vocab][H]: single sentences only
    d->emb_g = (const float *)w[2];
    d->emb_b = (const float *)w[3];
    auto fail = [&](const char *what) { set_error(what); ak_nomic_destroy(d); return -10; };
    const int Ip = d->Ip = padded_intermediate(I);
    d->zero_bias = d->dev_as<float>(std::max<size_t>((size_t)3 * H, (size_t)2 * Ip), true);
    if (!d->zero_bias) return fail("ak_nomic_create: hipMalloc failed");
    // one rotary table, positions 0 .. min(max_position, 8192) - 1, at head size 64
    d->n_pos = c.max_position < NB_MAX_S ? c.max_position : NB_MAX_S;
    if (!d->rope_tables(c.rope_theta, NB_HD, &d->rope_c, &d->rope_s)) return fail("ak_nomic_create: rotary table upload failed");
    for (int l = 0; l < L; l++) {
        const void *const *p = w + 4 + 11 * l;     // wq wk wv wo ln1_g ln1_b w_gate w_up w_down ln2_g ln2_b
        NbLayer ly{};
        uint16_t *wqkv = d->dev_as<uint16_t>((size_t)3 * H * H);
        uint16_t *wgu = d->dev_as<uint16_t>((size_t)2 * Ip * H, Ip != I);
        if (!wqkv || !wgu) return fail("ak_nomic_create: hipMalloc failed");
        if (!d->concat_rows(wqkv, H, {{p[0], (size_t)H}, {p[1], (size_t)H}, {p[2], (size_t)H}})) return fail("ak_nomic_create: QKV concatenation failed");
        // row 2 j = gate row j, row 2 j + 1 = up row j (gemm.hip MODE 7)
        if (!d->interleave_rows(wgu, p[6], p[7], I, H)) return fail("ak_nomic_create: gate / up interleave failed");
        ly.wqkv = wqkv; ly.wo = (const uint16_t *)p[3]; ly.ln1_g = (const float *)p[4]; ly.ln1_b = (const float *)p[5];
        ly.wgu = wgu; ly.wdown = (const uint16_t *)p[8]; ly.ln2_g = (const float *)p[9]; ly.ln2_b = (const float *)p[10];
        if (Ip != I && !(ly.wdown = d->pad_cols(p[8], H, I, Ip))) return fail("ak_nomic_create: w_down padding failed");
        d->layers.push_back(ly);
    }
    const size_t row16 = (size_t)H * 2;
    d->buffer(&d->x32, (size_t)H * 4); d->buffer(&d->y32, (size_t)H * 4); d->buffer(&d->h16, row16);
    d->buffer(&d->q, row16); d->buffer(&d->k, row16); d->buffer(&d->vt, row16); d->buffer(&d->ctx, row16);
    d->buffer(&d->f, (size_t)Ip * 2); d->buffer(&d->mask, 4); d->buffer(&d->lens, 0, 4);
    d->buffer(&d->part, (size_t)H * 4 / POOL_CHUNK, (size_t)H * 4);      // B ceil(S / 64) <= T / 64 + B rows of H floats
    if (hipDeviceSynchronize() != hipSuccess) return fail("ak_nomic_create: weight preparation failed");
    *out = d;
    return 0;
}

extern "C" int ak_nomic_forward_lens(ak_nomic_t h, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S, int pooling,
                                     int normalise, float *out, void *stream) {
    AK_BIND();
    if (!h) AK_FAIL(-1, "ak_nomic_forward_lens: NULL handle");
    RoctxRange range("ak_nomic_forward_lens");
    Nomic &d = *(Nomic *)h;
    if (B <= 0) return 0;
    const bool pool_ok = pooling == AK_POOL_MEAN || pooling == AK_POOL_CLS;
    if (check_forward_lens("ak_nomic_forward_lens", ids, lens, out, ld_ids, lens_stride, B, S, NB_MAX_S, d.n_pos,
                           pool_ok ? nullptr : "pooling must be AK_POOL_MEAN or AK_POOL_CLS", 65535))
        return -1;
    std::lock_guard<std::mutex> lk(d.mu);
    return nb_forward_locked(d, ids, ld_ids, lens, lens_stride, B, S, pooling, normalise, out, (hipStream_t)stream);
}
