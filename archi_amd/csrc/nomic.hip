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
// LayerNorms carry a bias. Here: the config struct's own checks, the layer struct, the order of a layer (block, join, block, join)
// and the family's kernels: the embedding, the join k_nb_add_ln, the identity transform of the pool. stack.h holds the token-slot
// prologue, the LayerNorm of a row in registers, both pooling bodies and the NJ dispatch; enc64.h (shared with mbert.hip) the handle's
// workspace, the common create steps, the attention and FFN blocks and the body of ak_nomic_forward_lens. Nothing here reads the
// environment.
// LDS per workgroup: k_nb_embed / k_nb_add_ln none; k_nb_pool_part 4 * H * 4 bytes (dynamic: 12 KB at H = 768); k_nb_pool_fin 16 bytes.
#include "enc64.h"

namespace ak {

namespace {
// The tail both row kernels share, one wave per row held in registers (NJ float4 per lane, feature c = 4 lane + 256 j; lanes at or
// past H hold zeros and store nothing): s = the lane's share of the row's sum. The statistics: row_ln_stats (stack.h); x32 row =
// (f - mean) rstd g + b in float32, h16 row = bf16 of it.
template <int NJ>
__device__ inline void nb_ln_store(float4 (&f)[NJ], float s, int H, int lane, const float *__restrict__ g, const float *__restrict__ b, float eps,
                                   float *__restrict__ xr, uint16_t *__restrict__ hr) {
    float mean, rstd;
    row_ln_stats(f, s, H, lane, eps, mean, rstd);
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
    float4 f[NJ];
    const float s = row_load_sum<false>(word + (int64_t)id * H, type0, H, lane, f);
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
    float4 f[NJ];
    const float s = row_load_sum<false>(xr, y32 + t * H, H, lane, f);
    nb_ln_store<NJ>(f, s, H, lane, g, b, eps, xr, h16 + t * H);
}

// Pooling, stage 1 (pool_part of stack.h) over the pooled tokens of a row -- mean: its length; cls: token 0 --, the per-token
// transform the identity: the model has no final norm.
struct NbIdentity {
    int pooling;
    struct Token {
        __device__ float apply(float x) const { return x; }
    };
    __device__ int count(int len) const { return pooled_count(len, pooling); }
    __device__ Token begin(const float *, int, int) const { return Token{}; }
};
__global__ __launch_bounds__(256) void k_nb_pool_part(const float *__restrict__ x32, const int *__restrict__ lens, int S, int H, int pooling,
                                                      float *__restrict__ part) {
    pool_part(x32, lens, S, H, NbIdentity{pooling}, part);
}

// Pooling, stage 2 (pool_fin of stack.h) without a weight: sum / n, then the L2 normalisation
__global__ __launch_bounds__(256) void k_nb_pool_fin(const float *__restrict__ part, int nch, const int *__restrict__ lens, int H, int pooling,
                                                     int normalise, float *__restrict__ out) {
    pool_fin<false>(part, nch, lens, H, nullptr, pooling, normalise, out);
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
    return launch_pool_stages(
        B, S, H, [&](dim3 grid, size_t lds) { k_nb_pool_part<<<grid, 256, lds, st>>>(x32, lens, S, H, pooling, part); },
        [&](int nch) { k_nb_pool_fin<<<B, 256, 0, st>>>(part, nch, lens, H, pooling, normalise, out); });
}

namespace {
struct NbLayer {
    const uint16_t *wqkv, *wo, *wgu, *wdown;   // wqkv (concatenated) and wgu (gate / up interleaved) are owned, wdown too when I is padded
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
};
struct Nomic : Enc64 {
    AkNomicBertConfig cfg;
    const uint16_t *word = nullptr; const float *type0 = nullptr, *emb_g = nullptr, *emb_b = nullptr;
    std::vector<NbLayer> layers;
    float *rope_c = nullptr, *rope_s = nullptr;

    int forward(const int32_t *ids, int ld_ids, const int32_t *lens_in, int lens_stride, int B, int S, int pooling, int normalise, float *out,
                hipStream_t st) {
        const float eps = cfg.ln_eps;
        const int64_t T = (int64_t)B * S, tpad = (T + 255) / 256 * 256;
        if (reserve(tpad, B)) return -10;
        if (launch_nb_embed(ids, ld_ids, lens_in, lens_stride, B, S, H, cfg.vocab_size, word, type0, emb_g, emb_b, eps, x32, h16, mask, lens, st))
            return -10;
        for (const NbLayer &ly : layers) {
            // x = LayerNorm(x + attention(h) Wo^T; ln1), every key
            if (attention_block(tpad, B, S, ly.wqkv, ly.wo, rope_c, rope_s, -1, st)) return -10;
            if (launch_nb_add_ln(x32, y32, T, H, ly.ln1_g, ly.ln1_b, eps, h16, st)) return -10;
            // x = LayerNorm(x + (silu(h Wgate^T) (h Wup^T)) Wdown^T; ln2)
            if (ffn_block(7, tpad, ly.wgu, ly.wdown, st)) return -10;
            if (launch_nb_add_ln(x32, y32, T, H, ly.ln2_g, ly.ln2_b, eps, h16, st)) return -10;
        }
        return launch_nb_pool(x32, lens, B, S, H, pooling, normalise, part, out, st) ? -10 : 0;
    }
};
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
    if (Enc64::check_sizes("ak_nomic_create", H, I, c.heads, L, c.vocab_size, c.max_position, c.type_vocab > 0)) return -1;
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
    auto fail = [&](const char *what) { return enc64_create_failed(d, "ak_nomic_create", what); };
    if (const char *what = d->init(H, c.heads, I, c.max_position)) return fail(what);
    if (!d->rope_table(c.rope_theta, &d->rope_c, &d->rope_s)) return fail("rotary table upload failed");
    for (int l = 0; l < L; l++) {
        const void *const *p = w + 4 + 11 * l;     // wq wk wv wo ln1_g ln1_b w_gate w_up w_down ln2_g ln2_b
        NbLayer ly{};
        uint16_t *wqkv = d->dev_as<uint16_t>((size_t)3 * H * H);
        if (!wqkv) return fail("hipMalloc failed");
        if (!d->concat_rows(wqkv, H, {{p[0], (size_t)H}, {p[1], (size_t)H}, {p[2], (size_t)H}})) return fail("QKV concatenation failed");
        if (const char *what = d->prepare_gated(p[6], p[7], I, p[8], &ly.wgu, &ly.wdown)) return fail(what);
        ly.wqkv = wqkv; ly.wo = (const uint16_t *)p[3]; ly.ln1_g = (const float *)p[4]; ly.ln1_b = (const float *)p[5];
        ly.ln2_g = (const float *)p[9]; ly.ln2_b = (const float *)p[10];
        d->layers.push_back(ly);
    }
    if (hipDeviceSynchronize() != hipSuccess) return fail("weight preparation failed");
    *out = d;
    return 0;
}

extern "C" int ak_nomic_forward_lens(ak_nomic_t h, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S, int pooling,
                                     int normalise, float *out, void *stream) {
    return enc64_forward_lens<Nomic>("ak_nomic_forward_lens", h, ids, ld_ids, lens, lens_stride, B, S, pooling, normalise, out, stream);
}
