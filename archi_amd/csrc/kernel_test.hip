// kernel_test.hip -- single-launch entry points for the kernel-level tests (tests/test_kernels_gpu.py and its siblings). They exist in
// libarchi_hip_dbg.so only (-DAK_DBG_KERNELS=1); the product library gets an empty object from this file and exports no ak_kt_*.
// Every wrapper fills the launcher's argument block from device pointers and calls the launcher the forward pass calls: no
// arithmetic, no kernel selection of its own. With no AK_* switch set the instantiation that runs is the one the product launches;
// a shape the launcher refuses comes back as its error code (ak_last_error has the text).
#include "encoder_kernels.h"
#include "index.h"

#if AK_DBG_KERNELS

using namespace ak;

// the GemmArgs fields that modes 0, 1, 2, 4, 7 and 8 read (tests/kernel_worker.py mirrors this struct with ctypes)
struct AkKtGemm {
    const uint16_t *X, *W; const float *bias;
    int T, N, K;
    uint16_t *out_bf16; int ldo;
    float *out_f32;
    const uint16_t *res16;
    uint16_t *q, *k, *vt; int H, S; float qscale;
};

static AttnArgs kt_attn_args(const uint16_t *q, const uint16_t *k, const uint16_t *vt, const int *mask, uint16_t *ctx, int B, int S, int H,
                             int heads, int qk_ld, int qk_hs) {
    AttnArgs a{};
    a.q = q; a.k = k; a.vt = vt; a.mask = mask; a.ctx = ctx;
    a.B = B; a.S = S; a.H = H; a.heads = heads;
    a.qk_ld = qk_ld; a.qk_hs = qk_hs;
    return a;
}

// launch_attn_prepare + launch_attn (S <= 512). maskf [B][S] floats and blkmask [B] words are workspace; unstreamed != 0 passes
// maskf = blkmask = NULL to launch_attn (k_attn). rel: [heads][REL_ROW] floats or NULL.
extern "C" int ak_kt_attn(const uint16_t *q, const uint16_t *k, const uint16_t *vt, const int *mask, uint16_t *ctx, int B, int S, int H,
                          int heads, int qk_ld, int qk_hs, const float *rel, float *maskf, uint32_t *blkmask, int unstreamed,
                          void *stream) {
    AK_BIND();
    hipStream_t st = (hipStream_t)stream;
    AttnArgs a = kt_attn_args(q, k, vt, mask, ctx, B, S, H, heads, qk_ld, qk_hs);
    a.rel = rel;
    if (!unstreamed) {
        if (int rc = launch_attn_prepare(mask, B, S, maskf, blkmask, st)) return rc;
        a.maskf = maskf; a.blkmask = blkmask;
    }
    return launch_attn(a, st);
}

extern "C" int ak_kt_attn_long(const uint16_t *q, const uint16_t *k, const uint16_t *vt, const int *mask, const int *rowlen, uint16_t *ctx,
                               int B, int S, int H, int heads, int qk_ld, int qk_hs, void *stream) {
    AK_BIND();
    AttnArgs a = kt_attn_args(q, k, vt, mask, ctx, B, S, H, heads, qk_ld, qk_hs);
    a.rowlen = rowlen;
    return launch_attn_long(a, (hipStream_t)stream);
}

extern "C" int ak_kt_attn_window(const uint16_t *q, const uint16_t *k, const uint16_t *vt, const int *mask, const int *rowlen, uint16_t *ctx,
                                 int B, int S, int H, int heads, int qk_ld, int qk_hs, int window, void *stream) {
    AK_BIND();
    AttnArgs a = kt_attn_args(q, k, vt, mask, ctx, B, S, H, heads, qk_ld, qk_hs);
    a.rowlen = rowlen;
    return launch_attn_window(a, window, (hipStream_t)stream);
}

extern "C" int ak_kt_attn_causal(const uint16_t *q, const uint16_t *k, const uint16_t *v, const int *lens, uint16_t *ctx, int B, int S,
                                 int nq, int nkv, void *stream) {
    AK_BIND();
    CausalAttnArgs a{};
    a.q = q; a.k = k; a.v = v; a.lens = lens; a.ctx = ctx;
    a.B = B; a.S = S; a.nq = nq; a.nkv = nkv;
    return launch_attn_causal(a, (hipStream_t)stream);
}

extern "C" int ak_kt_gemm(int mode, const AkKtGemm *g, void *stream) {
    AK_BIND();
    if (!g) AK_FAIL(-1, "ak_kt_gemm: NULL argument block");
    if (mode != 0 && mode != 1 && mode != 2 && mode != 4 && mode != 7 && mode != 8) AK_FAIL(-1, "ak_kt_gemm: mode must be 0, 1, 2, 4, 7 or 8");
    GemmArgs a{};
    a.X = g->X; a.W = g->W; a.bias = g->bias;
    a.T = g->T; a.N = g->N; a.K = g->K;
    a.out_bf16 = g->out_bf16; a.ldo = g->ldo;
    a.out_f32 = g->out_f32;
    a.res16 = g->res16;
    a.q = g->q; a.k = g->k; a.vt = g->vt; a.H = g->H; a.S = g->S; a.qscale = g->qscale;
    return launch_gemm(mode, a, (hipStream_t)stream);
}

extern "C" int ak_kt_gemm_skinny(const uint16_t *X, const uint16_t *W, const float *bias, int rows, int N, int K, float *out_f32,
                                 uint16_t *out_bf16, int ldo, void *stream) {
    AK_BIND();
    return launch_gemm_skinny(X, W, bias, rows, N, K, out_f32, out_bf16, ldo, (hipStream_t)stream);
}

extern "C" int ak_kt_gemm_skinny_qkv(const uint16_t *X, const uint16_t *W, const float *bias, int rows, int H, int K, uint16_t *q,
                                     uint16_t *k, uint16_t *vt, int S, int T, float qscale, void *stream) {
    AK_BIND();
    return launch_gemm_skinny_qkv(X, W, bias, rows, H, K, q, k, vt, S, T, qscale, (hipStream_t)stream);
}

// launch_gemm_ln: x32 != NULL the float32 residual stream (in place) with its bf16 copy x16; x32 == NULL: x16 alone, in place
extern "C" int ak_kt_gemm_ln(const uint16_t *X, const uint16_t *W, const float *bias, const float *gamma, const float *beta, float *x32,
                             uint16_t *x16, int T, int K, float eps, void *stream) {
    AK_BIND();
    if (!gemm_ln_supported(384, T, K)) AK_FAIL(-1, "ak_kt_gemm_ln: gemm_ln_supported refuses this shape");
    GemmLnArgs a{X, W, bias, gamma, beta, x32, x16, T, K, eps, nullptr};
    return launch_gemm_ln(a, (hipStream_t)stream);
}

// ffn_relayout into wbuf (ak_kt_ffn384_weight_bytes(I) bytes), as ak_encoder_create does, then launch_ffn384. ctx == NULL: the
// feed-forward block alone (wo, bo, gamma1, beta1 unused by the kernel; wo is still laid out: one relayout call)
extern "C" long long ak_kt_ffn384_weight_bytes(int I) { return (long long)ffn_weight_bytes(I); }
extern "C" int ak_kt_ffn384(uint16_t *x16, const uint16_t *wo, const uint16_t *w1, const uint16_t *w2, const float *b1, const float *b2,
                            const float *gamma2, const float *beta2, const uint16_t *ctx, const float *bo, const float *gamma1,
                            const float *beta1, uint16_t *wbuf, int T, int I, float eps, void *stream) {
    AK_BIND();
    hipStream_t st = (hipStream_t)stream;
    if (!ffn_fused_supported(384, I, T)) AK_FAIL(-1, "ak_kt_ffn384: ffn_fused_supported refuses this shape");
    const uint16_t *wf = nullptr;
    if (int rc = ffn_relayout(wo, w1, w2, I, wbuf, &wf, st)) return rc;
    FfnArgs a{x16, wf, b1, b2, gamma2, beta2, ctx, ctx ? wbuf : nullptr, ctx ? bo : nullptr, ctx ? gamma1 : nullptr, ctx ? beta1 : nullptr, T, I, eps, nullptr};
    return launch_ffn384(a, st);
}

// qkv384_relayout into wbuf (ak_kt_qkv384_weight_bytes() bytes), then launch_qkv384
extern "C" long long ak_kt_qkv384_weight_bytes() { return (long long)qkv384_weight_bytes(); }
extern "C" int ak_kt_qkv384(const uint16_t *x16, const uint16_t *wqkv, const float *bqkv, uint16_t *wbuf, uint16_t *q, uint16_t *k,
                            uint16_t *vt, int Tpad, int T, int S, float qscale, int head_major, void *stream) {
    AK_BIND();
    hipStream_t st = (hipStream_t)stream;
    if (!qkv384_supported(384, Tpad, S) || T < 0 || T > Tpad) AK_FAIL(-1, "ak_kt_qkv384: qkv384_supported refuses this shape");
    if (int rc = qkv384_relayout(wqkv, bqkv, wbuf, st)) return rc;
    QkvArgs a{x16, wbuf, nullptr, q, k, vt, Tpad, T, S, qscale, 0, head_major};
    return launch_qkv384(a, st);
}

// the GemmArgs fields the lazy-LayerNorm modes 0, 1 and 4 read (tests/kernel_worker.py mirrors this struct with ctypes)
struct AkKtGemmLazy {
    const uint16_t *X, *W; const float *bias;
    int T, N, K;
    uint16_t *out_bf16; int ldo;
    const uint16_t *res16;
    uint16_t *q, *k, *vt; int H, S; float qscale;
    const float *fold_c, *a_stats, *res_stats, *res_g, *res_b, *out_g;
    float *out_stats;
    int nslot; float inv_h, eps;
};

extern "C" int ak_kt_gemm_lazy(int mode, const AkKtGemmLazy *g, void *stream) {
    AK_BIND();
    if (!g) AK_FAIL(-1, "ak_kt_gemm_lazy: NULL argument block");
    GemmArgs a{};
    a.X = g->X; a.W = g->W; a.bias = g->bias;
    a.T = g->T; a.N = g->N; a.K = g->K;
    a.out_bf16 = g->out_bf16; a.ldo = g->ldo;
    a.res16 = g->res16;
    a.q = g->q; a.k = g->k; a.vt = g->vt; a.H = g->H; a.S = g->S; a.qscale = g->qscale;
    a.fold_c = g->fold_c; a.a_stats = g->a_stats; a.res_stats = g->res_stats; a.res_g = g->res_g; a.res_b = g->res_b; a.out_g = g->out_g;
    a.out_stats = g->out_stats;
    a.nslot = g->nslot; a.inv_h = g->inv_h; a.eps = g->eps;
    return launch_gemm_lazy(mode, a, (hipStream_t)stream);
}

extern "C" int ak_kt_ln_finalize(const float *part, int nslot, long long T, float inv_h, float eps, float *out, void *stream) {
    AK_BIND();
    if (nslot <= 0 || T <= 0) AK_FAIL(-1, "ak_kt_ln_finalize: nslot, T > 0");
    return launch_ln_finalize(part, nslot, T, inv_h, eps, out, (hipStream_t)stream);
}

extern "C" int ak_kt_fold_ln(const uint16_t *W, const float *gamma, const float *beta, const float *bias, int N, int K, float *c, float *bf,
                             void *stream) {
    AK_BIND();
    if (N <= 0 || K <= 0) AK_FAIL(-1, "ak_kt_fold_ln: N, K > 0");
    return launch_fold_ln(W, gamma, beta, bias, N, K, c, bf, (hipStream_t)stream);
}

// the stand-alone LayerNorm launches of the forward pass (encoder.hip)
extern "C" int ak_kt_layernorm(const float *x, const float *res, const uint16_t *res16, const float *g, const float *bta, int T, int H,
                               float eps, float *y32, uint16_t *y16, const uint16_t *x16in, void *stream) {
    AK_BIND();
    if (T <= 0 || H <= 0 || H % 4 || H > 1024) AK_FAIL(-1, "ak_kt_layernorm: H % 4 == 0, H <= 1024");
    launch_layernorm(x, res, res16, g, bta, T, H, eps, y32, y16, x16in, (hipStream_t)stream);
    AK_HIP(hipGetLastError());
    return 0;
}

extern "C" int ak_kt_layernorm16(const uint16_t *x16in, const float *g, const float *bta, int T, int H, float eps, uint16_t *y16, void *stream) {
    AK_BIND();
    if (T <= 0 || !launch_layernorm16(H, x16in, g, bta, T, eps, y16, (hipStream_t)stream)) AK_FAIL(-1, "ak_kt_layernorm16: H % 128 == 0, H <= 1024");
    AK_HIP(hipGetLastError());
    return 0;
}

extern "C" int ak_kt_ln_apply16(const uint16_t *rt, const float *stats, const float *g, const float *bta, long long T, int H, uint16_t *y16,
                                void *stream) {
    AK_BIND();
    if (T <= 0 || H <= 0 || H % 8) AK_FAIL(-1, "ak_kt_ln_apply16: H % 8 == 0");
    launch_ln_apply16(rt, stats, g, bta, T, H, y16, (hipStream_t)stream);
    AK_HIP(hipGetLastError());
    return 0;
}

// host only: where key s sits inside its V^T row
extern "C" int ak_kt_vt_pos(int s) { return vt_pos(s); }

// ---- EmbeddingGemma (tests/test_gemma_kernels_gpu.py). Named ak_ktg_*: they are not part of the ak_kt_* set ----
// one launch_attn_gqa: q [B][nq][S][256], k [B][nkv][S][256], vt [B][nkv][256][S] (vt_pos order), ctx [B * S][nq * 256]; half_window 0 = every key
extern "C" int ak_ktg_attn_gqa(const uint16_t *q, const uint16_t *k, const uint16_t *vt, const int *lens, uint16_t *ctx, int B, int S, int nq,
                               int nkv, int half_window, void *stream) {
    AK_BIND();
    GqaAttnArgs a{};
    a.q = q; a.k = k; a.vt = vt; a.lens = lens; a.ctx = ctx;
    a.B = B; a.S = S; a.nq = nq; a.nkv = nkv;
    return launch_attn_gqa(a, half_window, (hipStream_t)stream);
}

// one k_gm_qk_norm_rope launch: qkv [B * S][(nq + 2 nkv) 256]; qn / kn the folded (1 + w) head-norm weights; rc / rs [n_pos][128]
extern "C" int ak_ktg_qk_norm_rope(const uint16_t *qkv, int B, int S, int nq, int nkv, const float *qn, const float *kn, float eps,
                                   const float *rc, const float *rs, float qscale, uint16_t *q, uint16_t *k, uint16_t *vt, void *stream) {
    AK_BIND();
    return launch_gm_qk_norm_rope(qkv, B, S, nq, nkv, qn, kn, eps, rc, rs, qscale, q, k, vt, (hipStream_t)stream);
}

// one launch_gemm(9): the tanh-GeGLU epilogue; X [T][K], W [N][K] (gate / up rows interleaved), out [T][N / 2] bf16
extern "C" int ak_ktg_gemm_geglu_tanh(const uint16_t *X, const uint16_t *W, const float *bias, int T, int N, int K, uint16_t *out, void *stream) {
    AK_BIND();
    GemmArgs a{};
    a.X = X; a.W = W; a.bias = bias; a.T = T; a.N = N; a.K = K; a.out_bf16 = out; a.ldo = N / 2;
    return launch_gemm(9, a, (hipStream_t)stream);
}

// ---- the small kernels of the stacks, NomicBERT's among them (tests/test_stack_kernels_gpu.py). Named ak_kts_*: a set of their own, like ak_ktg_*.
// Each wrapper hands its arguments to the launch_* function the forward pass calls; it refuses only what that function's callers
// guarantee (the shape rules of the handles' create and of check_forward_lens), so that a mistaken test shape cannot leave a buffer ----
static bool kts_rows(long long T, int H, int max_H) { return T > 0 && T <= 0x7fffffff && H > 0 && H % 128 == 0 && (!max_H || H <= max_H); }
static bool kts_embed(const int *ids, const int *lens, int ld_ids, int lens_stride, int B, int S, int H, int vocab, int max_H) {
    return ids && lens && B > 0 && S > 0 && S % 32 == 0 && ld_ids >= S && lens_stride >= 1 && vocab > 0 && kts_rows((long long)B * S, H, max_H);
}

extern "C" int ak_kts_dec_embed(const int *ids, int ld_ids, const int *lens, int lens_stride, int B, int S, int H, int vocab, const uint16_t *emb,
                                const float *w, float eps, float *x32, uint16_t *h16, int *lens_out, void *stream) {
    AK_BIND();
    if (!kts_embed(ids, lens, ld_ids, lens_stride, B, S, H, vocab, 0)) AK_FAIL(-1, "ak_kts_dec_embed: bad shape");
    return launch_dec_embed(ids, ld_ids, lens, lens_stride, B, S, H, vocab, emb, w, eps, x32, h16, lens_out, (hipStream_t)stream);
}

extern "C" int ak_kts_dec_add_rmsnorm(float *x32, const float *y32, long long T, int H, const float *w, float eps, uint16_t *h16, void *stream) {
    AK_BIND();
    if (!kts_rows(T, H, 0)) AK_FAIL(-1, "ak_kts_dec_add_rmsnorm: bad shape");
    return launch_dec_add_rmsnorm(x32, y32, T, H, w, eps, h16, (hipStream_t)stream);
}

// qkv [B * S][(nq + 2 nkv) 128]; rc / rs [>= S][64]; q [B][nq][S][128], k / v [B][nkv][S][128]
extern "C" int ak_kts_dec_qk_rope(const uint16_t *qkv, int B, int S, int nq, int nkv, const float *qn, const float *kn, float eps, const float *rc,
                                  const float *rs, float qscale, uint16_t *q, uint16_t *k, uint16_t *v, void *stream) {
    AK_BIND();
    if (B <= 0 || S <= 0 || nq <= 0 || nkv <= 0 || (long long)B * S > 0x7fffffff) AK_FAIL(-1, "ak_kts_dec_qk_rope: bad shape");
    return launch_dec_qk_rope(qkv, B, S, nq, nkv, qn, kn, eps, rc, rs, qscale, q, k, v, (hipStream_t)stream);
}

extern "C" int ak_kts_dec_pool(const float *x32, const int *lens, int B, int S, int H, const float *w, float eps, int normalise, float *out,
                               void *stream) {
    AK_BIND();
    if (B <= 0 || S <= 0 || H <= 0) AK_FAIL(-1, "ak_kts_dec_pool: bad shape");
    return launch_dec_pool(x32, lens, B, S, H, w, eps, normalise, out, (hipStream_t)stream);
}

// launch_attn_causal through the new arguments (decoder128.hip): window 0 = the plain causal kernel, w > 0 the sliding window; bidirectional != 0: every key below the length
extern "C" int ak_kts_ll_attn(const uint16_t *q, const uint16_t *k, const uint16_t *v, const int *lens, uint16_t *ctx, int B, int S, int nq,
                              int nkv, int window, int bidirectional, void *stream) {
    AK_BIND();
    CausalAttnArgs a{};
    a.q = q; a.k = k; a.v = v; a.lens = lens; a.ctx = ctx;
    a.B = B; a.S = S; a.nq = nq; a.nkv = nkv; a.window = window; a.bidirectional = bidirectional;
    return launch_attn_causal(a, (hipStream_t)stream);
}

// launch_attn_causal_split (Qwen2: 5 to 8 query heads per kv head), the arguments of ak_kts_ll_attn without the window.
// Named ak_kts_q2_*: the ak_kts_ll_* set stays the three it is
extern "C" int ak_kts_q2_attn(const uint16_t *q, const uint16_t *k, const uint16_t *v, const int *lens, uint16_t *ctx, int B, int S, int nq,
                              int nkv, int bidirectional, void *stream) {
    AK_BIND();
    CausalAttnArgs a{};
    a.q = q; a.k = k; a.v = v; a.lens = lens; a.ctx = ctx;
    a.B = B; a.S = S; a.nq = nq; a.nkv = nkv; a.bidirectional = bidirectional;
    return launch_attn_causal_split(a, (hipStream_t)stream);
}

// qkv [B * S][(nq + 2 nkv) 128]; rc / rs [>= S][64]; q [B][nq][S][128], k / v [B][nkv][S][128]
extern "C" int ak_kts_ll_rope(const uint16_t *qkv, int B, int S, int nq, int nkv, const float *rc, const float *rs, float qscale, uint16_t *q,
                              uint16_t *k, uint16_t *v, void *stream) {
    AK_BIND();
    return launch_ll_rope(qkv, B, S, nq, nkv, rc, rs, qscale, q, k, v, (hipStream_t)stream);
}

// part: [B][ceil(S / 64)][H] floats of workspace
extern "C" int ak_kts_ll_pool(const float *x32, const int *lens, int B, int S, int H, const float *w, float eps, int normalise, float *part,
                              float *out, void *stream) {
    AK_BIND();
    return launch_ll_pool(x32, lens, B, S, H, w, eps, normalise, part, out, (hipStream_t)stream);
}

extern "C" int ak_kts_mb_embed(const int *ids, int ld_ids, const int *lens, int lens_stride, int B, int S, int H, int vocab, const uint16_t *emb,
                               const float *w, float eps, float *x32, uint16_t *h16, int *mask, int *lens_out, void *stream) {
    AK_BIND();
    if (!kts_embed(ids, lens, ld_ids, lens_stride, B, S, H, vocab, 1024)) AK_FAIL(-1, "ak_kts_mb_embed: bad shape");
    return launch_mb_embed(ids, ld_ids, lens, lens_stride, B, S, H, vocab, emb, w, eps, x32, h16, mask, lens_out, (hipStream_t)stream);
}

extern "C" int ak_kts_mb_add_ln(float *x32, const float *y32, long long T, int H, const float *w, float eps, uint16_t *h16, void *stream) {
    AK_BIND();
    if (!kts_rows(T, H, 1024)) AK_FAIL(-1, "ak_kts_mb_add_ln: bad shape");
    return launch_mb_add_ln(x32, y32, T, H, w, eps, h16, (hipStream_t)stream);
}

// q, k [T][H] bf16 in place; rc / rs [>= S][32]
extern "C" int ak_kts_mb_rope(uint16_t *q, uint16_t *k, long long T, int S, int H, const float *rc, const float *rs, void *stream) {
    AK_BIND();
    if (!kts_rows(T, H, 0) || S <= 0 || T % S) AK_FAIL(-1, "ak_kts_mb_rope: bad shape");
    return launch_mb_rope(q, k, T, S, H, rc, rs, (hipStream_t)stream);
}

extern "C" int ak_kts_mb_pool(const float *x32, const int *lens, int B, int S, int H, float eps, const float *w, int pooling, int normalise,
                              float *part, float *out, void *stream) {
    AK_BIND();
    if (B <= 0 || B > 65535 || S <= 0 || !kts_rows(S, H, 1024) || (pooling != AK_POOL_MEAN && pooling != AK_POOL_CLS))
        AK_FAIL(-1, "ak_kts_mb_pool: bad shape");
    return launch_mb_pool(x32, lens, B, S, H, eps, w, pooling, normalise, part, out, (hipStream_t)stream);
}

// NomicBERT's row kernels. type0: row 0 of the float32 token-type table; g / b: the LayerNorm's weight and bias
extern "C" int ak_kts_nb_embed(const int *ids, int ld_ids, const int *lens, int lens_stride, int B, int S, int H, int vocab, const uint16_t *word,
                               const float *type0, const float *g, const float *b, float eps, float *x32, uint16_t *h16, int *mask, int *lens_out,
                               void *stream) {
    AK_BIND();
    if (!kts_embed(ids, lens, ld_ids, lens_stride, B, S, H, vocab, 1024)) AK_FAIL(-1, "ak_kts_nb_embed: bad shape");
    return launch_nb_embed(ids, ld_ids, lens, lens_stride, B, S, H, vocab, word, type0, g, b, eps, x32, h16, mask, lens_out, (hipStream_t)stream);
}

extern "C" int ak_kts_nb_add_ln(float *x32, const float *y32, long long T, int H, const float *g, const float *b, float eps, uint16_t *h16,
                                void *stream) {
    AK_BIND();
    if (!kts_rows(T, H, 1024)) AK_FAIL(-1, "ak_kts_nb_add_ln: bad shape");
    return launch_nb_add_ln(x32, y32, T, H, g, b, eps, h16, (hipStream_t)stream);
}

// part: [B][ceil(S / 64)][H] floats of workspace
extern "C" int ak_kts_nb_pool(const float *x32, const int *lens, int B, int S, int H, int pooling, int normalise, float *part, float *out,
                              void *stream) {
    AK_BIND();
    if (B <= 0 || B > 65535 || S <= 0 || !kts_rows(S, H, 1024) || (pooling != AK_POOL_MEAN && pooling != AK_POOL_CLS))
        AK_FAIL(-1, "ak_kts_nb_pool: bad shape");
    return launch_nb_pool(x32, lens, B, S, H, pooling, normalise, part, out, (hipStream_t)stream);
}

extern "C" int ak_kts_gm_fold1p(const float *w, int n, float *w1, void *stream) {
    AK_BIND();
    if (n <= 0) AK_FAIL(-1, "ak_kts_gm_fold1p: bad shape");
    return launch_gm_fold1p(w, n, w1, (hipStream_t)stream);
}

extern "C" int ak_kts_gm_embed(const int *ids, int ld_ids, const int *lens, int lens_stride, int B, int S, int H, int vocab, const uint16_t *emb,
                               const float *w, float eps, float *x32, uint16_t *h16, int *lens_out, void *stream) {
    AK_BIND();
    if (!kts_embed(ids, lens, ld_ids, lens_stride, B, S, H, vocab, 1024)) AK_FAIL(-1, "ak_kts_gm_embed: bad shape");
    return launch_gm_embed(ids, ld_ids, lens, lens_stride, B, S, H, vocab, emb, w, eps, x32, h16, lens_out, (hipStream_t)stream);
}

// out32 != NULL: the second norm as float32 rows (out32 may be y32), h16 unused
extern "C" int ak_kts_gm_norm_add_norm(float *x32, const float *y32, long long T, int H, const float *w_post, const float *w_pre, float eps,
                                       uint16_t *h16, float *out32, void *stream) {
    AK_BIND();
    if (!kts_rows(T, H, 1024)) AK_FAIL(-1, "ak_kts_gm_norm_add_norm: bad shape");
    return launch_gm_norm_add_norm(x32, y32, T, H, w_post, w_pre, eps, h16, out32, (hipStream_t)stream);
}

extern "C" int ak_kts_gm_pool(const float *y32, const int *lens, int B, int S, int H, float *part, float *pooled, void *stream) {
    AK_BIND();
    if (B <= 0 || B > 65535 || S <= 0 || !kts_rows(S, H, 1024)) AK_FAIL(-1, "ak_kts_gm_pool: bad shape");
    return launch_gm_pool(y32, lens, B, S, H, part, pooled, (hipStream_t)stream);
}

extern "C" int ak_kts_gm_dense(const float *in, const float *W, int B, int N, int K, float *out, void *stream) {
    AK_BIND();
    if (B <= 0 || B > 65535 || N <= 0 || K <= 0 || K % 4) AK_FAIL(-1, "ak_kts_gm_dense: bad shape");
    return launch_gm_dense(in, W, B, N, K, out, (hipStream_t)stream);
}

extern "C" int ak_kts_gm_l2(const float *in, int B, int D, int normalise, float *out, void *stream) {
    AK_BIND();
    if (B <= 0 || D <= 0) AK_FAIL(-1, "ak_kts_gm_l2: bad shape");
    return launch_gm_l2(in, B, D, normalise, out, (hipStream_t)stream);
}

// one launch_gemm(3): plain bf16 rows, X [T][K], W [N][K] -> out [T][N] (the Qwen3 and Gemma QKV projections)
extern "C" int ak_kts_gemm_bf16(const uint16_t *X, const uint16_t *W, const float *bias, int T, int N, int K, uint16_t *out, void *stream) {
    AK_BIND();
    GemmArgs a{};
    a.X = X; a.W = W; a.bias = bias; a.T = T; a.N = N; a.K = K; a.out_bf16 = out; a.ldo = N;
    return launch_gemm(3, a, (hipStream_t)stream);
}

// ---- T5 (tests/test_t5_kernels_gpu.py). Named ak_kts_t5_*: the other ak_kts_* subsets stay what they are ----
// one launch_attn_relbias: k_attn_long_relbias, every key below the length, rbias [heads][2 D + 1] floats (base-2 domain)
extern "C" int ak_kts_t5_attn(const uint16_t *q, const uint16_t *k, const uint16_t *vt, const int *mask, const int *rowlen, uint16_t *ctx, int B,
                              int S, int H, int heads, int qk_ld, int qk_hs, const float *rbias, int D, void *stream) {
    AK_BIND();
    AttnArgs a = kt_attn_args(q, k, vt, mask, ctx, B, S, H, heads, qk_ld, qk_hs);
    a.rowlen = rowlen;
    a.rbias = rbias; a.rbias_D = D;
    return launch_attn_relbias(a, (hipStream_t)stream);
}

// one launch_gemm(10): the ReLU epilogue; X [T][K], W [N][K] -> out [T][N] bf16
extern "C" int ak_kts_t5_gemm_relu(const uint16_t *X, const uint16_t *W, const float *bias, int T, int N, int K, uint16_t *out, void *stream) {
    AK_BIND();
    GemmArgs a{};
    a.X = X; a.W = W; a.bias = bias; a.T = T; a.N = N; a.K = K; a.out_bf16 = out; a.ldo = N;
    return launch_gemm(10, a, (hipStream_t)stream);
}

// ---- the re-rank kernels of the kNN fast path (tests/test_rerank_panel_gpu.py). Named ak_kts_rr_*: the other subsets stay what they are ----
// query_norms, then ONE re-rank launch on a caller-built candidate array cand [nq][kp] (approximate keys, row slot in the low 32
// bits, KEY_INVALID padding) -> okeys / oids [nq][kp]. which = 0: the thread-per-candidate kernel, 1: the panel kernel (an error on a
// shape it does not take, never the other kernel). nb [nq] floats is workspace. The caller keeps writers away from the index.
extern "C" int ak_kts_rr_rerank(void *index, const float *queries, int nq, int kp, const uint64_t *cand, uint64_t *okeys, int64_t *oids,
                                float *nb, int which, void *stream) {
    AK_BIND();
    if (!index || !queries || !cand || !okeys || !oids || !nb) AK_FAIL(-1, "ak_kts_rr_rerank: NULL argument");
    if (nq <= 0 || kp <= 0 || (which != 0 && which != 1)) AK_FAIL(-1, "ak_kts_rr_rerank: nq, kp > 0, which 0 or 1");
    Index &ix = *(Index *)index;
    std::shared_lock<std::shared_mutex> lk(ix.mu);
    if (int rc = query_norms(queries, nq, ix.dim, nb, (hipStream_t)stream)) return rc;
    return rerank_with(ix, queries, nb, nq, kp, cand, okeys, oids, which == 1, (hipStream_t)stream);
}
// the kernel rerank() launches for this index under the current switches (AK_RERANK_OLD): 0 thread-per-candidate, 1 panel
extern "C" int ak_kts_rr_choice(void *index) {
    if (!index) AK_FAIL(-1, "ak_kts_rr_choice: NULL argument");
    return rerank_takes_panel(*(Index *)index) ? 1 : 0;
}

// ---- the float32 and split-bf16 parity modes (tests/test_parity_kernels_gpu.py). Named ak_ktp_*: a set of their own, like ak_ktg_* and
// ak_kts_*. Each wrapper hands its arguments to the launcher forward_f32 calls; it refuses only what forward_f32 and the handle's
// create guarantee (positive sizes, S <= 512, rows of whole float4, a residual where the epilogue reads one), so that a mistaken test shape
// cannot leave a buffer. Shapes the launchers themselves refuse (N % 128, K % 32, head size 48, ...) reach them and come back as their code ----
static bool ktp_gemm(int epi, const void *X, const void *W, const void *bias, const void *R, int T, int N, int K, const void *Y, int ldc, int col0) {
    return X && W && bias && Y && epi >= 0 && epi <= 2 && (epi != 2 || R) && T > 0 && N > 0 && K > 0 && col0 >= 0 && col0 % 4 == 0 && ldc % 4 == 0 &&
           (int64_t)col0 + N <= ldc;
}
extern "C" int ak_ktp_gemm_f32(int epi, const float *X, const float *W, const float *bias, const float *R, int T, int N, int K, float *Y, int ldc,
                               int col0, void *stream) {
    AK_BIND();
    if (!ktp_gemm(epi, X, W, bias, R, T, N, K, Y, ldc, col0)) AK_FAIL(-1, "ak_ktp_gemm_f32: bad arguments");
    return launch_gemm_f32(epi, X, W, bias, R, T, N, K, Y, ldc, col0, (hipStream_t)stream);
}
extern "C" int ak_ktp_gemm_x3(int epi, const float *X, const uint16_t *Whi, const uint16_t *Wlo, const float *bias, const float *R, int T, int N,
                              int K, float *Y, int ldc, int col0, void *stream) {
    AK_BIND();
    if (!ktp_gemm(epi, X, Whi, bias, R, T, N, K, Y, ldc, col0) || !Wlo) AK_FAIL(-1, "ak_ktp_gemm_x3: bad arguments");
    return launch_gemm_x3(epi, X, Whi, Wlo, bias, R, T, N, K, Y, ldc, col0, (hipStream_t)stream);
}
// the scalar kernel the comment of k32m_gemm names as its cross-check: k32_gemm<gelu != 0>, Y [T][N]
extern "C" int ak_ktp_gemm_f32_scalar(int gelu, const float *X, const float *W, const float *bias, int T, int N, int K, float *Y, void *stream) {
    AK_BIND();
    if (!X || !W || !bias || !Y || T <= 0 || N <= 0 || K <= 0 || N % 64 || K % 16) AK_FAIL(-1, "ak_ktp_gemm_f32_scalar: N % 64 == 0, K % 16 == 0");
    return launch_gemm_f32_scalar(gelu, X, W, bias, T, N, K, Y, (hipStream_t)stream);
}

static bool ktp_attn(const void *qkv, const void *mask, const void *out, int B, int S, int H, int heads, int ldq) {
    return qkv && mask && out && B > 0 && S > 0 && S <= 512 && heads > 0 && H > 0 && H % heads == 0 && (H / heads) % 4 == 0 && ldq >= 3 * H && ldq % 4 == 0 &&
           (int64_t)B * S <= 0x7fffffff;
}
// qkv [B * S][3 H] float32 (q | k | v), mask [B][S], ctx [B * S][H]; rel: [heads][REL_ROW] floats (natural domain) or NULL
extern "C" int ak_ktp_attn_f32(const float *qkv, const int *mask, int B, int S, int H, int heads, float *ctx, const float *rel, void *stream) {
    AK_BIND();
    if (!ktp_attn(qkv, mask, ctx, B, S, H, heads, 3 * H)) AK_FAIL(-1, "ak_ktp_attn_f32: bad arguments");
    return launch_attn_f32(qkv, mask, B, S, H, heads, ctx, (hipStream_t)stream, rel);
}
// rel: the table times log2(e) (the base-2 kernel)
extern "C" int ak_ktp_attn_x3(const float *qkv, const int *mask, int B, int S, int H, int heads, float *ctx, const float *rel, void *stream) {
    AK_BIND();
    if (!ktp_attn(qkv, mask, ctx, B, S, H, heads, 3 * H)) AK_FAIL(-1, "ak_ktp_attn_x3: bad arguments");
    return launch_attn_x3(qkv, mask, B, S, H, heads, ctx, (hipStream_t)stream, rel);
}
// qkv rows of ldq >= 3 H floats, ctx2 [B * S][2 H] bf16 = [hi | lo]
extern "C" int ak_ktp_attn_x3_split(const float *qkv, int ldq, const int *mask, int B, int S, int H, int heads, uint16_t *ctx2, const float *rel,
                                    void *stream) {
    AK_BIND();
    if (!ktp_attn(qkv, mask, ctx2, B, S, H, heads, ldq)) AK_FAIL(-1, "ak_ktp_attn_x3_split: bad arguments");
    return launch_attn_x3_split(qkv, ldq, mask, B, S, H, heads, ctx2, (hipStream_t)stream, rel);
}

extern "C" int ak_ktp_split_hilo(const float *w, long long n, uint16_t *hi, uint16_t *lo, void *stream) {
    AK_BIND();
    if (!w || !hi || !lo || n <= 0) AK_FAIL(-1, "ak_ktp_split_hilo: bad arguments");
    return split_hilo(w, n, hi, lo, (hipStream_t)stream);
}
extern "C" int ak_ktp_split_rows(const float *x, long long rows, int K, uint16_t *out, void *stream) {
    AK_BIND();
    if (!x || !out || rows <= 0 || K <= 0) AK_FAIL(-1, "ak_ktp_split_rows: bad arguments");
    return split_rows(x, rows, K, out, (hipStream_t)stream);
}

static bool ktp_rows(long long T, int H) { return T > 0 && T <= 0x7fffffff && H > 0; }
// word [vocab][H], pos [>= S rows, or every row posid names][H], type [H]; out [T][H] float32, out2 [T][2 H] bf16
extern "C" int ak_ktp_embed_split(const int *ids, long long T, int S, int H, int vocab, const float *word, const float *pos, const float *type,
                                  const float *g, const float *b, float eps, float *out, uint16_t *out2, const int *posid, void *stream) {
    AK_BIND();
    if (!ids || !word || !pos || !type || !g || !b || !out || !out2 || !ktp_rows(T, H) || S <= 0 || vocab <= 0) AK_FAIL(-1, "ak_ktp_embed_split: bad arguments");
    return launch_embed_split(ids, T, S, H, vocab, word, pos, type, g, b, eps, out, out2, (hipStream_t)stream, posid);
}
extern "C" int ak_ktp_add_ln_split(const float *y, int ldy, const float *r, long long T, int H, const float *g, const float *b, float eps, float *out,
                                   uint16_t *out2, void *stream) {
    AK_BIND();
    if (!y || !g || !b || !out || !out2 || !ktp_rows(T, H) || ldy < H || ldy % 4) AK_FAIL(-1, "ak_ktp_add_ln_split: bad arguments");
    return launch_add_ln_split(y, ldy, r, T, H, g, b, eps, out, out2, (hipStream_t)stream);
}
// the launches forward_f32 makes itself (encoder.hip launch_embed_f32 / launch_add_ln_f32 / launch_pool_f32)
extern "C" int ak_ktp_embed_f32(const int *ids, long long T, int S, int H, int vocab, const float *word, const float *pos, const float *type,
                                const float *g, const float *b, float eps, float *x, const int *posid, void *stream) {
    AK_BIND();
    if (!ids || !word || !pos || !type || !g || !b || !x || !ktp_rows(T, H) || H > 1024 || S <= 0 || vocab <= 0) AK_FAIL(-1, "ak_ktp_embed_f32: bad arguments");
    return launch_embed_f32(ids, T, S, H, vocab, word, pos, type, g, b, eps, x, posid, (hipStream_t)stream);
}
extern "C" int ak_ktp_add_ln_f32(const float *x, const float *r, long long T, int H, const float *g, const float *b, float eps, float *y, void *stream) {
    AK_BIND();
    if (!x || !g || !b || !y || !ktp_rows(T, H) || H > 1024) AK_FAIL(-1, "ak_ktp_add_ln_f32: bad arguments");
    return launch_add_ln_f32(x, r, T, H, g, b, eps, y, (hipStream_t)stream);
}
extern "C" int ak_ktp_pool_f32(const float *x, const int *mask, int B, int S, int H, int pooling, int normalise, float *out, void *stream) {
    AK_BIND();
    if (!x || !mask || !out || B <= 0 || B > 65535 || S <= 0 || S > 512 || H <= 0 || H % 8 || H > 1024 || (pooling != AK_POOL_MEAN && pooling != AK_POOL_CLS))
        AK_FAIL(-1, "ak_ktp_pool_f32: bad arguments");
    return launch_pool_f32(x, mask, B, S, H, pooling, normalise, out, (hipStream_t)stream);
}

// launch_gemm_x3w: X [T][2 K1], W [N][2 K1] bf16 rows [hi | lo], bias [N]; mode 5 -> out_f32 [T][N] (columns >= nvalid unwritten),
// mode 6 -> out_bf16 [T][2 N] = [hi | lo] of gelu(.)
extern "C" int ak_ktp_gemm_x3w(int mode, const uint16_t *X, const uint16_t *W, const float *bias, int T, int N, int K1, float *out_f32,
                               uint16_t *out_bf16, int nvalid, void *stream) {
    AK_BIND();
    if (!X || !W || !bias || T <= 0 || N <= 0 || K1 <= 0 || K1 > 0x7fffffff / 3 || (mode == 5 && !out_f32) || (mode == 6 && !out_bf16))
        AK_FAIL(-1, "ak_ktp_gemm_x3w: bad arguments");
    GemmArgs g{};
    g.X = X; g.W = W; g.bias = bias; g.T = T; g.N = N; g.K = 3 * K1; g.out_f32 = out_f32; g.out_bf16 = out_bf16; g.ldo = 2 * N; g.nvalid = nvalid;
    return launch_gemm_x3w(mode, g, (hipStream_t)stream);
}
// launch_gemm_ln_x3 (hidden 384): X [T][2 K1], W [384][2 K1], x32 [T][384] in place, x16 [T][768] = [hi | lo]
extern "C" int ak_ktp_gemm_ln_x3(const uint16_t *X, const uint16_t *W, const float *bias, const float *gamma, const float *beta, float *x32,
                                 uint16_t *x16, int T, int K1, float eps, void *stream) {
    AK_BIND();
    if (!X || !W || !bias || !gamma || !beta || T <= 0 || K1 <= 0 || K1 > 0x7fffffff / 3 || !gemm_ln_supported(384, T, K1))
        AK_FAIL(-1, "ak_ktp_gemm_ln_x3: gemm_ln_supported refuses this shape");
    GemmLnArgs a{X, W, bias, gamma, beta, x32, x16, T, 3 * K1, eps, nullptr};
    return launch_gemm_ln_x3(a, (hipStream_t)stream);
}

#endif  // AK_DBG_KERNELS
