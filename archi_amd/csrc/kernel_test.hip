// kernel_test.hip -- single-launch entry points for the kernel-level tests (tests/test_kernels_gpu.py). They exist in
// libarchi_hip_dbg.so only (-DAK_DBG_KERNELS=1); the product library gets an empty object from this file and exports no ak_kt_*.
// Every wrapper fills the launcher's argument block from device pointers and calls the launcher the forward pass calls: no
// arithmetic, no kernel selection of its own. With no AK_* switch set the instantiation that runs is the one the product launches;
// a shape the launcher refuses comes back as its error code (ak_last_error has the text).
#include "encoder_kernels.h"

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

// host only: where key s sits inside its V^T row
extern "C" int ak_kt_vt_pos(int s) { return vt_pos(s); }

#endif  // AK_DBG_KERNELS
