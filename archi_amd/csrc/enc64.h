// enc64.h -- the head-64 encoder that mbert.hip (ModernBERT) and nomic.hip (NomicBERT) are built on: hidden = heads x 64, a float32
// residual stream x32, bf16 GEMM rows, and per layer
//   attention_block: k_gemm MODE 0 (q scaled | k | V^T) -> k_mb_rope -> k_attn_long<WIN> -> k_gemm MODE 2 into y32
//   ffn_block:       the gated k_gemm (MODE 7 SwiGLU / 8 GeGLU) -> k_gemm MODE 2 into y32
// T5 (t5.hip) takes the two other forms: attention_block_relbias (no RoPE launch, the caller's q scale, k_attn_long_relbias with
// the clamped relative bias) and ffn_block_plain (an un-gated activation mode, no interleaving),
// with the family's own join kernel (what becomes of x32 + y32) behind each block. Here: the workspace, the create steps both
// families make and the body of ak_*_forward_lens. A family keeps its config struct and that struct's own checks, its layers' norm
// pointers, the rotary table / window of a layer, its embed, join and pooling kernels. stack.hip holds the bodies.
#pragma once
#include "stack.h"

namespace ak {

struct Enc64 : Stack {
    static constexpr int HD = 64, MAX_S = ATTN_LONG_MAX_S, MAX_H = POOL_MAX_H;
    int H = 0, heads = 0;
    int Ip = 0;                                // intermediate size as the GEMMs see it (padded_intermediate)
    float *x32 = nullptr, *y32 = nullptr;
    uint16_t *h16 = nullptr, *q = nullptr, *k = nullptr, *vt = nullptr, *ctx = nullptr, *f = nullptr;
    float *part = nullptr;                     // pooling: chunk sums [B][ceil(S / 64)][H]
    int *mask = nullptr, *lens = nullptr;

    // -- create, under the entry point's name `fn`
    // the size rules of a config: others_positive = the family's further sizes are all positive
    static int check_sizes(const char *fn, int H, int I, int heads, int L, int vocab, int max_position, bool others_positive);
    // zero_bias, Ip, n_pos = min(max_position, 8192), the workspace buffers. NULL, or what failed.
    const char *init(int hidden, int n_heads, int I, int max_position);
    bool rope_table(float theta, float **c, float **s) { return rope_tables(theta, HD, c, s); }
    // *wgu [2 Ip][H]: row 2 j = a row j, row 2 j + 1 = b row j, zero rows past 2 I; *wdown = down [H][I], padded with zero columns
    // when Ip != I. NULL, or what failed.
    const char *prepare_gated(const void *a, const void *b, int I, const void *down, const uint16_t **wgu, const uint16_t **wdown);

    // -- forward: both read h16 and leave the sub-layer's float32 output in y32
    // rc / rs: the layer's rotary table; half_window < 0: every key
    int attention_block(int64_t tpad, int B, int S, const uint16_t *wqkv, const uint16_t *wo, const float *rc, const float *rs, int half_window,
                        hipStream_t st);
    int ffn_block(int mode, int64_t tpad, const uint16_t *wgu, const uint16_t *wdown, hipStream_t st);
    // no RoPE; q scaled by qscale (the softmax runs in base 2: log2(e) times the model's scale); rbias [heads][2 D + 1]: the bias of
    // clamp(key - query, -D, D), in the base-2 domain (AttnArgs::rbias)
    int attention_block_relbias(int64_t tpad, int B, int S, const uint16_t *wqkv, const uint16_t *wo, float qscale, const float *rbias, int D,
                                hipStream_t st);
    // the un-gated pair f = act(h wi^T) (mode 10: ReLU), y32 = f wo^T on what prepare_plain left: *wi_out [Ip][H] with zero rows past I,
    // *wo_out [H][Ip] with zero columns past I (the given matrices themselves when Ip == I). NULL, or what failed.
    const char *prepare_plain(const void *wi, int I, const void *wo, const uint16_t **wi_out, const uint16_t **wo_out);
    int ffn_block_plain(int mode, int64_t tpad, const uint16_t *wi, const uint16_t *wo, hipStream_t st);

private:
    int qkv_gemm(int64_t tpad, int64_t T, int S, const uint16_t *wqkv, float qscale, hipStream_t st);      // MODE 0: q (scaled) | k | V^T
};

// what a create says and does when a step after `new T` failed
template <class T>
inline int enc64_create_failed(T *d, const char *fn, const char *what) {
    set_error(std::string(fn) + ": " + what);
    stack_destroy<T>(d);
    return -10;
}

// ak_*_forward_lens of a handle type T derived from Enc64, under its name `fn`; T::forward runs under the handle's lock
template <class T>
inline int enc64_forward_lens(const char *fn, void *h, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S, int pooling,
                              int normalise, float *out, void *stream) {
    AK_BIND();
    if (!h) AK_FAIL(-1, std::string(fn) + ": NULL handle");
    RoctxRange range(fn);
    T &d = *(T *)h;
    if (B <= 0) return 0;
    const bool pool_ok = pooling == AK_POOL_MEAN || pooling == AK_POOL_CLS;
    if (check_forward_lens(fn, ids, lens, out, ld_ids, lens_stride, B, S, Enc64::MAX_S, d.n_pos,
                           pool_ok ? nullptr : "pooling must be AK_POOL_MEAN or AK_POOL_CLS", 65535))
        return -1;
    std::lock_guard<std::mutex> lk(d.mu);
    return d.forward(ids, ld_ids, lens, lens_stride, B, S, pooling, normalise, out, (hipStream_t)stream);
}

}  // namespace ak
