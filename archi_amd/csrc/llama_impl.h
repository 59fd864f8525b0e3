// llama_impl.h -- the handle and the layer loop of llama.hip as qwen2.hip reaches them: one pre-norm RMSNorm / rotate_half RoPE / GQA /
// SwiGLU stack at head size 128 behind two ABIs. ak_llama_* (llama.hip) builds it without biases on launch_attn_causal; ak_qwen2_*
// (qwen2.hip) with a q | k | v bias per layer and, at 5 to 8 query heads per kv head, on launch_attn_causal_split. Each ABI keeps the
// config checks of its own create; what is here takes a checked config.
#pragma once
#include <string>

#include "stack.h"

namespace ak {

constexpr int LL_HD = 128, LL_MAX_S = 8192;

struct LlLayer {
    const uint16_t *wqkv, *wo, *wgu, *wd;      // wqkv [(nq + 2 nkv) 128][H] and wgu [2 I][H] (interleaved) are owned
    const float *ln_in, *ln_post;
    const float *bqkv;                         // [(nq + 2 nkv) 128] float32 in wqkv's row order (owned), or NULL: zero_bias
};
struct Llama : Stack {
    AkLlamaConfig cfg;
    bool split_attn = false;                   // launch_attn_causal_split (5 to 8 query heads per kv head) in place of launch_attn_causal
    const uint16_t *emb = nullptr; const float *norm = nullptr;
    std::vector<LlLayer> layers;
    float *rope_c = nullptr, *rope_s = nullptr;
    float *x32 = nullptr, *y32 = nullptr, *part = nullptr;
    uint16_t *h16 = nullptr, *qkv = nullptr, *q = nullptr, *k = nullptr, *v = nullptr, *ctx = nullptr, *f = nullptr;
    int *lens = nullptr;
};

// `fn`: the entry point's name as the messages carry it. w: embed_tokens, norm, then per layer wq wk wv [bq bk bv: qkv_bias] wo ln_in
// ln_post w_gate w_up w_down, every pointer non-NULL.
int ll_create(const char *fn, const AkLlamaConfig &c, const void *const *w, bool qkv_bias, bool split_attn, void **out);
int ll_set_rope_inv_freq(const char *fn, void *h, const float *inv_freq);
int ll_forward_lens(const char *fn, void *h, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S, int pooling,
                    int normalise, float *out, void *stream);

}  // namespace ak
