// decoder128.h -- the head-128 decoder stack (decoder128.hip) as its three ABIs reach it: one pre-norm RMSNorm / rotate_half RoPE / GQA /
// SwiGLU stack with a float32 residual stream behind ak_decoder_* (decoder.hip: Qwen3), ak_llama_* (llama.hip: Mistral / Llama) and
// ak_qwen2_* (qwen2.hip: Qwen2). An ABI file states its family as an LlFeatures and its group limit, turns its config struct into an
// AkLlamaConfig and calls what is here; it holds no check, weight preparation or launch of its own.
#pragma once
#include <string>

#include "stack.h"

namespace ak {

constexpr int LL_HD = 128, LL_MAX_S = 8192;

// What a family adds to the plain Mistral / Llama layer. Per layer it hands over 9 + 3 * qkv_bias + 2 * qk_norm pointers: wq wk wv
// [bq bk bv: qkv_bias] [q_norm k_norm: qk_norm] wo ln_in ln_post w_gate w_up w_down.
struct LlFeatures {
    bool qkv_bias = false;                     // Qwen2: a float32 bias on the q | k | v projection
    bool qk_norm = false;                      // Qwen3: RMSNorm over each q and k head before the rotation
    bool split_attn = false;                   // launch_attn_causal_split (5 to 8 query heads per kv head) in place of launch_attn_causal
    bool unfused_swiglu = false;               // Qwen3's A/B baseline (AK_DEC_SWIGLU=unfused): a 2I-wide GEMM + k_dec_swiglu, not k_gemm MODE 7
    bool mean_pool = false;                    // the ABI's forward takes AK_POOL_MEAN: the handle carries launch_ll_pool's workspace
    int per_layer() const { return 9 + 3 * qkv_bias + 2 * qk_norm; }
};

struct LlLayer {
    const uint16_t *wqkv, *wo, *wgu, *wd;      // wqkv [(nq + 2 nkv) 128][H] and wgu [2 I][H] (interleaved) are owned
    const float *ln_in, *ln_post;
    const float *bqkv;                         // [(nq + 2 nkv) 128] float32 in wqkv's row order (owned), or NULL: zero_bias
    const float *qn, *kn;                      // [128] each, or NULL (no qk_norm)
};
struct Llama : Stack {
    AkLlamaConfig cfg;
    LlFeatures feat;
    const uint16_t *emb = nullptr; const float *norm = nullptr;
    std::vector<LlLayer> layers;
    float *rope_c = nullptr, *rope_s = nullptr;
    float *x32 = nullptr, *y32 = nullptr, *part = nullptr;
    uint16_t *h16 = nullptr, *qkv = nullptr, *q = nullptr, *k = nullptr, *v = nullptr, *ctx = nullptr, *f = nullptr;
    int *lens = nullptr;
};

// `fn`: the entry point's name as the messages carry it.
// Every refusal of a create: sizes, head_dim, the head ratio (max_group: 4, or 8 where the family runs the split attention), the GEMM
// tile multiples, eps / theta, the window and bidirectional ranges, the weight count for `feat`, NULL weight pointers. 0: cfg is fine.
int ll_check_config(const char *fn, const AkLlamaConfig &c, const LlFeatures &feat, int max_group, const void *const *w, int n_weights);
// The handle of a checked config: the concatenated / interleaved matrices, the rotary table, the workspace.
// w: embed_tokens, norm, then feat.per_layer() pointers per layer in LlFeatures' order.
int ll_create(const char *fn, const AkLlamaConfig &c, const void *const *w, const LlFeatures &feat, void **out);
int ll_set_rope_inv_freq(const char *fn, void *h, const float *inv_freq);
int ll_forward_lens(const char *fn, void *h, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S, int pooling,
                    int normalise, float *out, void *stream);

}  // namespace ak
