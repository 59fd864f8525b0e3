// qwen2.hip -- the Qwen2 / Qwen2.5 decoder embedders (Alibaba-NLP/gte-Qwen2-1.5B-instruct and -7B-instruct, gte-Qwen1.5-7B-instruct,
// infly/inf-retriever-v1) behind ak_qwen2_*. HF Qwen2Model is the Mistral / Llama layer of the head-128 decoder stack (decoder128.hip)
// with two differences, and this file states only those:
//   q | k | v = h [Wq; Wk; Wv]^T + [bq; bk; bv]   qkv_bias: the three biases concatenated at create, k_gemm MODE 3's bias
//   5 to 8 query heads per kv head                split_attn: launch_attn_causal_split (attn_causal.hip), a kv group over two workgroups;
//                                                 up to 4 heads per kv head run launch_attn_causal as Llama does
// No sliding window (a config that slides some layers is refused by archi_amd.qwen2). Last-token or mean pooling.
#include "decoder128.h"

using namespace ak;

extern "C" int ak_qwen2_destroy(ak_qwen2_t h) { return stack_destroy<Llama>(h); }

extern "C" int ak_qwen2_create(const AkQwen2Config *cfg, const void *const *w, int n_weights, ak_qwen2_t *out) {
    AK_BIND();
    if (!cfg || !w || !out) AK_FAIL(-1, "ak_qwen2_create: NULL argument");
    *out = nullptr;
    const AkQwen2Config c = *cfg;
    const AkLlamaConfig lc{c.vocab_size, c.hidden, c.layers, c.q_heads, c.kv_heads, c.head_dim, c.intermediate, c.max_position, c.rms_eps,
                           c.rope_theta, 0, c.bidirectional};
    LlFeatures feat;
    feat.qkv_bias = feat.mean_pool = true;
    if (ll_check_config("ak_qwen2_create", lc, feat, 8, w, n_weights)) return -1;
    feat.split_attn = attn_causal_split_supported(c.q_heads, c.kv_heads, c.head_dim, 32);
    return ll_create("ak_qwen2_create", lc, w, feat, out);
}

extern "C" int ak_qwen2_set_rope_inv_freq(ak_qwen2_t h, const float *inv_freq) {
    AK_BIND();
    return ll_set_rope_inv_freq("ak_qwen2_set_rope_inv_freq", h, inv_freq);
}

extern "C" int ak_qwen2_forward_lens(ak_qwen2_t h, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S, int pooling,
                                     int normalise, float *out, void *stream) {
    AK_BIND();
    return ll_forward_lens("ak_qwen2_forward_lens", h, ids, ld_ids, lens, lens_stride, B, S, pooling, normalise, out, stream);
}
