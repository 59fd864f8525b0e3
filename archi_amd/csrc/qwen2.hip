// qwen2.hip -- the Qwen2 / Qwen2.5 decoder embedders (Alibaba-NLP/gte-Qwen2-1.5B-instruct and -7B-instruct, gte-Qwen1.5-7B-instruct,
// infly/inf-retriever-v1) behind ak_qwen2_*. HF Qwen2Model is the Mistral / Llama layer of llama.hip with two differences, and this file
// states only those:
//   q | k | v = h [Wq; Wk; Wv]^T + [bq; bk; bv]   the three biases concatenated at create in the row order of the concatenated matrix and
//                                                 handed to k_gemm MODE 3 as its bias: added in float32 before the bf16 store
//   5 to 8 query heads per kv head                launch_attn_causal_split (attn_causal.hip): a kv group over two workgroups; up to 4
//                                                 heads per kv head run launch_attn_causal as Llama does
// No sliding window (a config that slides some layers is refused by archi_amd.qwen2). The handle, the layer loop, the rotary table and
// the pooling are llama.hip's (llama_impl.h).
#include "llama_impl.h"

using namespace ak;

extern "C" int ak_qwen2_destroy(ak_qwen2_t h) { return stack_destroy<Llama>(h); }

extern "C" int ak_qwen2_create(const AkQwen2Config *cfg, const void *const *w, int n_weights, ak_qwen2_t *out) {
    AK_BIND();
    if (!cfg || !w || !out) AK_FAIL(-1, "ak_qwen2_create: NULL argument");
    *out = nullptr;
    const AkQwen2Config c = *cfg;
    const int H = c.hidden, I = c.intermediate, L = c.layers, nq = c.q_heads, nkv = c.kv_heads;
    if (L <= 0 || c.vocab_size <= 0 || nq <= 0 || nkv <= 0 || H <= 0 || I <= 0 || c.max_position <= 0) AK_FAIL(-1, "ak_qwen2_create: sizes must be positive");
    if (c.head_dim != LL_HD) AK_FAIL(-1, "ak_qwen2_create: head_dim must be 128");
    if (nq % nkv) AK_FAIL(-1, "ak_qwen2_create: q_heads must be a multiple of kv_heads");
    const bool split = attn_causal_split_supported(nq, nkv, c.head_dim, 32);
    if (!split && !attn_causal_supported(nq, nkv, c.head_dim, 32)) AK_FAIL(-1, "ak_qwen2_create: q_heads / kv_heads: more than 8 query heads per kv head");
    if (H % 128 || I % 64) AK_FAIL(-1, "ak_qwen2_create: hidden must be a multiple of 128, intermediate a multiple of 64");
    if (c.bidirectional != 0 && c.bidirectional != 1) AK_FAIL(-1, "ak_qwen2_create: bidirectional must be 0 or 1");
    if (!(c.rms_eps > 0.f) || !(c.rope_theta > 0.f)) AK_FAIL(-1, "ak_qwen2_create: rms_eps and rope_theta must be positive");
    if (n_weights != 2 + 12 * L) AK_FAIL(-1, "ak_qwen2_create: expected 2 + 12 * layers weight pointers");
    for (int i = 0; i < n_weights; i++)
        if (!w[i]) AK_FAIL(-1, "ak_qwen2_create: NULL weight pointer");
    const AkLlamaConfig lc{c.vocab_size, H, L, nq, nkv, c.head_dim, I, c.max_position, c.rms_eps, c.rope_theta, 0, c.bidirectional};
    return ll_create("ak_qwen2_create", lc, w, true, split, out);
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
