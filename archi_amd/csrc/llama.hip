// llama.hip -- the Mistral / Llama decoder embedders (intfloat/e5-mistral-7b-instruct, Salesforce/SFR-Embedding-Mistral,
// Linq-AI-Research/Linq-Embed-Mistral, the Llama-3.1-8B based embedders) behind ak_llama_*. HF MistralModel / LlamaModel is the plain
// layer of the head-128 decoder stack (decoder128.hip): no bias, no per-head norm, at most 4 query heads per kv head; Mistral's sliding
// window and the bidirectional mode are the config's. Last-token or mean pooling.
#include "decoder128.h"

using namespace ak;

extern "C" int ak_llama_destroy(ak_llama_t h) { return stack_destroy<Llama>(h); }

extern "C" int ak_llama_create(const AkLlamaConfig *cfg, const void *const *w, int n_weights, ak_llama_t *out) {
    AK_BIND();
    if (!cfg || !w || !out) AK_FAIL(-1, "ak_llama_create: NULL argument");
    *out = nullptr;
    LlFeatures feat;
    feat.mean_pool = true;
    if (ll_check_config("ak_llama_create", *cfg, feat, 4, w, n_weights)) return -1;
    return ll_create("ak_llama_create", *cfg, w, feat, out);
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
