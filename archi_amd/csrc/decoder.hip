// decoder.hip -- the Qwen3 decoder embedders (Qwen3-Embedding-0.6B / 4B / 8B) behind ak_decoder_*. HF Qwen3Model is the Mistral / Llama
// layer of the head-128 decoder stack (decoder128.hip) with one difference, and this file states only that:
//   q, k = RoPE(RMSNorm_head(q | k))              qk_norm: per-head RMSNorm over 128 (q_norm / k_norm) before the rotation, k_dec_qk_rope
// No bias, no window, causal attention at up to 4 query heads per kv head, last-token pooling only. AK_DEC_SWIGLU=unfused (read here,
// once per process) builds the handle on the un-fused SwiGLU, the A/B baseline of k_gemm MODE 7. Also here: the host rotary table
// routines ak_decoder_rope_table*, thin wrappers of stack.hip's.
#include "decoder128.h"
#include "switches.h"

using namespace ak;

// the rotary table routines of stack.hip, for callers that hold HF's own buffers (host only)
extern "C" int ak_decoder_rope_table(float theta, int head_dim, int n_pos, float *cos_out, float *sin_out) {
    if (!cos_out || !sin_out || head_dim <= 0 || head_dim % 2 || n_pos < 0 || !(theta > 0.f))
        AK_FAIL(-1, "ak_decoder_rope_table: bad arguments");
    rope_table_host(theta, head_dim, n_pos, cos_out, sin_out);
    return 0;
}

extern "C" int ak_decoder_rope_table_inv(const float *inv_freq, int half, int n_pos, float *cos_out, float *sin_out) {
    if (!inv_freq || !cos_out || !sin_out || half <= 0 || n_pos < 0) AK_FAIL(-1, "ak_decoder_rope_table_inv: bad arguments");
    rope_table_from_inv(inv_freq, half, n_pos, cos_out, sin_out);
    return 0;
}

extern "C" int ak_decoder_destroy(ak_decoder_t h) { return stack_destroy<Llama>(h); }

extern "C" int ak_decoder_create(const AkDecoderConfig *cfg, const void *const *w, int n_weights, ak_decoder_t *out) {
    AK_BIND();
    if (!cfg || !w || !out) AK_FAIL(-1, "ak_decoder_create: NULL argument");
    *out = nullptr;
    const AkDecoderConfig c = *cfg;
    const AkLlamaConfig lc{c.vocab_size, c.hidden, c.layers, c.q_heads, c.kv_heads, c.head_dim, c.intermediate, c.max_position, c.rms_eps,
                           c.rope_theta, 0, 0};
    static const bool unfused = env_get("AK_DEC_SWIGLU") && std::string(env_get("AK_DEC_SWIGLU")) == "unfused";
    LlFeatures feat;
    feat.qk_norm = true;
    feat.unfused_swiglu = unfused;
    if (ll_check_config("ak_decoder_create", lc, feat, 4, w, n_weights)) return -1;
    return ll_create("ak_decoder_create", lc, w, feat, out);
}

extern "C" int ak_decoder_forward_lens(ak_decoder_t h, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S,
                                       int normalise, float *out, void *stream) {
    AK_BIND();
    return ll_forward_lens("ak_decoder_forward_lens", h, ids, ld_ids, lens, lens_stride, B, S, AK_POOL_LAST, normalise, out, stream);
}
