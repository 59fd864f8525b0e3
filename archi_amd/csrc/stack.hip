// stack.hip -- the host side of stack.h: rotary tables, owned device memory and weight preparation, the workspace, the argument
// checks of the ak_*_forward_lens entry points, and of enc64.h: the create steps and the two forward blocks of the head-64 encoders.
// No kernels.
#include <algorithm>
#include <cmath>
#include <string>

#include "enc64.h"

namespace ak {

// ---- RoPE table (host): HF's default rotary embedding in float32 --------------------------------------------------------
// inv_freq[i] = 1 / theta^(2 i / hd) (the exponent 2 i / hd is exact in float32; the power is rounded once from double),
// angle = float(pos) * inv_freq[i] (one float32 product, as HF's float32 matmul of a 1-deep product), cos / sin rounded once from
// double. Table rows [n_pos][hd / 2]: HF's cos / sin are these rows twice (cat(freqs, freqs)).
// the second half of the routine on given inverse frequencies (ak_decoder_rope_table_inv: a caller that holds HF's own buffer)
void rope_table_from_inv(const float *inv, int half, int n_pos, float *c, float *s) {
    for (int p = 0; p < n_pos; p++)
        for (int i = 0; i < half; i++) {
            const float ang = (float)p * inv[i];
            c[(size_t)p * half + i] = (float)std::cos((double)ang);
            s[(size_t)p * half + i] = (float)std::sin((double)ang);
        }
}
void rope_table_host(float theta, int hd, int n_pos, float *c, float *s) {
    const int half = hd / 2;
    std::vector<float> inv(half);
    for (int i = 0; i < half; i++) {
        const float e = (float)(2 * i) / (float)hd;
        inv[i] = 1.0f / (float)std::pow((double)theta, (double)e);
    }
    rope_table_from_inv(inv.data(), half, n_pos, c, s);
}

static bool upload(float *dst, const std::vector<float> &src) {
    return hipMemcpy(dst, src.data(), src.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
}

bool Stack::rope_tables(float theta, int hd, float **c, float **s) {
    std::vector<float> hc((size_t)n_pos * (hd / 2)), hs(hc.size());
    rope_table_host(theta, hd, n_pos, hc.data(), hs.data());
    *c = dev_as<float>(hc.size());
    *s = dev_as<float>(hs.size());
    return *c && *s && upload(*c, hc) && upload(*s, hs);
}

int Stack::rope_tables_set_inv(const float *inv, int half, float *c, float *s) {
    std::vector<float> hc((size_t)n_pos * half), hs(hc.size());
    rope_table_from_inv(inv, half, n_pos, hc.data(), hs.data());
    AK_HIP(hipMemcpy(c, hc.data(), hc.size() * 4, hipMemcpyHostToDevice));
    AK_HIP(hipMemcpy(s, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
    return 0;
}

// ---- owned memory and weight preparation ----------------------------------------------------------------------------------
Stack::~Stack() {
    for (void *p : owned) hipFree(p);
}

void *Stack::dev(size_t bytes, bool zero) {
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    owned.push_back(p);
    if (zero && hipMemset(p, 0, bytes) != hipSuccess) return nullptr;
    return p;
}

bool Stack::concat_rows(uint16_t *dst, int H, std::initializer_list<Rows> blocks) {
    for (const Rows &b : blocks) {
        if (hipMemcpy(dst, b.p, b.rows * H * 2, hipMemcpyDeviceToDevice) != hipSuccess) return false;
        dst += b.rows * H;
    }
    return true;
}

bool Stack::interleave_rows(uint16_t *dst, const void *a, const void *b, int I, int H) {
    return hipMemcpy2D(dst, (size_t)4 * H, a, (size_t)2 * H, (size_t)2 * H, I, hipMemcpyDeviceToDevice) == hipSuccess &&
           hipMemcpy2D(dst + H, (size_t)4 * H, b, (size_t)2 * H, (size_t)2 * H, I, hipMemcpyDeviceToDevice) == hipSuccess;
}

const uint16_t *Stack::pad_cols(const void *w, int H, int I, int Ip) {
    uint16_t *p = dev_as<uint16_t>((size_t)H * Ip, true);
    if (!p || hipMemcpy2D(p, (size_t)2 * Ip, w, (size_t)2 * I, (size_t)2 * I, H, hipMemcpyDeviceToDevice) != hipSuccess) return nullptr;
    return p;
}

// ---- workspace -------------------------------------------------------------------------------------------------------------
void Stack::release() {
    for (Buf &b : bufs) {
        if (*b.p) hipFree(*b.p);
        *b.p = nullptr;
    }
    cap = 0; cap_B = 0;
}

int Stack::reserve(int64_t tpad, int B) {
    if (tpad <= cap && B <= cap_B) return 0;
    if (tpad < cap) tpad = cap;
    if (B < cap_B) B = cap_B;
    release();
    for (Buf &b : bufs) {
        const size_t bytes = (size_t)tpad * b.per_token + (size_t)B * b.per_row;
        AK_HIP(hipMalloc(b.p, bytes));
        AK_HIP(hipMemset(*b.p, 0, bytes));
    }
    cap = tpad; cap_B = B;
    return 0;
}

// ---- entry-point checks ------------------------------------------------------------------------------------------------------
int check_forward_lens(const char *fn, const void *ids, const void *lens, const void *out, int ld_ids, int lens_stride, int B, int S, int max_S,
                       int n_pos, const char *pooling_error, int max_B) {
    const std::string f = std::string(fn) + ": ";
    if (!ids || !lens || !out || ld_ids < S || lens_stride < 1) AK_FAIL(-1, f + "bad arguments");
    if (pooling_error) AK_FAIL(-1, f + pooling_error);
    if (S <= 0 || S % 32 || S > max_S) AK_FAIL(-1, f + "S must be a positive multiple of 32, <= " + std::to_string(max_S));
    if (S > n_pos) AK_FAIL(-1, f + "S exceeds max_position");
    if (max_B && B > max_B) AK_FAIL(-1, f + "at most " + std::to_string(max_B) + " rows per call");
    return 0;
}

// ---- the head-64 encoder base (enc64.h) --------------------------------------------------------------------------------------
int Enc64::check_sizes(const char *fn, int H, int I, int heads, int L, int vocab, int max_position, bool others_positive) {
    const std::string f = std::string(fn) + ": ";
    if (L <= 0 || vocab <= 0 || heads <= 0 || H <= 0 || I <= 0 || max_position <= 0 || !others_positive) AK_FAIL(-1, f + "sizes must be positive");
    if (L > AK_MBERT_MAX_LAYERS) AK_FAIL(-1, f + "more than AK_MBERT_MAX_LAYERS layers");
    if (H != heads * HD) AK_FAIL(-1, f + "head size (hidden / heads) must be 64");
    if (H % 128 || H > MAX_H || I % 64) AK_FAIL(-1, f + "hidden must be a multiple of 128 (<= 1024), intermediate a multiple of 64");
    return 0;
}

const char *Enc64::init(int hidden, int n_heads, int I, int max_position) {
    H = hidden; heads = n_heads;
    Ip = padded_intermediate(I);               // ModernBERT large: 2624 -> 2688
    zero_bias = dev_as<float>(std::max<size_t>((size_t)3 * H, (size_t)2 * Ip), true);
    if (!zero_bias) return "hipMalloc failed";
    n_pos = max_position < MAX_S ? max_position : MAX_S;
    const size_t row16 = (size_t)H * 2;
    buffer(&x32, (size_t)H * 4); buffer(&y32, (size_t)H * 4); buffer(&h16, row16);
    buffer(&q, row16); buffer(&k, row16); buffer(&vt, row16); buffer(&ctx, row16);
    buffer(&f, (size_t)Ip * 2); buffer(&mask, 4); buffer(&lens, 0, 4);
    buffer(&part, (size_t)H * 4 / POOL_CHUNK, (size_t)H * 4);      // B ceil(S / 64) <= T / 64 + B rows of H floats
    return nullptr;
}

const char *Enc64::prepare_gated(const void *a, const void *b, int I, const void *down, const uint16_t **wgu, const uint16_t **wdown) {
    uint16_t *w = dev_as<uint16_t>((size_t)2 * Ip * H, Ip != I);
    if (!w) return "hipMalloc failed";
    if (!interleave_rows(w, a, b, I, H)) return "gate / up interleave failed";
    *wgu = w;
    *wdown = (const uint16_t *)down;
    if (Ip != I && !(*wdown = pad_cols(down, H, I, Ip))) return "down projection padding failed";
    return nullptr;
}

const char *Enc64::prepare_plain(const void *wi, int I, const void *wo, const uint16_t **wi_out, const uint16_t **wo_out) {
    *wi_out = (const uint16_t *)wi;
    *wo_out = (const uint16_t *)wo;
    if (Ip == I) return nullptr;
    uint16_t *w = dev_as<uint16_t>((size_t)Ip * H, true);
    if (!w) return "hipMalloc failed";
    if (!concat_rows(w, H, {{wi, (size_t)I}})) return "input projection padding failed";
    *wi_out = w;
    if (!(*wo_out = pad_cols(wo, H, I, Ip))) return "output projection padding failed";
    return nullptr;
}

int Enc64::qkv_gemm(int64_t tpad, int64_t T, int S, const uint16_t *wqkv, float qscale, hipStream_t st) {
    GemmArgs g = gemm(tpad, h16, wqkv, 3 * H, H);
    g.q = q; g.k = k; g.vt = vt; g.H = H; g.S = S; g.qscale = qscale;
    g.ldo = (int)T;                                            // MODE 0: number of real tokens (rows beyond it have no V^T slot)
    return launch_gemm(0, g, st);
}

int Enc64::attention_block(int64_t tpad, int B, int S, const uint16_t *wqkv, const uint16_t *wo, const float *rc, const float *rs, int half_window,
                           hipStream_t st) {
    const int64_t T = (int64_t)B * S;
    if (qkv_gemm(tpad, T, S, wqkv, 1.4426950408889634f / sqrtf((float)HD), st)) return -10;
    if (launch_mb_rope(q, k, T, S, H, rc, rs, st)) return -10;
    AttnArgs a{q, k, vt, mask, ctx, B, S, H, heads, nullptr, nullptr, 0, 0, nullptr, lens};
    if (launch_attn_window(a, half_window, st)) return -10;
    return launch_gemm(2, gemm_f32(tpad, ctx, wo, H, H, y32), st) ? -10 : 0;
}

int Enc64::attention_block_relbias(int64_t tpad, int B, int S, const uint16_t *wqkv, const uint16_t *wo, float qscale, const float *rbias, int D,
                                   hipStream_t st) {
    if (qkv_gemm(tpad, (int64_t)B * S, S, wqkv, qscale, st)) return -10;
    AttnArgs a{q, k, vt, mask, ctx, B, S, H, heads, nullptr, nullptr, 0, 0, nullptr, lens};
    a.rbias = rbias; a.rbias_D = D;
    if (launch_attn_relbias(a, st)) return -10;
    return launch_gemm(2, gemm_f32(tpad, ctx, wo, H, H, y32), st) ? -10 : 0;
}

int Enc64::ffn_block_plain(int mode, int64_t tpad, const uint16_t *wi, const uint16_t *wo, hipStream_t st) {
    if (launch_gemm(mode, gemm_bf16(tpad, h16, wi, Ip, H, f), st)) return -10;
    return launch_gemm(2, gemm_f32(tpad, f, wo, H, Ip, y32), st) ? -10 : 0;
}

int Enc64::ffn_block(int mode, int64_t tpad, const uint16_t *wgu, const uint16_t *wdown, hipStream_t st) {
    if (launch_gemm(mode, gemm_gated(tpad, h16, wgu, Ip, H, f), st)) return -10;
    return launch_gemm(2, gemm_f32(tpad, f, wdown, H, Ip, y32), st) ? -10 : 0;
}

}  // namespace ak
