// gemma.hip -- the EmbeddingGemma forward pass (google/embeddinggemma-300m: a Gemma3 text stack run bidirectionally) behind ak_gemma_*:
// orchestration and the small kernels. As HF Gemma3TextModel with use_bidirectional_attention, then the sentence-transformers tail:
//   x = embed_tokens[id] * sqrt(H); h = RMSNorm(x; input_ln of layer 0)      k_gm_embed (float32 x, bf16 h)
// per layer (four RMSNorms -- "sandwich" norms --, no bias anywhere; every RMSNorm is x rsqrt(mean(x^2) + eps) (1 + w), 1 + w folded at create):
//   q | k | v = h [Wq; Wk; Wv]^T                       k_gemm MODE 3 (gemm.hip): one launch over the matrices concatenated at create
//   q, k = RoPE(RMSNorm_head(q; q_norm)), ...          k_gm_qk_norm_rope: per-head RMSNorm over 256, rotate_half RoPE from the table of the
//                                                      layer's type (global theta / local theta), q scaled by log2(e) scalar^-0.5;
//                                                      q / k head-major, v transposed for the attention kernel
//   a = softmax(q k^T + band + pad mask) v             k_attn_gqa (attn_gqa.hip): head size 256, G = nq / nkv query heads per kv head;
//                                                      the half-window in a sliding layer, every key in a full one
//   x += RMSNorm(a Wo^T; post_attn_ln); h = RMSNorm(x; pre_ffn_ln)           k_gemm MODE 2 (float32 out) + k_gm_norm_add_norm
//   f = gelu_tanh(h Wgate^T) (h Wup^T)                 k_gemm MODE 9 (tanh-GeGLU epilogue; gate / up rows interleaved at create, and padded
//                                                      with zero rows to 2 I % 256 == 0 for the wide tile: padded_intermediate, stack.h)
//   x += RMSNorm(f Wdown^T; post_ffn_ln); h = RMSNorm(x; next input_ln)      k_gemm MODE 2 + k_gm_norm_add_norm
// after the last layer the second norm of the join is the model's final norm, written as float32 rows; then mean pooling over the valid
// tokens in chunks of 64 (k_gm_pool_part, k_gm_pool_fin: which tokens meet in which sum depends on the row's length alone), the Dense
// head of the sentence-transformers checkpoint in float32 (0 - 2 matrices without bias, k_gm_dense) and the L2 normalisation (k_gm_l2).
// The residual stream x is float32 throughout; GEMM operands are bf16. Token counts are padded to the GEMM tile (256) as in mbert.hip.
// Here: the config checks, the layer struct, the layer loop and the family's own kernels and formulas. The plumbing shared with decoder128.hip
// and mbert.hip is stack.h / stack.hip: the token-slot prologue and the row load of k_gm_embed, the body of k_gm_pool_part, the L2 tail of
// k_gm_l2, the NJ dispatch, the workspace, the weight preparation at create (concatenation, interleave, the pad-to-256 rule), the rotary
// tables (also behind ak_gemma_set_rope_inv_freq), the GemmArgs of the launches.
// LDS per workgroup: k_gm_embed / k_gm_norm_add_norm / k_gm_dense none; k_gm_qk_norm_rope 16 KB (the V transposition); k_gm_pool_part
// 4 * H * 4 bytes (dynamic); k_gm_l2 16 bytes; the GEMMs and the attention kernel as their files state.
#include <algorithm>
#include <cmath>

#include "stack.h"

namespace ak {

namespace {
constexpr int GM_HD = 256, GM_MAX_S = ATTN_GQA_MAX_S, GM_MAX_H = POOL_MAX_H, GM_MAX_DENSE = 4096;

// w1[i] = 1 + w[i]: the RMSNorm weights as the kernels multiply by them
__global__ __launch_bounds__(256) void k_gm_fold1p(const float *__restrict__ w, int n, float *__restrict__ w1) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) w1[i] = 1.0f + w[i];
}

// one wave per token slot t < B * S: ids past the row's length read as 0; x32 = embed_tokens[id] * scale (scale = float32 sqrt(H)),
// h16 = RMSNorm(x32) * w (layer 0's input_layernorm). The wave of a row's slot 0 stores the clamped length.
template <int NJ>
__global__ __launch_bounds__(256) void k_gm_embed(const int *__restrict__ ids, int ld_ids, const int *__restrict__ lens, int lens_stride, int B, int S,
                                                  int H, int vocab, const uint16_t *__restrict__ emb, float scale, const float *__restrict__ w, float eps,
                                                  float *__restrict__ x32, uint16_t *__restrict__ h16, int *__restrict__ lens_out) {
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= (int64_t)B * S) return;
    const int id = token_slot<false>(ids, ld_ids, lens, lens_stride, S, vocab, t, lane, nullptr, lens_out);
    const uint16_t *e = emb + (int64_t)id * H;
    float4 f[NJ];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int c = lane * 4 + j * 256;
        f[j] = float4{0.f, 0.f, 0.f, 0.f};
        if (c < H) {
            const float4 v = load_bf16x4(e + c);
            f[j] = float4{v.x * scale, v.y * scale, v.z * scale, v.w * scale};
            *(float4 *)(x32 + t * H + c) = f[j];
            ss += (f[j].x * f[j].x + f[j].y * f[j].y) + (f[j].z * f[j].z + f[j].w * f[j].w);
        }
    }
    const float rs = rsqrtf(wave_sum(ss) / (float)H + eps);
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int c = lane * 4 + j * 256;
        if (c < H) {
            const float4 g = *(const float4 *)(w + c);
            *(uint2 *)(h16 + t * H + c) = uint2{mt::pack_bf16x2(f[j].x * rs * g.x, f[j].y * rs * g.y), mt::pack_bf16x2(f[j].z * rs * g.z, f[j].w * rs * g.w)};
        }
    }
}

// The sandwich join, one wave per token t < T: x32 += RMSNorm(y32; w_post) (y32 the sub-layer's float32 GEMM output), then the norm in
// front of what follows, RMSNorm(x32; w_pre): as bf16 GEMM rows h16 or, out32 != NULL (the model's final norm), as float32 rows out32
// (which may be y32: a lane rewrites only what it has read). The row stays in registers between the two reductions (NJ float4 per lane,
// NJ = ceil(H / 256)): one pass over memory, as k_mb_add_ln.
template <int NJ>
__global__ __launch_bounds__(256) void k_gm_norm_add_norm(float *__restrict__ x32, const float *__restrict__ y32, int64_t T, int H,
                                                          const float *__restrict__ w_post, const float *__restrict__ w_pre, float eps,
                                                          uint16_t *__restrict__ h16, float *__restrict__ out32) {
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= T) return;
    float4 y[NJ], f[NJ];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int c = lane * 4 + j * 256;
        y[j] = f[j] = float4{0.f, 0.f, 0.f, 0.f};
        if (c < H) {
            y[j] = *(const float4 *)(y32 + t * H + c);
            f[j] = *(const float4 *)(x32 + t * H + c);
            ss += (y[j].x * y[j].x + y[j].y * y[j].y) + (y[j].z * y[j].z + y[j].w * y[j].w);
        }
    }
    const float rp = rsqrtf(wave_sum(ss) / (float)H + eps);
    float s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int c = lane * 4 + j * 256;
        if (c < H) {
            const float4 g = *(const float4 *)(w_post + c);
            f[j].x += y[j].x * rp * g.x; f[j].y += y[j].y * rp * g.y; f[j].z += y[j].z * rp * g.z; f[j].w += y[j].w * rp * g.w;
            *(float4 *)(x32 + t * H + c) = f[j];
            s2 += (f[j].x * f[j].x + f[j].y * f[j].y) + (f[j].z * f[j].z + f[j].w * f[j].w);
        }
    }
    const float rs = rsqrtf(wave_sum(s2) / (float)H + eps);
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int c = lane * 4 + j * 256;
        if (c < H) {
            const float4 g = *(const float4 *)(w_pre + c);
            const float4 o = {f[j].x * rs * g.x, f[j].y * rs * g.y, f[j].z * rs * g.z, f[j].w * rs * g.w};
            if (out32) *(float4 *)(out32 + t * H + c) = o;
            else *(uint2 *)(h16 + t * H + c) = uint2{mt::pack_bf16x2(o.x, o.y), mt::pack_bf16x2(o.z, o.w)};
        }
    }
}

// Workgroup (32-token block tb, head slot hs) over the QKV rows [T][(nq + 2 nkv) 256] (S % 32 == 0: a block lies inside one sequence).
// q and k slots: 8 threads per token, thread u of them takes the 16-byte chunks 2 u, 2 u + 1 of the head and their rotate_half partners
// 16 + 2 u, 17 + 2 u (elements d and d + 128): RMSNorm over the 256 (sum of squares over the 8 threads by shuffles), times the folded
// norm weight, then x' = x cos + rot(x) sin at position t % S, rot(x)[d] = -x[d + 128], rot(x)[d + 128] = x[d]; q also times qscale.
// Stored head-major, q [B][nq][S][256] and k [B][nkv][S][256], 16 bytes per access.
// v slots: the block's [32 tokens][256] tile goes through LDS and leaves transposed, thread d writing the 64 bytes of row d of
// vt [B][nkv][256][S] with the keys of each 16-group in vt_pos order (what the attention kernel's V^T staging reads).
__global__ __launch_bounds__(256) void k_gm_qk_norm_rope(const uint16_t *__restrict__ qkv, int S, int nq, int nkv, const float *__restrict__ qn,
                                                         const float *__restrict__ kn, float eps, const float *__restrict__ rc,
                                                         const float *__restrict__ rs, float qscale, uint16_t *__restrict__ q, uint16_t *__restrict__ k,
                                                         uint16_t *__restrict__ vt) {
    __shared__ __attribute__((aligned(16))) uint16_t sT[32 * GM_HD];
    const int tid = threadIdx.x, hs = blockIdx.y, slots = nq + 2 * nkv;
    const int64_t t0 = (int64_t)blockIdx.x * 32;
    const int b = (int)(t0 / S), sq0 = (int)(t0 - (int64_t)b * S);
    if (hs >= nq + nkv) {                                      // a value head: transpose
        const int hv = hs - nq - nkv;
#pragma unroll
        for (int n = 0; n < 4; n++) {
            const int i = tid + n * 256, tok = i >> 5, c = i & 31;
            *(uint4 *)(sT + tok * GM_HD + c * 8) = *(const uint4 *)(qkv + ((t0 + tok) * slots + hs) * GM_HD + c * 8);
        }
        __syncthreads();
        const int d = tid;
        uint32_t w[16];
#pragma unroll
        for (int p = 0; p < 32; p += 2) {                      // vt_pos swaps bits 2 and 3: it is its own inverse
            const uint32_t lo = sT[vt_pos(p) * GM_HD + d], hi = sT[vt_pos(p + 1) * GM_HD + d];
            w[p >> 1] = lo | (hi << 16);
        }
        uint16_t *dst = vt + (((int64_t)b * nkv + hv) * GM_HD + d) * S + sq0;
#pragma unroll
        for (int c = 0; c < 4; c++) *(uint4 *)(dst + c * 8) = uint4{w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3]};
        return;
    }
    const int tok = tid >> 3, u = tid & 7, sq = sq0 + tok;
    const bool isq = hs < nq;
    const uint16_t *row = qkv + ((t0 + tok) * slots + hs) * GM_HD + u * 16;
    const uint4 a0 = *(const uint4 *)row, a1 = *(const uint4 *)(row + 8), b0 = *(const uint4 *)(row + 128), b1 = *(const uint4 *)(row + 136);
    const uint32_t aw[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}, bw[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    float xa[16], xb[16];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        xa[2 * i] = bf16_to_f32((uint16_t)aw[i]); xa[2 * i + 1] = bf16_to_f32((uint16_t)(aw[i] >> 16));
        xb[2 * i] = bf16_to_f32((uint16_t)bw[i]); xb[2 * i + 1] = bf16_to_f32((uint16_t)(bw[i] >> 16));
        ss += (xa[2 * i] * xa[2 * i] + xa[2 * i + 1] * xa[2 * i + 1]) + (xb[2 * i] * xb[2 * i] + xb[2 * i + 1] * xb[2 * i + 1]);
    }
    ss += __shfl_xor(ss, 1); ss += __shfl_xor(ss, 2); ss += __shfl_xor(ss, 4);
    const float rn = rsqrtf(ss * (1.0f / GM_HD) + eps);
    const float *wn = (isq ? qn : kn) + u * 16;
    const float *cr = rc + (int64_t)sq * 128 + u * 16, *sr = rs + (int64_t)sq * 128 + u * 16;
    const float sc = isq ? qscale : 1.0f;
    uint32_t ao[8], bo[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        float ya[2], yb[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int d = 2 * i + e;
            const float x0 = xa[d] * rn * wn[d], x1 = xb[d] * rn * wn[128 + d];
            ya[e] = (x0 * cr[d] - x1 * sr[d]) * sc;
            yb[e] = (x1 * cr[d] + x0 * sr[d]) * sc;
        }
        ao[i] = mt::pack_bf16x2(ya[0], ya[1]);
        bo[i] = mt::pack_bf16x2(yb[0], yb[1]);
    }
    uint16_t *dst = (isq ? q + (((int64_t)b * nq + hs) * S + sq) * GM_HD : k + (((int64_t)b * nkv + (hs - nq)) * S + sq) * GM_HD) + u * 16;
    *(uint4 *)dst = uint4{ao[0], ao[1], ao[2], ao[3]};
    *(uint4 *)(dst + 8) = uint4{ao[4], ao[5], ao[6], ao[7]};
    *(uint4 *)(dst + 128) = uint4{bo[0], bo[1], bo[2], bo[3]};
    *(uint4 *)(dst + 136) = uint4{bo[4], bo[5], bo[6], bo[7]};
}

// Pooling, stage 1 (pool_part of stack.h) over the float32 final-norm rows below the row's length, as they are.
struct GmIdentity {
    struct Token {
        __device__ float apply(float x) const { return x; }
    };
    __device__ int count(int len) const { return len; }
    __device__ Token begin(const float *, int, int) const { return Token{}; }
};
__global__ __launch_bounds__(256) void k_gm_pool_part(const float *__restrict__ y32, const int *__restrict__ lens, int S, int H, float *__restrict__ part) {
    pool_part(y32, lens, S, H, GmIdentity{}, part);
}

// Pooling, stage 2. One workgroup per row b: the chunk sums added in chunk order, / n -> pooled[b][H] (a row of length 0: zeros)
__global__ __launch_bounds__(256) void k_gm_pool_fin(const float *__restrict__ part, int nch, const int *__restrict__ lens, int H, float *__restrict__ pooled) {
    const int b = blockIdx.x, n = lens[b];
    const int used = n <= 0 ? 0 : (n + POOL_CHUNK - 1) / POOL_CHUNK;
    const float inv_n = n > 0 ? 1.0f / (float)n : 0.f;
    for (int c = threadIdx.x; c < H; c += 256) {
        float y = 0.f;
        for (int ck = 0; ck < used; ck++) y += part[((int64_t)b * nch + ck) * H + c];
        pooled[(int64_t)b * H + c] = y * inv_n;
    }
}

// A Dense module of the sentence-transformers tail on the B pooled rows: out[b][n] = sum_k W[n][k] in[b][k], float32 throughout
// (W [N][K] as torch.nn.Linear.weight, no bias, identity activation). One wave per output element; K % 4 == 0. Not a hot path.
__global__ __launch_bounds__(256) void k_gm_dense(const float *__restrict__ in, const float *__restrict__ W, int N, int K, float *__restrict__ out) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y, lane = threadIdx.x & 63;
    if (n >= N) return;
    const float *wr = W + (int64_t)n * K, *xr = in + (int64_t)b * K;
    float s = 0.f;
    for (int c = lane * 4; c < K; c += 256) {
        const float4 w = *(const float4 *)(wr + c), x = *(const float4 *)(xr + c);
        s += (w.x * x.x + w.y * x.y) + (w.z * x.z + w.w * x.w);
    }
    s = wave_sum(s);
    if (lane == 0) out[(int64_t)b * N + n] = s;
}

// out[b] = in[b] / max(|in[b]|, 1e-12) (normalise != 0; torch.nn.functional.normalize's eps) or a copy; one workgroup per row
__global__ __launch_bounds__(256) void k_gm_l2(const float *__restrict__ in, int D, int normalise, float *__restrict__ out) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *x = in + (int64_t)b * D;
    float s2 = 0.f;
    for (int c = tid; c < D; c += 256) s2 += x[c] * x[c];
    const float sc = block_l2_scale(s2, tid & 63, tid >> 6, normalise);
    for (int c = tid; c < D; c += 256) out[(int64_t)b * D + c] = x[c] * sc;
}

}  // namespace

// ---- launches: the one place each kernel's grid is spelled (create, the forward pass below and the single-launch tests call these) ----
int launch_gm_fold1p(const float *w, int n, float *w1, hipStream_t st) {
    k_gm_fold1p<<<(n + 255) / 256, 256, 0, st>>>(w, n, w1);
    AK_HIP(hipGetLastError());
    return 0;
}

int launch_gm_embed(const int *ids, int ld_ids, const int *lens, int lens_stride, int B, int S, int H, int vocab, const uint16_t *emb, const float *w,
                    float eps, float *x32, uint16_t *h16, int *lens_out, hipStream_t st) {
    const unsigned rows4 = (unsigned)(((int64_t)B * S + 3) / 4);
    const float scale = sqrtf((float)H);
    dispatch_nj(H, [&](auto nj) {
        k_gm_embed<decltype(nj)::value><<<rows4, 256, 0, st>>>(ids, ld_ids, lens, lens_stride, B, S, H, vocab, emb, scale, w, eps, x32, h16, lens_out);
    });
    AK_HIP(hipGetLastError());
    return 0;
}

int launch_gm_norm_add_norm(float *x32, const float *y32, int64_t T, int H, const float *w_post, const float *w_pre, float eps, uint16_t *h16,
                            float *out32, hipStream_t st) {
    const unsigned rows4 = (unsigned)((T + 3) / 4);
    dispatch_nj(H, [&](auto nj) { k_gm_norm_add_norm<decltype(nj)::value><<<rows4, 256, 0, st>>>(x32, y32, T, H, w_post, w_pre, eps, h16, out32); });
    AK_HIP(hipGetLastError());
    return 0;
}

// both pooling stages: part [B][ceil(S / 64)][H] floats of workspace -> pooled [B][H]
int launch_gm_pool(const float *y32, const int *lens, int B, int S, int H, float *part, float *pooled, hipStream_t st) {
    const int nch = (S + POOL_CHUNK - 1) / POOL_CHUNK;
    k_gm_pool_part<<<dim3((unsigned)nch, (unsigned)B), 256, (size_t)4 * H * 4, st>>>(y32, lens, S, H, part);
    AK_HIP(hipGetLastError());
    k_gm_pool_fin<<<B, 256, 0, st>>>(part, nch, lens, H, pooled);
    AK_HIP(hipGetLastError());
    return 0;
}

int launch_gm_dense(const float *in, const float *W, int B, int N, int K, float *out, hipStream_t st) {
    k_gm_dense<<<dim3((unsigned)((N + 3) / 4), (unsigned)B), 256, 0, st>>>(in, W, N, K, out);
    AK_HIP(hipGetLastError());
    return 0;
}

int launch_gm_l2(const float *in, int B, int D, int normalise, float *out, hipStream_t st) {
    k_gm_l2<<<B, 256, 0, st>>>(in, D, normalise, out);
    AK_HIP(hipGetLastError());
    return 0;
}

namespace {
struct GmLayer {
    const uint16_t *wqkv, *wo, *wgu, *wdown;       // wqkv (concatenated) and wgu (interleaved) are owned, wdown too when I is padded
    const float *input_ln, *q_norm, *k_norm, *post_attn_ln, *pre_ffn_ln, *post_ffn_ln;      // owned: 1 + w
    bool global;
};
struct Gemma : Stack {
    AkGemmaConfig cfg;
    const uint16_t *emb = nullptr; const float *final_norm = nullptr;
    std::vector<GmLayer> layers;
    const float *dense[2] = {nullptr, nullptr};
    int dense_in[2] = {0, 0}, dense_out[2] = {0, 0}, out_dim = 0;
    float *rope_c[2] = {nullptr, nullptr}, *rope_s[2] = {nullptr, nullptr};      // [0] local theta, [1] global theta
    int Ip = 0, NQKV = 0;                          // Ip: intermediate size as the GEMMs see it (padded_intermediate)
    float qscale = 0.f;
    float *x32 = nullptr, *y32 = nullptr, *part = nullptr, *pool_a = nullptr, *pool_b = nullptr;
    uint16_t *h16 = nullptr, *qkv = nullptr, *q = nullptr, *k = nullptr, *vt = nullptr, *ctx = nullptr, *f = nullptr;
    int *lens = nullptr;
};

int gm_forward_locked(Gemma &d, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S, int normalise, float *out,
                      hipStream_t st) {
    const AkGemmaConfig &c = d.cfg;
    const int H = c.hidden, I = d.Ip, nq = c.q_heads, nkv = c.kv_heads;
    const int64_t T = (int64_t)B * S, tpad = (T + 255) / 256 * 256;
    if (d.reserve(tpad, B)) return -10;
    if (launch_gm_embed(ids, ld_ids, lens, lens_stride, B, S, H, c.vocab_size, d.emb, d.layers[0].input_ln, c.rms_eps, d.x32, d.h16, d.lens, st)) return -10;
    for (size_t l = 0; l < d.layers.size(); l++) {
        const GmLayer &ly = d.layers[l];
        const bool last = l + 1 == d.layers.size();
        // q | k | v rows
        if (launch_gemm(3, d.gemm_bf16(tpad, d.h16, ly.wqkv, d.NQKV, H, d.qkv), st)) return -10;
        const int tb = ly.global ? 1 : 0;
        if (launch_gm_qk_norm_rope(d.qkv, B, S, nq, nkv, ly.q_norm, ly.k_norm, c.rms_eps, d.rope_c[tb], d.rope_s[tb], d.qscale, d.q, d.k, d.vt, st)) return -10;
        GqaAttnArgs a{d.q, d.k, d.vt, d.lens, d.ctx, B, S, nq, nkv};
        if (launch_attn_gqa(a, ly.global ? 0 : c.half_window, st)) return -10;
        // x += RMSNorm(ctx Wo^T; post_attn_ln); h = RMSNorm(x; pre_ffn_ln)
        if (launch_gemm(2, d.gemm_f32(tpad, d.ctx, ly.wo, H, nq * GM_HD, d.y32), st)) return -10;
        if (launch_gm_norm_add_norm(d.x32, d.y32, T, H, ly.post_attn_ln, ly.pre_ffn_ln, c.rms_eps, d.h16, nullptr, st)) return -10;
        // f = gelu_tanh(h Wgate^T) (h Wup^T)
        if (launch_gemm(9, d.gemm_gated(tpad, d.h16, ly.wgu, I, H, d.f), st)) return -10;
        // x += RMSNorm(f Wdown^T; post_ffn_ln); h = RMSNorm(x; next layer's input_ln) (after the last layer: the final norm, float32 rows)
        if (launch_gemm(2, d.gemm_f32(tpad, d.f, ly.wdown, H, I, d.y32), st)) return -10;
        if (launch_gm_norm_add_norm(d.x32, d.y32, T, H, ly.post_ffn_ln, last ? d.final_norm : d.layers[l + 1].input_ln, c.rms_eps, d.h16,
                                    last ? d.y32 : nullptr, st))
            return -10;
    }
    if (launch_gm_pool(d.y32, d.lens, B, S, H, d.part, d.pool_a, st)) return -10;
    float *cur = d.pool_a, *nxt = d.pool_b;
    for (int i = 0; i < c.n_dense; i++) {
        if (launch_gm_dense(cur, d.dense[i], B, d.dense_out[i], d.dense_in[i], nxt, st)) return -10;
        std::swap(cur, nxt);
    }
    return launch_gm_l2(cur, B, d.out_dim, normalise, out, st) ? -10 : 0;
}
}  // namespace

int launch_gm_qk_norm_rope(const uint16_t *qkv, int B, int S, int nq, int nkv, const float *qn, const float *kn, float eps, const float *rc,
                           const float *rs, float qscale, uint16_t *q, uint16_t *k, uint16_t *vt, hipStream_t st) {
    if (B <= 0 || S <= 0 || S % 32 || nq <= 0 || nkv <= 0 || nq + 2 * nkv > 65535) AK_FAIL(-1, "gm_qk_norm_rope: S must be a positive multiple of 32");
    const int64_t nblk = (int64_t)B * S / 32;
    if (nblk > 0x7fffffff) AK_FAIL(-1, "gm_qk_norm_rope: too many tokens");
    k_gm_qk_norm_rope<<<dim3((unsigned)nblk, (unsigned)(nq + 2 * nkv)), 256, 0, st>>>(qkv, S, nq, nkv, qn, kn, eps, rc, rs, qscale, q, k, vt);
    AK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ak

using namespace ak;

extern "C" int ak_gemma_destroy(ak_gemma_t h) { return stack_destroy<Gemma>(h); }

extern "C" int ak_gemma_create(const AkGemmaConfig *cfg, const void *const *w, int n_weights, ak_gemma_t *out) {
    AK_BIND();
    if (!cfg || !w || !out) AK_FAIL(-1, "ak_gemma_create: NULL argument");
    *out = nullptr;
    const AkGemmaConfig c = *cfg;
    const int H = c.hidden, I = c.intermediate, L = c.layers, nq = c.q_heads, nkv = c.kv_heads;
    if (L <= 0 || c.vocab_size <= 0 || nq <= 0 || nkv <= 0 || H <= 0 || I <= 0 || c.max_position <= 0) AK_FAIL(-1, "ak_gemma_create: sizes must be positive");
    if (L > AK_GEMMA_MAX_LAYERS) AK_FAIL(-1, "ak_gemma_create: layers: more than AK_GEMMA_MAX_LAYERS");
    if (c.head_dim != GM_HD) AK_FAIL(-1, "ak_gemma_create: head_dim must be 256");
    if (nq % nkv) AK_FAIL(-1, "ak_gemma_create: q_heads must be a multiple of kv_heads");
    if (nq / nkv > 4) AK_FAIL(-1, "ak_gemma_create: q_heads / kv_heads (the group) must be <= 4");
    if (H % 128 || H > GM_MAX_H) AK_FAIL(-1, "ak_gemma_create: hidden must be a multiple of 128, <= 1024");
    if (I % 64) AK_FAIL(-1, "ak_gemma_create: intermediate must be a multiple of 64");
    if (c.attn_softcap != 0.f || c.final_softcap != 0.f) AK_FAIL(-1, "ak_gemma_create: attn_softcap / final_softcap: soft-capping is not implemented");
    if (c.rope_type != 0) AK_FAIL(-1, "ak_gemma_create: rope_type: default RoPE only");
    if (c.activation != 0) AK_FAIL(-1, "ak_gemma_create: activation must be gelu_pytorch_tanh");
    if (c.attention_bias != 0) AK_FAIL(-1, "ak_gemma_create: attention_bias is not supported");
    if (c.half_window < 1) AK_FAIL(-1, "ak_gemma_create: half_window must be >= 1");
    if (!(c.rms_eps > 0.f) || !(c.global_rope_theta > 0.f) || !(c.local_rope_theta > 0.f) || !(c.query_pre_attn_scalar > 0.f))
        AK_FAIL(-1, "ak_gemma_create: rms_eps, the rope thetas and query_pre_attn_scalar must be positive");
    if (c.n_dense < 0 || c.n_dense > 2) AK_FAIL(-1, "ak_gemma_create: n_dense must be 0, 1 or 2");
    int din = H;
    for (int i = 0; i < c.n_dense; i++) {
        if (c.dense_out[i] <= 0 || c.dense_out[i] > GM_MAX_DENSE || c.dense_out[i] % 4) AK_FAIL(-1, "ak_gemma_create: dense_out must be a multiple of 4 in (0, 4096]");
        din = c.dense_out[i];
    }
    if (n_weights != 2 + 13 * L + c.n_dense) AK_FAIL(-1, "ak_gemma_create: expected 2 + 13 * layers + n_dense weight pointers");
    for (int i = 0; i < n_weights; i++)
        if (!w[i]) AK_FAIL(-1, "ak_gemma_create: NULL weight pointer");
    Gemma *d = new Gemma();
    d->cfg = c;
    d->out_dim = din;
    d->emb = (const uint16_t *)w[0];
    d->NQKV = (nq + 2 * nkv) * GM_HD;
    d->qscale = 1.4426950408889634f / sqrtf(c.query_pre_attn_scalar);
    auto fail = [&](const char *what) { set_error(what); ak_gemma_destroy(d); return -10; };
    auto fold = [&](const void *src, int n) -> const float * {      // 1 + w
        float *p = d->dev_as<float>(n);
        if (!p) return nullptr;
        return launch_gm_fold1p((const float *)src, n, p, nullptr) ? nullptr : p;
    };
    if (!(d->final_norm = fold(w[1], H))) return fail("ak_gemma_create: hipMalloc failed");
    const int Ip = d->Ip = padded_intermediate(I);
    d->zero_bias = d->dev_as<float>(std::max<size_t>(std::max<size_t>((size_t)d->NQKV, (size_t)2 * Ip), (size_t)H), true);
    if (!d->zero_bias) return fail("ak_gemma_create: hipMalloc failed");
    // the two rotary tables, positions 0 .. min(max_position, 2048) - 1, at head size 256
    d->n_pos = c.max_position < GM_MAX_S ? c.max_position : GM_MAX_S;
    for (int tb = 0; tb < 2; tb++)
        if (!d->rope_tables(tb ? c.global_rope_theta : c.local_rope_theta, GM_HD, &d->rope_c[tb], &d->rope_s[tb]))
            return fail("ak_gemma_create: rotary table upload failed");
    const size_t NQ = (size_t)nq * GM_HD, NK = (size_t)nkv * GM_HD;
    for (int l = 0; l < L; l++) {
        // input_ln wq wk wv q_norm k_norm wo post_attn_ln pre_ffn_ln w_gate w_up w_down post_ffn_ln
        const void *const *p = w + 2 + 13 * l;
        GmLayer ly{};
        uint16_t *wqkv = d->dev_as<uint16_t>((size_t)d->NQKV * H);
        if (!wqkv || !d->concat_rows(wqkv, H, {{p[1], NQ}, {p[2], NK}, {p[3], NK}})) return fail("ak_gemma_create: QKV concatenation failed");
        uint16_t *wgu = d->dev_as<uint16_t>((size_t)2 * Ip * H, Ip != I);
        if (!wgu) return fail("ak_gemma_create: hipMalloc failed");
        // row 2 j = gate_proj row j, row 2 j + 1 = up_proj row j (gemm.hip MODE 9)
        if (!d->interleave_rows(wgu, p[9], p[10], I, H)) return fail("ak_gemma_create: gate / up interleave failed");
        ly.wqkv = wqkv; ly.wo = (const uint16_t *)p[6]; ly.wgu = wgu; ly.wdown = (const uint16_t *)p[11];
        if (Ip != I && !(ly.wdown = d->pad_cols(p[11], H, I, Ip))) return fail("ak_gemma_create: down_proj padding failed");
        ly.input_ln = fold(p[0], H); ly.q_norm = fold(p[4], GM_HD); ly.k_norm = fold(p[5], GM_HD);
        ly.post_attn_ln = fold(p[7], H); ly.pre_ffn_ln = fold(p[8], H); ly.post_ffn_ln = fold(p[12], H);
        if (!ly.input_ln || !ly.q_norm || !ly.k_norm || !ly.post_attn_ln || !ly.pre_ffn_ln || !ly.post_ffn_ln) return fail("ak_gemma_create: norm weight fold failed");
        ly.global = c.layer_global[l] != 0;
        d->layers.push_back(ly);
    }
    din = H;
    for (int i = 0; i < c.n_dense; i++) {
        d->dense[i] = (const float *)w[2 + 13 * L + i];
        d->dense_in[i] = din; d->dense_out[i] = c.dense_out[i];
        din = c.dense_out[i];
    }
    const size_t pw = (size_t)std::max(H, std::max(d->dense_out[0], d->dense_out[1])) * 4;      // widest pooled row
    d->buffer(&d->x32, (size_t)H * 4); d->buffer(&d->y32, (size_t)H * 4); d->buffer(&d->h16, (size_t)H * 2);
    d->buffer(&d->qkv, (size_t)d->NQKV * 2); d->buffer(&d->q, NQ * 2); d->buffer(&d->k, NK * 2); d->buffer(&d->vt, NK * 2);
    d->buffer(&d->ctx, NQ * 2); d->buffer(&d->f, (size_t)Ip * 2); d->buffer(&d->lens, 0, 4);
    d->buffer(&d->part, (size_t)H * 4 / POOL_CHUNK, (size_t)H * 4);      // B ceil(S / 64) <= T / 64 + B rows of H floats
    d->buffer(&d->pool_a, 0, pw); d->buffer(&d->pool_b, 0, pw);
    if (hipDeviceSynchronize() != hipSuccess) return fail("ak_gemma_create: weight preparation failed");
    *out = d;
    return 0;
}

extern "C" int ak_gemma_set_rope_inv_freq(ak_gemma_t h, const float *global_inv, const float *local_inv) {
    AK_BIND();
    if (!h || !global_inv || !local_inv) AK_FAIL(-1, "ak_gemma_set_rope_inv_freq: NULL argument");
    Gemma &d = *(Gemma *)h;
    std::lock_guard<std::mutex> lk(d.mu);
    AK_HIP(hipDeviceSynchronize());                            // no forward of this handle reads the tables while they change
    for (int tb = 0; tb < 2; tb++)                             // [0] local theta, [1] global theta
        if (d.rope_tables_set_inv(tb ? global_inv : local_inv, GM_HD / 2, d.rope_c[tb], d.rope_s[tb])) return -10;
    return 0;
}

extern "C" int ak_gemma_forward_lens(ak_gemma_t h, const int32_t *ids, int ld_ids, const int32_t *lens, int lens_stride, int B, int S, int pooling,
                                     int normalise, float *out, void *stream) {
    AK_BIND();
    if (!h) AK_FAIL(-1, "ak_gemma_forward_lens: NULL handle");
    RoctxRange range("ak_gemma_forward_lens");
    Gemma &d = *(Gemma *)h;
    if (B <= 0) return 0;
    if (check_forward_lens("ak_gemma_forward_lens", ids, lens, out, ld_ids, lens_stride, B, S, GM_MAX_S, d.n_pos,
                           pooling == AK_POOL_MEAN ? nullptr : "pooling must be AK_POOL_MEAN", 65535))
        return -1;
    std::lock_guard<std::mutex> lk(d.mu);
    return gm_forward_locked(d, ids, ld_ids, lens, lens_stride, B, S, normalise, out, (hipStream_t)stream);
}
