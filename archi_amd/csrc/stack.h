// stack.h -- what the stacks (decoder128.hip: Qwen3 / Llama / Qwen2, mbert.hip: ModernBERT, gemma.hip: EmbeddingGemma, nomic.hip: NomicBERT) share: a
// float32 residual stream feeding bf16 GEMM rows, one wave per token in the row kernels, pooling in chunks of 64 tokens. Plumbing
// only: each family keeps its own kernels, and where a formula is stated here (the LayerNorm statistics of a row in registers, the
// pooling stages) the order of its sums is part of the statement.
//   device: wave_sum, token_slot, load_bf16x4 / store_bf16x4, row_sum4 / row_sq4, row_load_sum / row_ln_stats (the LayerNorm
//           families: mbert.hip, nomic.hip), block_l2_scale, pooled_count, pool_part, pool_fin
//   host:   dispatch_nj, launch_pool_stages, Stack (owned device memory, weight preparation, workspace, rotary tables, GemmArgs),
//           stack_destroy, check_forward_lens (stack.hip holds what is better not inlined)
// enc64.h builds the head-64 encoder base of mbert.hip and nomic.hip on Stack.
#pragma once
#include <mutex>
#include <type_traits>
#include <vector>

#include "encoder_kernels.h"
#include "mfma_tile.h"

namespace ak {

constexpr int POOL_CHUNK = 64, POOL_MAX_H = 1024;      // pooling: tokens per chunk; widest row pool_part holds in registers

// ---- device ------------------------------------------------------------------------------------------------------------------
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// The embedding kernels' prologue, one wave per token slot t < B * S: slot -> (row b, position sq), the row's length clamped to
// [0, S] (the wave of a row's slot 0 stores it to lens_out: attention and pooling read it) and, MASK, the int key mask [B * S]
// (slot < length). Returns the slot's token id: 0 past the length, and 0 for a stray id, which must not read out of bounds.
template <bool MASK>
__device__ inline int token_slot(const int *__restrict__ ids, int ld_ids, const int *__restrict__ lens, int lens_stride, int S, int vocab, int64_t t,
                                 int lane, int *__restrict__ mask, int *__restrict__ lens_out) {
    const int b = (int)(t / S), sq = (int)(t - (int64_t)b * S);
    int len = lens[(int64_t)b * lens_stride];
    len = len < 0 ? 0 : (len > S ? S : len);
    if (lane == 0) {
        if (MASK) mask[t] = sq < len;
        if (sq == 0) lens_out[b] = len;
    }
    int id = sq < len ? ids[(int64_t)b * ld_ids + sq] : 0;
    if (id < 0 || id >= vocab) id = 0;
    return id;
}

// four bf16 of a row (8-byte aligned) as float4, and back
__device__ inline float4 load_bf16x4(const uint16_t *p) {
    const uint2 v = *(const uint2 *)p;
    return float4{bf16_to_f32((uint16_t)v.x), bf16_to_f32((uint16_t)(v.x >> 16)), bf16_to_f32((uint16_t)v.y), bf16_to_f32((uint16_t)(v.y >> 16))};
}
__device__ inline void store_bf16x4(uint16_t *p, float x, float y, float z, float w) {
    *(uint2 *)p = uint2{mt::pack_bf16x2(x, y), mt::pack_bf16x2(z, w)};
}

// ---- a LayerNorm row in registers: NJ float4 per lane, feature c = 4 lane + 256 j; lanes at or past H hold zeros ----
__device__ inline float4 load_row4(const float *p) { return *(const float4 *)p; }
__device__ inline float4 load_row4(const uint16_t *p) { return load_bf16x4(p); }
// one float4's share of a row's sum, and of its sum of squares about `mean`: the pairing is part of the statement
__device__ inline float row_sum4(const float4 &f) { return (f.x + f.y) + (f.z + f.w); }
__device__ inline float row_sq4(const float4 &f, float mean) {
    const float a = f.x - mean, b = f.y - mean, c = f.z - mean, d = f.w - mean;
    return (a * a + b * b) + (c * c + d * d);
}
// f = row a (float32, or bf16 widened) + row b, one float32 add per feature; STORE: the sum goes back to a. Returns the lane's share
// of the row's sum.
template <bool STORE, int NJ, class A>
__device__ inline float row_load_sum(A *__restrict__ ar, const float *__restrict__ br, int H, int lane, float4 (&f)[NJ]) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int c = lane * 4 + j * 256;
        f[j] = float4{0.f, 0.f, 0.f, 0.f};
        if (c < H) {
            f[j] = load_row4(ar + c);
            const float4 y = *(const float4 *)(br + c);
            f[j].x += y.x; f[j].y += y.y; f[j].z += y.z; f[j].w += y.w;
            if constexpr (STORE) *(float4 *)(ar + c) = f[j];
            s += row_sum4(f[j]);
        }
    }
    return s;
}
// s = the lane's share of the row's sum -> mean, then the variance about it (two passes, as torch's float32 kernel -- not
// E[x^2] - mean^2), rstd = rsqrt(var + eps)
template <int NJ>
__device__ inline void row_ln_stats(const float4 (&f)[NJ], float s, int H, int lane, float eps, float &mean, float &rstd) {
    mean = wave_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; j++)
        if (lane * 4 + j * 256 < H) q += row_sq4(f[j], mean);
    rstd = rsqrtf(wave_sum(q) / (float)H + eps);
}

// The L2 tail of a 4-wave workgroup (thread = 64 wave + lane): s2 = each thread's share of a row's sum of squares; the wave sums
// meet in wave order through 16 bytes of LDS. Returns 1 / max(|row|, 1e-12) (torch.nn.functional.normalize's eps), or 1 when normalise == 0.
__device__ inline float block_l2_scale(float s2, int lane, int wave, int normalise) {
    __shared__ float red[4];
    s2 = wave_sum(s2);
    if (lane == 0) red[wave] = s2;
    __syncthreads();
    const float tot = ((red[0] + red[1]) + red[2]) + red[3];
    return normalise ? 1.0f / fmaxf(sqrtf(tot), 1e-12f) : 1.0f;
}

// tokens that mean / cls pooling sums in a row of length len
__device__ inline int pooled_count(int len, int pooling) { return len <= 0 ? 0 : (pooling == AK_POOL_CLS ? 1 : len); }

// Pooling, stage 1, of workgroup (chunk ck = blockIdx.x, row b = blockIdx.y), 4 waves: tokens 64 ck .. 64 ck + 63 below n of row b,
// each through the per-token transform, summed: wave v takes tokens v, v + 4, ...; the four wave partials are added in wave order
// -> part[b][ck][H]. Chunks at or past n write nothing (stage 2 does not read them). Which tokens meet in which sum depends on n
// alone, not on S or the batch around it. A row wider than POOL_MAX_H is pooled in column slices of POOL_MAX_H, slice blockIdx.z
// (gridDim.z = ceil(H / 1024); the per-token transform still sees the whole row). Row: n = count(the row's length); tok = begin(xr, H, lane) once per token row, then
// tok.apply(x) per feature.
template <class Row>
__device__ inline void pool_part(const float *x32, const int *lens, int S, int H, Row row, float *part) {
    extern __shared__ float lds[];                             // [4][W]: the launch's dynamic LDS
    const int ck = blockIdx.x, b = blockIdx.y, nch = gridDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.z * POOL_MAX_H, W = min(H - c0, POOL_MAX_H);      // the workgroup's columns (H <= 1024: all of them)
    const int n = row.count(lens[b]);
    if (ck * POOL_CHUNK >= n) return;
    const int stop = min(n, (ck + 1) * POOL_CHUNK);
    float4 acc[POOL_MAX_H / 256];
#pragma unroll
    for (int j = 0; j < POOL_MAX_H / 256; j++) acc[j] = float4{0.f, 0.f, 0.f, 0.f};
    for (int tk = ck * POOL_CHUNK + wave; tk < stop; tk += 4) {
        const float *xr = x32 + ((int64_t)b * S + tk) * H;
        const auto tok = row.begin(xr, H, lane);
#pragma unroll
        for (int j = 0; j < POOL_MAX_H / 256; j++) {
            const int c = lane * 4 + j * 256;
            if (c < W) {
                const float4 f = *(const float4 *)(xr + c0 + c);
                acc[j].x += tok.apply(f.x); acc[j].y += tok.apply(f.y); acc[j].z += tok.apply(f.z); acc[j].w += tok.apply(f.w);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < POOL_MAX_H / 256; j++) {
        const int c = lane * 4 + j * 256;
        if (c < W) *(float4 *)(lds + wave * W + c) = acc[j];
    }
    __syncthreads();
    float *o = part + ((int64_t)b * nch + ck) * H + c0;
    for (int c = tid; c < W; c += 256) o[c] = ((lds[c] + lds[W + c]) + lds[2 * W + c]) + lds[3 * W + c];
}

// Pooling, stage 2, of workgroup b = blockIdx.x (256 threads) behind pool_part on pooled_count tokens: the chunk sums added in chunk
// order, WEIGHT: * w[c], / n, then the L2 normalisation. A row of length 0 embeds to zeros.
template <bool WEIGHT>
__device__ inline void pool_fin(const float *part, int nch, const int *lens, int H, const float *w, int pooling, int normalise, float *out) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = lens[b];
    float *o = out + (int64_t)b * H;
    if (len <= 0) {
        for (int c = tid; c < H; c += 256) o[c] = 0.f;
        return;
    }
    const int n = pooled_count(len, pooling), used = (n + POOL_CHUNK - 1) / POOL_CHUNK;
    const float inv_n = 1.0f / (float)n;
    float y[POOL_MAX_H / 256];
    float s2 = 0.f;
#pragma unroll
    for (int j = 0; j < POOL_MAX_H / 256; j++) {
        const int c = tid + j * 256;
        y[j] = 0.f;
        if (c < H) {
            for (int ck = 0; ck < used; ck++) y[j] += part[((int64_t)b * nch + ck) * H + c];
            y[j] = WEIGHT ? y[j] * w[c] * inv_n : y[j] * inv_n;
            s2 += y[j] * y[j];
        }
    }
    const float sc = block_l2_scale(s2, lane, wave, normalise);
#pragma unroll
    for (int j = 0; j < POOL_MAX_H / 256; j++) {
        const int c = tid + j * 256;
        if (c < H) o[c] = y[j] * sc;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// The row kernels that hold a row in registers are templates over NJ = ceil(H / 256) float4 per lane, H <= 1024:
// f(std::integral_constant<int, NJ>)
template <class F>
inline void dispatch_nj(int H, F &&f) {
    switch ((H + 255) / 256) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}

// Both stages of a pool_part / pool_fin pair: part(grid, lds_bytes) launches stage 1 on (chunk, row) workgroups with its [4][H]
// floats of dynamic LDS, fin(nch) stage 2 on the nch = ceil(S / 64) chunk sums per row
template <class P, class F>
inline int launch_pool_stages(int B, int S, int H, P &&part, F &&fin) {
    const int nch = (S + POOL_CHUNK - 1) / POOL_CHUNK;
    part(dim3((unsigned)nch, (unsigned)B), (size_t)4 * H * 4);
    AK_HIP(hipGetLastError());
    fin(nch);
    AK_HIP(hipGetLastError());
    return 0;
}

// 2 I off the wide GEMM tile (ModernBERT large: 5248 = 41 x 128): the interleaved gate / up matrix gets zero rows up to a multiple
// of 256 and the down projection zero columns to match (act(0) 0 = 0 meets a zero weight: bit-identical results). Measured,
// ModernBERT large 128 x 512: 62.9 ms against 67.2. Returns the intermediate size as the GEMMs see it.
inline int padded_intermediate(int I) { return (2 * I) % 256 ? (I + 127) / 128 * 128 : I; }

// HF's default rotary embedding in float32, table rows [n_pos][hd / 2] (stack.hip)
void rope_table_from_inv(const float *inv, int half, int n_pos, float *c, float *s);
void rope_table_host(float theta, int hd, int n_pos, float *c, float *s);

// What a family's handle is built on: the device memory it owns, the weight preparation at create, the per-call workspace and the
// GemmArgs of its launches.
struct Stack {
    std::vector<void *> owned;                 // freed at destroy
    float *zero_bias = nullptr;                // no family has a bias: the GEMMs read zeros
    int n_pos = 0;                             // rows of the rotary tables
    std::mutex mu;
    ~Stack();                                  // frees `owned`; stack_destroy releases the workspace first

    // -- create: every routine returns NULL / false on a HIP failure and leaves the message to the caller
    void *dev(size_t bytes, bool zero = false);
    template <class T> T *dev_as(size_t n, bool zero = false) { return (T *)dev(n * sizeof(T), zero); }
    // dst [sum rows][H] bf16 = the row blocks one under the other ([Wq; Wk; Wv])
    struct Rows { const void *p; size_t rows; };
    bool concat_rows(uint16_t *dst, int H, std::initializer_list<Rows> blocks);
    // dst [2 I][H] bf16: row 2 j = a row j, row 2 j + 1 = b row j (the gated GEMM epilogues, gemm.hip MODE 7 / 8 / 9). Rows past
    // 2 I of a dst padded to Ip are the caller's zeros (dev(.., Ip != I)).
    bool interleave_rows(uint16_t *dst, const void *a, const void *b, int I, int H);
    // w [H][I] bf16 -> a zeroed [H][Ip] with the columns behind I zero
    const uint16_t *pad_cols(const void *w, int H, int I, int Ip);
    // cos / sin tables of n_pos positions at head size hd on the device
    bool rope_tables(float theta, int hd, float **c, float **s);
    int rope_tables_set_inv(const float *inv, int half, float *c, float *s);      // existing tables from given inverse frequencies

    // -- workspace: buffers are registered once at create, bytes = tpad * per_token + B * per_row. reserve() never shrinks; when
    // either size grows it frees all, allocates all and zeroes them, so rows that no kernel writes (GEMM padding rows past B * S)
    // stay finite.
    struct Buf { void **p; size_t per_token, per_row; };
    std::vector<Buf> bufs;
    int64_t cap = 0; int cap_B = 0;
    template <class T> void buffer(T **p, size_t per_token, size_t per_row = 0) { bufs.push_back({(void **)p, per_token, per_row}); }
    int reserve(int64_t tpad, int B);
    void release();

    // -- launches: X [tpad][K] bf16 times W [N][K]^T
    GemmArgs gemm(int64_t tpad, const uint16_t *X, const uint16_t *W, int N, int K) const {
        GemmArgs g{};
        g.bias = zero_bias; g.T = (int)tpad; g.X = X; g.W = W; g.N = N; g.K = K;
        return g;
    }
    GemmArgs gemm_bf16(int64_t tpad, const uint16_t *X, const uint16_t *W, int N, int K, uint16_t *out) const {      // [tpad][N] bf16 rows
        GemmArgs g = gemm(tpad, X, W, N, K);
        g.out_bf16 = out; g.ldo = N;
        return g;
    }
    GemmArgs gemm_f32(int64_t tpad, const uint16_t *X, const uint16_t *W, int N, int K, float *out) const {          // [tpad][N] float32 rows
        GemmArgs g = gemm(tpad, X, W, N, K);
        g.out_f32 = out;
        return g;
    }
    GemmArgs gemm_gated(int64_t tpad, const uint16_t *X, const uint16_t *W, int I, int K, uint16_t *out) const {     // W interleaved [2 I][K] -> [tpad][I]
        GemmArgs g = gemm(tpad, X, W, 2 * I, K);
        g.out_bf16 = out; g.ldo = I;
        return g;
    }
};

// ak_*_destroy of a handle type derived from Stack
template <class T>
inline int stack_destroy(void *h) {
    AK_BIND();
    if (!h) return 0;
    hipDeviceSynchronize();
    T *d = (T *)h;
    d->release();                              // (while T's buffer pointers are alive)
    delete d;
    return 0;
}

// The argument checks every ak_*_forward_lens makes after its handle check, in their order, under the entry point's name `fn`:
// pointers and strides; the family's pooling rule (pooling_error: what `fn` says about a pooling it refuses, NULL when it is fine);
// S a positive multiple of 32 up to max_S and up to the rotary tables' n_pos; max_B != 0: at most that many rows (a grid dimension
// of the attention and pooling launches).
int check_forward_lens(const char *fn, const void *ids, const void *lens, const void *out, int ld_ids, int lens_stride, int B, int S, int max_S,
                       int n_pos, const char *pooling_error, int max_B);

}  // namespace ak
