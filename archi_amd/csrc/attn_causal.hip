// attn_causal.hip -- causal grouped-query flash attention at head dim 128 (the decoder's attention, decoder.hip):
//   ctx[t][h * 128 + d] = sum_{s' <= s} softmax_s'(q_h[s] . k_g[s']) v_g[s'][d],   g = h / (nq / nkv)
// q arrives pre-scaled by log2(e) / sqrt(128) (decoder.hip k_dec_qk_rope), so the softmax runs in the base-2 domain on v_exp_f32.
//
// Layouts (decoder.hip writes them): q [B][nq][S][128], k and v [B][nkv][S][128] bf16; ctx [T][nq * 128] bf16 (the out-projection's
// A operand). Rows are right-padded; lens[b] is the row's length, clamped to [0, S] by the embedding kernel.
//
// Workgroup = (query block, kv head, sequence) and holds every query head of the group: wave w computes query head g = w % G of the
// group for the 32 query rows q0 = (block) * QR + 32 (w / G), QR = 32 R, R = max(1, 4 / G): four waves per workgroup for G = 1, 2, 4
// (G <= 4: 256 threads, so that the compiler may give a lane the registers the kernel needs -- at 1024 threads it spilled 34).
// Each 32-key block of K and V is staged into LDS ONCE for all G heads and R row blocks. Per wave and key block:
//   S^T = K Q^T    8 x v_mfma_f32_32x32x16_bf16: A = K (rows = keys, from LDS), B = Q^T (columns = queries, 32 VGPRs held for the
//                  whole loop). A lane owns ONE query column and 16 of the 32 keys; the other 16 are in lane ^ 32, so the row max
//                  and the row sum take one cross-lane step each.
//   O^T += V^T P^T 8 MFMAs: A = V^T (rows = d, staged transposed with the keys of each 16-group in vt_pos order), B = P^T straight
//                  from the S^T accumulators (the lane's 16 keys are exactly the two k-steps' B operands in vt_pos order).
// Key blocks above a wave's diagonal are not computed (the workgroup stages up to its last wave's diagonal); inside the diagonal
// block keys past the query are masked. Query blocks wholly past the row's length are not computed: their context rows are zero
// (finite, and nothing valid reads them: a valid query never sees a pad key under the causal mask).
#include "encoder_kernels.h"
#include "mfma_tile.h"

namespace ak {
using namespace mt;

namespace {
constexpr int CA_HD = 128;
// K tile [32 keys][128 d]: 256-byte rows, 16-byte chunk c of key r stored at chunk c ^ (r & 7) (the 8 lanes of a ds_read_b128 phase
// read 8 keys' same chunk: 8 distinct bank groups). V^T tile [128 d][32 keys]: 64-byte rows, chunk c of row d at c ^ ((d >> 1) & 3).
constexpr int CA_K_BYTES = 32 * 256, CA_V_BYTES = 128 * 64;

__global__ __launch_bounds__(256) void k_attn_causal(CausalAttnArgs a) {
    __shared__ __attribute__((aligned(16))) char sK[CA_K_BYTES];
    __shared__ __attribute__((aligned(16))) char sV[CA_V_BYTES];
    const int G = a.nq / a.nkv, R = G >= 4 ? 1 : 4 / G, QR = 32 * R;
    const int kvh = blockIdx.y, b = blockIdx.z;
    const int qblk = gridDim.x - 1 - blockIdx.x;              // the longest causal rows first
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = wave % G, j = wave / G, h = kvh * G + g;
    const int S = a.S, len = a.lens[b];
    const int q_begin = qblk * QR, q0 = q_begin + 32 * j;
    const int r = lane & 31, kh = lane >> 5;
    const int ldc = a.nq * CA_HD;
    uint16_t *ctx_row = a.ctx + ((int64_t)b * S + q0 + r) * ldc + h * CA_HD;
    const bool live = q0 < S && q0 < len;                      // this wave's 32 rows hold a valid query
    if (q0 < S && !live) {                                     // wholly past the length: zero rows
        for (int c = kh; c < CA_HD / 8; c += 2) *(uint4 *)(ctx_row + c * 8) = uint4{0, 0, 0, 0};
    }
    if (q_begin >= len) return;                                // (uniform over the workgroup: no barrier below is skipped by some waves only)
    // key blocks the workgroup stages: up to the diagonal of its last row block, and not past the row's length
    int q_end = q_begin + QR;
    if (q_end > S) q_end = S;
    const int kb_stop = min((q_end + 31) / 32, (len + 31) / 32);
    const int kb_diag = q0 / 32;

    // this lane's query: 8 chunks of 16 bytes (d = 16 c + 8 kh .. + 7), the B operand of every S^T MFMA
    uint4 qf[8];
    if (live) {
        const uint16_t *qrow = a.q + (((int64_t)b * a.nq + h) * S + q0 + r) * CA_HD + kh * 8;
#pragma unroll
        for (int c = 0; c < 8; c++) qf[c] = *(const uint4 *)(qrow + c * 16);
    }
    f32x16 o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    const uint16_t *kbase = a.k + ((int64_t)b * a.nkv + kvh) * S * CA_HD;
    const uint16_t *vbase = a.v + ((int64_t)b * a.nkv + kvh) * S * CA_HD;

    for (int kb = 0; kb < kb_stop; kb++) {
        __syncthreads();                                       // every wave is done with the previous tile
        // stage K (row-major, swizzled chunks) and V^T (keys in vt_pos order inside each 16-group)
        for (int i = tid; i < 32 * 16; i += nthr) {
            const int key = i >> 4, c = i & 15;
            const uint4 kv = *(const uint4 *)(kbase + (int64_t)(kb * 32 + key) * CA_HD + c * 8);
            *(uint4 *)(sK + key * 256 + ((c ^ (key & 7)) << 4)) = kv;
            const uint4 vv = *(const uint4 *)(vbase + (int64_t)(kb * 32 + key) * CA_HD + c * 8);
            const int p = vt_pos(key);
            const uint32_t w[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int d = c * 8 + e;
                const uint16_t val = (uint16_t)(w[e >> 1] >> ((e & 1) * 16));
                *(uint16_t *)(sV + d * 64 + ((((p >> 3) ^ ((d >> 1) & 3))) << 4) + (p & 7) * 2) = val;
            }
        }
        __syncthreads();
        if (!live || kb > kb_diag) continue;
        // S^T block: rows = keys kb * 32 + 8 (i / 4) + 4 kh + i % 4 (i = accumulator index), column = this lane's query
        f32x16 s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const uint4 ka = *(const uint4 *)(sK + r * 256 + (((2 * c + kh) ^ (r & 7)) << 4));
            s = mfma_bf16(ka, qf[c], s);
        }
        if (kb == kb_diag) {                                   // causal mask inside the diagonal block (key > query)
#pragma unroll
            for (int i = 0; i < 16; i++)
                if (8 * (i >> 2) + 4 * kh + (i & 3) > r) s[i] = -INFINITY;
        }
        float mb = s[0];
#pragma unroll
        for (int i = 1; i < 16; i++) mb = fmaxf(mb, s[i]);
        mb = fmaxf(mb, __shfl_xor(mb, 32));
        const float mn = fmaxf(m, mb);                         // finite: key kb * 32 <= every query of a block at or below the diagonal
        const float alpha = exp2f(m - mn);
        m = mn;
        float ps = 0.f;
#pragma unroll
        for (int i = 0; i < 16; i++) { s[i] = exp2f(s[i] - mn); ps += s[i]; }
        l = l * alpha + ps;
#pragma unroll
        for (int db = 0; db < 4; db++) o[db] = o[db] * alpha;
        // P^T as the B operand: k-step t takes accumulators 8 t .. 8 t + 7 (keys 16 t + 4 kh + {0-3, 8-11})
        uint4 pb[2];
#pragma unroll
        for (int t = 0; t < 2; t++)
            pb[t] = uint4{pack_bf16x2(s[8 * t + 0], s[8 * t + 1]), pack_bf16x2(s[8 * t + 2], s[8 * t + 3]),
                          pack_bf16x2(s[8 * t + 4], s[8 * t + 5]), pack_bf16x2(s[8 * t + 6], s[8 * t + 7])};
#pragma unroll
        for (int db = 0; db < 4; db++) {
            const int d = db * 32 + r;
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const uint4 va = *(const uint4 *)(sV + d * 64 + (((2 * t + kh) ^ ((d >> 1) & 3)) << 4));
                o[db] = mfma_bf16(va, pb[t], o[db]);
            }
        }
    }
    if (!live) return;
    const float inv = 1.0f / (l + __shfl_xor(l, 32));
    // O^T accumulators: d = 32 db + 8 (i / 4) + 4 kh + i % 4 of this lane's query: four consecutive d per 8-byte store
#pragma unroll
    for (int db = 0; db < 4; db++)
#pragma unroll
        for (int gq = 0; gq < 4; gq++) {
            const int d = db * 32 + 8 * gq + 4 * kh;
            *(uint2 *)(ctx_row + d) = uint2{pack_bf16x2(o[db][4 * gq + 0] * inv, o[db][4 * gq + 1] * inv),
                                            pack_bf16x2(o[db][4 * gq + 2] * inv, o[db][4 * gq + 3] * inv)};
        }
}
}  // namespace

bool attn_causal_supported(int nq, int nkv, int head_dim, int S) {
    if (head_dim != CA_HD || nkv <= 0 || nq % nkv) return false;
    const int G = nq / nkv, R = G >= 4 ? 1 : 4 / G;
    return G * R <= 4 && S % 32 == 0 && S > 0 && S <= 8192;
}

int launch_attn_causal(const CausalAttnArgs &a, hipStream_t st) {
    if (!attn_causal_supported(a.nq, a.nkv, CA_HD, a.S)) AK_FAIL(-1, "attn_causal: unsupported head layout or sequence length");
    const int G = a.nq / a.nkv, R = G >= 4 ? 1 : 4 / G, QR = 32 * R;
    const dim3 grid((a.S + QR - 1) / QR, a.nkv, a.B);
    k_attn_causal<<<grid, 64 * G * R, 0, st>>>(a);
    AK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ak
