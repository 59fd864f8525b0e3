// attn_causal.hip -- causal grouped-query flash attention at head dim 128 (the decoder's attention, decoder.hip):
//   ctx[t][h * 128 + d] = sum_{s' <= s} softmax_s'(q_h[s] . k_g[s']) v_g[s'][d],   g = h / (nq / nkv)
// q arrives pre-scaled by log2(e) / sqrt(128) (decoder.hip k_dec_qk_rope). The per-key-block algorithm is flash_tile.h's; this file's own:
//
// Layouts (decoder.hip writes them): q [B][nq][S][128], k and v [B][nkv][S][128] bf16; ctx [T][nq * 128] bf16 (the out-projection's
// A operand). Rows are right-padded; lens[b] is the row's length, clamped to [0, S] by the embedding kernel.
//
// Workgroup = (query block, kv head, sequence) and holds every query head of the group: wave w computes query head g = w % G of the
// group for the 32 query rows q0 = (block) * QR + 32 (w / G), QR = 32 R, R = rows_per_group(G): four waves per workgroup for G = 1, 2, 4,
// three for G = 3 (G <= 4: 256 threads, so that the compiler may give a lane the registers the kernel needs -- at 1024 threads it spilled 34).
// Staging: each 32-key block of K and V is staged into ONE LDS buffer inside the loop, once for all G heads and R row blocks; V arrives
// key-major and is transposed on the way (a 2-byte scatter into the V^T tile).
// Mask: key blocks above a wave's diagonal are not computed (the workgroup stages up to its last wave's diagonal); inside the diagonal
// block keys past the query are masked. The first block always holds a visible key (key 0), so the softmax step runs without its -inf
// guard. Query blocks wholly past the row's length are not computed: their context rows are zero (finite, and nothing valid reads
// them: a valid query never sees a pad key under the causal mask).
#include "flash_tile.h"

namespace ak {
using namespace ft;

namespace {
constexpr int CA_HD = 128;
using Tile = FlashTile<CA_HD>;

__global__ __launch_bounds__(256) void k_attn_causal(CausalAttnArgs a) {
    __shared__ __attribute__((aligned(16))) char sK[Tile::K_BYTES];
    __shared__ __attribute__((aligned(16))) char sV[Tile::V_BYTES];
    const int G = a.nq / a.nkv, R = rows_per_group(G), QR = 32 * R;
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
    if (q0 < S && !live) Tile::zero_row(ctx_row, kh);          // wholly past the length
    if (q_begin >= len) return;                                // (uniform over the workgroup: no barrier below is skipped by some waves only)
    // key blocks the workgroup stages: up to the diagonal of its last row block, and not past the row's length
    int q_end = q_begin + QR;
    if (q_end > S) q_end = S;
    const int kb_stop = min((q_end + 31) / 32, (len + 31) / 32);
    const int kb_diag = q0 / 32;

    uint4 qf[Tile::NC];
    if (live) Tile::load_q(qf, a.q + (((int64_t)b * a.nq + h) * S + q0 + r) * CA_HD, kh);
    f32x16 o[Tile::NDB];
#pragma unroll
    for (int i = 0; i < Tile::NDB; i++) o[i] = zero16();
    float m = -INFINITY, l = 0.f;
    const uint16_t *kbase = a.k + ((int64_t)b * a.nkv + kvh) * S * CA_HD;
    const uint16_t *vbase = a.v + ((int64_t)b * a.nkv + kvh) * S * CA_HD;

    for (int kb = 0; kb < kb_stop; kb++) {
        __syncthreads();                                       // every wave is done with the previous tile
        // stage K (row-major, swizzled chunks) and V^T (keys in vt_pos order inside each 16-group)
        for (int i = tid; i < 32 * 16; i += nthr) {
            const int key = i >> 4, c = i & 15;
            const uint4 kv = *(const uint4 *)(kbase + (int64_t)(kb * 32 + key) * CA_HD + c * 8);
            *(uint4 *)(sK + Tile::k_off(key, c)) = kv;
            const uint4 vv = *(const uint4 *)(vbase + (int64_t)(kb * 32 + key) * CA_HD + c * 8);
            const int p = vt_pos(key);
            const uint32_t w[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int d = c * 8 + e;
                const uint16_t val = (uint16_t)(w[e >> 1] >> ((e & 1) * 16));
                *(uint16_t *)(sV + Tile::v_off(d, p >> 3) + (p & 7) * 2) = val;
            }
        }
        __syncthreads();
        if (!live || kb > kb_diag) continue;
        f32x16 s = Tile::scores(sK, qf, r, kh);
        if (kb == kb_diag) {                                   // causal mask inside the diagonal block (key > query)
#pragma unroll
            for (int i = 0; i < 16; i++)
                if (Tile::acc_row(i, kh) > r) s[i] = -INFINITY;
        }
        float alpha;
        s = Tile::softmax_step<false>(s, m, l, alpha);       // key kb * 32 <= every query of a block at or below the diagonal
#pragma unroll
        for (int db = 0; db < Tile::NDB; db++) o[db] = o[db] * alpha;
        uint4 pb[2];
        Tile::pack_p(s, pb);
#pragma unroll
        for (int db = 0; db < Tile::NDB; db++) o[db] = Tile::pv(sV, pb, o[db], db, r, kh);
    }
    if (!live) return;
    const float inv = 1.0f / (l + __shfl_xor(l, 32));
#pragma unroll
    for (int db = 0; db < Tile::NDB; db++) Tile::store_ctx(ctx_row, o[db], db, kh, [&](float x) { return x * inv; });
}
}  // namespace

bool attn_causal_supported(int nq, int nkv, int head_dim, int S) {
    if (head_dim != CA_HD || nkv <= 0 || nq % nkv) return false;
    const int G = nq / nkv, R = rows_per_group(G);
    return G * R <= 4 && S % 32 == 0 && S > 0 && S <= 8192;
}

int launch_attn_causal(const CausalAttnArgs &a, hipStream_t st) {
    if (!attn_causal_supported(a.nq, a.nkv, CA_HD, a.S)) AK_FAIL(-1, "attn_causal: unsupported head layout or sequence length");
    const int G = a.nq / a.nkv, R = rows_per_group(G), QR = 32 * R;
    const dim3 grid((a.S + QR - 1) / QR, a.nkv, a.B);
    k_attn_causal<<<grid, 64 * G * R, 0, st>>>(a);
    AK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ak
