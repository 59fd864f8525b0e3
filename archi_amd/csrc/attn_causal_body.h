// attn_causal_body.h -- the kernel of attn_causal.hip, which includes this file once per kernel it defines (inside its namespace, behind
// CA_HD and Tile): AK_CAUSAL_KERNEL names the kernel, AK_CAUSAL_VIS its visibility: 0 causal, 1 causal + sliding window, 2 bidirectional
// (every key below the row's length). Three kernels of one text rather than instantiations of a template or callers of an inlined body: k_attn_causal keeps its name and, compiled as a plain
// kernel, the register allocation it had before the band existed (153 VGPRs; through an inlined body: 154). No include guard on purpose.
// AK_CAUSAL_SPLIT (k_attn_causal_gs, k_attn_bidir_gs: 5 to 8 query heads per kv head, Qwen2): the group's G heads are split over
// P = ceil(G / 4) workgroups of GP = ceil(G / P) waves, blockIdx.y = kvh * P + part, one 32-row query block per workgroup; wave w of
// part p computes head p * GP + w of the group. The last part of G = 5 and G = 7 has one wave more than heads: that wave owns no
// head -- it stages and meets every barrier, loads no q and stores nothing. Both split kernels store zeros for every query at or past
// the length (k_attn_causal leaves those of a live row block finite but unspecified). Without the macro the text below is what it was.
__global__ __launch_bounds__(256) void AK_CAUSAL_KERNEL(CausalAttnArgs a) {
    constexpr bool BAND = AK_CAUSAL_VIS == 1, BIDIR = AK_CAUSAL_VIS == 2;
    __shared__ __attribute__((aligned(16))) char sK[Tile::K_BYTES];
    __shared__ __attribute__((aligned(16))) char sV[Tile::V_BYTES];
#if AK_CAUSAL_SPLIT
    const int G = a.nq / a.nkv, P = (G + 3) / 4, GP = (G + P - 1) / P, QR = 32;
    const int kvh = blockIdx.y / P, part = blockIdx.y % P, b = blockIdx.z;
#else
    const int G = a.nq / a.nkv, R = rows_per_group(G), QR = 32 * R;
    const int kvh = blockIdx.y, b = blockIdx.z;
#endif
    const int qblk = gridDim.x - 1 - blockIdx.x;              // the longest causal rows first
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#if AK_CAUSAL_SPLIT
    const int g = part * GP + wave, j = 0;
    const bool owns = g < G;                                   // false: the surplus wave of the last part
    const int h = kvh * G + (owns ? g : G - 1);                // (a surplus wave's addresses stay inside its own group; it uses none of them)
#else
    const int g = wave % G, j = wave / G, h = kvh * G + g;
#endif
    const int S = a.S, len = a.lens[b];
    const int q_begin = qblk * QR, q0 = q_begin + 32 * j;
    const int r = lane & 31, kh = lane >> 5;
    const int ldc = a.nq * CA_HD;
    uint16_t *ctx_row = a.ctx + ((int64_t)b * S + q0 + r) * ldc + h * CA_HD;
#if AK_CAUSAL_SPLIT
    const bool live = owns && q0 < S && q0 < len;              // this wave has a head and its 32 rows hold a valid query
    if (owns && q0 < S && !live) Tile::zero_row(ctx_row, kh);  // wholly past the length
#else
    const bool live = q0 < S && q0 < len;                      // this wave's 32 rows hold a valid query
    if (q0 < S && !live) Tile::zero_row(ctx_row, kh);          // wholly past the length
#endif
    if (q_begin >= len) return;                                // (uniform over the workgroup: no barrier below is skipped by some waves only)
    // key blocks the workgroup stages: up to the diagonal of its last row block, and not past the row's length
    int q_end = q_begin + QR;
    if (q_end > S) q_end = S;
    const int kb_stop = BIDIR ? (len + 31) / 32 : min((q_end + 31) / 32, (len + 31) / 32);      // BIDIR: every block that holds a key below the length
    const int kb_diag = q0 / 32;
    const int W = a.window - 1;                                // BAND: the half-width
    const int kb_start = BAND ? max(q_begin - W, 0) / 32 : 0;  // the lowest band edge of the workgroup's waves

    uint4 qf[Tile::NC];
    if (live) Tile::load_q(qf, a.q + (((int64_t)b * a.nq + h) * S + q0 + r) * CA_HD, kh);
    f32x16 o[Tile::NDB];
#pragma unroll
    for (int i = 0; i < Tile::NDB; i++) o[i] = zero16();
    float m = -INFINITY, l = 0.f;
    const uint16_t *kbase = a.k + ((int64_t)b * a.nkv + kvh) * S * CA_HD;
    const uint16_t *vbase = a.v + ((int64_t)b * a.nkv + kvh) * S * CA_HD;

    for (int kb = kb_start; kb < kb_stop; kb++) {
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
        if (!live || (!BIDIR && kb > kb_diag)) continue;
        Band band = BAND_IN;
        if constexpr (BAND) {
            band = band_of(kb, q0, W);
            if (band == BAND_OUT) continue;
        }
        f32x16 s = Tile::scores(sK, qf, r, kh);
        if constexpr (BAND) {
            if (kb == kb_diag || band == BAND_EDGE) {          // the diagonal and the band's lower edge, per pair
                const int dk0 = kb * 32 - q0 - r;              // key - query of the block's key 0
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int dk = dk0 + Tile::acc_row(i, kh);
                    if ((dk > 0) | band_hides(dk, W)) s[i] = -INFINITY;
                }
            }
        } else if constexpr (BIDIR) {
            if (kb * 32 + 32 > len) {                          // pad keys inside the last partial block (key 0 of block 0 is below the length)
#pragma unroll
                for (int i = 0; i < 16; i++)
                    if (kb * 32 + Tile::acc_row(i, kh) >= len) s[i] = -INFINITY;
            }
        } else if (kb == kb_diag) {                            // causal mask inside the diagonal block (key > query)
#pragma unroll
            for (int i = 0; i < 16; i++)
                if (Tile::acc_row(i, kh) > r) s[i] = -INFINITY;
        }
        float alpha;
        // no band: key kb * 32 <= every query of a block at or below the diagonal, so no guard. BAND: see the head of the file
        s = Tile::softmax_step<BAND>(s, m, l, alpha);
#pragma unroll
        for (int db = 0; db < Tile::NDB; db++) o[db] = o[db] * alpha;
        uint4 pb[2];
        Tile::pack_p(s, pb);
#pragma unroll
        for (int db = 0; db < Tile::NDB; db++) o[db] = Tile::pv(sV, pb, o[db], db, r, kh);
    }
    if (!live) return;
    float inv = 1.0f / (l + __shfl_xor(l, 32));
#if AK_CAUSAL_SPLIT
    if (q0 + r >= len) inv = 0.f;                                         // a query past the length: o is finite, the row is stored as zeros (causal too)
#else
    if ((BAND || BIDIR) && q0 + r >= len) inv = 0.f;                      // a query past the length: o is finite, the row is stored as zeros
#endif
#pragma unroll
    for (int db = 0; db < Tile::NDB; db++) Tile::store_ctx(ctx_row, o[db], db, kh, [&](float x) { return x * inv; });
}
