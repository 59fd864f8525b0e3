// attn_long_body.h -- the body of the long-row attention kernels of attn_long.hip (which documents it), included once per kernel with
// the compile-time constants WIN (the band) and BIAS (T5's relative bias) and the argument block `a` in scope. No include guard.
static_assert(!(WIN && BIAS), "the biased kernel walks every key block");
    __shared__ __attribute__((aligned(16))) char sK[2][Tile::K_BYTES];
    __shared__ __attribute__((aligned(16))) char sV[2][Tile::V_BYTES];
    __shared__ float sM[2][32];
    const int h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S, H = a.H;
    const int len = min(max(a.rowlen[b], 0), S);
    const int q_begin = blockIdx.x * AL_QB, q0 = q_begin + 32 * wave;
    const int r = lane & 31, kh = lane >> 5;
    const int64_t row0 = (int64_t)b * S;
    const bool has_q = q0 < S;                                 // this wave's 32 rows exist (S % 32 == 0)
    if (q_begin >= len) {                                      // wholly past the length (uniform): zero context rows
        if (has_q) Tile::zero_row(a.ctx + (row0 + q0 + r) * H + h * AL_HD, kh);
        return;
    }
    int kb_stop = (len + 31) / 32, kb_start = 0;
    if constexpr (WIN) {
        kb_start = max(q_begin - a.window, 0) / 32;            // q_begin < len: block q_begin / 32 is inside [kb_start, kb_stop)
        kb_stop = min(kb_stop, (q_begin + AL_QB - 1 + a.window) / 32 + 1);
    }
    // staging assignment: thread tid moves K chunk (key tid / 8, chunk tid % 8) and V^T chunk (row d = tid / 4, chunk tid % 4)
    const int k_key = tid >> 3, k_c = tid & 7, v_d = tid >> 2, v_c = tid & 3;
    const uint16_t *kg = a.k + row0 * H + (int64_t)h * a.qk_hs + (int64_t)k_key * a.qk_ld + k_c * 8;
    const int c0 = kb_start & 1;                               // LDS buffer of the first block (buffers go by block parity)
    const uint16_t *vg = a.vt + ((int64_t)b * H + h * AL_HD + v_d) * S + v_c * 8;
    const int k_dst = Tile::k_off(k_key, k_c), v_dst = Tile::v_off(v_d, v_c);
    uint4 kreg = *(const uint4 *)(kg + (int64_t)kb_start * 32 * a.qk_ld), vreg = *(const uint4 *)(vg + kb_start * 32);
    float mreg = tid < 32 ? (a.mask[row0 + kb_start * 32 + tid] ? 0.f : -INFINITY) : 0.f;
    *(uint4 *)(sK[c0] + k_dst) = kreg;
    *(uint4 *)(sV[c0] + v_dst) = vreg;
    if (tid < 32) sM[c0][tid] = mreg;
    [[maybe_unused]] float *sB = nullptr;
    [[maybe_unused]] int D = 0;
    if constexpr (BIAS) {                                      // the head's table -> LDS; the barrier in front of the block loop covers it
        sB = rbias_lds();
        D = a.rbias_D;
        const float *tab = a.rbias + (int64_t)h * (2 * D + 1);
        for (int j = tid; j <= 2 * D + 2 * RB_PAD; j += 256) sB[j] = tab[min(max(j - RB_PAD, 0), 2 * D)];
    }

    uint4 qf[Tile::NC];
    Tile::load_q(qf, a.q + row0 * H + (int64_t)h * a.qk_hs + (int64_t)(has_q ? q0 + r : S - 1) * a.qk_ld, kh);
    f32x16 o[Tile::NDB];
#pragma unroll
    for (int i = 0; i < Tile::NDB; i++) o[i] = zero16();
    float m = -INFINITY, l = 0.f;
    __syncthreads();
    for (int kb = kb_start; kb < kb_stop; kb++) {
        const int cur = kb & 1;
        const bool more = kb + 1 < kb_stop;
        if (more) {                                            // next block into registers: in flight under this block's MFMAs
            kreg = *(const uint4 *)(kg + (int64_t)(kb + 1) * 32 * a.qk_ld);
            vreg = *(const uint4 *)(vg + (kb + 1) * 32);
            if (tid < 32) mreg = a.mask[row0 + (kb + 1) * 32 + tid] ? 0.f : -INFINITY;
        }
        const Band band = WIN ? band_of(kb, q0, a.window) : BAND_IN;       // the block against this wave's queries (wave-uniform)
        if (has_q && band != BAND_OUT) {
            f32x16 s = Tile::scores(sK[cur], qf, r, kh);
            if constexpr (BIAS) {
                // the lane's table index of the block's first key, clamped into the padded table: a lane wholly beyond -D - RB_PAD or
                // D + RB_PAD reads 32 copies of the end entry, which is what the clamp gives each of its pairs
                const float *bq = sB + (min(max(kb * 32 - (q0 + r) + D + RB_PAD, 0), 2 * D + RB_PAD) + 4 * kh);
#pragma unroll
                for (int i = 0; i < 16; i++) s[i] += bq[8 * (i >> 2) + (i & 3)];      // + Tile::acc_row(i, kh), its 4 kh in bq
            }
#pragma unroll
            for (int i = 0; i < 16; i++) s[i] += sM[cur][Tile::acc_row(i, kh)];
            if (WIN && band == BAND_EDGE) {                    // the band, per (query r, key) pair
                const int dq = kb * 32 - (q0 + r);             // key - query of the block's first key
#pragma unroll
                for (int i = 0; i < 16; i++)
                    if (band_hides(dq + Tile::acc_row(i, kh), a.window)) s[i] = -INFINITY;
            }
            float alpha;
            s = Tile::softmax_step<true>(s, m, l, alpha);
#pragma unroll
            for (int db = 0; db < Tile::NDB; db++) o[db] = o[db] * alpha;
            uint4 pb[2];
            Tile::pack_p(s, pb);
#pragma unroll
            for (int db = 0; db < Tile::NDB; db++) o[db] = Tile::pv(sV[cur], pb, o[db], db, r, kh);
        }
        if (more) {                                            // the other buffer: its last readers passed the previous barrier
            *(uint4 *)(sK[cur ^ 1] + k_dst) = kreg;
            *(uint4 *)(sV[cur ^ 1] + v_dst) = vreg;
            if (tid < 32) sM[cur ^ 1][tid] = mreg;
        }
        __syncthreads();
    }
    if (!has_q) return;
    const float lt = l + __shfl_xor(l, 32);
    const float inv = lt > 0.f ? 1.0f / lt : 0.f;
    uint16_t *crow = a.ctx + (row0 + q0 + r) * H + h * AL_HD;
#pragma unroll
    for (int db = 0; db < Tile::NDB; db++) Tile::store_ctx(crow, o[db], db, kh, [&](float x) { return x * inv; });
