// scan.hip -- the hot kernel: query x corpus similarity as a 16-bit MFMA GEMM
// with LDS-staged tiles and a fused top-k' candidate filter, followed by an
// exact re-rank in the reference arithmetic (exact.hip) and a certificate.
//
// Replaces, for the common case, the sequential scan + top-N heapsort that one
// Postgres backend runs for
//   SELECT ... c.embedding <op> %s::vector AS distance ... ORDER BY distance LIMIT k
// (/root/reference/src/data_manager/vectorstore/postgres_vectorstore.py:317-332).
//
// Structure (gfx950, wave64) -- DESIGN.md sections 3 and 4 have the full account:
//   grid   = nslices x nqg persistent workgroups; block b -> XCD b%8, and the nqg query groups of one corpus
//            slice get consecutive slots on ONE XCD, so the slice is read from HBM once and re-read from that L2.
//   tile   = ScanCfg: 256 corpus rows x {32,64,128,256} queries (8 or 4 waves), K-step 64 (128 B per row), a 2- or
//            3-slot LDS ring filled by global_load_lds (16 B/lane; the 1 KiB wave piece is 8 rows x 128 B ->
//            full-line coalesced reads). LDS rows are XOR-swizzled on the SOURCE address (chunk ^= (row>>1)&7) so
//            the ds_read_b128 fragment reads are bank-conflict free.
//   mfma   = v_mfma_f32_32x32x16_{bf16,f16}; A = corpus rows, B = queries, so a lane owns ONE query column (lane&31)
//            and 16 corpus rows per 32x32 block: the top-k reduction axis is lane-local. The phased tiles also exist on
//            v_mfma_f32_16x16x32 (ScanCfg::MFMA = 16: a lane owns two columns and 8 rows per 32x32 block; same LDS image, phases
//            and output tile per wave) -- the chip holds a higher clock on that shape; the 256 x 256 tile ships on it.
//   filter = per 16-row group an upper bound from precomputed per-block maxima; groups that can reach the query's
//            threshold are scored exactly and appended to a per-(block,query) buffer in global memory (L2 resident)
//            with an LDS counter, threshold and trigger. A wave compacts a buffer that nears capacity to
//            (k-th best - 3 eps) and above (bitwise binary search over 64-bit keys with ballots).
//   passes = pre-seeding (SEED variant: group maxima over a strided sample) -> seeding pass (3% of the rows, 12% on small shards) ->
//            main pass; thresholds flow from one to the next.
//   output = [nq][slots][k'] keys (score key << 32 | row slot) + each workgroup's final threshold
// then: select top-k' per query -> re-rank k' candidates in reference arithmetic -> top-k + certificate (the k-th exact
// score beats every non-candidate's upper bound), else the caller falls back to the exact path.
// This file: the kernels, then the host side that launches them. Which tile runs, how a search is sliced and where its
// buffers lie in the workspace is host-only arithmetic in scan_plan.h (tile types and table, pick_cfg, scan_plan, ScanWorkspace).
#include <atomic>
#include "index.h"
#include "scan_plan.h"
#include "switches.h"
#include "mfma_tile.h"

#include <type_traits>

namespace ak {
using namespace mt;

// Candidate entries are written by other waves of the same workgroup (plain stores, then
// vmcnt(0) + barrier) and must not be served from a stale L1 line: non-temporal loads bypass the
// vector L1 (L2-served) and, unlike __hip_atomic_load, stay ordinary loads the compiler pipelines.
__device__ inline uint64_t ld_sc1(const uint64_t *p) { return __builtin_nontemporal_load(p); }

// k-th smallest of the keys held by one wave (key[j] of lane l = entry j*64+l; KEY_INVALID pads).
// v_max3_f32 without the operand canonicalisation hipcc puts in front of fmaxf in IEEE mode (scan filter, tile_epilogue)
__device__ inline float max3f(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ inline float max3z(float a, float b) {      // max(a, b, 0)
    float r;
    asm("v_max3_f32 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// MFMA -> VALU fence for the inline-asm reads above. LLVM's hazard recogniser inserts the wait states between an MFMA and a VALU
// read of its destination only for instructions it can see; the operands of an asm statement are opaque to it (attention.hip
// records a v_max3 that read accumulators before the MFMA had written them). Every accumulator of the wave is tied through this
// one statement ("+v": the MFMAs that write them are ordered before it, every later reader after it), and its s_nops cover the
// longest window -- 18 wait states after a 16-pass MFMA issues -- so the reads no longer depend on how far hipcc happens to
// schedule them from the K-loop. ~20 cycles per 256-row tile, under the partner wave's matrix phase.
template <int N>
__device__ __forceinline__ void mfma_settle(f32x16 (&a)[N]) {
    static_assert(N == 1 || N == 2 || N == 3, "accumulator columns per wave row");
    if constexpr (N == 1) asm volatile("s_nop 15\n\ts_nop 3" : "+v"(a[0]));
    if constexpr (N == 2) asm volatile("s_nop 15\n\ts_nop 3" : "+v"(a[0]), "+v"(a[1]));
    if constexpr (N == 3) asm volatile("s_nop 15\n\ts_nop 3" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]));
}
template <int M, int N>
__device__ __forceinline__ void mfma_settle(f32x16 (&a)[M][N]) {
    static_assert(M == 2 || M == 4, "accumulator rows per wave");
    if constexpr (N == 1 && M == 2) asm volatile("s_nop 15\n\ts_nop 3" : "+v"(a[0][0]), "+v"(a[1][0]));
    else if constexpr (N == 1 && M == 4) asm volatile("s_nop 15\n\ts_nop 3" : "+v"(a[0][0]), "+v"(a[1][0]), "+v"(a[2][0]), "+v"(a[3][0]));
    else if constexpr (N == 2 && M == 2) asm volatile("s_nop 15\n\ts_nop 3" : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[1][0]), "+v"(a[1][1]));
    else if constexpr (N == 2 && M == 4)
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[1][0]), "+v"(a[1][1]), "+v"(a[2][0]), "+v"(a[2][1]),
                     "+v"(a[3][0]), "+v"(a[3][1]));
    else if constexpr (N == 3 && M == 2)
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(a[0][0]), "+v"(a[0][1]), "+v"(a[0][2]), "+v"(a[1][0]), "+v"(a[1][1]), "+v"(a[1][2]));
    else static_assert(M * N == 0, "unsupported accumulator shape");
}

// one 16x16x32 MFMA into slice Q of a 32 x 32 block's accumulator (zero: the block's first MFMA of a corpus tile)
template <bool IS_BF16, int Q>
__device__ __forceinline__ void mfma16_into(f32x16 &d, uint4 a, uint4 b, bool zero) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    acc_set_slice<Q>(d, mfma16<IS_BF16>(a, b, zero ? z : acc_slice<Q>(d)));
}

// ... and its int8 form, v_mfma_i32_16x16x64_i8: twice the K in the same pipe cycles. A lane supplies 16 consecutive bytes of row /
// column l & 15, K-group l >> 4 -- the bytes the 16x16x32 fragment read already fetches -- and receives the same four results. The
// accumulators keep their f32x16 type and hold int32 BITS (a register is a register; nothing but the filter below reads them).
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
template <int Q>
__device__ __forceinline__ void mfma16_i8_into(f32x16 &d, uint4 a, uint4 b, bool zero) {
    const i32x4 z = {0, 0, 0, 0};
    const i32x4 c = zero ? z : __builtin_bit_cast(i32x4, acc_slice<Q>(d));
    acc_set_slice<Q>(d, __builtin_bit_cast(f32x4, __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b), c, 0, 0, 0)));
}

// Bitwise binary search with ballots: 32 steps over the score half of the keys and -- only when
// equal scores straddle the cut -- 32 more over the row half of the tied keys. Needs >= kk valid keys.
template <int NS>
__device__ inline uint64_t kth_key(const uint64_t (&key)[NS], int kk) {
    uint32_t th = 0;
    for (int bit = 31; bit >= 0; bit--) {
        const uint32_t test = th | ((1u << bit) - 1u);
        int c = 0;
#pragma unroll
        for (int j = 0; j < NS; j++) c += __popcll(__ballot((uint32_t)(key[j] >> 32) <= test));
        if (c < kk) th |= (1u << bit);
    }
    int less = 0, eq = 0;
#pragma unroll
    for (int j = 0; j < NS; j++) {
        const uint32_t hi = (uint32_t)(key[j] >> 32);
        less += __popcll(__ballot(hi < th));
        eq += __popcll(__ballot(hi == th));
    }
    const int r = kk - less;          // entries still needed from the tie group (1 <= r <= eq)
    uint32_t tl = 0xffffffffu;
    if (r < eq) {
        tl = 0;
        for (int bit = 31; bit >= 0; bit--) {
            const uint32_t test = tl | ((1u << bit) - 1u);
            int c = 0;
#pragma unroll
            for (int j = 0; j < NS; j++) c += __popcll(__ballot((uint32_t)(key[j] >> 32) == th && (uint32_t)key[j] <= test));
            if (c < r) tl |= (1u << bit);
        }
    }
    return ((uint64_t)th << 32) | tl;
}

// One wave tightens one query's append buffer (m <= NS*64 entries):
//   threshold = (k-th best score in the buffer) - margin     (margin = 3 eps in scan units)
// Any workgroup's k-th best is a lower bound of the global k-th best, so a row whose approximate
// score is below that threshold cannot reach the exact top-k; everything at or above it is kept
// (a variable number >= k, capped at `limit` best). Raises *thr_io, rewrites the buffer compacted
// (or writes the survivors to final_out), sets the next compaction trigger.
template <int NS>
__device__ __noinline__ int compact_impl(uint64_t *buf, int m, int k, int limit, float mar, int lane,
                                          float *thr_io, int *cnt_out, int *trig_out, int trig_max,
                                          uint64_t *final_out /* nullable: write survivors here, pad to limit */) {
    uint64_t key[NS];
#pragma unroll
    for (int j = 0; j < NS; j++) {
        const int idx = j * 64 + lane;
        key[j] = idx < m ? ld_sc1(buf + idx) : KEY_INVALID;
    }
    float thr = *thr_io;
    if (m >= k) {
        const uint64_t tk = kth_key<NS>(key, k);
        const float t = key_score((uint32_t)(tk >> 32)) - mar;
        if (t > thr) thr = t;           // NaN-safe: comparisons with NaN are false
    }
    // survivors: score >= thr  <=>  score key <= key(thr)
    uint64_t cut = ((uint64_t)score_key(thr) << 32) | 0xffffffffull;
    int c = 0;
#pragma unroll
    for (int j = 0; j < NS; j++) c += __popcll(__ballot(key[j] != KEY_INVALID && key[j] <= cut));
    if (c > limit) cut = kth_key<NS>(key, limit);   // near-tie pile-up: keep the `limit` best
    uint64_t *dst = final_out ? final_out : buf;
    int run = 0;
#pragma unroll
    for (int j = 0; j < NS; j++) {
        const bool keep = key[j] != KEY_INVALID && key[j] <= cut;
        const uint64_t mask = __ballot(keep);
        const int pos = run + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep) dst[pos] = key[j];
        run += __popcll(mask);
    }
    if (final_out) {
        for (int i = run + lane; i < limit; i += 64) final_out[i] = KEY_INVALID;
    } else if (lane == 0) {
        *cnt_out = run;
        const int tr = 2 * run > 64 ? 2 * run : 64;
        *trig_out = tr < trig_max ? tr : trig_max;
    }
    if (lane == 0) *thr_io = thr;
    return run;
}

template <int CAP>
__device__ inline int compact_wave(uint64_t *buf, int m, int k, int limit, float mar, int lane, float *thr_io,
                                    int *cnt_out, int *trig_out, int trig_max, uint64_t *final_out) {
    if (m <= 64) return compact_impl<1>(buf, m, k, limit, mar, lane, thr_io, cnt_out, trig_out, trig_max, final_out);
    else if (m <= 128) return compact_impl<2>(buf, m, k, limit, mar, lane, thr_io, cnt_out, trig_out, trig_max, final_out);
    else if (m <= 256) return compact_impl<4>(buf, m, k, limit, mar, lane, thr_io, cnt_out, trig_out, trig_max, final_out);
    else if (CAP >= 512 && m <= 512) return compact_impl<8>(buf, m, k, limit, mar, lane, thr_io, cnt_out, trig_out, trig_max, final_out);
    else return compact_impl<CAP / 64>(buf, m, k, limit, mar, lane, thr_io, cnt_out, trig_out, trig_max, final_out);
}

// rows: [n][D] 16-bit (allocated in whole 256-row tiles: the phased loop reads the rows of a tail tile past n, the
// epilogue masks them); qs: [nq_pad][D] 16-bit (queries rounded to the scan dtype)
// SEED = true is the pre-seeding variant: the same tiles and MFMA loop over a strided sample of the corpus
// (tile j of the sample is corpus tile j*tstride, sample_tiles of them), but instead of filtering and
// appending, every lane keeps the running maximum score of the 16-row groups it owns. Each (workgroup,
// lane group) is a disjoint set of rows, so the k-th largest of those maxima is a lower bound of the k-th
// best score of the whole corpus -- a valid initial threshold that costs one GEMM pass over ~0.2% of the
// rows and no selection. Output: thr_out[q][slice*GPB + g], GPB = WM*MI*2 groups per workgroup.
// INSTR = true is the measurement build (AK_SCAN_DBG phase cycle counters, AK_SCAN_ABLATE bits): the production
// instantiation carries neither -- no s_memtime, no flag tests, none of their registers.
// SEEDPASS only names the launch: the seeding pass over the first ~3 % of the rows runs the very code of the main pass, and with
// the tag rocprofv3 lists the two under their own names (profiles/: main pass = `..., false, false, false>`).
template <bool IS_BF16, class C, bool SEED, bool INSTR, bool SEEDPASS = false>
__global__ __launch_bounds__(C::THREADS, C::MINW) void k_scan(
    const uint16_t *__restrict__ rows, const float *__restrict__ ea, const float *__restrict__ eb,
    const float *__restrict__ gb, int64_t gb_blocks, const uint8_t *__restrict__ filter, int64_t row_begin, int64_t n, int D, const uint16_t *__restrict__ qs, int nq,
    int nslices, int nqg, int k, int kp, const float *__restrict__ thr0, const float *__restrict__ mar,
    int slice_off, int nslices_total, uint64_t *__restrict__ cand, uint64_t *__restrict__ out_c,
    float *__restrict__ thr_out, int flags_arg, long long *__restrict__ dbg_arg, int64_t sample_tiles, int tstride,
    int *__restrict__ dense_cnt, unsigned int *__restrict__ dense_thr) {
    // scans rows [row_begin, n); row_begin is a multiple of BM. thr0 (nullable): per-query initial
    // thresholds in scan-score units (from the seeding pass). Output slot: slice_off + slice.
    constexpr int BM = C::BM, BN = C::BN, NW = C::NW, MI = C::MI, NI = C::NI, NSTAGE = C::NSTAGE, CAP = C::CAP;
    constexpr bool I8 = C::I8;               // int8 shadow rows and int8 queries: K-step 128 elements, int32 accumulator bits
    constexpr int EB = I8 ? 1 : 2;           // bytes per element of rows / qs
    static_assert(!I8 || (C::MFMA == 16 && C::PHASED && !SEED), "the int8 scan is the phased tile on the 16x16 shape; its pre-seeding stays on 16 bits");
    constexpr int FILT_K = SEEDPASS ? C::FILT_SEED : C::FILT;      // filter arrangement of this launch
    constexpr bool M16 = C::MFMA == 16;      // 16x16x32 MFMAs: a lane owns query columns 16c + (lane & 15) and rows 16h + 4 * (lane >> 4) + j
    static_assert(!(M16 && SEED), "the pre-seeding launch runs the 32x32x16 shape (C::Shape32)");
    const int flags = INSTR ? flags_arg : 0;
    long long *const dbg = INSTR ? dbg_arg : nullptr;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *sA = smem;                                   // [NSTAGE][BM][BKB bytes]   (phased: [2 buffers][4 half-tiles][128][128 B])
    char *sB = smem + NSTAGE * C::A_BYTES;             // [NSTAGE][BN][BKB bytes]
    float *s_ea = (float *)(smem + NSTAGE * (C::A_BYTES + C::B_BYTES));
    float *s_eb = s_ea + 2 * BM;                       // s_ea / s_eb / s_gb are double-buffered by tile parity
    float *s_thr = s_eb + 2 * BM;
    int *s_cnt = (int *)(s_thr + BN);
    float *s_mar = (float *)(s_cnt + BN);
    int *s_trig = (int *)(s_mar + BN);
    int *s_need = s_trig + BN;
    float *s_gb = (float *)(s_need + 4);      // [2][64]: [BM/32][4] per-32-row-block bounds of a tile
    long long t_loop = 0, t_epi = 0, t_sync = 0, t_comp = 0, t_fin = 0, t_mark = 0, n_slow = 0, n_comp = 0, n_drain = 0;
    auto TICK = [&]() -> long long {
        if constexpr (INSTR) return dbg ? (long long)__builtin_readcyclecounter() : 0;
        else return 0;
    };

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / C::WN, wc = wave % C::WN;
    // XCD-aware slot mapping: block b runs on XCD b%8; consecutive slots of one XCD
    // walk the query groups of one slice, so the query groups of a slice share an L2.
    const int b = blockIdx.x;
    int slice, qg;
    if ((nslices & 7) == 0) {
        int xcd = b & 7, j = b >> 3;
        qg = j % nqg;
        slice = xcd + 8 * (j / nqg);
    } else {
        qg = b % nqg;
        slice = b / nqg;
    }
    const int64_t tb = row_begin / BM;
    const int64_t ntiles_all = SEED ? sample_tiles : (n + BM - 1) / BM - tb;
    const int64_t t0 = tb + ntiles_all * slice / nslices;
    const int64_t tmul = SEED ? tstride : 1;
    const int ntiles = (int)(tb + ntiles_all * (slice + 1) / nslices - t0);
    constexpr int BKB = C::BKB, CPR = C::CPR, RPP = C::RPP;
    const int KS = D * EB / BKB;
    const int nsteps = ntiles * KS;
    const int q0 = qg * BN;

    for (int i = tid; i < BN; i += C::THREADS) {
        float t = -3.4028234663852886e38f;
        if (thr0 && q0 + i < nq) t = fmaxf(t, thr0[q0 + i]);
        s_thr[i] = (q0 + i < nq) ? t : __builtin_inff();  // padded queries never append
        s_cnt[i] = 0;
        s_mar[i] = (q0 + i < nq) ? mar[q0 + i] : 0.f;
        s_trig[i] = 64 < CAP - 2 * BM ? 64 : CAP - 2 * BM;
    }
    if (tid == 0) *s_need = 0;

    uint64_t *my_cand = cand + ((size_t)blockIdx.x * BN) * CAP;

    // fragment addressing: row r = lane&31, k-half kh = lane>>5, chunk ^= (row>>1)&7
    const int r = lane & 31, kh = lane >> 5;
    auto swz = [](int row) { return (row >> 1) & 7; };
    const int c0 = kh ^ swz(r);
    const uint32_t ldsE = lds_addr(s_ea);
    const int st_row = lane / CPR, st_chunk = lane % CPR;

    f32x16 acc[MI][NI];
    constexpr bool GM_LDS = SEED && C::SEED_GM_LDS;
    float gm[GM_LDS ? 1 : MI][GM_LDS ? 1 : NI];
    float *const s_gmx = (float *)(smem + C::LDS_BYTES) + (size_t)wave * (MI * NI * 64) + lane;      // [wave][mi * NI + ni][lane] (SEED, wide phased tile)
#pragma unroll
    for (int mi = 0; mi < MI; mi++)
#pragma unroll
        for (int ni = 0; ni < NI; ni++) {
            if constexpr (GM_LDS) s_gmx[(mi * NI + ni) * 64] = -__builtin_inff();
            else gm[mi][ni] = -__builtin_inff();
        }

    // per-row epilogue terms of tile t -> LDS buffer of parity t&1 (consumed in that tile's filter, >= 1 barrier and one
    // vmcnt wait of the staging wave later; the other parity may still be read by a wave finishing the previous filter)
    auto stage_terms = [&](int t, int64_t tile_row0) {
        const int par = t & 1;
        float *t_ea = s_ea + par * BM, *t_eb = s_eb + par * BM, *t_gb = s_gb + par * 64;
        if (!filter) {
            if (wave < BM / 64) {
                int64_t grow = tile_row0 + wave * 64 + lane;
                if (grow >= n) grow = n - 1;
                glds4(ea + grow, __builtin_amdgcn_readfirstlane(ldsE + par * BM * 4 + wave * 256));
                glds4(eb + grow, __builtin_amdgcn_readfirstlane(ldsE + (2 + par) * BM * 4 + wave * 256));
            }
            if (wave == NW - 1) {   // 4 floats per 32-row block, BM/32 blocks: lanes beyond that re-read block 0..
                int64_t blk = tile_row0 / 32 + ((lane & 31) >> 2);
                if (blk >= gb_blocks) blk = gb_blocks - 1;
                glds4(gb + blk * 4 + (lane & 3), __builtin_amdgcn_readfirstlane(lds_addr(t_gb)));
            }
        } else {
            for (int i = tid; i < BM; i += C::THREADS) {
                int64_t grow = tile_row0 + i;
                bool ok = grow < n && filter[grow];
                t_ea[i] = ok ? ea[grow] : 0.f;
                t_eb[i] = ok ? eb[grow] : -__builtin_inff();
            }
            if (tid < BM / 8) {
                int64_t blk = tile_row0 / 32 + (tid >> 2);
                if (blk >= gb_blocks) blk = gb_blocks - 1;
                t_gb[tid] = gb[blk * 4 + (tid & 3)];
            }
        }
    };

    // lazy compaction: a request raised while filtering an EARLIER tile is served between two K-loops, after barriers
    // every wave has passed since. The common case costs one LDS read; buffers hold two more tiles of appends beyond
    // the trigger, so waiting a tile is safe.
    auto serve_compaction = [&]() {
        for (int q = wave; q < BN; q += NW) {
            int m = s_cnt[q];
            if (m > s_trig[q]) {
                if constexpr (INSTR) n_comp++;
                compact_wave<CAP>(my_cand + (size_t)q * CAP, m, k, CAP - 2 * BM, s_mar[q], lane, &s_thr[q], &s_cnt[q],
                                  &s_trig[q], CAP - 2 * BM, nullptr);
            }
        }
        wait_vm<0>();
        __syncthreads();
        if (tid == 0) *s_need = 0;
        __syncthreads();
    };

    // fused epilogue of one tile: score = fma(dot, ea[row], eb[row]); append if >= threshold (SEED: group maxima)
    auto tile_epilogue = [&](int t, int64_t tile_row0) {
        const int par = t & 1;
        const float *t_ea = s_ea + par * BM, *t_eb = s_eb + par * BM, *t_gb = s_gb + par * 64;
        const bool tail = tile_row0 + BM > n;          // rows past n: mask them
        const int rows_left = tail ? (int)(n - tile_row0) : BM;      // 32-bit row tests: the 64-bit form kept sixteen lane
        //                                                              addresses (32 registers) live through the K-loop
        if constexpr (SEED) {
#pragma unroll
            for (int mi = 0; mi < MI; mi++) {
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const int base = (wr * MI + mi) * 32 + 8 * g + 4 * kh;
                    float4 e4 = *(const float4 *)&t_ea[base], b4 = *(const float4 *)&t_eb[base];
                    if (tail) {
                        float *pe = (float *)&e4, *pb = (float *)&b4;
#pragma unroll
                        for (int j = 0; j < 4; j++)
                            if (base + j >= rows_left) { pe[j] = 0.f; pb[j] = -__builtin_inff(); }
                    }
#pragma unroll
                    for (int ni = 0; ni < NI; ni++) {
                        const f32x16 &a = acc[mi][ni];
                        float &gmx = GM_LDS ? s_gmx[(mi * NI + ni) * 64] : gm[GM_LDS ? 0 : mi][GM_LDS ? 0 : ni];
                        gmx = fmaxf(fmaxf(gmx, fmaf(a[4 * g + 0], e4.x, b4.x)),
                                    fmaxf(fmaxf(fmaf(a[4 * g + 1], e4.y, b4.y), fmaf(a[4 * g + 2], e4.z, b4.z)),
                                          fmaf(a[4 * g + 3], e4.w, b4.w)));
                    }
                }
                __builtin_amdgcn_sched_barrier(0);   // one 32-row block at a time: hoisting all the term loads spills
            }
            return;
        }
        if (INSTR && (flags & 1)) {   // ablation: keep the accumulators live, skip the filter
#pragma unroll
            for (int mi = 0; mi < MI; mi++)
#pragma unroll
                for (int ni = 0; ni < NI; ni++) keep_live(acc[mi][ni]);
            return;
        }
        if constexpr (M16) {
            // 16x16x32 mapping: slice 2h + c of acc[mi][ni] holds, in element j, corpus row (wr*MI + mi)*32 + 16h + 4kq + j against
            // query (wc*NI + ni)*32 + 16c + r16. A filter group is the 8 rows a lane holds of one 32-row block for one query column
            // (h = 0, 1). All of them have row bit 2 = kq & 1, so they are a subset of the row class whose maxima t_gb keeps
            // (computed at ingest for the 32x32x16 mapping, where the class is kh): the bound holds with no new ingest data, and
            // a group of 8 passes it about half as often as the other shape's group of 16. 4 v_max3_f32 + fma + compare per 8
            // values (12 VALU per 16; the 32x32x16 filter: 10 per 16). Nothing past this point knows the shape: keys carry the
            // row, and the margin of k_query_setup (4 D 2^-24 + the operand rounding) bounds ANY summation order of the dot
            // product, so the candidates' consumers (out_c, thr_slots, dense_cnt, dense_thr: the tails, the certificate) and
            // the certificate itself are unchanged; ids and distances come from the exact re-rank.
            // (the threshold is read per column block inside the loop: 2 * NI of them held across the filter, on top of 128 accumulators
            // and a full register file, made hipcc spill two registers of the 256 x 256 tile)
            // The lane's row / column numbers are rebuilt per tile from an opaque copy of the lane id, so no address derived from them
            // stays live through the K-loop.
            int ln = lane;
            asm volatile("" : "+v"(ln));
            const int r16 = ln & 15, kq = ln >> 4;
            // bound of one filter group (site): max(0, its 8 dot products) -> U = fma(dpos, gea, geb)
            // int8: the group maximum is taken on the integers and only the maximum is converted (|dot| <= 127^2 D < 2^24
            // up to D = 1040 and the conversion is monotone beyond: the bound holds either way); plain integer max, which
            // the compiler sees -- no inline-asm read of accumulators on this path
            auto imax = [](int x, int y) { return x > y ? x : y; };
            auto site_dpos = [&](int mi, int ni, int c) -> float {
                const f32x16 &a = acc[mi][ni];
                const int lo = 4 * c, hi = 8 + 4 * c;     // slices (h = 0, c) and (h = 1, c)
                if constexpr (I8) {
                    const i32x16 ia = __builtin_bit_cast(i32x16, a);
                    return (float)imax(imax(imax(imax(ia[lo], ia[lo + 1]), imax(ia[lo + 2], ia[lo + 3])),
                                            imax(imax(ia[hi], ia[hi + 1]), imax(ia[hi + 2], ia[hi + 3]))), 0);
                } else {
#if AK_DBG_KERNELS
                    return fmaxf(fmaxf(fmaxf(fmaxf(a[lo], a[lo + 1]), fmaxf(a[lo + 2], a[lo + 3])),
                                       fmaxf(fmaxf(a[hi], a[hi + 1]), fmaxf(a[hi + 2], a[hi + 3]))), 0.f);
#else
                    return max3z(max3f(max3f(a[lo], a[lo + 1], a[lo + 2]), max3f(a[lo + 3], a[hi], a[hi + 1]), a[hi + 2]), a[hi + 3]);
#endif
                }
            };
            // per-row terms of the 2 x 4 rows a lane holds of 32-row block mi (the same for every query column), rows past n masked
            auto row_terms = [&](int mi, float4 (&e4)[2], float4 (&b4)[2]) {
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int base = (wr * MI + mi) * 32 + 16 * h + 4 * kq;   // rows base .. base+3 of the tile
                    e4[h] = *(const float4 *)&t_ea[base];
                    b4[h] = *(const float4 *)&t_eb[base];
                    if (tail) {
                        float *pe = (float *)&e4[h], *pb = (float *)&b4[h];
#pragma unroll
                        for (int j = 0; j < 4; j++)
                            if (base + j >= rows_left) { pe[j] = 0.f; pb[j] = -__builtin_inff(); }
                    }
                }
            };
            // exact scores of one site: score = fma(dot, ea[row], eb[row]) of the 8 rows a lane holds for one query column; returns their maximum
            auto site_scores = [&](int mi, int ni, int c, const float4 (&e4s)[2], const float4 (&b4s)[2], float (&sc)[8]) -> float {
                const f32x16 &a = acc[mi][ni];
                const i32x16 ia = __builtin_bit_cast(i32x16, a);
                float mx = -__builtin_inff();
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const float4 e4 = e4s[h], b4 = b4s[h];
                    const int o = 8 * h + 4 * c;
                    const float d0 = I8 ? (float)ia[o + 0] : a[o + 0], d1 = I8 ? (float)ia[o + 1] : a[o + 1],
                                d2 = I8 ? (float)ia[o + 2] : a[o + 2], d3 = I8 ? (float)ia[o + 3] : a[o + 3];
                    sc[4 * h + 0] = fmaf(d0, e4.x, b4.x); sc[4 * h + 1] = fmaf(d1, e4.y, b4.y);
                    sc[4 * h + 2] = fmaf(d2, e4.z, b4.z); sc[4 * h + 3] = fmaf(d3, e4.w, b4.w);
                    mx = fmaxf(fmaxf(mx, sc[4 * h + 0]), fmaxf(fmaxf(sc[4 * h + 1], sc[4 * h + 2]), sc[4 * h + 3]));
                }
                return mx;
            };
            // the lanes of a site that hold a hit: one LDS atomic per lane reserves room for its hits of the group, then the appends
            auto site_append = [&](int mi, int ni, int c, float thr, const float (&sc)[8]) {
                if (INSTR && (flags & 64)) return;      // (ablation bit 64: exact scores, no appends)
                const int qcol = (wc * NI + ni) * 32 + 16 * c + r16;
                int nh = 0;
#pragma unroll
                for (int e = 0; e < 8; e++) nh += sc[e] >= thr ? 1 : 0;
                int pos = atomicAdd(&s_cnt[qcol], nh);
                if (pos + nh > s_trig[qcol]) *s_need = 1;
                uint64_t *dstq = my_cand + (size_t)qcol * CAP;
                const uint32_t rbase = (uint32_t)(tile_row0 + (wr * MI + mi) * 32 + 4 * kq);
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    if (sc[e] >= thr) {
                        dstq[pos] = ((uint64_t)score_key(sc[e]) << 32) | (uint64_t)(rbase + (e & 3) + 16 * (e >> 2));
                        pos++;
                    }
                }
            };
            if constexpr (FILT_K == 2) {
                // Queued. What the other two arrangements pay for is wave divergence: each of the sixteen sites is its own unrolled
                // code over its own accumulator registers, and the wave runs a site's exact scores and appends in full when ONE of
                // its 64 lanes needs them. Here the sixteen bounds come first, branch-free (16 of the whole-tile arrangement's 128
                // conversions and fma). Then, site by site, the lanes that passed are balloted; an empty ballot skips the site on a
                // scalar branch, otherwise each passing lane writes its eight raw dot products and its (site, lane) to slot
                // `queue count + its rank in the ballot` of the wave's own LDS queue. The queue is drained once, after the last
                // site -- lane i takes entry i, gathers the entry's row terms and threshold, and scores and appends as site_scores /
                // site_append do -- or, where a site's entries would not fit in the 64 slots, before that site as well. Nothing
                // stays queued when the tile ends: the terms' parity buffers and the two tiles of append room behind a buffer's
                // trigger stand as they are. A row is appended iff its score reaches the threshold, every lane-site with such a row
                // passes its bound, and s_thr only changes behind barriers: the same keys as the other arrangements, in another
                // order. One copy of the drain's code, behind the straight-line sites in a loop that runs again only for
                // the sites that did not fit.
                static_assert(I8, "the queued filter exists for the int8 tile");
                constexpr int NSITE = 2 * MI * NI, HQS = C::HQ_SLOTS;
                int *const s_hq = (int *)(smem + C::LDS_BYTES - C::HQ_BYTES) + wave * (C::HQ_WORDS * HQS);      // [word][slot]
                float thr_s[NI][2];
#pragma unroll
                for (int ni = 0; ni < NI; ni++)
#pragma unroll
                    for (int c = 0; c < 2; c++) thr_s[ni][c] = s_thr[(wc * NI + ni) * 32 + 16 * c + r16];
                float gea[MI], geb[MI];
#pragma unroll
                for (int mi = 0; mi < MI; mi++) {
                    gea[mi] = t_gb[(wr * MI + mi) * 4 + (kq & 1)];
                    geb[mi] = t_gb[(wr * MI + mi) * 4 + 2 + (kq & 1)];
                }
                // the sixteen bounds, branch-free: a site's compare IS its ballot (an SGPR pair), and the lanes' own bits of it mask the push
                bool pb[NSITE];
                uint64_t bal[NSITE];
#pragma unroll
                for (int S = 0; S < NSITE; S++) {
                    const int mi = S / (2 * NI), ni = (S >> 1) % NI, c = S & 1;
                    pb[S] = fmaf(site_dpos(mi, ni, c), gea[mi], geb[mi]) >= thr_s[ni][c];
                    bal[S] = __builtin_amdgcn_ballot_w64(pb[S]);
                }
                // sites still to queue, a scalar bit each. A round runs the sites of `todo` in order: the ballot's test
                // and the push, until a site's entries do not fit; then the drain, and the sites left over
                // make the next round. Straight-line code with forward scalar branches, one copy of the drain behind it.
                uint32_t todo = (INSTR && (flags & 16)) ? 0u : (1u << NSITE) - 1u;
                int qn = 0;                                  // entries queued: wave-uniform
                auto site = [&](auto S_, uint32_t &open) {
                    constexpr int S = decltype(S_)::value, mi = S / (2 * NI), ni = (S >> 1) % NI, c = S & 1;
                    if (!(open & (1u << S))) return;
                    const bool p = pb[S];
                    const uint64_t b = bal[S];
                    // (scalar copies: the compiler's uniformity analysis loses the ballot through the loop and would run the
                    // sites on vector compares and exec masks)
                    const uint32_t blo = __builtin_amdgcn_readfirstlane((uint32_t)b), bhi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
                    if ((blo | bhi) != 0) {
                        const int cnt = __builtin_popcount(blo) + __builtin_popcount(bhi);
                        if (qn + cnt > HQS) { open = 0; return; }       // this site and those behind it: after the drain
                        if (p) {
                            const int slot = qn + (int)__builtin_amdgcn_mbcnt_hi(bhi, __builtin_amdgcn_mbcnt_lo(blo, 0u));
                            const i32x16 ia = __builtin_bit_cast(i32x16, acc[mi][ni]);
#pragma unroll
                            for (int e = 0; e < 8; e++) s_hq[e * HQS + slot] = ia[8 * (e >> 2) + 4 * c + (e & 3)];
                            s_hq[8 * HQS + slot] = S * 64 + ln;
                        }
                        qn = __builtin_amdgcn_readfirstlane(qn + cnt);
                        if constexpr (INSTR) n_slow += cnt;
                    }
                    todo &= ~(1u << S);
                };
                auto drain = [&]() {
                    if constexpr (INSTR) n_drain++;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // the pushes of other lanes, this wave's
                    __builtin_amdgcn_wave_barrier();
                    if (ln < qn) {
                        const int id = s_hq[8 * HQS + ln];
                        const int site = id >> 6, el = id & 63;
                        const int rb = (wr * MI + site / (2 * NI)) * 32 + 4 * (el >> 4);        // tile-relative row of element 0
                        const int qcol = (wc * NI + (site >> 1) % NI) * 32 + 16 * (site & 1) + (el & 15);
                        const float thr = s_thr[qcol];
                        float sc[8];
                        float mx = -__builtin_inff();
#pragma unroll
                        for (int h = 0; h < 2; h++) {
                            const int base = rb + 16 * h;
                            float4 e4 = *(const float4 *)&t_ea[base], b4 = *(const float4 *)&t_eb[base];
                            if (tail) {
                                float *pe = (float *)&e4, *pb = (float *)&b4;
#pragma unroll
                                for (int j = 0; j < 4; j++)
                                    if (base + j >= rows_left) { pe[j] = 0.f; pb[j] = -__builtin_inff(); }
                            }
                            sc[4 * h + 0] = fmaf((float)s_hq[(4 * h + 0) * HQS + ln], e4.x, b4.x);
                            sc[4 * h + 1] = fmaf((float)s_hq[(4 * h + 1) * HQS + ln], e4.y, b4.y);
                            sc[4 * h + 2] = fmaf((float)s_hq[(4 * h + 2) * HQS + ln], e4.z, b4.z);
                            sc[4 * h + 3] = fmaf((float)s_hq[(4 * h + 3) * HQS + ln], e4.w, b4.w);
                            mx = fmaxf(fmaxf(mx, sc[4 * h + 0]), fmaxf(fmaxf(sc[4 * h + 1], sc[4 * h + 2]), sc[4 * h + 3]));
                        }
                        if (mx >= thr && !(INSTR && (flags & 64))) {       // (ablation bit 64: exact scores, no appends)
                            int nh = 0;
#pragma unroll
                            for (int e = 0; e < 8; e++) nh += sc[e] >= thr ? 1 : 0;
                            int pos = atomicAdd(&s_cnt[qcol], nh);
                            if (pos + nh > s_trig[qcol]) *s_need = 1;
                            uint64_t *dstq = my_cand + (size_t)qcol * CAP;
                            const uint32_t rbase = (uint32_t)(tile_row0 + rb);
#pragma unroll
                            for (int e = 0; e < 8; e++) {
                                if (sc[e] >= thr) {
                                    dstq[pos] = ((uint64_t)score_key(sc[e]) << 32) | (uint64_t)(rbase + (e & 3) + 16 * (e >> 2));
                                    pos++;
                                }
                            }
                        }
                    }
                    __builtin_amdgcn_wave_barrier();          // the next pushes overwrite the slots read above
                    qn = 0;
                };
                static_assert(NSITE == 16, "the sites below");
                while (todo) {
                    todo = __builtin_amdgcn_readfirstlane(todo);
                    uint32_t open = todo;
#define AK_HQ_SITE(S) site(std::integral_constant<int, S>{}, open);
                    AK_HQ_SITE(0) AK_HQ_SITE(1) AK_HQ_SITE(2) AK_HQ_SITE(3) AK_HQ_SITE(4) AK_HQ_SITE(5) AK_HQ_SITE(6) AK_HQ_SITE(7)
                    AK_HQ_SITE(8) AK_HQ_SITE(9) AK_HQ_SITE(10) AK_HQ_SITE(11) AK_HQ_SITE(12) AK_HQ_SITE(13) AK_HQ_SITE(14) AK_HQ_SITE(15)
#undef AK_HQ_SITE
                    if (qn) drain();
                }
                return;
            }
            if constexpr (FILT_K == 1 && I8) {
                // The int8 tile's whole-tile arrangement works on the BOUNDS. The int8 shadow gives the rows of a filter class one
                // shared ea8 wherever they can adopt it (shadow8_scale.h), and eb is 0 for every live row of the metrics this plan
                // takes: fma(site_dpos, gea, geb) is then bit for bit the site's maximum score -- the one positive factor is monotone
                // and rounds identically -- so the sixteen bounds ARE the exact maxima the 16-bit body below computes from 128
                // conversions and 128 fma per lane, and no row term is held across the tile. The 2 * NI thresholds and the tile's
                // block terms are read once, the bounds go branch-free into a hit mask, one branch goes around everything else, and
                // behind it only the sites where some lane passed are entered: the row terms of that block are read there, then
                // site_scores and site_append as they stand. Nothing here depends on a class being uniform: for a mixed class (a
                // row the cap excluded, a removed or filtered row, the block an append extended) the bound is still an upper
                // bound and the site is merely entered without a hit. The same holds in a tail tile: a 32-row block past the corpus
                // takes the LAST block's terms (stage_terms clamps the block number to gb_blocks - 1, so no unwritten gb8 is read)
                // against whatever the allocated rows past n hold, and it is row_terms' masking of those rows (ea = 0, eb = -inf)
                // that keeps them out -- the exact-maxima body relied on that masking alone. A row is appended iff its score reaches
                // the threshold, and the bound never skips a site that holds such a row: the same keys as the other arrangements,
                // in another order.
                static_assert(2 * MI * NI <= 32, "one hit bit per site");
                float thr_s[NI][2];
#pragma unroll
                for (int ni = 0; ni < NI; ni++)
#pragma unroll
                    for (int c = 0; c < 2; c++) thr_s[ni][c] = s_thr[(wc * NI + ni) * 32 + 16 * c + r16];
                float gea[MI], geb[MI];
#pragma unroll
                for (int mi = 0; mi < MI; mi++) {
                    gea[mi] = t_gb[(wr * MI + mi) * 4 + (kq & 1)];
                    geb[mi] = t_gb[(wr * MI + mi) * 4 + 2 + (kq & 1)];
                }
                uint32_t hits = 0;
#pragma unroll
                for (int mi = 0; mi < MI; mi++)
#pragma unroll
                    for (int ni = 0; ni < NI; ni++)
#pragma unroll
                        for (int c = 0; c < 2; c++)
                            hits |= fmaf(site_dpos(mi, ni, c), gea[mi], geb[mi]) >= thr_s[ni][c] ? 1u << ((mi * NI + ni) * 2 + c) : 0u;
                if (INSTR && (flags & 16)) hits = 0;
                if (hits) {
#pragma unroll
                    for (int mi = 0; mi < MI; mi++) {
                        if (!(hits & (((1u << (2 * NI)) - 1u) << (mi * NI * 2)))) continue;
                        float4 e4[2], b4[2];
                        row_terms(mi, e4, b4);
#pragma unroll
                        for (int ni = 0; ni < NI; ni++)
#pragma unroll
                            for (int c = 0; c < 2; c++)
                                if (hits & (1u << ((mi * NI + ni) * 2 + c))) {
                                    if constexpr (INSTR) n_slow++;
                                    float sc[8];
                                    if (site_scores(mi, ni, c, e4, b4, sc) >= thr_s[ni][c]) site_append(mi, ni, c, thr_s[ni][c], sc);
                                    else if constexpr (INSTR) n_drain++;     // entered without a hit (every lane counts its own: summed at the end)
                                }
                    }
                }
                return;
            }
            if constexpr (FILT_K == 1) {
                // (the 16-bit tiles; the int8 tile's body of this arrangement is the one above)
                // Exact maxima of the whole tile first. What the site-by-site arrangement costs is not its bound but what follows it: a
                // lane-site passes the bound about once in a hundred in the main pass, so about half of the wave's sites have SOME lane
                // in the slow path, and the wave pays for each -- four LDS reads of row terms and their wait, the eight exact scores,
                // and where a lane holds a true hit the atomic and the appends (measured: 1.3 k cycles per tile for all sixteen bounds,
                // 3.7 k for the slow paths behind them). Here the per-row terms are read ONCE per tile, with the 2 * NI thresholds
                // (s_thr changes only inside serve_compaction, behind barriers; the terms belong to this tile) -- all in flight
                // before one wait --, the exact maximum of every site is computed branch-free, which costs what the bound cost on 16
                // bits and eight conversions more on int8, and only the sites where a lane holds a TRUE hit are entered, behind one
                // branch around them all. The block bounds (t_gb) are not read. A row is appended iff its score reaches the
                // threshold in either arrangement -- the bound only ever skipped sites without one -- and scores, keys and counts
                // are the same expressions: the same keys are appended, in another order. The accumulators are read by plain
                // expressions only (no inline asm), so the compiler's own hazard handling covers them and mfma_settle is not needed.
                static_assert(2 * MI * NI <= 32, "one hit bit per site");
                // TG row blocks' terms at a time: all of the tile's, except on the 128-accumulator 16-bit tile, where the 64 registers
                // of four blocks' terms beside the accumulators made hipcc spill two -- two blocks at a time there, read again in
                // the slow section for a pair of blocks with a hit
                constexpr int TG = (!I8 && MI * NI >= 8) ? 2 : MI;
                float4 e4[TG][2], b4[TG][2];
                float thr_s[NI][2];
#pragma unroll
                for (int ni = 0; ni < NI; ni++)
#pragma unroll
                    for (int c = 0; c < 2; c++) thr_s[ni][c] = s_thr[(wc * NI + ni) * 32 + 16 * c + r16];
                uint32_t hits = 0;
#pragma unroll
                for (int g = 0; g < MI / TG; g++) {
#pragma unroll
                    for (int j = 0; j < TG; j++) row_terms(g * TG + j, e4[j], b4[j]);
#pragma unroll
                    for (int j = 0; j < TG; j++)
#pragma unroll
                        for (int ni = 0; ni < NI; ni++)
#pragma unroll
                            for (int c = 0; c < 2; c++) {
                                float sc[8];
                                const int mi = g * TG + j;
                                hits |= site_scores(mi, ni, c, e4[j], b4[j], sc) >= thr_s[ni][c] ? 1u << ((mi * NI + ni) * 2 + c) : 0u;
                            }
                    if (MI / TG > 1) __builtin_amdgcn_sched_barrier(0);   // one group at a time: hoisting all the term loads spills
                }
                if (INSTR && (flags & 16)) hits = 0;
                if (hits) {
#pragma unroll
                    for (int g = 0; g < MI / TG; g++) {
                        if (MI / TG > 1) {
                            if (!(hits & (((1u << (2 * NI * TG)) - 1u) << (g * TG * NI * 2)))) continue;
#pragma unroll
                            for (int j = 0; j < TG; j++) row_terms(g * TG + j, e4[j], b4[j]);
                        }
#pragma unroll
                        for (int j = 0; j < TG; j++)
#pragma unroll
                            for (int ni = 0; ni < NI; ni++)
#pragma unroll
                                for (int c = 0; c < 2; c++) {
                                    const int mi = g * TG + j;
                                    if (hits & (1u << ((mi * NI + ni) * 2 + c))) {
                                        if constexpr (INSTR) n_slow++;
                                        float sc[8];
                                        site_scores(mi, ni, c, e4[j], b4[j], sc);
                                        site_append(mi, ni, c, thr_s[ni][c], sc);
                                    }
                                }
                    }
                }
                return;
            }
            // slow path of one site whose bound reached the threshold: per-row terms, exact scores, appends where a lane holds a hit
            auto site_slow = [&](int mi, int ni, int c, float thr) {
                if constexpr (INSTR) n_slow++;
                float4 e4[2], b4[2];
                row_terms(mi, e4, b4);
                float sc[8];
                if (site_scores(mi, ni, c, e4, b4, sc) >= thr) site_append(mi, ni, c, thr, sc);
            };
#if !AK_DBG_KERNELS
            mfma_settle(acc);
#endif
#pragma unroll
            for (int mi = 0; mi < MI; mi++) {
                const float gea = t_gb[(wr * MI + mi) * 4 + (kq & 1)], geb = t_gb[(wr * MI + mi) * 4 + 2 + (kq & 1)];
#pragma unroll
                for (int ni = 0; ni < NI; ni++) {
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        const float U = fmaf(site_dpos(mi, ni, c), gea, geb);
                        const float thr = s_thr[(wc * NI + ni) * 32 + 16 * c + r16];
                        if (U >= thr && !(INSTR && (flags & 16))) site_slow(mi, ni, c, thr);
                    }
                }
            }
            return;
        }
        // Common path: for the 16 rows a lane holds of a 32-row block, U = max(dot,0)*max(ea)+max(eb) is an
        // upper bound of their scores (ea >= 0); the per-block maxima are precomputed at ingest (Index::gb).
        // Only a group whose bound reaches the threshold is scored exactly -- about the true hit rate.
        float thr_q[NI];
#pragma unroll
        for (int ni = 0; ni < NI; ni++) thr_q[ni] = s_thr[(wc * NI + ni) * 32 + r];
#if !AK_DBG_KERNELS
        mfma_settle(acc);   // the v_max3_f32 below read MFMA results through inline asm: close the MFMA -> VALU window here
#endif
#pragma unroll
        for (int mi = 0; mi < MI; mi++) {
            const float gea = t_gb[(wr * MI + mi) * 4 + kh], geb = t_gb[(wr * MI + mi) * 4 + 2 + kh];
#pragma unroll
            for (int ni = 0; ni < NI; ni++) {
                const f32x16 &a = acc[mi][ni];
#if AK_DBG_KERNELS
                // the fmaxf tree of rounds 1-4 (A/B reference in the dbg library): IEEE mode makes hipcc quiet every operand first --
                // 12 x `v_max_f32 x, x, x` + 11 max instructions per group, 25 VALU per group with the bound and the compare
                const float m01 = fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])), m23 = fmaxf(fmaxf(a[4], a[5]), fmaxf(a[6], a[7])),
                            m45 = fmaxf(fmaxf(a[8], a[9]), fmaxf(a[10], a[11])), m67 = fmaxf(fmaxf(a[12], a[13]), fmaxf(a[14], a[15]));
                const float dmax = fmaxf(fmaxf(m01, m23), fmaxf(m45, m67));     // NaN-ignoring
                const float dpos = fmaxf(dmax, 0.f);
#else
                // max(0, the 16 dot products) as eight v_max3_f32 (round 5): 10 VALU per group instead of 25. MFMA results are
                // never signalling NaNs and v_max3 skips quiet ones like fmaxf does (NaN-ignoring). The hazard recogniser does
                // not see asm operands: mfma_settle(acc) above holds these reads 18 wait states behind the last MFMA.
                const float dpos = max3z(max3f(max3f(a[0], a[1], a[2]), max3f(a[3], a[4], a[5]), max3f(a[6], a[7], a[8])),
                                         max3f(max3f(a[9], a[10], a[11]), max3f(a[12], a[13], a[14]), a[15]));
#endif
                const float U = fmaf(dpos, gea, geb);
                const float thr = thr_q[ni];
                if (U >= thr && !(INSTR && (flags & 16))) {
                    if constexpr (INSTR) n_slow++;
                    // exact scores of the group: score = fma(dot, ea[row], eb[row])
                    float sc[16];
                    float mx = -__builtin_inff();
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const int base = (wr * MI + mi) * 32 + 8 * g + 4 * kh;   // rows base .. base+3 of the tile
                        float4 e4 = *(const float4 *)&t_ea[base], b4 = *(const float4 *)&t_eb[base];
                        if (tail) {
                            float *pe = (float *)&e4, *pb = (float *)&b4;
#pragma unroll
                            for (int j = 0; j < 4; j++)
                                if (base + j >= rows_left) { pe[j] = 0.f; pb[j] = -__builtin_inff(); }
                        }
                        sc[4 * g + 0] = fmaf(a[4 * g + 0], e4.x, b4.x); sc[4 * g + 1] = fmaf(a[4 * g + 1], e4.y, b4.y);
                        sc[4 * g + 2] = fmaf(a[4 * g + 2], e4.z, b4.z); sc[4 * g + 3] = fmaf(a[4 * g + 3], e4.w, b4.w);
                        mx = fmaxf(fmaxf(mx, sc[4 * g + 0]), fmaxf(fmaxf(sc[4 * g + 1], sc[4 * g + 2]), sc[4 * g + 3]));
                    }
                    if (mx >= thr) {
                        const int qcol = (wc * NI + ni) * 32 + r;
                        // one LDS atomic per lane reserves room for all of its hits in this 16-row group
                        int nh = 0;
#pragma unroll
                        for (int e = 0; e < 16; e++) nh += sc[e] >= thr ? 1 : 0;
                        int pos = atomicAdd(&s_cnt[qcol], nh);
                        if (pos + nh > s_trig[qcol]) *s_need = 1;
                        uint64_t *dstq = my_cand + (size_t)qcol * CAP;
                        const uint32_t rbase = (uint32_t)(tile_row0 + (wr * MI + mi) * 32 + 4 * kh);
#pragma unroll
                        for (int e = 0; e < 16; e++) {
                            if (sc[e] >= thr) {
                                dstq[pos] = ((uint64_t)score_key(sc[e]) << 32) | (uint64_t)(rbase + (e & 3) + 8 * (e >> 2));
                                pos++;
                            }
                        }
                    }
                }
            }
        }
    };

    if constexpr (C::PHASED) {
        // ------------------------------------------------------------------------------------------------------------
        // Phased K-loop (256 x 256 tile). A K-tile (64 deep) lives in LDS as FOUR half-tiles of 16 KiB -- Ah0, Bh0, Bh1,
        // Ah1: 128 rows x 128 B each; half h of A holds, for each wave row, its 32-row blocks 2h and 2h+1, half h of B
        // each wave column's block h -- in one of two buffers, and is computed in two phases of 16 MFMAs:
        //   X: read Ah0, Bh0, Bh1 (16 fragment reads), quadrants (A0,B0) (A0,B1);  Y: read Ah1 (8 reads), (A1,B1) (A1,B0).
        // A phase is  [LOAD: fragment reads + LDS-DMA issue + lgkmcnt(0) + counted vmcnt]  barrier  [MFMA x 16]  barrier.
        // Waves 4-7 (the SIMD partners of waves 0-3) run ONE BARRIER behind: while one wave of a SIMD owns the matrix
        // pipe, its partner reads fragments and issues DMA pieces, then they swap. In step (the K-loop of rounds 1-2),
        // both issued their loads together -- matrix pipe idle -- and then shared the pipe: per K-step 1304 cycles of issue +
        // 1006 of exposed wait against 2048 of pipe work, MFMA pipe 51 % busy; this schedule: 70 % (PMC, profiles/).
        // Measured on the way (10M x 768, Q = 1024, same box): in-step loop 13.8-14.0 ms; four quadrant phases of 8 MFMAs,
        // one half-tile issued per phase five ahead: 12.6-13.4; those with the fragment reads evened out to 8/4/8/4 per phase:
        // +2 %; without s_setprio around the MFMAs: same; without the stagger (same barriers): 13.8; ONE barrier per phase
        // with the halves staggered by program order ([MFMA, LOAD] vs [LOAD, MFMA]): 14.1 (the younger half's read latency
        // lands on the critical path of every interval); these two phases: 12.2-12.5. With staging, waits and filter ablated
        // the loop runs at the same speed (12.2): it is bound by the matrix pipe at the clock the power limit leaves
        // (1.65 GHz at 70 % busy against 2.05 GHz at 51 %).
        // Hazards (barriers numbered per workgroup; the older half's LOAD(p) lies in barrier interval (2p-1, 2p), the
        // younger half's in (2p, 2p+1); LOAD X(g) = phase 2g, LOAD Y(g) = phase 2g+1):
        //   WAR  every LOAD ends with lgkmcnt(0), so a half-tile read in LOAD(p) is retired before that wave's next barrier
        //        and may be replaced from LOAD(p+1) on by either half: LOAD Y(g) issues Ah0, Bh0, Bh1 of K-tile g+2 into
        //        the slots LOAD X(g) read, LOAD X(g) issues Ah1 of K-tile g+1 into the slot LOAD Y(g-1) read.
        //   RAW  what LOAD(p+1) reads was issued in LOAD(p-1): the vmcnt(8) that ends LOAD(p) leaves exactly the 8 pieces
        //        issued since in flight; every wave passes a barrier after that wait and before ANY wave's LOAD(p+1).
        // The halves stay one barrier apart across tiles (the filter of one runs under the other's MFMAs); only a compaction
        // -- rare, workgroup-uniform -- re-aligns them.
        // What that boundary costs (10M x 768, Q = 1024, int8 tile, instrumented build, per wave and tile): the K-loop 20.3 k cycles, the
        // filter 5.9 k, of which 1.3 k are the sixteen bounds and the rest the slow paths behind them -- a lane-site passes its bound
        // once in a hundred, so half of the wave's sites are entered by SOME lane. The next barrier after a tile's last MFMA phase
        // comes when the younger half has filtered too, i.e. one phase + one filter later: the filter is exposed on both halves
        // whatever runs under its first 512 cycles. The whole-tile arrangement of the filter (ScanCfg::FILT = 1, tile_epilogue)
        // shortens it instead: 4.2 k cycles. It neither defers a part of the filter into a later LOAD section nor moves the
        // s_need sample: the sampling argument in the tile loop below stands for both arrangements.
        // The queued arrangement (FILT = 2, int8 tile) shortens what divergence is left: lane-sites that pass their bound go to a per-wave
        // LDS queue and are scored once per tile, one lane per entry. Beside the partner's MFMA stream a filter's cycles follow its
        // INSTRUCTION COUNT (8 to 10 cycles each, vector or scalar), so it pays where the whole-tile filter enters most sites: the seeding
        // pass, 14.5 k -> 9.8 k cycles and 892 -> 763 us per launch; in the main pass (ten entries per wave and tile) its ~450
        // instructions buy nothing over the whole-tile filter's ~420 and it does not ship there (docs/EXPERIMENTS.md, "hit queue").
        // It too ends inside tile_epilogue with an empty queue: nothing of a tile's filter crosses into the next tile.
        // Class scales (shadow8_scale.h) take the work away at its source: with one ea8 per filter class a site's bound IS its exact
        // maximum, the int8 tile's whole-tile filter keeps the sixteen bounds and drops the 128 conversions and fma per lane, and a
        // lane-site passes about once in a thousand, the true hit rate: main-pass filter 4.25 k -> 3.1 k cycles per wave and tile, the
        // seeding pass's queue gets a third of the pushes (docs/EXPERIMENTS.md, "class scales").
        // 16x16x32 (C::MFMA = 16; the MFMA shape as a lever of its own in a loop whose clock the chip holds down): the same buffers, phases, barriers and 16 fragment reads per phase X (8 in Y), but a fragment is 16 rows x K32
        // (lane: row l & 15, chunk 4s + (l >> 4) of K32 sub-step s) and a phase issues twice as many MFMAs of half the length -- the
        // same 512 pipe cycles. The accumulators stay f32x16 per 32 x 32 block, each MFMA works on a four-float slice of one (slice
        // 2h + c = rows 16h.., columns 16c..), so mfma_settle ties them through one statement as before. Which tile ships on which
        // shape is decided by wall time on the benchmark's workload against the parent in the same job (docs/EXPERIMENTS.md,
        // "16x16x32"): cycles do not rank the shapes, the clock the chip sustains on each does.
        // ------------------------------------------------------------------------------------------------------------
        constexpr int HT = 16384;                          // an A half-tile: 128 corpus rows
        // A K-tile buffer: Ah0 | B part 0 .. NI-1 | Ah1. Half h of A holds, per wave row, its AH = MI / 2 blocks h*AH ..; a B part
        // holds one 32-query block per wave column. 256 x 256 (WM 2, WN 4, MI 4, NI 2): four 16 KiB pieces of a buffer, phases
        // of 16 MFMAs; 256 x 128 (NI 1): no second B part, phases of 8; 256 x 192 (WM 4, WN 2, MI 2, NI 3: 64 x 96 per wave, the
        // tile of batches between the regimes): B parts of 8 KiB (64 rows, one piece per wave), phases of 12.
        constexpr int AH = MI / 2;
        constexpr int BPB = C::WN * 32 * BKB;              // bytes of a B part
        constexpr int BPP = BPB / 1024 / NW;               // its pieces per wave (2 or 1)
        constexpr int KTB = 2 * HT + NI * BPB;             // bytes of a K-tile buffer
        constexpr int NPW = 4 + NI * BPP;                  // pieces per wave and K-tile
        constexpr int O_A0 = 0, O_B = HT, O_A1 = HT + NI * BPB;
        static_assert(BPP == 1 || BPP == 2, "a B part is one or two pieces per wave");
        const bool young = wave >= NW / 2;                          // wave-uniform
        // staging sources: one SGPR base per K-tile and operand + one 32-bit VGPR offset per piece, constant for the
        // whole launch (a piece = 8 rows x 128 B: full-line reads; the LDS image is lane-linear, the XOR swizzle is on
        // the source chunk)
        // (these sixteen lane constants are recomputed at the top of every tile from an opaque copy of the lane id: kept
        // live across the filter -- 128 accumulators + 16 scores + terms -- they were what the register allocator spilled)
        uint32_t voA[2][2], voB[NI][BPP];
        int ra[4], rb[4];
        auto lane_consts = [&](int ln) {
            const int srow = ln / CPR, schunk = ln % CPR, rr = ln & 31, kk = ln >> 5;
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int p = 0; p < 2; p++) {
                    const int lr = (wave * 2 + p) * RPP + srow;                                 // row of the A half-tile
                    const int trow = ((lr / (AH * 32)) * MI + AH * h + ((lr >> 5) % AH)) * 32 + (lr & 31);   // corpus row of the tile
                    voA[h][p] = (uint32_t)trow * (uint32_t)D * (uint32_t)EB + ((schunk ^ swz(lr)) << 4);
                }
#pragma unroll
            for (int t = 0; t < NI; t++)
#pragma unroll
                for (int p = 0; p < BPP; p++) {
                    const int lr = (wave * BPP + p) * RPP + srow;                               // row of the B part
                    const int qrow = ((lr >> 5) * NI + t) * 32 + (lr & 31);                      // query of the block
                    voB[t][p] = (uint32_t)qrow * (uint32_t)D * (uint32_t)EB + ((schunk ^ swz(lr)) << 4);
                }
            // fragment read offsets: A rows wr*AH*32 + m*32 + r of a half-tile, B rows wc*32 + r of a part; chunk (2*k2 + kh) ^ swz(row)
            // 16x16x32: fragment f = 2 * b + s is the 16-row block b (A: h, B: c) of a 32-row block at K32 sub-step s: rows 16b + r16,
            // chunk (4s + kq) ^ swz(row) -- swz(16b + r16) = swz(r16), the source-side swizzle stands. The 16 lanes ds_read_b128
            // serves together ({0-3, 12-15, 20-27}, ...) hold 16 rows and, with kq and the swizzle, 16 distinct bank quads.
            if constexpr (M16) {
                const int r6 = ln & 15, k6 = ln >> 4;
#pragma unroll
                for (int f = 0; f < 4; f++) {
                    const int coff = ((4 * (f & 1) + k6) ^ swz(r6)) << 4;
                    ra[f] = (wr * AH * 32 + 16 * (f >> 1) + r6) * BKB + coff;
                    rb[f] = (wc * 32 + 16 * (f >> 1) + r6) * BKB + coff;
                }
            } else {
            const int cc0 = kk ^ swz(rr);
#pragma unroll
            for (int k2 = 0; k2 < 4; k2++) {
                const int coff = (cc0 ^ (k2 << 1)) << 4;
                ra[k2] = (wr * AH * 32 + rr) * BKB + coff;
                rb[k2] = (wc * 32 + rr) * BKB + coff;
            }
            }
        };
        lane_consts(lane);
        const char *const rows_b = (const char *)rows;
        const char *const qs_b = (const char *)qs + (int64_t)q0 * D * EB;
        int c_kk = 0, c_tile = 0;                          // staging cursor (K-tile), clamped to the last K-tile: past the
        auto c_adv = [&]() {                               // end it re-stages that K-tile into slots nobody reads any more
            if (c_kk + 1 < KS) c_kk++;
            else if (c_tile + 1 < ntiles) { c_kk = 0; c_tile++; }
        };
        auto sgpr64 = [](const char *ptr) {                // a wave-uniform pointer, pinned to an SGPR pair for the asm below
            const uint64_t u = (uint64_t)ptr;
            const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
            return ((uint64_t)hi << 32) | lo;
        };
        auto c_pa = [&]() { return sgpr64(rows_b + (t0 + c_tile) * tmul * BM * D * EB + (int64_t)c_kk * 128); };
        auto c_pb = [&]() { return sgpr64(qs_b + c_kk * 128); };
        const uint32_t lds_w = lds_addr(smem) + wave * 2048;      // this wave's two pieces of an A half-tile
        const uint32_t lds_wb = lds_addr(smem) + wave * (BPP * 1024);   // ... and its piece(s) of a B part
        // two 1 KiB pieces: LDS[M0 + lane*16] <- gbase[off]; s_nop 4 covers a base SGPR written just before the statement
        auto issue = [&](uint64_t gbase, uint32_t o0, uint32_t o1, uint32_t dst) {
            if (INSTR && (flags & 2)) return;
            asm volatile("s_mov_b32 m0, %3\n\ts_nop 4\n\tglobal_load_lds_dwordx4 %0, %2\n\t"
                         "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                         :: "v"(o0), "v"(o1), "s"(gbase), "s"(dst) : "memory", "m0", "scc");
        };
        auto issue1 = [&](uint64_t gbase, uint32_t o0, uint32_t dst) {
            if (INSTR && (flags & 2)) return;
            asm volatile("s_mov_b32 m0, %2\n\ts_nop 4\n\tglobal_load_lds_dwordx4 %0, %1"
                         :: "v"(o0), "s"(gbase), "s"(dst) : "memory", "m0");
        };
        auto issue_a = [&](auto htag, uint64_t pa, int buf) {          // half h of A of the K-tile at pa -> buffer buf
            constexpr int H = decltype(htag)::value;
            issue(pa, voA[H][0], voA[H][1], __builtin_amdgcn_readfirstlane(lds_w + buf * KTB + (H ? O_A1 : O_A0)));
        };
        auto issue_b = [&](uint64_t pb, int buf) {                      // every B part of the K-tile at pb
#pragma unroll
            for (int t = 0; t < NI; t++) {
                const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_wb + buf * KTB + O_B + t * BPB);
                if constexpr (BPP == 2) issue(pb, voB[t][0], voB[t][BPP - 1], dst);
                else issue1(pb, voB[t][0], dst);
            }
        };
        constexpr std::integral_constant<int, 0> H0{};
        constexpr std::integral_constant<int, 1> H1{};
        // K-tile state while K-tile g is computed: the cursor stands on g+2; pX1 = sources of K-tile g+1, pX2 of g+2
        uint64_t pa1, pb1, pa2, pb2;
        int cur = 0, need = 0;
        auto kt_advance = [&]() { pa1 = pa2; pb1 = pb2; c_adv(); pa2 = c_pa(); pb2 = c_pb(); cur ^= 1; };
        // prologue: K-tile 0 whole, then Ah0, Bh0, Bh1 of K-tile 1 (what LOAD Y(-1) would have issued); LOAD X(0)'s three
        // half-tiles must have landed: the 8 youngest pieces may stay in flight
        {
            const uint64_t pa = c_pa(), pb = c_pb();
            issue_a(H0, pa, 0);
            issue_b(pb, 0);
            issue_a(H1, pa, 0);
        }
        c_adv();
        pa1 = c_pa(); pb1 = c_pb();
        issue_a(H0, pa1, 1);
        issue_b(pb1, 1);
        c_adv();
        pa2 = c_pa(); pb2 = c_pb();
        wait_vm<NPW>();
        __syncthreads();

        uint4 fa[AH][4], fb[NI][4];
        long long t_load = 0, t_bar = 0;
        auto BAR = [&]() {
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        };
        auto phase = [&](auto ytag, auto first_tag) {
            constexpr bool Y = decltype(ytag)::value;
            constexpr bool FIRST = decltype(first_tag)::value;      // first K-tile of a corpus tile: accumulators start from 0
            const long long ts0 = TICK();
            if (young) BAR();
            const long long ts1 = TICK();
            const char *rbase = smem + cur * KTB;
            if constexpr (!Y) {
#pragma unroll
                for (int k2 = 0; k2 < 4; k2++) fb[0][k2] = *(const uint4 *)(rbase + O_B + rb[k2]);
#pragma unroll
                for (int m = 0; m < AH; m++)
#pragma unroll
                    for (int k2 = 0; k2 < 4; k2++) fa[m][k2] = *(const uint4 *)(rbase + O_A0 + m * 32 * BKB + ra[k2]);
#pragma unroll
                for (int t = 1; t < NI; t++)
#pragma unroll
                    for (int k2 = 0; k2 < 4; k2++) fb[t][k2] = *(const uint4 *)(rbase + O_B + t * BPB + rb[k2]);
                issue_a(H1, pa1, cur ^ 1);
            } else {
#pragma unroll
                for (int m = 0; m < AH; m++)
#pragma unroll
                    for (int k2 = 0; k2 < 4; k2++) fa[m][k2] = *(const uint4 *)(rbase + O_A1 + m * 32 * BKB + ra[k2]);
                issue_a(H0, pa2, cur);
                issue_b(pb2, cur);
            }
            __builtin_amdgcn_s_waitcnt(0xc07f);             // lgkmcnt(0): this wave's reads are retired before its barrier
            if (!(INSTR && (flags & 4))) wait_vm<NPW>();
            const long long ts2 = TICK();
            BAR();
            const long long ts3 = TICK();
            __builtin_amdgcn_s_setprio(1);
            constexpr int MB = Y ? AH : 0;                  // 32-row blocks MB .. MB + AH - 1
            if constexpr (M16) {
                // the same 512 pipe cycles as twice as many MFMAs of half the length: per K32 sub-step s and 32 x 32 block its four
                // 16 x 16 blocks (h, c) = slice 2h + c of the block's accumulator, from fragments fa[m][2h + s], fb[nb][2c + s]
#pragma unroll
                for (int s = 0; s < 2; s++)
#pragma unroll
                    for (int m = 0; m < AH; m++)
#pragma unroll
                        for (int e = 0; e < NI; e++) {
                            const int nb = Y ? NI - 1 - e : e;
                            const bool zero = FIRST && s == 0;
                            f32x16 &d = acc[MB + m][nb];
                            if constexpr (I8) {
                                mfma16_i8_into<0>(d, fa[m][s], fb[nb][s], zero);
                                mfma16_i8_into<1>(d, fa[m][s], fb[nb][2 + s], zero);
                                mfma16_i8_into<2>(d, fa[m][2 + s], fb[nb][s], zero);
                                mfma16_i8_into<3>(d, fa[m][2 + s], fb[nb][2 + s], zero);
                                continue;
                            }
                            mfma16_into<IS_BF16, 0>(d, fa[m][s], fb[nb][s], zero);
                            mfma16_into<IS_BF16, 1>(d, fa[m][s], fb[nb][2 + s], zero);
                            mfma16_into<IS_BF16, 2>(d, fa[m][2 + s], fb[nb][s], zero);
                            mfma16_into<IS_BF16, 3>(d, fa[m][2 + s], fb[nb][2 + s], zero);
                        }
            } else
#pragma unroll
            for (int k2 = 0; k2 < 4; k2++)
#pragma unroll
                for (int m = 0; m < AH; m++)
#pragma unroll
                    for (int e = 0; e < NI; e++) {
                        const int nb = Y ? NI - 1 - e : e;              // Y runs the B parts backwards: (A1,B1) then (A1,B0)
                        const uint4 bf = fb[nb][k2];
                        if (FIRST && k2 == 0) {
                            f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                            acc[MB + m][nb] = mfma32<IS_BF16>(fa[m][k2], bf, z);
                        } else {
                            acc[MB + m][nb] = mfma32<IS_BF16>(fa[m][k2], bf, acc[MB + m][nb]);
                        }
                    }
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            const long long ts4 = TICK();
            if (!young) BAR();
            if constexpr (INSTR) { t_load += ts2 - ts1; t_bar += (ts1 - ts0) + (ts3 - ts2) + (TICK() - ts4); }
        };
        auto ktile = [&](auto first_tag) {
            phase(std::false_type{}, first_tag);
            phase(std::true_type{}, first_tag);
            kt_advance();
        };
        for (int t = 0; t < ntiles; t++) {
            const int64_t tile_row0 = (t0 + t) * tmul * BM;
            stage_terms(t, tile_row0);
#if AK_DBG_KERNELS       // (A/B reference: the per-tile recomputation of rounds 3-4)
            {
                int ln = lane;
                asm volatile("" : "+v"(ln));                // opaque: the constants below are recomputed, not carried
                lane_consts(ln);
            }
#endif
            t_mark = TICK();
            ktile(std::true_type{});
            for (int kk = 1; kk < KS; kk++) {
                // Compaction requests are raised in filters only. The halves stay one barrier apart ACROSS tiles (below), so
                // the younger half filters tile t-1 one interval after the older half; by the last K-step of tile t (KS >= 2:
                // the host sends shorter rows to the in-step tiles) both filters are behind, and nobody filters again before
                // both halves have sampled: every wave reads the same value, the branch below is workgroup-uniform.
                if (!SEED && kk == KS - 1) need = *s_need;
                ktile(std::false_type{});
            }
            { long long now = TICK(); t_loop += now - t_mark; t_mark = now; }
            if (!SEED && need && !(INSTR && (flags & 32))) {
                // rare: a wave compacts a query's buffer while nobody may append to it -> the halves re-align first (the
                // older half waits out the younger half's last MFMAs; for the younger half this is that phase's closing
                // barrier), compact in step, filter in step, and fall one barrier apart again in the next tile's first phase
                BAR();
                wait_vm<0>();                               // every wave's candidate stores of the earlier filters have landed
                __syncthreads();
                serve_compaction();
            }
            { long long now = TICK(); t_comp += now - t_mark; t_mark = now; }
            // No re-alignment in the common case: the older half filters tile t (VALU + LDS) and reads the next tile's first
            // fragments while the younger half's last 16 MFMAs run, then they swap -- the filter, 5 % of the main pass at
            // D = 768 and 10 % at D = 384 when both halves stopped for it, hides under the partner's matrix phase. The per-tile
            // terms are double-buffered by tile parity and staged by waves that pass a counted vmcnt wait and a barrier
            // every phase, so the half that filters later finds them too.
            tile_epilogue(t, tile_row0);
            { long long now = TICK(); t_epi += now - t_mark; t_mark = now; }
        }
        if constexpr (INSTR) t_sync = (t_load & 0xffffffffll) + (t_bar << 32);
    } else {
    const int a_off = (wr * MI * 32 + r) * BKB;   // + mi*32*BKB
    const int b_off = (wc * NI * 32 + r) * BKB;   // + ni*32*BKB

    // ---- staging cursor (runs NSTAGE-1 steps ahead of the compute cursor) ----
    const uint32_t ldsA = lds_addr(sA) + wave * C::A_PW * 1024;
    const uint32_t ldsB = lds_addr(sB) + wave * C::B_PW * 1024;
    const char *aptr[C::A_PW];
    const char *bptr[C::B_PW];
    int s_tile = 0, s_kk = 0, s_buf = 0, issued = 0;
    auto set_aptr = [&](int trel) {
#pragma unroll
        for (int p = 0; p < C::A_PW; p++) {
            int row = (wave * C::A_PW + p) * RPP + st_row;
            int64_t grow = (t0 + trel) * tmul * BM + row;
            if (grow >= n) grow = n - 1;
            int gchunk = st_chunk ^ swz(row);
            aptr[p] = (const char *)rows + grow * D * 2 + gchunk * 16;
        }
    };
#pragma unroll
    for (int p = 0; p < C::B_PW; p++) {
        int row = (wave * C::B_PW + p) * RPP + st_row;
        int gchunk = st_chunk ^ swz(row);
        bptr[p] = (const char *)qs + (int64_t)(q0 + row) * D * 2 + gchunk * 16;
    }
    set_aptr(0);
    auto stage_next = [&]() {   // issue the loads of the staging cursor, then advance it
        const int goff = s_kk * BKB;
        glds16xN<C::A_PW>(aptr, goff, __builtin_amdgcn_readfirstlane(ldsA + s_buf * C::A_BYTES));
        glds16xN<C::B_PW>(bptr, goff, __builtin_amdgcn_readfirstlane(ldsB + s_buf * C::B_BYTES));
        s_buf = (s_buf + 1 == NSTAGE) ? 0 : s_buf + 1;
        if (++s_kk == KS) { s_kk = 0; s_tile++; set_aptr(s_tile); }
        issued++;
    };

    // one K-step (64 deep) out of ring slot `cur`; FIRST: accumulators start from 0.
    // Fragments are double-buffered in registers: the six ds_read_b128 of sub-step k2+1 are issued before
    // the MFMAs of sub-step k2, so the LDS round trip hides under the matrix pipe instead of preceding
    // every MFMA pair (what hipcc schedules when it is left one fragment set).
    auto compute = [&](int cur, auto first_tag) {
        constexpr bool FIRST = decltype(first_tag)::value;
        const char *bufA = sA + cur * C::A_BYTES + a_off;
        const char *bufB = sB + cur * C::B_BYTES + b_off;
        uint4 av[2][MI], bv[2][NI];
        auto load_frags = [&](int k2, uint4 (&a)[MI], uint4 (&b)[NI]) {
            const int coff = (c0 ^ (k2 << 1)) << 4;
#pragma unroll
            for (int ni = 0; ni < NI; ni++) b[ni] = *(const uint4 *)(bufB + ni * 32 * BKB + coff);
#pragma unroll
            for (int mi = 0; mi < MI; mi++) a[mi] = *(const uint4 *)(bufA + mi * 32 * BKB + coff);
        };
        load_frags(0, av[0], bv[0]);
#pragma unroll
        for (int k2 = 0; k2 < C::NSUB; k2++) {
            if (k2 < C::NSUB - 1) load_frags(k2 + 1, av[(k2 + 1) & 1], bv[(k2 + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);   // keep the prefetch above the MFMAs (hipcc would sink it)
#pragma unroll
            for (int mi = 0; mi < MI; mi++)
#pragma unroll
                for (int ni = 0; ni < NI; ni++) {
                    if (FIRST && k2 == 0) {
                        f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                        acc[mi][ni] = mfma32<IS_BF16>(av[k2 & 1][mi], bv[k2 & 1][ni], z);
                    } else {
                        acc[mi][ni] = mfma32<IS_BF16>(av[k2 & 1][mi], bv[k2 & 1][ni], acc[mi][ni]);
                    }
                }
        }
    };

    // prologue: fill the slots the staging cursor runs ahead by, wait for the first
#pragma unroll
    for (int i = 0; i < C::AHEAD; i++)
        if (issued < nsteps) stage_next();
    // the first slot must have landed; the stages issued after it may stay in flight
    if (C::AHEAD >= 3 && issued >= 3) wait_vm<2 * C::LOADS>();
    else if (C::AHEAD >= 2 && issued >= 2) wait_vm<C::LOADS>();
    else wait_vm<0>();
    __syncthreads();

    int cur = 0, step = 0, need = 0;
    for (int t = 0; t < ntiles; t++) {
        const int64_t tile_row0 = (t0 + t) * tmul * BM;
        stage_terms(t, tile_row0);
        t_mark = TICK();
        for (int kk = 0; kk < KS; kk++, step++) {
            const long long ts0 = TICK();
            if (issued < nsteps) { if (!(INSTR && (flags & 2))) stage_next(); else { issued++; } }
            const long long ts1 = TICK();
            if (kk == 0) compute(cur, std::true_type{}); else compute(cur, std::false_type{});
            const long long ts2 = TICK();
            // the NEXT step's slot must have landed; a slot beyond it may stay in flight
            if (!(INSTR && (flags & 4))) {
                const int ahead = issued - (step + 2);          // ring stages issued beyond the one the next step needs
                if (C::AHEAD >= 3 && ahead >= 2) wait_vm<2 * C::LOADS>();
                else if (C::AHEAD >= 2 && ahead >= 1) wait_vm<C::LOADS>();
                else wait_vm<0>();
            }
            // sample the compaction request BEFORE the step's barrier: requests are only raised in the filter,
            // i.e. after this barrier (this tile) or before the first barrier of the k-loop (previous tile), so
            // every wave reads the same value and the branch below is workgroup-uniform
            if (!SEED && kk == KS - 1) {
                if (KS == 1) __syncthreads();   // single-step tiles: no k-loop barrier separates the previous filter yet
                need = *s_need;
            }
            __syncthreads();
            if constexpr (INSTR) { if (dbg) t_sync += (ts1 - ts0) + ((TICK() - ts2) << 32); }   // low half: staging issue, high half: wait + barrier
            cur = (cur + 1 == NSTAGE) ? 0 : cur + 1;
        }
        { long long now = TICK(); t_loop += now - t_mark; t_mark = now; }
        // every wave has passed a vmcnt wait and a barrier since the earlier filters: their candidate stores have landed
        if (!SEED && need && !(INSTR && (flags & 32))) serve_compaction();
        { long long now = TICK(); t_comp += now - t_mark; t_mark = now; }
        tile_epilogue(t, tile_row0);
        { long long now = TICK(); t_epi += now - t_mark; t_mark = now; }
        // no wait and no barrier here: a compaction request raised in this filter is served one tile later
    }
    }
    wait_vm<0>();
    __syncthreads();
    if constexpr (SEED) {
        constexpr int GPB = C::WM * MI * 2;
        const int G = nslices * GPB;
#pragma unroll
        for (int mi = 0; mi < MI; mi++)
#pragma unroll
            for (int ni = 0; ni < NI; ni++) {
                const int qcol = q0 + (wc * NI + ni) * 32 + r;
                if (qcol < nq) thr_out[(size_t)qcol * G + slice * GPB + (wr * MI + mi) * 2 + kh] =
                        GM_LDS ? s_gmx[(mi * NI + ni) * 64] : gm[GM_LDS ? 0 : mi][GM_LDS ? 0 : ni];
            }
        return;
    }

    // final: every query's survivors (<= kp best) -> out_c[q][slot][0..kp), and the final threshold
    // (every row this workgroup discarded scored below it) -> thr_out[q][slot] for the certificate
    // Common case: the buffer holds no more than min(64, kp) entries -> they ARE the survivors (a buffer is a dense
    // append list and every entry passed the threshold of its time, which is all the certificate needs), so the wave
    // copies them and keeps the threshold as it stands; the k-th-best search only runs for fuller buffers. The next
    // query's entries are fetched while this one is written (the loop was one dependent L2 round trip + a 32-step
    // ballot search per query: ~3 kcycles x 32 queries per wave, 2 tiles' worth of time on a small shard).
    if (!(INSTR && (flags & 8))) {
        const int qend = nq - q0 < BN ? nq - q0 : BN;
        // DENSE export, common case (a buffer of <= min(64, kp) entries is copied as it stands): the room in the query's list is one
        // returning device-scope atomic per (workgroup, query) -- a ~2-3 k-cycle round trip that the loop below paid once per query,
        // 16-32 times in a row per wave (12 % of a 1M x 384 launch at Q = 256). Lane j makes the reservation of the wave's j-th query:
        // all of them are in flight at once, and the threshold's atomic max (fire-and-forget, the threshold of such a buffer does
        // not move any more) goes out beside it.
        int res_base = 0;
        if (dense_cnt) {
            static_assert(BN / NW <= 64, "one lane per query of the wave");
            const int rq = wave + lane * NW;
            if (rq < qend) {
                const int rm = s_cnt[rq];
                if (rm <= 64 && rm <= kp) {
                    if (rm > 0) res_base = atomicAdd(&dense_cnt[q0 + rq], rm);
                    const float t = s_thr[rq];
                    if (t > -3.0e38f) atomicMax(&dense_thr[q0 + rq], ~score_key(t));
                }
            }
        }
        uint64_t nxt = KEY_INVALID;
        if (wave < qend && lane < s_cnt[wave]) nxt = ld_sc1(my_cand + (size_t)wave * CAP + lane);
        for (int q = wave; q < qend; q += NW) {
            const uint64_t cur = nxt;
            const int qn = q + NW;
            if (qn < qend && lane < s_cnt[qn]) nxt = ld_sc1(my_cand + (size_t)qn * CAP + lane);
            else nxt = KEY_INVALID;
            const int m = s_cnt[q];
            if (dense_cnt) {
                // dense export: the survivors are APPENDED to the query's list (one L2 atomic per (workgroup, query) reserves
                // the room), the final threshold is max-reduced over the workgroups. The lists hold a few dozen keys per
                // query instead of nslices x k' mostly-padding slots, and the certificate reads one threshold, not nslices.
                uint64_t *lst = out_c + (size_t)(q0 + q) * ((size_t)nslices_total * kp);
                if (m <= 64 && m <= kp) {
                    const int base = __shfl(res_base, (q - wave) / NW);      // reserved above, by the lane that stands for this query
                    if (lane < m) lst[base + lane] = cur;
                    continue;                                                // (its threshold went out with the reservation)
                } else {
                    uint64_t *buf = my_cand + (size_t)q * CAP;
                    const int run = compact_wave<CAP>(buf, m, k, kp, s_mar[q], lane, &s_thr[q], &s_cnt[q], &s_trig[q], CAP, nullptr);
                    wait_vm<0>();                    // the compacted buffer was written by this wave: read it back from L2
                    int base = 0;
                    if (lane == 0 && run > 0) base = atomicAdd(&dense_cnt[q0 + q], run);
                    base = __builtin_amdgcn_readfirstlane(base);
                    for (int i = lane; i < run; i += 64) lst[base + i] = ld_sc1(buf + i);
                }
                __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): compact_wave's lane-0 write of s_thr
                if (lane == 0) {
                    const float t = s_thr[q];
                    if (t > -3.0e38f) atomicMax(&dense_thr[q0 + q], ~score_key(t));
                }
                continue;
            }
            const size_t slot = (size_t)(q0 + q) * nslices_total + slice_off + slice;
            if (m <= 64 && m <= kp) {
                uint64_t *dst = out_c + slot * kp;
                for (int i = lane; i < kp; i += 64) dst[i] = i < m ? cur : KEY_INVALID;
            } else {
                compact_wave<CAP>(my_cand + (size_t)q * CAP, m, k, kp, s_mar[q], lane, &s_thr[q], nullptr, nullptr, 0,
                                  out_c + slot * kp);
            }
            if (lane == 0) thr_out[slot] = s_thr[q];
        }
    }
    if constexpr (INSTR) {
        if (dbg) {
            t_fin = TICK() - t_mark;
            if constexpr (I8 && FILT_K == 1) {
                // the whole-tile int8 filter has no drains: the high half of slot 5 holds the WAVE's lane-sites that were entered and
                // appended nothing -- 0 where every class of the corpus is uniform and no row is masked
                int e = (int)n_drain;
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) e += __shfl_xor(e, off);
                n_drain = e;
            }
            if (lane == 0) {
                long long *d = dbg + ((size_t)blockIdx.x * NW + wave) * 8;
                d[0] = t_loop; d[1] = t_epi; d[2] = t_sync; d[3] = t_comp; d[4] = t_fin; d[5] = n_slow | (n_drain << 32); d[6] = n_comp; d[7] = ntiles;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// query preparation for the scan: round to the scan dtype, zero-pad to BN, and
// the per-query terms of the certificate.
//   prep[q] = { eps (score units), scale a, offset b } with
//   s~_units = a * s~' + b  where s~' is the scan's score.
// eps: erel is the operand-rounding error relative to |a||q| -- the query's own rounding rho_q, measured here, and rho_c, for an f32
// corpus scanned through its bf16 shadow the max of |a - shadow(a)| / |a| measured at ingest -- plus the float32 summation (gamma).
// cosine: erel and the normalisation's 4 gamma. ip: erel |q| max|a|.
// l2: -d^2 = 2 a.q - |a|^2 - |q|^2: the operand-rounding part of the error (erel, relative to |a||q|) enters through
// the dot product only, twice; the float32 summation / fma parts scale with the magnitudes (|a| + |q|)^2.
// (Was (2 erel + 6 gamma)(|a| + |q|)^2: four times the needed margin on unit vectors, and f32 corpora under l2
// -- rho_c = 2^-8 -- sent 23-100% of their queries to the wide second scan.)
// ---------------------------------------------------------------------------
// One launch in front of the scans instead of three (memset of the statistics, a norms kernel, a preparation kernel: ~5 us each on
// a search whose whole fixed cost is ~80 us): nb in the reference's arithmetic (sequential float32 chain over the row staged in
// LDS, every lane walks it with broadcast reads -- k_query_norms' method), then the terms above; block 0 also zeroes the
// statistics and every block its query's dense-list counter / threshold.
template <bool IS_BF16>
__global__ __launch_bounds__(64) void k_query_setup(const float *__restrict__ q, float *__restrict__ nb, int compute_nb, int nq,
                                                    int nq_pad, int D, int metric, float max_na, float corpus_rho,
                                                    uint16_t *__restrict__ qs, QPrep *__restrict__ prep, float *__restrict__ mar,
                                                    int64_t *__restrict__ stats, int *__restrict__ dense_cnt,
                                                    unsigned int *__restrict__ dense_thr) {
    __shared__ __attribute__((aligned(16))) float s_row[1024];
    const int qi = blockIdx.x, lane = threadIdx.x;
    if (qi == 0 && stats && lane < 4) stats[lane] = 0;
    uint16_t *dst = qs + (int64_t)qi * D;
    if (qi >= nq) {
        for (int i = lane; i < D; i += 64) dst[i] = 0;
        return;
    }
    if (dense_cnt && lane == 0) { dense_cnt[qi] = 0; dense_thr[qi] = 0u; }
    const float *v = q + (int64_t)qi * D;
    double err2 = 0.0;
    float s = 0.0f;
    for (int j0 = 0; j0 < D; j0 += 1024) {
        const int len = D - j0 < 1024 ? D - j0 : 1024;
        for (int j = lane; j < len; j += 64) {
            const float x = v[j0 + j];
            s_row[j] = x;
            const uint16_t h = IS_BF16 ? f32_to_bf16(x) : f32_to_f16(x);
            const float y = IS_BF16 ? bf16_to_f32(h) : f16_to_f32(h);
            dst[j0 + j] = h;
            const double d = (double)x - (double)y;
            err2 += d * d;
        }
        if (compute_nb) {
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xc07f);    // lgkmcnt(0): the wave's LDS writes have landed
            int j = 0;
            for (; j + 4 <= len; j += 4) {
                const float4 x = *(const float4 *)(s_row + j);
                s = __fadd_rn(s, __fmul_rn(x.x, x.x));
                s = __fadd_rn(s, __fmul_rn(x.y, x.y));
                s = __fadd_rn(s, __fmul_rn(x.z, x.z));
                s = __fadd_rn(s, __fmul_rn(x.w, x.w));
            }
            for (; j < len; j++) s = __fadd_rn(s, __fmul_rn(s_row[j], s_row[j]));
            __builtin_amdgcn_wave_barrier();
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) err2 += __shfl_xor(err2, off);
    if (lane == 0) {
        if (compute_nb) nb[qi] = s; else s = nb[qi];
        double nq2 = (double)s;
        double qn = sqrt(nq2);
        double gamma = (double)D * 5.9604644775390625e-08;           // D * 2^-24
        double rho_q = qn > 0 ? sqrt(err2) / qn : 0.0;
        double rho_c = (double)corpus_rho;
        double erel = 4.0 * gamma + rho_q + rho_c + rho_q * rho_c + 1e-6;
        double maxn = sqrt((double)max_na) * (1.0 + gamma);
        QPrep p;
        if (metric == AK_METRIC_COSINE) {
            p.eps = erel + 4.0 * gamma;
            p.a = qn > 0 ? 1.0 / qn : 0.0;
            p.b = 0.0;
        } else if (metric == AK_METRIC_IP) {
            p.eps = erel * qn * maxn;
            p.a = 1.0; p.b = 0.0;
        } else {
            double ss = qn + maxn;                                   // (the l2 derivation above the kernel)
            p.eps = 2.0 * erel * qn * maxn + 6.0 * gamma * ss * ss;
            p.a = 2.0; p.b = -nq2;
        }
        prep[qi] = p;
        mar[qi] = p.a > 0.0 ? (float)(3.0 * p.eps / p.a * 1.0001) : 3.0e38f;   // 3 eps in scan-score units
    }
}

// ---------------------------------------------------------------------------
// The int8 plan (AK_SCAN_I8): seeding and main pass read an int8 shadow of the 16-bit corpus and int8 queries, with one scale per
// query and, for the rows, one scan-side term per filter class wherever the class's rows can share it (shadow8_scale.h; a row's
// own scale otherwise). The kernel's score is s' = dot_i32 * ea8[row] (ea8 = row scale * ea); with the query's scale folded
// into QPrep::a the true-unit score is a * s' + b as for every other plan, so thresholds, keys and margins of ONE query live in
// that query's own units and QPrep is the only place that converts (lists are per query: nothing compares across queries).
//   eps: |a.q - (s_r a8).(s_q q8)| <= (rho_q + rho_c + rho_q rho_c) |a| |q| with rho_c the measured maximum over the rows
//   (Index::max_rho8) and rho_q measured here; the integer dot product is exact, the one float multiply and the stored terms are
//   covered by the 4 gamma the 16-bit plans carry. At D = 768 on unit Gaussian rows eps ~ 0.6 sigma of the scores, ten times the
//   bf16 scan's: the plan therefore re-ranks k' = 512 candidates and starts the main pass from an EXACT seed threshold.
// ---------------------------------------------------------------------------
__device__ inline float f32_round_down(double s) {
    float f = (float)s;
    if ((double)f > s) {
        uint32_t u = f32_bits(f);
        f = f > 0.f ? bits_f32(u - 1) : (f < 0.f ? bits_f32(u + 1) : -1.0e-45f);
    }
    return f;
}

__global__ __launch_bounds__(64) void k_query_setup8(const float *__restrict__ q, const float *__restrict__ nb, int nq, int D, int metric,
                                                     float max_na, float corpus_rho, int8_t *__restrict__ qs8, QPrep *__restrict__ prep,
                                                     float *__restrict__ mar) {
    const int qi = blockIdx.x, lane = threadIdx.x;
    uint32_t *dst = (uint32_t *)(qs8 + (int64_t)qi * D);
    if (qi >= nq) {
        for (int i = lane; i < D / 4; i += 64) dst[i] = 0u;
        return;
    }
    const float *v = q + (int64_t)qi * D;
    float mx = 0.f;
    for (int i = lane; i < D; i += 64) {
        const float ax = fabsf(v[i]);
        if (ax < __builtin_inff() && ax > mx) mx = ax;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    const float sq = mx / 127.f, inv = sq > 0.f ? 1.f / sq : 0.f;
    double err2 = 0.0;
    for (int i = lane * 4; i < D; i += 256) {
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float x = v[i + j];
            float y = rintf(x * inv);
            y = y > 127.f ? 127.f : (y < -127.f ? -127.f : y);
            if (!(y == y)) y = 0.f;
            const double d = (double)x - (double)sq * (double)y;
            err2 += d * d;
            w |= ((uint32_t)(int)y & 0xffu) << (8 * j);
        }
        dst[i >> 2] = w;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) err2 += __shfl_xor(err2, off);
    if (lane == 0) {
        const double nq2 = (double)nb[qi], qn = sqrt(nq2);
        const double gamma = (double)D * 5.9604644775390625e-08;           // D * 2^-24
        const double rho_q = qn > 0 ? sqrt(err2) / qn : 0.0, rho_c = (double)corpus_rho;
        const double erel = 4.0 * gamma + rho_q + rho_c + rho_q * rho_c + 1e-6;
        const double maxn = sqrt((double)max_na) * (1.0 + gamma);
        QPrep p;
        if (metric == AK_METRIC_COSINE) {
            p.eps = erel + 4.0 * gamma;
            p.a = qn > 0 ? (double)sq / qn : 0.0;
        } else {                                   // inner product (l2 never takes this plan: its additive row term)
            p.eps = erel * qn * maxn;
            p.a = (double)sq;
        }
        p.b = 0.0;
        if (!(p.eps == p.eps) || !(p.a == p.a)) { p.eps = __builtin_inf(); p.a = 0.0; }
        prep[qi] = p;
        mar[qi] = p.a > 0.0 ? (float)(3.0 * p.eps / p.a * 1.0001) : 3.0e38f;   // 3 eps in this query's scan units
    }
}

// A threshold of the 16-bit pre-seeding launch -> the int8 scan's units. t16 is already three eps16 below a k-th best, so
// a16 t16 + b is a lower bound L of the exact k-th best; a row of the exact top-k has a8 s8 + b >= exact - eps8 >= L - eps8.
__global__ void k_thr_to_i8(const QPrep *__restrict__ p16, const QPrep *__restrict__ p8, int nq, float *__restrict__ thr0) {
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    const float t16 = thr0[qi];
    float t = -3.4028234663852886e38f;
    const QPrep a = p16[qi], b = p8[qi];
    if (t16 > -3.0e38f && t16 == t16 && b.a > 0.0) {
        const float f = f32_round_down((a.a * (double)t16 + a.b - b.eps - b.b) / b.a);
        if (f == f && f > t) t = f;
    }
    thr0[qi] = t;
}

// The exact seed threshold: dist [nq][k] are the exact distances of the k best of the seed candidates' best 64, re-ranked by the
// fused tail. The exact k-th best of ANY k rows is a lower bound of the global exact k-th best, whether or not that list
// certified; theta = (it - eps) in the query's scan units is where the main pass starts (raises thr0 only).
__global__ void k_seed_exact_thr(const double *__restrict__ dist, const int *__restrict__ cnt, const QPrep *__restrict__ prep, int nq, int k,
                                 int metric, bool keep, float *__restrict__ thr0) {
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    float t0 = keep ? thr0[qi] : -3.4028234663852886e38f;      // keep: the pre-seeding threshold stands where it is higher
    if (!(t0 == t0)) t0 = -3.4028234663852886e38f;
    const QPrep p = prep[qi];
    if (cnt[qi] == k && p.a > 0.0) {
        const double dk = dist[(int64_t)qi * k + (k - 1)];
        const double t = metric == AK_METRIC_COSINE ? 1.0 - dk : -dk;
        const float f = f32_round_down((t - p.eps - p.b) / p.a);
        if (dk == dk && f == f && f > t0) t0 = f;
    }
    thr0[qi] = t0;
}

// Tail selection of the int8 plan: the dense per-query list -> drop what lies below the cut (the main pass's starting threshold
// and the max-reduced workgroup thresholds, as k_tail does) -> the best kp (512) keys by a bitwise binary search over the 64-bit
// keys (distinct: they carry the row), unordered except that a full selection ends with its worst key, which is what
// k_finalize's list-full rule reads. The keys stay in registers, 16 per thread of a 1024-thread workgroup: the int8 margin lets
// 3-6 k keys per query through at 10M rows, more than an LDS array of the size k_tail sorts would hold. thr_fin[q]: the cut, for
// the certificate; +inf (never certified) when the list is longer than the workgroup holds.
constexpr int SD_THREADS = 1024, SD_EPT = 16, SD_CAP = SD_THREADS * SD_EPT, SD_WAVES = SD_THREADS / 64;
__global__ __launch_bounds__(SD_THREADS) void k_select_dense(const uint64_t *__restrict__ list, int64_t lcap, const int *__restrict__ cnt_g,
                                                             const unsigned int *__restrict__ thr_g, const float *__restrict__ thr0, int kp,
                                                             uint64_t *__restrict__ top, float *__restrict__ thr_fin) {
    __shared__ int s_pos;
    __shared__ int s_c[2][SD_WAVES];
    const int qi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float theta = thr0 ? thr0[qi] : -__builtin_inff();
    if (!(theta == theta)) theta = -__builtin_inff();
    const unsigned int tg = thr_g[qi];
    const float tmax = tg ? key_score(~tg) : -__builtin_inff();
    const float cutoff = tmax > theta ? tmax : theta;
    const uint32_t cut_key = score_key(cutoff);
    int64_t n = cnt_g[qi];
    if (n > lcap) n = lcap;
    const bool overflow = n > SD_CAP;
    if (overflow) n = SD_CAP;
    if (tid == 0) {
        s_pos = 0;
        thr_fin[qi] = overflow ? __builtin_inff() : (cutoff > -3.0e38f ? cutoff : -3.4028234663852886e38f);
    }
    const uint64_t *lst = list + (int64_t)qi * lcap;
    uint64_t key[SD_EPT];
    int c = 0;
#pragma unroll
    for (int e = 0; e < SD_EPT; e++) {
        const int idx = e * SD_THREADS + tid;
        uint64_t k = idx < n ? lst[idx] : KEY_INVALID;
        if ((uint32_t)(k >> 32) > cut_key) k = KEY_INVALID;
        key[e] = k;
        c += __popcll(__ballot(k != KEY_INVALID));
    }
    auto block_sum = [&](int v, int par) {          // v is wave-uniform; one barrier, the two parities alternate
        if (lane == 0) s_c[par][wave] = v;
        __syncthreads();
        int tot = 0;
#pragma unroll
        for (int w = 0; w < SD_WAVES; w++) tot += s_c[par][w];
        return tot;
    };
    const int have = block_sum(c, 0);
    uint64_t *dst = top + (int64_t)qi * kp;
    uint64_t th = KEY_INVALID;                       // keep every key below th; th itself goes last
    if (have >= kp) {                                // (exactly kp survivors: all are kept, the search finds the worst of them)
        th = 0;
        for (int bit = 63; bit >= 0; bit--) {
            const uint64_t test = th | ((1ull << bit) - 1ull);
            int cc = 0;
#pragma unroll
            for (int e = 0; e < SD_EPT; e++) cc += __popcll(__ballot(key[e] <= test));
            if (block_sum(cc, bit & 1) < kp) th |= (1ull << bit);      // bit 63 takes parity 1: the count above took 0
        }
        // th = the kp-th smallest key: kp - 1 keys lie below it
    }
#pragma unroll
    for (int e = 0; e < SD_EPT; e++) {
        if (key[e] < th) dst[atomicAdd(&s_pos, 1)] = key[e];
        else if (key[e] == th && have >= kp) dst[kp - 1] = key[e];
    }
    if (have < kp)
        for (int i = have + tid; i < kp; i += SD_THREADS) dst[i] = KEY_INVALID;
}

// Seeding pass -> per-query initial threshold for the main pass, in scan-score units:
// (k-th best approximate score of the seed rows) - 3 eps'. The k-th best of a subset is a lower
// bound of the global k-th best, so no row that could reach the exact top-k is discarded.
__device__ inline float seed_threshold(float kth_score, const QPrep &p) {
    float t = -3.4028234663852886e38f;
    if (kth_score > -__builtin_inff() && p.a > 0.0) {
        double s = (double)kth_score - 3.0 * p.eps / p.a;
        float f = (float)s;
        if ((double)f > s) {   // round toward -inf: step one ulp down
            uint32_t u = f32_bits(f);
            f = f > 0.f ? bits_f32(u - 1) : (f < 0.f ? bits_f32(u + 1) : -1.0e-45f);
        }
        if (f == f && f > t) t = f;
    }
    return t;
}

// thr0[q] = max(thr0[q] if KEEP, threshold from the k-th best seed candidate)
template <bool KEEP>
__global__ void k_seed_thr(const uint64_t *__restrict__ top_kp, const QPrep *__restrict__ prep, int nq, int k,
                           int kp, float *__restrict__ thr0) {
    int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    uint64_t key = top_kp[(int64_t)qi * kp + (k - 1)];
    float t = key != KEY_INVALID ? seed_threshold(key_score((uint32_t)(key >> 32)), prep[qi]) : -3.4028234663852886e38f;
    if (KEEP) t = fmaxf(t, thr0[qi]);
    thr0[qi] = t;
}

// Seeding pass -> threshold: k-th best approximate score among the seed candidates of query q
// (keys[q*in_stride .. +n_in), unordered, KEY_INVALID padded), minus 3 eps'. Only the k-th score is
// needed, so instead of a top-k selection this is a bitwise binary search over the score halves of the
// keys: 256 threads hold EPT keys each; every step is a ballot count and one barrier.
// dense_cnt (nullable): the lists are the dense per-query append lists of the scan; only cnt[q] entries are valid.
template <int EPT, bool KEEP>
__global__ __launch_bounds__(256) void k_seed_kth_lists(const uint64_t *__restrict__ keys, int64_t n_in, int64_t in_stride,
                                                        const QPrep *__restrict__ prep, int k, float *__restrict__ thr0,
                                                        const int *__restrict__ dense_cnt) {
    __shared__ int s_c[2][4];
    const int qi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t *kin = keys + (int64_t)qi * in_stride;
    if (dense_cnt) { const int64_t c = dense_cnt[qi]; n_in = c < n_in ? c : n_in; }
    const int e_used = (int)((n_in + 255) >> 8);          // block-uniform: short lists skip most of the ballots
    uint32_t key[EPT];
#pragma unroll
    for (int e = 0; e < EPT; e++) {
        const int64_t idx = (int64_t)e * 256 + tid;
        key[e] = (e < e_used && idx < n_in) ? (uint32_t)(kin[idx] >> 32) : 0xffffffffu;
    }
    uint32_t th = 0;
    for (int bit = 31; bit >= 0; bit--) {
        const uint32_t test = th | ((1u << bit) - 1u);
        int c = 0;
#pragma unroll
        for (int e = 0; e < EPT; e++) if (e < e_used) c += __popcll(__ballot(key[e] <= test));
        if (lane == 0) s_c[bit & 1][wave] = c;
        __syncthreads();
        const int tot = s_c[bit & 1][0] + s_c[bit & 1][1] + s_c[bit & 1][2] + s_c[bit & 1][3];
        if (tot < k) th |= (1u << bit);
    }
    if (tid == 0) {
        float t = th != 0xffffffffu ? seed_threshold(key_score(th), prep[qi]) : -3.4028234663852886e38f;
        if (KEEP) t = fmaxf(t, thr0[qi]);
        thr0[qi] = t;
    }
}

// Pre-seeding: thr0[q] = (k-th largest of the G group maxima of query q) - 3 eps'. One wave per query,
// bitwise binary search over the order-preserving score keys (<= 16 per lane, register-resident).
__global__ __launch_bounds__(64) void k_seed_kth(const float *__restrict__ gmax, int G, const QPrep *__restrict__ prep,
                                                 int k, float *__restrict__ thr0) {
    const int qi = blockIdx.x, lane = threadIdx.x;
    uint32_t key[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int idx = j * 64 + lane;
        float v = idx < G ? gmax[(int64_t)qi * G + idx] : -__builtin_inff();
        key[j] = score_key(v == v ? v : -__builtin_inff());
    }
    uint32_t th = 0;
    for (int bit = 31; bit >= 0; bit--) {
        const uint32_t test = th | ((1u << bit) - 1u);
        int c = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) c += __popcll(__ballot(key[j] <= test));
        if (c < k) th |= (1u << bit);
    }
    // fewer than k finite maxima: the search ends on the -inf key (or all ones) and no threshold is set
    if (lane == 0) thr0[qi] = seed_threshold(key_score(th), prep[qi]);
}

// Final selection + certificate + output, one wave per query (replaces a k-round block select plus a
// one-thread-per-query certificate kernel: ~70 us -> ~10 us at 1024 queries).
//   top_kp  [nq][kp]  approx keys, ascending (best first)
//   rr_keys/rr_ids [nq][kp] exact distance keys / ids of the re-ranked candidates (any order)
// The k best by (distance key asc, id asc) go to out_ids/out_dist; cert[q] = 1 when no non-candidate row
// can reach them: k-th exact score > bound of every discarded row.
template <int NS>
__global__ __launch_bounds__(64) void k_finalize(const uint64_t *__restrict__ top_kp, const uint64_t *__restrict__ rr_keys,
                                                 const int64_t *__restrict__ rr_ids, const QPrep *__restrict__ prep,
                                                 const float *__restrict__ nb, const float *__restrict__ thr_slots, int nslots,
                                                 int k, int kp, int metric, int64_t *__restrict__ out_ids,
                                                 double *__restrict__ out_dist, int *__restrict__ out_cnt,
                                                 int *__restrict__ cert, int64_t *__restrict__ stats) {
    const int qi = blockIdx.x, lane = threadIdx.x;
    uint64_t ek[NS];
    int64_t ei[NS];
    int valid_c = 0;
    uint64_t last_c = KEY_INVALID;
#pragma unroll
    for (int j = 0; j < NS; j++) {
        const int idx = j * 64 + lane;
        ek[j] = idx < kp ? rr_keys[(int64_t)qi * kp + idx] : KEY_INVALID;
        ei[j] = (idx < kp && ek[j] != KEY_INVALID) ? rr_ids[(int64_t)qi * kp + idx] : INT64_MAX;
        const uint64_t c = idx < kp ? top_kp[(int64_t)qi * kp + idx] : KEY_INVALID;
        valid_c += __popcll(__ballot(c != KEY_INVALID));
        if (idx == kp - 1) last_c = c;
    }
    last_c = __shfl(last_c, (kp - 1) & 63);
    int cnt = 0;
    double dk = 0.0;
    for (int round = 0; round < k; round++) {
        uint64_t bk = KEY_INVALID;
        int64_t bi = INT64_MAX;
#pragma unroll
        for (int j = 0; j < NS; j++)
            if (ek[j] < bk || (ek[j] == bk && ei[j] < bi)) { bk = ek[j]; bi = ei[j]; }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const uint64_t k2 = __shfl_xor(bk, off);
            const int64_t i2 = __shfl_xor(bi, off);
            if (k2 < bk || (k2 == bk && i2 < bi)) { bk = k2; bi = i2; }
        }
        const bool valid = bk != KEY_INVALID;
        const double d = valid ? key_dist(bk) : __builtin_nan("");
        if (lane == 0) {
            out_ids[(int64_t)qi * k + round] = valid ? bi : -1;
            out_dist[(int64_t)qi * k + round] = d;
        }
        if (!valid) {   // exhausted (wave-uniform): pad the tail
            for (int r2 = round + 1 + lane; r2 < k; r2 += 64) {
                out_ids[(int64_t)qi * k + r2] = -1;
                out_dist[(int64_t)qi * k + r2] = __builtin_nan("");
            }
            break;
        }
        cnt++; dk = d;
#pragma unroll
        for (int j = 0; j < NS; j++)
            if (ek[j] == bk && ei[j] == bi) { ek[j] = KEY_INVALID; ei[j] = INT64_MAX; }
    }
    // non-candidates: rows below a workgroup's final threshold, and (when the merged candidate list is
    // full) rows below its kp-th entry
    float smin = -__builtin_inff();
    for (int j = lane; j < nslots; j += 64) {
        const float t = thr_slots[(int64_t)qi * nslots + j];
        if (t > -3.0e38f) smin = fmaxf(smin, t);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) smin = fmaxf(smin, __shfl_xor(smin, off));
    if (lane != 0) return;
    if (out_cnt) out_cnt[qi] = cnt;
    int ok = 0;
    const float nbq = nb[qi];
    const bool qfinite = nbq > 0.f && nbq < __builtin_inff();
    if (cnt == k && qfinite && dk == dk) {
        const QPrep p = prep[qi];
        if (valid_c == kp) smin = fmaxf(smin, key_score((uint32_t)(last_c >> 32)));
        if (smin == -__builtin_inff()) ok = 1;  // every finite-score row was a candidate
        else {
            const double bound = p.a * (double)smin + p.b + p.eps;   // upper bound of any non-candidate's exact score
            double t;
            if (metric == AK_METRIC_COSINE) t = 1.0 - dk;
            else if (metric == AK_METRIC_IP) t = -dk;
            else t = -dk * dk;
            ok = t > bound;
        }
    }
    cert[qi] = ok;
    if (stats) atomicAdd((unsigned long long *)&stats[2], (unsigned long long)valid_c);
}

// ---------------------------------------------------------------------------
// host side: plan entry points, launch, the stages of a search (scan_plan.h: the tile table, the plan, the workspace layout)
// ---------------------------------------------------------------------------
static ScanShape shape_of(const Index &ix) { return ScanShape{ix.n, ix.dim, ix.dtype, ix.metric}; }
static int sw_get(const std::atomic<int> &s) { return s.load(std::memory_order_relaxed); }
static PlanSwitches plan_switches() {
    const Switches &s = switches();
    return PlanSwitches{sw_get(s.scan_cfg), sw_get(s.scan_i8), sw_get(s.scan_blocks), sw_get(s.scan_r192_pm), sw_get(s.scan_no192),
                        sw_get(s.seed_ratio), sw_get(s.seed_div), sw_get(s.pre_div), sw_get(s.scan_noseed), sw_get(s.scan_nopre)};
}

bool fast_supported(const Index &ix, int nq, int k) { return fast_supported(shape_of(ix), nq, k); }

// the plan's workspace; the selection scratch behind its lists is sized by its owners (exact.hip, select.hip)
static ScanWorkspace workspace_of(const Index &ix, const FastPlan &p, int nq, int k) {
    const int64_t lists = (int64_t)(p.nslices + p.ns_seed) * p.kprime;
    return scan_workspace(p, shape_of(ix), nq, k, select_scratch_bytes(nq, lists, p.kprime) + select_keys_scratch_bytes(nq, lists, p.kprime));
}

FastPlan fast_plan(const Index &ix, int nq, int k, bool widest, bool allow_i8) {
    FastPlan p = scan_plan(shape_of(ix), plan_switches(), nq, k, widest, allow_i8);
    p.bytes = workspace_of(ix, p, nq, k).bytes;
    return p;
}

// AK_SCAN_DBG / AK_SCAN_ABLATE (measurement only) select the instrumented instantiation of the main-pass kernels
static int scan_ablate_flags() { return sw_get(switches().scan_ablate); }
static bool scan_instrumented() { return sw_get(switches().scan_dbg) != 0 || scan_ablate_flags() != 0; }

// One k_scan launch. The first line is the search's own; the three passes (pre-seeding, seeding, main) differ in the rest.
struct ScanArgs {
    const Index &ix; const uint8_t *filter_dev; hipStream_t st; const uint16_t *qs; const float *mar; int nq, nqg, k, kp;
    int64_t row_begin = 0, row_end = 0;
    int ns = 0, slice_off = 0, ns_total = 0;
    const float *thr0 = nullptr;
    uint64_t *cand = nullptr, *out_c = nullptr;
    float *thr_slots = nullptr;                              // (the pre-seeding launch: its group maxima)
    long long *dbg = nullptr;
    int64_t sample_tiles = 0; int tstride = 1;               // pre-seeding only
    int *dense_cnt = nullptr; unsigned int *dense_thr = nullptr;
};

template <bool BF, class C, bool SEED, bool SEEDPASS>
static int launch_scan(const ScanArgs &a) {
    static std::atomic<bool> attr_set{false};
    constexpr int LDSB = SEED ? C::SEED_LDS_BYTES : C::LDS_BYTES;
    if (!attr_set) {
        AK_HIP(hipFuncSetAttribute((const void *)k_scan<BF, C, SEED, false, SEEDPASS>, hipFuncAttributeMaxDynamicSharedMemorySize, LDSB));
        if constexpr (!SEED && DBG_KERNELS)
            AK_HIP(hipFuncSetAttribute((const void *)k_scan<BF, C, SEED, true, SEEDPASS>, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES));
        attr_set = true;
    }
    const Index &ix = a.ix;
    const uint16_t *rows16 = (const uint16_t *)(C::I8 ? (const void *)ix.rows8 : (ix.dtype == AK_DTYPE_F32 ? ix.shadow : ix.rows));
    const float *ea = C::I8 ? ix.ea8 : ix.ea, *gb = C::I8 ? ix.gb8 : ix.gb;      // int8: the scale-folded terms; eb (0 / -inf) is the index's own
    const int64_t gbb = (ix.n + 31) / 32;
    bool instr = false;
    if constexpr (!SEED) instr = scan_instrumented();
    if (instr) {
        if constexpr (!DBG_KERNELS) AK_FAIL(-1, "AK_SCAN_DBG and the scan ablation switch need libarchi_hip_dbg.so (make -C archi_amd/csrc dbg): the product library carries no instrumented scan kernels");
        if constexpr (!SEED && DBG_KERNELS)
            k_scan<BF, C, SEED, true, SEEDPASS><<<(unsigned)(a.ns * a.nqg), C::THREADS, C::LDS_BYTES, a.st>>>(
                rows16, ea, ix.eb, gb, gbb, a.filter_dev, a.row_begin, a.row_end, ix.dim, a.qs, a.nq, a.ns, a.nqg, a.k, a.kp, a.thr0, a.mar, a.slice_off,
                a.ns_total, a.cand, a.out_c, a.thr_slots, scan_ablate_flags(), a.dbg, a.sample_tiles, a.tstride, a.dense_cnt, a.dense_thr);
    } else {
        k_scan<BF, C, SEED, false, SEEDPASS><<<(unsigned)(a.ns * a.nqg), C::THREADS, LDSB, a.st>>>(
            rows16, ea, ix.eb, gb, gbb, a.filter_dev, a.row_begin, a.row_end, ix.dim, a.qs, a.nq, a.ns, a.nqg, a.k, a.kp, a.thr0, a.mar, a.slice_off,
            a.ns_total, a.cand, a.out_c, a.thr_slots, 0, nullptr, a.sample_tiles, a.tstride, a.dense_cnt, a.dense_thr);
    }
    AK_HIP(hipGetLastError());
    return 0;
}

// Tile dispatch: tile number -> f(tag), f's int. A tag names the type the tile ships on and, for the phased tiles, the family of
// its MFMA shapes and filter arrangements (Shaped<shape, arrangement>).
template <class C> struct TileTag { using Shipped = C; static constexpr bool PHASED = false; };
template <template <int, int> class T, class C> struct PhasedTag { using Shipped = C; static constexpr bool PHASED = true; template <int S, int F> using Shaped = T<S, F>; };
template <class F> static int visit_tile(int cfg, F &&f) {
    switch (cfg) {
        case CFG_L: return f(TileTag<CfgL>{});
        case CFG_M: return f(TileTag<CfgM>{});
        case CFG_S: return f(TileTag<CfgS>{});
        case CFG_P: return f(PhasedTag<CfgPs, CfgP>{});
        case CFG_Q: return f(PhasedTag<CfgQs, CfgQ>{});
        case CFG_R: return f(PhasedTag<CfgRs, CfgR>{});
    }
    AK_FAIL(-1, "scan: no such tile configuration");
}
// The type a seeding or main pass of a tile runs: the shipped one. The dbg library carries both shapes and both arrangements of the
// phased tiles and honours AK_SCAN_MFMA / AK_SCAN_FILTER (the product library's ak_debug_set refuses them, and a value in its
// environment is ignored).
template <class Tag, class F> static int with_forced_shape(Tag, F &&f) {
    using C = typename Tag::Shipped;
    if constexpr (DBG_KERNELS && Tag::PHASED) {
        const int mfma = sw_get(switches().scan_mfma), filt = sw_get(switches().scan_filter) - 1;      // 0 / -1: as the tile ships
        if ((mfma ? mfma : C::MFMA) == 32) return f(TileTag<typename Tag::template Shaped<32, 0>>{});
        if ((filt < 0 ? C::FILT : filt) == 1) return f(TileTag<typename Tag::template Shaped<16, 1>>{});
        return f(TileTag<typename Tag::template Shaped<16, 0>>{});
    } else {
        return f(TileTag<C>{});
    }
}
// Arrangement of a pass of the int8 tile, dbg library: AK_SCAN_HITQ says which passes run queued, the others -- and all of them
// without it -- what AK_SCAN_FILTER says or, unforced, what they ship on (whole tile where that is the queue and the queue is
// switched off)
static int p8_filt(bool seedpass) {
    const int hitq = sw_get(switches().scan_hitq), filt = sw_get(switches().scan_filter) - 1;
    const int shipped = seedpass ? SHIP_FILT_P8_SEED : SHIP_FILT_P8;
    if (hitq && hitq != 4 && (hitq & (seedpass ? 1 : 2))) return 2;
    if (filt >= 0) return filt;
    return hitq && shipped == 2 ? 1 : shipped;
}
// the int8 plan: one tile, one element type; its two passes take their arrangements on their own
template <bool SEEDPASS, class F> static int with_tile8(F &&f) {
    if constexpr (DBG_KERNELS) {
        switch (p8_filt(SEEDPASS)) {
            case 0: return f(TileTag<CfgP8of<SEEDPASS, 0>>{});
            case 1: return f(TileTag<CfgP8of<SEEDPASS, 1>>{});
            default: return f(TileTag<CfgP8of<SEEDPASS, 2>>{});
        }
    } else {
        return f(TileTag<CfgP8>{});
    }
}

// One fast_search call: what its stages share, and the stages in the order they run
struct Search {
    Index &ix; const FastPlan &plan; const float *queries_dev; float *nb_dev; int nq, k; const uint8_t *filter_dev;
    int64_t *out_ids_dev; double *out_dist_dev; int *out_cnt_dev, *cert_dev; int64_t *stats_dev; void *ws; hipStream_t st;
    ScanWorkspace w;
    bool i8, dense, bf;
    int kp, ns_tot;
    int *dcnt; unsigned int *dthr;                                   // the dense lists' counters and thresholds; NULL on the slot layout
    long long *dbg0 = nullptr, *dbg1 = nullptr;
    const float *thr_seed = nullptr, *thr_main = nullptr;            // starting thresholds of the seeding / the main pass
    template <class T> T *at(const WsRegion<T> &r) const { return r.at(ws); }

    int query_setup(bool nb_ready) const {
        const int nq_pad = plan.nqg * g_cfgs[plan.cfg].bn, compute_nb = nb_ready ? 0 : 1;
        // f32 corpora are scanned through their bf16 shadow (candidates only; the re-rank reads the f32 rows)
        const float rho = ix.dtype == AK_DTYPE_F32 ? ix.max_rho : 0.f;
        if (bf) k_query_setup<true><<<nq_pad, 64, 0, st>>>(queries_dev, nb_dev, compute_nb, nq, nq_pad, ix.dim, ix.metric, ix.max_na, rho, at(w.qs), at(w.prep),
                                                          at(w.mar), stats_dev, dcnt, dthr);
        else k_query_setup<false><<<nq_pad, 64, 0, st>>>(queries_dev, nb_dev, compute_nb, nq, nq_pad, ix.dim, ix.metric, ix.max_na, 0.f, at(w.qs), at(w.prep),
                                                        at(w.mar), stats_dev, dcnt, dthr);
        if (i8) k_query_setup8<<<nq_pad, 64, 0, st>>>(queries_dev, nb_dev, nq, ix.dim, ix.metric, ix.max_na, ix.max_rho8, at(w.qs8), at(w.prep8), at(w.mar8));
        AK_HIP(hipGetLastError());
        return 0;
    }

    // pre-seeding: group maxima over a strided sample -> first thresholds
    int pre_seed() {
        ScanArgs a{ix, filter_dev, st, at(w.qs), at(w.mar), nq, plan.nqg, k, kp};      // the 16-bit queries on every plan
        a.row_end = ix.n; a.ns = plan.pre_slices; a.thr_slots = at(w.gmax); a.sample_tiles = plan.pre_tiles; a.tstride = plan.pre_stride;
        // the pre-seeding launch stays on 32x32x16 whatever the tile ships
        const int rc = visit_tile(plan.cfg, [&](auto tag) {
            using C = typename decltype(tag)::Shipped::Shape32;
            return bf ? launch_scan<true, C, true, false>(a) : launch_scan<false, C, true, false>(a);
        });
        if (rc) return rc;
        k_seed_kth<<<nq, 64, 0, st>>>(at(w.gmax), plan.pre_slices * (g_cfgs[plan.cfg].bm / 16), at(w.prep), k, at(w.thr0));
        if (i8) k_thr_to_i8<<<(nq + 63) / 64, 64, 0, st>>>(at(w.prep), at(w.prep8), nq, at(w.thr0));      // the 16-bit sample's threshold in int8 units
        AK_HIP(hipGetLastError());
        thr_seed = thr_main = at(w.thr0);
        return 0;
    }

    // seeding (SEEDPASS) or main pass: rows [r0, r1) in ns slices, into slots [soff, soff + ns)
    template <bool SEEDPASS> int scan_pass(int64_t r0, int64_t r1, int ns, const float *thr, int soff, long long *dbg) const {
        ScanArgs a{ix, filter_dev, st, at(w.qs), at(w.mar), nq, plan.nqg, k, kp};
        a.row_begin = r0; a.row_end = r1; a.ns = ns; a.slice_off = soff; a.ns_total = ns_tot; a.thr0 = thr; a.dbg = dbg;
        a.cand = at(w.cand); a.out_c = at(w.out_c); a.thr_slots = at(w.thr_slots); a.dense_cnt = dcnt; a.dense_thr = dthr;
        if (i8) {
            a.qs = (const uint16_t *)at(w.qs8); a.mar = at(w.mar8);
            return with_tile8<SEEDPASS>([&](auto t) { return launch_scan<true, typename decltype(t)::Shipped, false, SEEDPASS>(a); });
        }
        return visit_tile(plan.cfg, [&](auto tag) {
            return with_forced_shape(tag, [&](auto t) {
                using C = typename decltype(t)::Shipped;
                return bf ? launch_scan<true, C, false, SEEDPASS>(a) : launch_scan<false, C, false, SEEDPASS>(a);
            });
        });
    }

    // seeding pass over rows [0, seed_rows) and its threshold: per-query thresholds for the main pass
    int seed_pass() {
        const int nss = plan.ns_seed;
        uint64_t *out_c = at(w.out_c);
        float *thr0 = at(w.thr0);
        int rc = scan_pass<true>(0, plan.seed_rows, nss, thr_seed, 0, dbg0);
        if (rc) return rc;
        if (i8) {
            // the int8 seeding pass is followed by the exact seed threshold: the fused tail re-ranks the best 64 seed candidates of every
            // query in the reference arithmetic (its usual work, on the lists as they stand before the main pass) and k_seed_exact_thr
            // turns their exact k-th best into theta. "k-th best approximate score - 3 eps" with the int8 eps lets 10-20 k rows
            // per query through the main pass (docs/EXPERIMENTS.md, "int8 shadow"); this one about as many as the bf16 plan.
            rc = fused_tail(ix, queries_dev, nb_dev, nq, k, out_c, (int64_t)ns_tot * kp, at(w.d_cnt), at(w.d_thr), thr_seed, at(w.prep8), at(w.fin_i),
                            at(w.fin_d), at(w.sd_cnt), at(w.sd_cert), nullptr, st);
            if (rc) return rc;
            k_seed_exact_thr<<<(nq + 63) / 64, 64, 0, st>>>(at(w.fin_d), at(w.sd_cnt), at(w.prep8), nq, k, ix.metric, thr_seed != nullptr, thr0);
        } else {
            // top-k of the seed candidates (slots [0,nss) of out_c -- or, dense, the lists as they stand; the main pass has not
            // written yet). Only the k-th best is needed here: k selection rounds, not kp
            const int64_t seed_in = (int64_t)nss * kp, seed_stride = (int64_t)ns_tot * kp;
#define KTH(EPT)                                                                                                                \
    do {                                                                                                                        \
        if (thr_seed) k_seed_kth_lists<EPT, true><<<nq, 256, 0, st>>>(out_c, seed_in, seed_stride, at(w.prep), k, thr0, dcnt);    \
        else k_seed_kth_lists<EPT, false><<<nq, 256, 0, st>>>(out_c, seed_in, seed_stride, at(w.prep), k, thr0, dcnt);            \
    } while (0)
            if (seed_in <= 16 * 256) KTH(16);
            else if (seed_in <= 32 * 256) KTH(32);
            else if (seed_in <= 64 * 256) KTH(64);
            else {
                if (dense) AK_FAIL(-1, "fast_search: dense lists with more than 16384 seed candidates");   // kp = 64, nss <= 256
                rc = select_topk_strided(out_c, nq, seed_in, seed_stride, k, at(w.top_k), at(w.top_i), at(w.scratch), st);
                if (rc) return rc;
                if (thr_seed) k_seed_thr<true><<<(nq + 63) / 64, 64, 0, st>>>(at(w.top_k), at(w.prep), nq, k, k, thr0);
                else k_seed_thr<false><<<(nq + 63) / 64, 64, 0, st>>>(at(w.top_k), at(w.prep), nq, k, k, thr0);
            }
#undef KTH
        }
        AK_HIP(hipGetLastError());
        thr_main = thr0;
        return 0;
    }

    int tail() const {
        const int64_t lists = (int64_t)ns_tot * kp;
        uint64_t *out_c = at(w.out_c), *top_k = at(w.top_k), *rr_k = at(w.rr_k);
        int64_t *rr_i = at(w.rr_i);
        int rc = 0;
        if (i8) {
            // the int8 tail: best 512 of the dense list -> exact re-rank against the stored 16-bit rows -> top-k + certificate with
            // the int8 eps (one cut for the whole query where the slot layout had one threshold per slice)
            ix.s8_searches.fetch_add(1, std::memory_order_relaxed);
            k_select_dense<<<nq, SD_THREADS, 0, st>>>(out_c, lists, at(w.d_cnt), at(w.d_thr), thr_main, kp, top_k, at(w.thr_fin));
            AK_HIP(hipGetLastError());
            rc = rerank(ix, queries_dev, nb_dev, nq, kp, top_k, rr_k, rr_i, st);
            if (rc) return rc;
            k_finalize<8><<<nq, 64, 0, st>>>(top_k, rr_k, rr_i, at(w.prep8), nb_dev, at(w.thr_fin), 1, k, kp, ix.metric, out_ids_dev, out_dist_dev,
                                             out_cnt_dev, cert_dev, stats_dev);
            AK_HIP(hipGetLastError());
            return 0;
        }
        if (dense)
            return fused_tail(ix, queries_dev, nb_dev, nq, k, out_c, lists, at(w.d_cnt), at(w.d_thr), thr_main, at(w.prep), out_ids_dev, out_dist_dev,
                              out_cnt_dev, cert_dev, stats_dev, st);
        rc = select_keys_topk(out_c, nq, lists, lists, kp, top_k, at(w.scratch), st);
        if (rc) return rc;
        rc = rerank(ix, queries_dev, nb_dev, nq, kp, top_k, rr_k, rr_i, st);
        if (rc) return rc;
#define FIN(NS) k_finalize<NS><<<nq, 64, 0, st>>>(top_k, rr_k, rr_i, at(w.prep), nb_dev, at(w.thr_slots), ns_tot, k, kp, ix.metric, out_ids_dev, \
                                                  out_dist_dev, out_cnt_dev, cert_dev, stats_dev)
        if (kp <= 64) FIN(1); else if (kp <= 128) FIN(2); else if (kp <= 256) FIN(4); else FIN(8);
#undef FIN
        AK_HIP(hipGetLastError());
        return 0;
    }
};

int fast_search(Index &ix, const float *queries_dev, float *nb_dev, bool nb_ready, int nq, int k, const uint8_t *filter_dev,
                int64_t *out_ids_dev, double *out_dist_dev, int *out_cnt_dev, int *cert_dev, int64_t *stats_dev,
                void *ws, const FastPlan &plan, hipStream_t st) {
    if (plan.i8) {
        // the shadow is +50 % of the corpus: on a device too full for it the search runs the 16-bit plan it ran before the int8
        // plan existed (same tile and slices, k' = 64) in the workspace it was handed: that plan's layout has to end inside it
        // (tests/native/scan_plan_main.cpp holds that over the plan's whole range)
        const int src = ensure_shadow8(ix, st);
        if (src == AK_SHADOW8_NOMEM) {
            const FastPlan alt = fast_plan(ix, nq, k, false, false);
            if (alt.bytes > plan.bytes) AK_FAIL(-10, "fast_search: no memory for the int8 shadow and the workspace does not hold the 16-bit plan");
            return fast_search(ix, queries_dev, nb_dev, nb_ready, nq, k, filter_dev, out_ids_dev, out_dist_dev, out_cnt_dev, cert_dev,
                               stats_dev, ws, alt, st);
        }
        if (src) return src;
        if (plan.cfg != CFG_P || plan.kprime != I8_KP) AK_FAIL(-1, "fast_search: the int8 plan is tile P with k' = 512");
    }
    Search s{ix, plan, queries_dev, nb_dev, nq, k, filter_dev, out_ids_dev, out_dist_dev, out_cnt_dev, cert_dev, stats_dev, ws, st,
             workspace_of(ix, plan, nq, k)};
    s.i8 = plan.i8 != 0;
    s.kp = plan.kprime;
    s.ns_tot = plan.nslices + plan.ns_seed;
    // The common plan (k' = 64, i.e. k <= 16) runs with dense candidate lists and the fused tail kernel; the wide plans
    // (k' = 128 / 256 / 512: large k, second-chance scans) keep the slot layout and the three-kernel tail.
    s.dense = s.i8 || (s.kp == TAIL_KP && ix.dim <= TAIL_MAX_DIM && !sw_get(switches().tail_old));
    s.dcnt = s.dense ? s.at(s.w.d_cnt) : nullptr;
    s.dthr = s.dense ? s.at(s.w.d_thr) : nullptr;
    s.bf = ix.dtype != AK_DTYPE_F16;
    int rc = s.query_setup(nb_ready);
    if (rc) return rc;

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::unique_lock<std::mutex> prof_lk(ix.prof_mu, std::defer_lock);   // concurrent host searches share the index under a shared lock
    const bool want_dbg = sw_get(switches().scan_dbg) != 0;
    if (ix.profile || want_dbg) prof_lk.lock();
    if (ix.profile) {
        if (ix.prof_used == ix.prof_events.size()) {
            hipEvent_t a, b;
            AK_HIP(hipEventCreate(&a));
            AK_HIP(hipEventCreate(&b));
            ix.prof_events.emplace_back(a, b);
        }
        ev0 = ix.prof_events[ix.prof_used].first;
        ev1 = ix.prof_events[ix.prof_used].second;
        ix.prof_used++;
    }
    if (want_dbg) {
        if (!ix.dbg_dev) { AK_HIP(hipMalloc((void **)&ix.dbg_dev, 2 * 65536 * 8)); }
        AK_HIP(hipMemsetAsync(ix.dbg_dev, 0, 2 * 65536 * 8, st));
        s.dbg0 = ix.dbg_dev; s.dbg1 = ix.dbg_dev + 65536;
    }
    if (plan.pre_tiles > 0 && (rc = s.pre_seed())) return rc;
    if (plan.ns_seed > 0 && (rc = s.seed_pass())) return rc;
    if (ev0) AK_HIP(hipEventRecord(ev0, st));   // the timed "dominant kernel" is the main-pass launch
    rc = s.scan_pass<false>(plan.seed_rows, ix.n, plan.nslices, s.thr_main, plan.ns_seed, s.dbg1);
    if (rc) return rc;
    if (ev1) AK_HIP(hipEventRecord(ev1, st));
    return s.tail();
}

}  // namespace ak
