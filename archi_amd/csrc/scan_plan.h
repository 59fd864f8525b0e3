// scan_plan.h -- the HOST-SIDE plan of the kNN scan (scan.hip), as host-only C++ (no HIP in here): the tile types and their table,
// which tile a batch runs on (pick_cfg), how a search is cut into slices, a seeding pass and a pre-seeding sample (scan_plan), and
// the ONE layout of the workspace those launches share (ScanWorkspace): FastPlan::bytes is the end of that layout and fast_search
// takes its pointers from it, so a region is added in one place. Pure integer arithmetic over (n, dim, dtype, metric, nq, k) and
// the ten plan switches; the switches arrive as a plain struct that scan.hip fills from switches(), their defaults stay in
// switches.h. tests/native/scan_plan_main.cpp drives this file alone under AddressSanitizer / UBSan: recorded plans
// (tests/golden/scan_plans.txt) and the invariants the launches rely on.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/archi_knn.h"

namespace ak {

constexpr int BK = 64;         // k per LDS stage (128 B per row)

// per-query certificate terms: s~_units = a * s~' + b where s~' is the scan's score; eps in score units
struct QPrep { double eps, a, b; };
constexpr int TAIL_KP = 64, TAIL_MAX_DIM = 4096;      // the fused tail (exact.hip): candidates it re-ranks per query, longest row it stages

// Tile configuration: WM x WN waves, each wave (MI*32) corpus rows x (NI*32) queries; K-step 64 (128 B per LDS row,
// 8-row staging pieces, chunk ^= (row>>1)&7 spreads the 16 lanes of a ds_read_b128 group over all 16 bank quads).
// PHASED_ (the 256 x 256 tile of the MFMA-bound batches): a K-step runs as two phases of 16 MFMAs and the two waves of
// every SIMD run them one barrier apart -- see the phased K-loop in k_scan.
// MFMA_ (phased tiles only): 32 = v_mfma_f32_32x32x16, 16 = v_mfma_f32_16x16x32 on the same LDS image, phases and output tile per
// wave -- other fragment reads, other accumulator mapping, other filter groups (k_scan, "16x16x32"). Shape32: the same tile on the
// 32x32x16 shape, which the pre-seeding launch always runs (its group-maxima layout feeds k_seed_kth).
// FILT_ (16x16x32 tiles only): arrangement of the per-tile filter. 0 = site by site (every filter group computes its bound, reads its
// threshold, waits and branches into its slow path), 1 = the exact maxima of the whole tile first, branch-free, from thresholds and
// row terms read once, and one branch around the sites that hold a true hit (tile_epilogue). Both append the same keys; which one
// a tile ships on is decided like its MFMA shape (SHIP_FILT_* below). On the int8 tile arrangement 1 takes the maxima from the
// sixteen BOUNDS: the int8 shadow gives the rows of a filter class one scale (shadow8_scale.h), which makes a site's bound its
// exact maximum -- 16 conversions and fma per lane instead of 128, no row terms held, the sites some lane passed entered behind
// the one branch (docs/EXPERIMENTS.md, "class scales").
// 2 (the int8 tile only) = queued: the sixteen bounds first, branch-free; the lane-sites that pass are gathered, site by site behind a
// ballot, into the wave's own LDS queue and scored once per tile, one lane per entry (tile_epilogue, "queued"). Same keys again.
template <int WM_, int WN_, int MI_, int NI_, int NSTAGE_, int MINW_, bool PHASED_ = false, int FILT_ = 0, int MFMA_ = 32>
struct ScanCfg {
    static constexpr int WM = WM_, WN = WN_, MI = MI_, NI = NI_, NSTAGE = NSTAGE_, MINW = MINW_;
    static constexpr bool PHASED = PHASED_;
    static constexpr int MFMA = MFMA_;
    static constexpr int FILT = FILT_;
    static constexpr int FILT_SEED = FILT_;       // the seeding pass's arrangement: the tile's, unless a tile type says otherwise (CfgP8 below)
    static constexpr bool I8 = false;             // int8 operands (one byte per element, K-step 128): CfgP8 below
    using Shape32 = ScanCfg<WM_, WN_, MI_, NI_, NSTAGE_, MINW_, PHASED_, 0, 32>;
    static_assert(MFMA_ == 32 || (MFMA_ == 16 && PHASED_), "the 16x16x32 shape exists for the phased tiles");
    static_assert(FILT_ == 0 || ((FILT_ == 1 || FILT_ == 2) && MFMA_ == 16), "the whole-tile and queued filters exist for the 16x16x32 tiles");
    static constexpr int AHEAD = NSTAGE_ - 1;     // ring stages issued ahead of the compute cursor
    static constexpr int BKB = 128;               // bytes per LDS row per K-step
    static constexpr int RPP = 1024 / BKB;        // rows per 1 KiB staging piece
    static constexpr int CPR = BKB / 16;          // 16-byte chunks per LDS row
    static constexpr int NSUB = BKB / 32;         // k16 MFMA sub-steps per K-step
    static constexpr int NW = WM * WN;
    static constexpr int THREADS = NW * 64;
    static constexpr int BM = WM * MI * 32;       // corpus rows per tile
    static constexpr int BN = WN * NI * 32;       // queries per block
    static constexpr int A_BYTES = BM * BKB, B_BYTES = BN * BKB;
    static constexpr int A_PW = BM / RPP / NW;    // 1 KiB pieces per wave per stage
    static constexpr int B_PW = BN / RPP / NW;
    static constexpr int LOADS = A_PW + B_PW;     // glds per wave per stage
    static constexpr int CAP = BM >= 256 ? 1024 : 512;   // append-buffer entries per (block, query)
    // the queued filter's per-wave queues, behind the common layout: [wave][9 words][64 slots] -- eight raw dot products and the
    // entry's (site, lane); slot-minor, so the pushes of a site's passing lanes (consecutive slots) and the drain (lane i reads slot
    // i) touch 64 distinct banks per word
    static constexpr int HQ_WORDS = 9, HQ_SLOTS = 64;
    static constexpr int HQ_BYTES = FILT_ == 2 ? WM_ * WN_ * HQ_WORDS * HQ_SLOTS * 4 : 0;
    static constexpr int LDS_BYTES = NSTAGE * (A_BYTES + B_BYTES) + (4 * BM + 4 * BN + 4 + 128) * 4 + HQ_BYTES;
    // the pre-seeding (SEED) instantiation of the 128-accumulator phased tile keeps its running group maxima -- MI * NI floats per
    // lane, live across every tile -- in LDS behind the common layout instead of in registers: those eight registers on top of a
    // full 256 made hipcc spill 62 (round-5 review); one read-modify-write per (tile, group) of a launch that runs ~50 us
    static constexpr bool SEED_GM_LDS = PHASED_ && MI_ * NI_ >= 8;
    static constexpr int SEED_LDS_BYTES = LDS_BYTES - HQ_BYTES + (SEED_GM_LDS ? NW * MI_ * NI_ * 64 * 4 : 0);    // (no queue in that launch)
    static_assert(SEED_LDS_BYTES <= 160 * 1024 && LDS_BYTES <= 160 * 1024, "LDS budget");
    static_assert((BM / RPP) % NW == 0 && (BN / RPP) % NW == 0, "pieces must divide over the waves");
    static_assert(NSTAGE >= 2 && NSTAGE <= 4, "ring depth");
    static_assert(BM / 64 <= NW, "ea/eb staging uses one wave per 64 rows");
    static_assert(!PHASED_ || (NSTAGE_ == 2 && ((WM_ == 2 && WN_ == 4 && MI_ == 4 && (NI_ == 2 || NI_ == 1)) ||
                                                 (WM_ == 4 && WN_ == 2 && MI_ == 2 && NI_ == 3))),
                  "phased K-loop: 256 x 256 / 256 x 128 tile (8 waves of 128 x 64 / 128 x 32) or 256 x 192 (8 waves of 64 x 96), two K-tile buffers");
};

//                      WM WN MI NI ring minw
// MFMA shape of the phased tiles in the product library: the winner by wall time on the benchmark's own workload, parent and variant
// alternating in one job, every run of the winner above every run of the other (docs/EXPERIMENTS.md "16x16x32": P +6.0 % at Q = 1024,
// R +5.7 % at 384, Q +3.0 % at 256 queries/s). libarchi_hip_dbg.so instantiates both shapes of each and AK_SCAN_MFMA = 16 / 32
// picks one there.
constexpr int SHIP_P = 16, SHIP_Q = 16, SHIP_R = 16;
// Filter arrangement of the 16x16x32 tiles in the product library (ScanCfg::FILT), by the same rule (docs/EXPERIMENTS.md, "whole-tile
// filter": the int8 tile -2.7 % of the step at Q = 1024, every run ahead; the 16-bit P and Q slightly slower, R ahead by no more
// than the spread: they keep the site-by-site filter; "hit queue": the int8 tile's main pass on the queue: ahead by less than the
// spread, stays on the whole tile). libarchi_hip_dbg.so instantiates both arrangements of P, P8, Q and R and
// AK_SCAN_FILTER = 1 (site by site) / 2 (whole tile) picks one there; the 32x32x16 shape has one filter.
constexpr int SHIP_FILT_P = 0, SHIP_FILT_P8 = 1, SHIP_FILT_Q = 0, SHIP_FILT_R = 0;
template <int S, int F = 0> using CfgPs = ScanCfg<2, 4, 4, 2, 2, 2, true, S == 16 ? F : 0, S>;
template <int S, int F = 0> using CfgQs = ScanCfg<2, 4, 4, 1, 2, 2, true, S == 16 ? F : 0, S>;
template <int S, int F = 0> using CfgRs = ScanCfg<4, 2, 2, 3, 2, 2, true, S == 16 ? F : 0, S>;
using CfgP = CfgPs<SHIP_P, SHIP_FILT_P>;                     // 256 x 256, 8 waves (128x64 each), phased K-loop, SIMD partners one barrier apart : MFMA-bound batches
using CfgQ = CfgQs<SHIP_Q, SHIP_FILT_Q>;                     // 256 x 128, 8 waves (128x32 each), phased K-loop (three half-tiles per K-step) : 128-query groups of MFMA-bound batches
// Measured and not kept (round 1-2; docs/EXPERIMENTS.md has the numbers): an L2 prefetch of the corpus lines three K-steps
// ahead of the staging cursor (the prefetch instruction costs half of what a wave's staging instructions issue per K-step:
// 15.9 vs 14.7 ms); the same 256 x 256 tile on FOUR waves of 128 x 128 (one wave per SIMD: nothing runs under the staging
// issue, the vmcnt wait, the barrier or the first fragment reads of a K-step: 27.3 vs 14.4 ms); K-step 32 with a 4-slot ring
// (twice the barriers: +4 %), and that ring with the SIMD partners one barrier apart (+2 % over itself in step, still behind
// the K-step-64 loop) -- the forerunner of CfgP, which keeps K-step 64 and staggers at quadrant granularity instead.
using CfgL = ScanCfg<4, 2, 2, 2, 3, 2>;   // 256 x 128, 8 waves (64x64 each), 3-slot ring
using CfgM = ScanCfg<4, 1, 2, 2, 3, 1>;   // 256 x 64 , 4 waves, 3-slot ring : HBM-bound, Q <= 64
using CfgS = ScanCfg<4, 1, 2, 1, 3, 1>;   // 256 x 32 , 4 waves, 3-slot ring : HBM-bound, Q <= 32
// the 256 x 256 phased tile on int8 operands (v_mfma_i32_16x16x64_i8): a type of its own, so the names of the 16-bit kernels stand
// The int8 tile has a third arrangement, the queued one (ScanCfg::FILT = 2), and its two passes choose on their own (FILT the main
// pass, FILT_SEED the seeding pass: k_scan takes the one its SEEDPASS tag names). CfgP8 is what ships: the main pass on the whole tile,
// the seeding pass on the queue (docs/EXPERIMENTS.md, "hit queue": the seeding pass -14.5 % per launch and -0.157 ms of the step at
// Q = 1024 on the queue, every run ahead of every parent run; the main pass ahead by less than the spread). CfgP8f and CfgP8g hold the
// other arrangements of either pass, in the dbg library -- AK_SCAN_FILTER as above, AK_SCAN_HITQ = 1 (seeding pass) / 2 (main pass) /
// 3 (both) / 4 (neither) puts a pass on the queue or takes it off. A type with a queued pass carries the queues' LDS.
constexpr int SHIP_FILT_P8_SEED = 2;
template <int FM, int FS> struct CfgP8T : CfgPs<16, FM> {
    using Base = CfgPs<16, FM>;
    static constexpr bool I8 = true;
    static constexpr int FILT_SEED = FS;
    static constexpr int HQ_BYTES = (FM == 2 || FS == 2) ? Base::NW * Base::HQ_WORDS * Base::HQ_SLOTS * 4 : 0;
    static constexpr int LDS_BYTES = Base::LDS_BYTES - Base::HQ_BYTES + HQ_BYTES;
    static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};
struct CfgP8 : CfgP8T<SHIP_FILT_P8, SHIP_FILT_P8_SEED> {};
struct CfgP8f : CfgP8T<0, 0> {};      // site by site, both passes
struct CfgP8g : CfgP8T<2, 1> {};      // main pass queued, seeding pass whole tile
static_assert(SHIP_FILT_P8 == 1 && SHIP_FILT_P8_SEED == 2, "CfgP8f / CfgP8g hold the arrangements CfgP8 does not");
// the type that runs arrangement F in the seeding (SEEDP) or the main pass
template <bool SEEDP, int F> using CfgP8of =
    std::conditional_t<(SEEDP ? CfgP8::FILT_SEED : CfgP8::FILT) == F, CfgP8, std::conditional_t<(SEEDP ? CfgP8f::FILT_SEED : CfgP8f::FILT) == F, CfgP8f, CfgP8g>>;
using CfgR = CfgRs<SHIP_R, SHIP_FILT_R>;                     // 256 x 192, 8 waves of 64 x 96, phased: batches between the regimes (Q mod 256 in (128, 192], ...)

// The tile numbers are what ak_index_scan_plan reports (archi_amd/index.py names them by position). 3 and 4 were the A/B reference
// tiles O (the first 128 x 128 version) and X (the 256 x 256 tile with the in-step K-loop of rounds 1-2): retired, the numbers
// stay reserved and no plan yields them.
struct CfgInfo { int bm, bn, cap, threads, lds, blocks_per_cu; };
template <class C> constexpr CfgInfo info_of(int bpc) { return CfgInfo{C::BM, C::BN, C::CAP, C::THREADS, C::LDS_BYTES, bpc}; }
constexpr CfgInfo g_cfgs[8] = {info_of<CfgL>(1), info_of<CfgM>(1), info_of<CfgS>(1), CfgInfo{}, CfgInfo{}, info_of<CfgP>(1), info_of<CfgQ>(1),
                               info_of<CfgR>(1)};
enum { CFG_L = 0, CFG_M = 1, CFG_S = 2, CFG_P = 5, CFG_Q = 6, CFG_R = 7 };

// what the plan reads of an index, and of the switches (switches.h holds their meanings and defaults; scan.hip fills this)
struct ScanShape { int64_t n; int dim, dtype, metric; };
struct PlanSwitches { int scan_cfg, scan_i8, scan_blocks, scan_r192_pm, scan_no192, seed_ratio, seed_div, pre_div, scan_noseed, scan_nopre; };

// Tile choice by (Q, N, D), from sweeps on the MI355X (scripts/gpu_ridge_sweep.sh, scripts/gpu_probe3.py; search time in ms,
// 10M x 768 bf16, round 3 -- P = 256-query groups on the phased 256 x 256 tile, Q = 128-query groups on the phased 256 x 128
// tile, L = 128-query groups on the in-step 256 x 128 tile of rounds 1-2):
//   queries   128    256    384    512    640   1024
//   P          -    3.93   6.43   6.82   9.74  12.75
//   Q        3.10   4.46   6.34   7.78   9.97  14.62
//   L        3.15   4.75   6.95    -      -      -
// and R = 192-query groups on the phased 256 x 192 tile (8 waves of 64 x 96: 24 MFMAs per K-tile and wave where P has 32),
// on another box, R / P / Q:  Q = 192: 3.72 / 3.84 / 4.59   320: 5.51 / 6.32 / -   384: 5.70 / 6.55 / 6.45   576: 8.32 / 9.70 / -
//   768: 10.44 / 10.22 / -   1024: 15.29 / 13.02 / -   -- a 192-query pass costs 0.77 (four groups) to 0.87 (two) of a 256-query one.
// A query group is a full pass over the slice's tiles whatever it holds, so what counts is the PADDED batch: a 128-query
// group costs ~0.62 of a 256-query group. Between the regimes -- Q in (256, 384], (768, 896] ... -- the narrower tile
// wastes less. Small shards (1M x 384 f32, Q = 256: L 0.455, Q 0.455, P 0.509 ms; 1.25M x 768 bf16: L 0.864, Q 0.872,
// P 0.759; Q = 1024: Q 2.15, P 1.91): the wide tile needs long rows and enough tiles per workgroup to pay.
// long rows and many tiles: where the wide tiles pay and the scan is bound by the matrix pipe (pick_cfg, the int8 plan's eligibility)
inline bool big_shard(const ScanShape &ix) { return ix.dim >= 768 && (ix.n + 255) / 256 >= 4096; }

inline int pick_cfg(int nq, const ScanShape &ix, const PlanSwitches &sw) {
    if (const int forced = sw.scan_cfg) {
        switch (forced) { case 'L': return CFG_L; case 'M': return CFG_M; case 'S': return CFG_S;
                        case 'P': return ix.dim < 128 ? CFG_L : CFG_P; case 'Q': return ix.dim < 128 ? CFG_L : CFG_Q;
                        case 'R': return ix.dim < 128 ? CFG_L : CFG_R; }
    }
    if (nq <= 32) return CFG_S;
    if (nq <= 64) return CFG_M;
    if (nq <= 128) return CFG_L;          // HBM-bound: the in-step loop with its three-slot ring
    if (ix.dim < 128) return CFG_L;       // one K-step per tile: the phased loop wants two (its compaction-request sampling)
    const int g128 = (nq + 127) / 128, g192 = (nq + 191) / 192, g256 = (nq + 255) / 256;
    const bool big = big_shard(ix);
    // A query group is a full pass over the slice's tiles whatever it holds; relative cost of a pass: 256-query group 1,
    // 192-query group 0.85, 128-query group 0.62. Long rows and many tiles: the cheapest padded batch. Small or short-row shards:
    // the wide tile pays later (two 128-groups at Q <= 256, the measured 1.62 rule above), the 192 tile when it beats that choice
    // (1M x 384 f32 Q = 384: R 0.551 / Q 0.569 / P 0.607 ms; 12.5M x 384 f16 Q = 384: 3.89 / 4.45 / 4.53; 1.25M x 768 Q = 576:
    // R 1.229 / P 1.426)
    const double r192 = sw.scan_r192_pm * 1e-3;
    const bool no192 = sw.scan_no192 != 0;
    const double cp = g256, cr = no192 ? 1e9 : g192 * r192, cq = g128 * 0.62;
    if (big) {
        if (cr < cp && cr < cq) return CFG_R;
        return cp <= cq ? CFG_P : CFG_Q;
    }
    const int base = nq <= 256 ? CFG_Q : (g256 * 1.62 < g128 ? CFG_P : CFG_Q);
    return cr < (base == CFG_P ? cp : cq) ? CFG_R : base;
}

constexpr int I8_KP = 512;      // candidates the int8 plan re-ranks per query (k_finalize<8>; the append buffers' limit)

inline bool fast_supported(const ScanShape &ix, int nq, int k) {
    if (ix.dim % BK != 0) return false;
    if (ix.n < 4096) return false;                          // tiny index: exact path is cheaper
    if (k > 128) return false;
    return nq > 0;
}

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

struct FastPlan {
    int cfg;        // tile configuration (g_cfgs)
    int kprime;     // candidates kept per (slice, query) and re-ranked per query
    int qtile;      // queries per block
    int nslices;    // corpus slices (blocks along the corpus) of the main pass
    int ns_seed;    // slices of the seeding pass (0 = single pass)
    int64_t seed_rows;  // rows [0, seed_rows) are scanned first to seed the thresholds
    int64_t pre_tiles;  // pre-seeding sample: pre_tiles tiles, every pre_stride-th tile of the corpus (0 = none)
    int pre_slices;     // workgroups along the sample
    int pre_stride;
    int nqg;        // query groups
    int i8;         // 1 = the main and seeding pass scan the int8 shadow (tile P on v_mfma_i32_16x16x64_i8, k' = 512 dense tail)
    size_t bytes;   // workspace bytes: where the plan's ScanWorkspace ends
};

// the plan but for `bytes` (0 here): that is scan_workspace's, which wants the selection scratch size of this plan's lists first
inline FastPlan scan_plan(const ScanShape &ix, const PlanSwitches &sw, int nq, int k, bool widest, bool allow_i8) {
    FastPlan p;
    p.cfg = pick_cfg(nq, ix, sw);
    const CfgInfo &c = g_cfgs[p.cfg];
    p.kprime = k <= 16 ? 64 : (k <= 48 ? 128 : 256);
    // the int8 plan: tile P, cosine / inner product (no additive row term), a 16-bit corpus, rows of >= two 128-element K-steps,
    // the common k' (k <= 16); by its own choice (AK_SCAN_I8 = 1) only where the scan is bound by the matrix pipe -- a big shard
    // and at least two 256-query groups. AK_SCAN_I8 = 2 takes every shape the kernel allows (tests, A/B runs).
    p.i8 = 0;
    if (const int i8m = sw.scan_i8) {
        const bool shape_ok = allow_i8 && !widest && p.cfg == CFG_P && ix.metric != AK_METRIC_L2 && ix.dtype != AK_DTYPE_F32 && ix.dim % 128 == 0 &&
                              ix.dim >= 256 && ix.dim <= TAIL_MAX_DIM && k <= 16;
        const bool big = big_shard(ix);
        if (shape_ok && (i8m >= 2 || (big && nq > 256))) p.i8 = 1;
    }
    if (p.i8) p.kprime = I8_KP;
    // second-chance plan (AUTO mode, queries the first pass could not certify): the widest candidate lists the
    // append buffers and k_finalize<8> allow, so a pile-up of up to 512 equal scores still certifies
    if (widest) p.kprime = 512;
    if (p.kprime > c.cap - c.bm) p.kprime = (c.cap - c.bm) / 64 * 64;
    p.qtile = c.bn;
    p.nqg = (nq + c.bn - 1) / c.bn;
    int64_t ntiles = (ix.n + c.bm - 1) / c.bm;
    int target = 256 * c.blocks_per_cu;                    // resident workgroups on 256 CUs
    if (const int forced = sw.scan_blocks) target = forced;
    int ns = target / p.nqg;
    if (ns < 8) ns = 8;
    ns = (ns / 8) * 8;
    while (ns > 8 && ntiles / ns < 2) ns -= 8;             // keep >= 2 tiles per slice
    if (ns > ntiles) ns = (int)ntiles;
    p.nslices = ns < 1 ? 1 : ns;
    // seeding pass: 3-12% of the rows first (seed_div below), so the main pass starts with thresholds close to the
    // final k-th best instead of discovering them slice by slice
    p.ns_seed = 0; p.seed_rows = 0; p.pre_tiles = 0; p.pre_slices = 0; p.pre_stride = 1;
    const int64_t seed_ratio = sw.seed_ratio;   // tiles per slice below which the seeding pass does not pay
    const bool noseed = sw.scan_noseed != 0;
    if (!noseed && ntiles >= seed_ratio * (int64_t)p.nslices && ntiles >= 256) {
        // share of the tiles the seeding pass scans: 1/32 on large shards, 1/8 below ~5M rows (round-3 sweep with the phased
        // tiles, search ms at Q = 1024 for 1/32, 1/16, 1/8: 10M x 768 12.97 / 12.94 / 12.97 and 12.5M x 384 f16 9.18 / 9.09 /
        // 9.13 -- flat; 1.25M x 768 1.96 / 1.91 / 1.88; 1M x 384 f32 1.19 / 1.10 / 1.04 -- on a small shard tighter thresholds
        // spare the main pass's filter more than the extra seed rows cost)
        int seed_div = sw.seed_div;
        // (round 5, after the filter got cheaper: 10M x 768 Q = 1024 search ms for 1/64 .. 1/8: 13.05 / 12.98 (1/48) / 12.87 (1/32) / 12.79
        // (1/24) / 12.77 (1/16) / 12.73 (1/12) / 12.74 -- and from 1/96 on queries lose their certificate: 1/12 up to 100k tiles)
        if (seed_div <= 0) seed_div = ntiles >= 100000 ? 32 : (ntiles >= 20000 ? 12 : 8);
        int64_t seed_tiles = ntiles / seed_div;
        int nss = p.nslices;
        while (nss > 8 && seed_tiles / nss < 2) nss -= 8;
        if (seed_tiles >= nss && nss >= 1) {
            p.ns_seed = nss;
            p.seed_rows = seed_tiles * c.bm;
        }
    }
    // pre-seeding (group maxima over a strided sample): spares the seeding pass -- or, on shards too small to
    // have one, the main pass -- its all-pass start. 16 groups per workgroup; want >= 4k
    // groups so the k-th largest is not starved. With a seeding pass behind it 0.2% of the rows is enough; on its
    // own it is the only source of the starting thresholds, so it samples 3% like the seeding pass would.
    if (!noseed && !sw.scan_nopre && ntiles >= 64) {
        int pre_div = sw.pre_div;
        if (pre_div <= 0) pre_div = p.ns_seed > 0 ? 512 : 32;
        int64_t pt = ntiles / pre_div;
        int64_t need_tiles = ((int64_t)4 * k + c.bm / 16 - 1) / (c.bm / 16);
        if (pt < 16) pt = 16;
        if (pt < need_tiles) pt = need_tiles;
        if (pt > ntiles) pt = ntiles;
        int ps = 1024 / (c.bm / 16);                   // k_seed_kth holds <= 1024 maxima per query
        if (ps > pt) ps = (int)pt;
        p.pre_tiles = pt;
        p.pre_slices = ps;
        p.pre_stride = (int)(ntiles / pt);
    }
    p.bytes = 0;
    return p;
}

// One region of the workspace: where it starts and what the plan needs of it (0: a region this plan does not have)
template <class T> struct WsRegion {
    size_t off = 0, bytes = 0;
    T *at(void *ws) const { return (T *)((char *)ws + off); }
};

// The workspace of one fast_search call. each() is the order of the regions, scan_workspace() their sizes; every region starts
// 256-aligned at the end of the one before it.
struct ScanWorkspace {
    WsRegion<uint16_t> qs;                   // [nq_pad][dim] queries rounded to the scan dtype
    WsRegion<QPrep> prep;
    WsRegion<float> thr0, mar;               // starting thresholds, margins
    WsRegion<int> d_cnt;                     // dense-list counters
    WsRegion<unsigned int> d_thr;            // max-reduced thresholds
    WsRegion<float> thr_slots;               // final thresholds per slot
    WsRegion<float> gmax;                    // pre-seeding group maxima
    WsRegion<uint64_t> cand, out_c;
    WsRegion<uint64_t> top_k; WsRegion<int64_t> top_i;      // top k' keys + ids
    WsRegion<uint64_t> rr_k; WsRegion<int64_t> rr_i;        // re-ranked keys + ids
    WsRegion<int64_t> fin_i; WsRegion<double> fin_d;        // final ids + distances (the int8 plan parks its seed re-rank here)
    // the int8 plan only: int8 queries, their prep and margins, the final cut, the seed re-rank's counts + flags
    WsRegion<int8_t> qs8; WsRegion<QPrep> prep8; WsRegion<float> mar8, thr_fin; WsRegion<int> sd_cnt, sd_cert;
    WsRegion<char> scratch;                  // selection scratch (exact.hip, select.hip)
    size_t bytes = 0;                        // end of the last region + slack

    template <class W, class F> static void each(W &w, F &&f) {
        f(w.qs); f(w.prep); f(w.thr0); f(w.mar); f(w.d_cnt); f(w.d_thr); f(w.thr_slots); f(w.gmax); f(w.cand); f(w.out_c); f(w.top_k); f(w.top_i);
        f(w.rr_k); f(w.rr_i); f(w.fin_i); f(w.fin_d); f(w.qs8); f(w.prep8); f(w.mar8); f(w.thr_fin); f(w.sd_cnt); f(w.sd_cert); f(w.scratch);
    }
};

// select_bytes: select_scratch_bytes + select_keys_scratch_bytes over the plan's candidate lists (their owners' figure)
inline ScanWorkspace scan_workspace(const FastPlan &p, const ScanShape &ix, int nq, int k, size_t select_bytes) {
    const CfgInfo &c = g_cfgs[p.cfg];
    const size_t nq_pad = (size_t)p.nqg * c.bn, ns_tot = (size_t)p.nslices + p.ns_seed, q = (size_t)nq;
    ScanWorkspace w;
    w.qs.bytes = nq_pad * ix.dim * 2;
    w.prep.bytes = q * sizeof(QPrep);
    w.thr0.bytes = w.mar.bytes = w.d_cnt.bytes = w.d_thr.bytes = q * 4;
    w.thr_slots.bytes = q * ns_tot * 4;
    w.gmax.bytes = q * 1024 * 4;
    w.cand.bytes = (size_t)p.nslices * nq_pad * c.cap * 8;
    w.out_c.bytes = q * ns_tot * p.kprime * 8;
    w.top_k.bytes = w.top_i.bytes = w.rr_k.bytes = w.rr_i.bytes = q * p.kprime * 8;
    w.fin_i.bytes = w.fin_d.bytes = q * k * 8;
    if (p.i8) {
        w.qs8.bytes = nq_pad * ix.dim;
        w.prep8.bytes = q * sizeof(QPrep);
        w.mar8.bytes = w.thr_fin.bytes = w.sd_cnt.bytes = w.sd_cert.bytes = q * 4;
    }
    w.scratch.bytes = select_bytes;
    size_t end = 0;
    ScanWorkspace::each(w, [&](auto &r) { r.off = end; end += al(r.bytes); });
    w.bytes = end + 4096;
    return w;
}

}  // namespace ak
