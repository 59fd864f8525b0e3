// CPU sanitizer harness for the kNN scan's plan and workspace layout (archi_amd/csrc/scan_plan.h; TEST INFRASTRUCTURE).
// Built by archi_amd/csrc/Makefile as `make asan-plan` (-fsanitize=address,undefined) and run by tests/test_abi_cpu.py.
//   golden check: tests/golden/scan_plans.txt (argv[1]) holds one case per line, integers only --
//       n dim dtype metric nq k widest allow_i8, the ten plan switches in PlanSwitches' order, the selection scratch bytes,
//       then every FastPlan field in its order, `bytes` last --
//     recorded from pick_cfg / fast_plan as they stood BEFORE the plan moved into scan_plan.h (with the selection sizes of exact.hip
//     and select.hip of that commit). The header has to reproduce every field exactly. Behind each int8 plan the file holds the
//     allow_i8 = 0 plan of the same arguments: the plan fast_search falls back to when the int8 shadow cannot be allocated.
//   invariants: what the launches rely on, for every golden case whose geometry switches are unforced (AK_SCAN_CFG, AK_SCAN_BLOCKS,
//     AK_SEED_DIV, AK_PRE_DIV at 0) and for a seeded random sweep of the same ranges under the first case's switches.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../archi_amd/csrc/scan_plan.h"
#include "../../include/archi_knn.h"

using namespace ak;

namespace {
#define CHECK(c)                                                                                                        \
    do {                                                                                                                \
        if (!(c)) {                                                                                                     \
            fprintf(stderr, "scan_plan: CHECK failed at line %d: %s\n  case: %s\n", __LINE__, #c, g_case);            \
            exit(1);                                                                                                    \
        }                                                                                                               \
    } while (0)
char g_case[512] = "";

struct Case {
    ScanShape sh; int nq, k, widest, allow_i8; PlanSwitches sw; size_t sel;
    FastPlan want;
};

void name_case(const Case &c) {
    snprintf(g_case, sizeof g_case, "n %" PRId64 " dim %d dtype %d metric %d nq %d k %d widest %d allow_i8 %d | cfg %d i8 %d blocks %d r192 %d no192 %d ratio %d sdiv %d pdiv %d noseed %d nopre %d",
             c.sh.n, c.sh.dim, c.sh.dtype, c.sh.metric, c.nq, c.k, c.widest, c.allow_i8, c.sw.scan_cfg, c.sw.scan_i8, c.sw.scan_blocks, c.sw.scan_r192_pm,
             c.sw.scan_no192, c.sw.seed_ratio, c.sw.seed_div, c.sw.pre_div, c.sw.scan_noseed, c.sw.scan_nopre);
}

std::vector<Case> read_golden(const char *path) {
    FILE *f = fopen(path, "r");
    if (!f) { fprintf(stderr, "scan_plan: cannot open %s\n", path); exit(1); }
    std::vector<Case> out;
    for (;;) {
        Case c{};
        long long n, seed_rows, pre_tiles;
        unsigned long long sel, bytes;
        PlanSwitches &s = c.sw;
        FastPlan &w = c.want;
        const int got = fscanf(f, "%lld %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %llu %d %d %d %d %d %lld %lld %d %d %d %d %llu", &n, &c.sh.dim, &c.sh.dtype,
                               &c.sh.metric, &c.nq, &c.k, &c.widest, &c.allow_i8, &s.scan_cfg, &s.scan_i8, &s.scan_blocks, &s.scan_r192_pm, &s.scan_no192,
                               &s.seed_ratio, &s.seed_div, &s.pre_div, &s.scan_noseed, &s.scan_nopre, &sel, &w.cfg, &w.kprime, &w.qtile, &w.nslices, &w.ns_seed,
                               &seed_rows, &pre_tiles, &w.pre_slices, &w.pre_stride, &w.nqg, &w.i8, &bytes);
        if (got == EOF) break;
        if (got != 31) { fprintf(stderr, "scan_plan: %s: malformed case %zu\n", path, out.size() + 1); exit(1); }
        c.sh.n = n; c.sel = (size_t)sel; w.seed_rows = seed_rows; w.pre_tiles = pre_tiles; w.bytes = (size_t)bytes;
        out.push_back(c);
    }
    fclose(f);
    return out;
}

// the regions other than the selection scratch, in order
struct Span { size_t off, bytes; };
std::vector<Span> spans_of(const ScanWorkspace &w) {
    std::vector<Span> v;
    ScanWorkspace::each(w, [&](const auto &r) { v.push_back(Span{r.off, r.bytes}); });
    return v;
}

void check_invariants(const Case &c, const FastPlan &p, const ScanWorkspace &w) {
    const CfgInfo &t = g_cfgs[p.cfg];
    CHECK(t.bm > 0);                                              // a tile this library has (3 and 4 are reserved)
    // the workspace: 256-aligned regions, ascending, disjoint, inside `bytes`
    size_t end = 0;
    for (const Span &r : spans_of(w)) {
        CHECK(r.off % 256 == 0);
        CHECK(r.off >= end);
        end = r.off + r.bytes;
    }
    CHECK(end <= w.bytes);
    CHECK(p.kprime <= t.cap - t.bm);                              // a full tile of appends behind k' kept entries
    CHECK(p.nslices >= 1);
    CHECK(p.seed_rows % t.bm == 0 && p.seed_rows < c.sh.n);
    CHECK(p.pre_slices * (t.bm / 16) <= 1024);                    // k_seed_kth holds at most 1024 maxima per query
    CHECK((p.pre_tiles > 0) == (p.pre_slices > 0) && p.pre_stride >= 1);
    if (p.i8) {
        CHECK(p.cfg == CFG_P && p.kprime == I8_KP);
        // the NOMEM fallback: the 16-bit plan of the same arguments, region by region no larger (the scratch is its owners' figure:
        // the golden pairs hold the two plans' whole sizes against each other)
        const FastPlan alt = scan_plan(c.sh, c.sw, c.nq, c.k, c.widest != 0, false);
        CHECK(!alt.i8 && alt.cfg == p.cfg && alt.nslices == p.nslices);
        const std::vector<Span> a = spans_of(scan_workspace(alt, c.sh, c.nq, c.k, 0)), b = spans_of(w);
        for (size_t i = 0; i + 1 < a.size(); i++) CHECK(a[i].bytes <= b[i].bytes);
        CHECK(a.back().off <= b.back().off);
    } else if (p.ns_seed > 0 && p.kprime == TAIL_KP && c.sh.dim <= TAIL_MAX_DIM) {
        CHECK(p.ns_seed * p.kprime <= 16384);                     // dense lists: the seeding stage's k-th best kernels take no more
    }
}

FastPlan plan_of(const Case &c, ScanWorkspace &w) {
    FastPlan p = scan_plan(c.sh, c.sw, c.nq, c.k, c.widest != 0, c.allow_i8 != 0);
    w = scan_workspace(p, c.sh, c.nq, c.k, c.sel);
    p.bytes = w.bytes;
    return p;
}
}  // namespace

int main(int argc, char **argv) {
    const std::vector<Case> golden = read_golden(argc > 1 ? argv[1] : "tests/golden/scan_plans.txt");
    if (golden.size() < 1000) { fprintf(stderr, "scan_plan: only %zu golden cases\n", golden.size()); return 1; }
    size_t n_inv = 0, n_i8 = 0, n_pairs = 0;
    for (size_t i = 0; i < golden.size(); i++) {
        const Case &c = golden[i];
        name_case(c);
        CHECK(fast_supported(c.sh, c.nq, c.k));
        ScanWorkspace w;
        const FastPlan p = plan_of(c, w), &e = c.want;
        CHECK(p.cfg == e.cfg && p.kprime == e.kprime && p.qtile == e.qtile && p.nslices == e.nslices && p.ns_seed == e.ns_seed);
        CHECK(p.seed_rows == e.seed_rows && p.pre_tiles == e.pre_tiles && p.pre_slices == e.pre_slices && p.pre_stride == e.pre_stride);
        CHECK(p.nqg == e.nqg && p.i8 == e.i8);
        CHECK(p.bytes == e.bytes);
        n_i8 += p.i8;
        if (p.i8) {      // the fallback pair: the next line is the same case with allow_i8 = 0, and its workspace fits this one
            CHECK(i + 1 < golden.size());
            const Case &f = golden[i + 1];
            CHECK(f.allow_i8 == 0 && f.sh.n == c.sh.n && f.sh.dim == c.sh.dim && f.nq == c.nq && f.k == c.k && f.want.i8 == 0);
            CHECK(f.want.bytes <= p.bytes);
            n_pairs++;
        }
        const PlanSwitches &s = c.sw;
        if (s.scan_cfg == 0 && s.scan_blocks == 0 && s.seed_div == 0 && s.pre_div == 0) { check_invariants(c, p, w); n_inv++; }
    }
    // the sweep: the first case's switches (the library's own, as recorded), AK_SCAN_I8 and the three on / off switches varied
    std::mt19937_64 rng(20241);
    auto pick = [&](int lo, int hi) { return (int)(lo + rng() % (uint64_t)(hi - lo + 1)); };
    const int dims[] = {64, 128, 192, 256, 384, 768, 1024, 4096}, edges[] = {32, 64, 128, 192, 256, 384, 1024};
    size_t n_sweep = 0;
    for (int it = 0; it < 40000; it++) {
        Case c{};
        c.sw = golden[0].sw;
        c.sw.scan_i8 = pick(0, 2); c.sw.scan_no192 = pick(0, 3) == 0; c.sw.scan_noseed = pick(0, 7) == 0; c.sw.scan_nopre = pick(0, 7) == 0;
        const int tiles_log = pick(4, 16);                        // 4 096 rows .. 32 M: across the 4 096-, 20 000- and 100 000-tile thresholds
        c.sh.n = ((int64_t)256 << tiles_log) * pick(16, 31) / 16 + pick(-300, 300);
        if (it % 16 == 0) c.sh.n = (int64_t)256 * (pick(0, 2) == 0 ? 4096 : (pick(0, 1) ? 20000 : 100000)) + pick(-257, 257);
        c.sh.dim = dims[pick(0, 7)]; c.sh.dtype = pick(0, 2); c.sh.metric = pick(0, 2);
        c.nq = pick(0, 1) ? edges[pick(0, 6)] + pick(-1, 1) : pick(1, 1100);
        c.k = pick(0, 1) ? pick(1, 128) : (pick(0, 1) ? 16 : 48) + pick(-1, 1);
        c.widest = pick(0, 9) == 0; c.allow_i8 = pick(0, 9) != 0;
        c.sel = (size_t)pick(0, 1 << 20) * 16;
        if (!fast_supported(c.sh, c.nq, c.k)) continue;
        name_case(c);
        ScanWorkspace w;
        const FastPlan p = plan_of(c, w);
        check_invariants(c, p, w);
        n_i8 += p.i8;
        n_sweep++;
    }
    printf("golden cases %zu (invariants on %zu, fallback pairs %zu), sweep cases %zu, int8 plans %zu\n", golden.size(), n_inv, n_pairs, n_sweep, n_i8);
    printf("scan_plan: ok\n");
    return 0;
}
