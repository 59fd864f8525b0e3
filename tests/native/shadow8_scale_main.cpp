// CPU harness for the scale rule of the int8 shadow (archi_amd/csrc/shadow8_scale.h; TEST INFRASTRUCTURE).
// Built by archi_amd/csrc/Makefile as `make asan-shadow8` (-fsanitize=address,undefined) and run by tests/test_shadow8_class_cpu.py.
// It runs one 32-row block on the host as k_shadow8 runs it -- the contributions into two 32-float arrays, then for every new row
// s8_block_row_scale, the very call the kernel makes on its LDS arrays (the class's E, the adopt decision) -- and checks:
//   a class with rows of zeros (ea = 0 as cosine gives them, ea = 1 as the inner product does), a removed row (ea = 0), a row with
//     a non-finite value and a row beyond the cap: they keep their own scale and ea8 = own * ea, every other row stores the very
//     bits of E;
//   a partly published class extended by an append: the published rows' values are not written, E takes their ea8 as it stands;
//   shared scale >= own scale, on those and on a seeded random sweep; ea8 of an adopting class is one value;
//   the class sets are k_group_bounds' sets: 16 rows of the block with one value of row bit 2, both classes a partition.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../archi_amd/csrc/shadow8_scale.h"

using namespace ak;

namespace {
#define CHECK(c)                                                                              \
    do {                                                                                      \
        if (!(c)) {                                                                           \
            fprintf(stderr, "shadow8_scale: CHECK failed at line %d: %s\n", __LINE__, #c);   \
            exit(1);                                                                          \
        }                                                                                     \
    } while (0)

uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }

struct Row { float max_abs; bool non_finite; float ea; };

// one block as k_shadow8 runs it: rows [0, pub) are published (ea8 given, never written), rows [pub, n) are new
struct Block {
    std::vector<S8Scale> sc = std::vector<S8Scale>(S8_BLOCK);
    std::vector<float> ea8 = std::vector<float>(S8_BLOCK, 0.f);
    std::vector<bool> written = std::vector<bool>(S8_BLOCK, false);
};

Block run_block(const std::vector<Row> &rows, int pub, int n, const std::vector<float> &published_ea8) {
    Block b;
    float own[S8_BLOCK], p[S8_BLOCK];
    for (int i = 0; i < S8_BLOCK; i++) {
        own[i] = 0.f; p[i] = 0.f;
        if (i < pub) { b.ea8[i] = published_ea8[i]; p[i] = s8_published(published_ea8[i]); }
        else if (i < n) { own[i] = s8_own_scale(rows[i].max_abs, rows[i].non_finite); p[i] = s8_product(own[i], rows[i].ea); }
    }
    for (int i = pub; i < n; i++) {
        b.sc[i] = s8_block_row_scale(own, p, i, rows[i].ea);          // the very call k_shadow8 makes on its LDS arrays
        // ... against the class's E worked out here, member by member
        float E = 0.f;
        for (int r = 0; r < S8_BLOCK; r++)
            if (((r >> 2) & 1) == ((i >> 2) & 1) && p[r] > E) E = p[r];
        CHECK(bits(E) == bits(s8_block_class_max(p, s8_class_of(i))));
        b.ea8[i] = b.sc[i].ea8;
        b.written[i] = true;
        // never below the own scale: no value leaves [-127, 127] before the clip
        CHECK(!(b.sc[i].scale < own[i]));
        if (b.sc[i].shared) {
            CHECK(bits(b.sc[i].ea8) == bits(E));
            CHECK(E <= S8_CLASS_CAP * p[i] && p[i] > 0.f);
            if (p[i] > 1e-30f && b.sc[i].scale > 1e-30f && b.sc[i].scale < 1e30f) {      // (normal range: the quotients below are full precision)
                CHECK(rintf(rows[i].max_abs * (1.f / b.sc[i].scale)) <= 127.f);        // k_shadow8's own expression: the clip is dead code
                const double applied = s8_applied_scale(b.sc[i], rows[i].ea);
                CHECK(std::fabs(applied - (double)b.sc[i].scale) <= 2e-7 * applied);  // the quantiser's scale is the applied one to a float ulp
            }
        } else {
            CHECK(bits(b.sc[i].scale) == bits(own[i]));
            const float want = own[i] * rows[i].ea;
            CHECK(bits(b.sc[i].ea8) == bits(want) || (want != want && b.sc[i].ea8 != b.sc[i].ea8));
        }
    }
    return b;
}

void test_class_sets() {
    bool seen[S8_BLOCK] = {};
    for (int half = 0; half < 2; half++)
        for (int m = 0; m < S8_CLASS_ROWS; m++) {
            const int r = s8_class_member(half, m);
            CHECK(r >= 0 && r < S8_BLOCK && !seen[r]);
            seen[r] = true;
            CHECK(s8_class_of(r) == half && ((r >> 2) & 1) == half);
            // k_group_bounds: row = 8 q + 4 half + j
            CHECK(r == 8 * (m / 4) + 4 * half + m % 4);
        }
    for (int r = 0; r < S8_BLOCK; r++) CHECK(seen[r]);
}

void test_special_rows() {
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<Row> rows(S8_BLOCK);
    for (int i = 0; i < S8_BLOCK; i++) rows[i] = {0.10f + 0.002f * (float)i, false, 1.0f};      // own * ea within a factor 2 of each other
    const int zero = s8_class_member(0, 1), removed = s8_class_member(0, 5), nonfin = s8_class_member(0, 9), capped = s8_class_member(0, 14);
    const int zero_ip = s8_class_member(0, 2), zero_inf = s8_class_member(0, 6);
    rows[zero] = {0.f, false, 0.f};                 // a row of zeros on cosine: k_row_stats gives it ea = 0 (and eb = -inf)
    rows[zero_ip] = {0.f, false, 1.0f};             // a row of zeros on the inner product: ea = 1
    rows[zero_inf] = {0.f, false, inf};             // robustness only (no metric produces it): an infinite term beside a zero scale
    rows[removed] = {0.12f, false, 0.f};            // removed before the build: ea = 0
    rows[nonfin] = {0.12f, true, 1.0f};             // holds an infinity
    rows[capped] = {0.01f, false, 1.0f};            // E / (own * ea) > 2
    const Block b = run_block(rows, 0, S8_BLOCK, {});
    float E0 = 0.f;
    for (int m = 0; m < S8_CLASS_ROWS; m++) {
        const int r = s8_class_member(0, m);
        const bool special = r == zero || r == zero_ip || r == zero_inf || r == removed || r == nonfin || r == capped;
        CHECK(b.sc[r].shared == !special);
        if (!special) { if (E0 == 0.f) E0 = b.ea8[r]; CHECK(bits(b.ea8[r]) == bits(E0)); }
    }
    CHECK(bits(E0) == bits(s8_own_scale(rows[s8_class_member(0, 15)].max_abs, false) * 1.0f));      // the class's largest product
    CHECK(b.sc[zero].scale == 0.f && b.sc[nonfin].scale == 0.f && b.ea8[nonfin] == 0.f && b.ea8[removed] == 0.f);
    CHECK(b.sc[zero_ip].scale == 0.f && b.sc[zero_inf].scale == 0.f && b.ea8[zero] == 0.f && b.ea8[zero_ip] == 0.f);
    CHECK(b.ea8[zero_inf] != b.ea8[zero_inf]);      // 0 * inf, as the per-row rule would have stored it; the class's E is untouched by it
    CHECK(bits(b.ea8[capped]) == bits(s8_own_scale(0.01f, false) * 1.0f));
    // the other class is untouched by them: all sixteen adopt one value
    for (int m = 0; m < S8_CLASS_ROWS; m++) {
        const int r = s8_class_member(1, m);
        CHECK(b.sc[r].shared && bits(b.ea8[r]) == bits(b.ea8[s8_class_member(1, 0)]));
    }
}

void test_append_into_a_published_class() {
    std::vector<Row> rows(S8_BLOCK);
    for (int i = 0; i < S8_BLOCK; i++) rows[i] = {0.10f, false, 1.0f};
    const int pub = 13;
    const Block first = run_block(rows, 0, pub, {});
    for (int i = pub; i < S8_BLOCK; i++) CHECK(!first.written[i]);
    // the appended rows are peakier than the published ones of their class
    for (int i = pub; i < S8_BLOCK; i++) rows[i].max_abs = 0.15f;
    const Block second = run_block(rows, pub, S8_BLOCK, first.ea8);
    for (int i = 0; i < pub; i++) { CHECK(!second.written[i]); CHECK(bits(second.ea8[i]) == bits(first.ea8[i])); }
    for (int i = pub; i < S8_BLOCK; i++) {
        CHECK(second.written[i] && second.sc[i].shared);
        CHECK(bits(second.ea8[i]) == bits(s8_own_scale(0.15f, false) * 1.0f));
        CHECK(second.ea8[i] > first.ea8[0]);        // the block is mixed: gb8, the maximum, still bounds every row
    }
    // appended rows flatter than the published ones: E comes from the published rows' ea8 as it stands
    for (int i = pub; i < S8_BLOCK; i++) rows[i].max_abs = 0.07f;
    const Block third = run_block(rows, pub, S8_BLOCK, first.ea8);
    for (int i = pub; i < S8_BLOCK; i++) CHECK(third.sc[i].shared && bits(third.ea8[i]) == bits(first.ea8[0]));
    // ... unless the cap excludes them
    for (int i = pub; i < S8_BLOCK; i++) rows[i].max_abs = 0.04f;
    const Block fourth = run_block(rows, pub, S8_BLOCK, first.ea8);
    for (int i = pub; i < S8_BLOCK; i++) CHECK(!fourth.sc[i].shared);
}

void test_random_sweep() {
    std::mt19937 rng(20251);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    const float inf = std::numeric_limits<float>::infinity();
    long adopted = 0, total = 0;
    for (int it = 0; it < 20000; it++) {
        std::vector<Row> rows(S8_BLOCK);
        const float spread = it % 3 == 0 ? 8.f : 1.5f;
        for (auto &r : rows) {
            r = {std::ldexp(0.5f + u(rng), (int)(u(rng) * 40.f) - 20) * (1.f + spread * u(rng)), false, std::ldexp(0.5f + u(rng), (int)(u(rng) * 30.f) - 15)};
            const float k = u(rng);
            if (k < 0.02f) r.max_abs = 0.f;
            else if (k < 0.04f) r.ea = 0.f;
            else if (k < 0.06f) r.non_finite = true;
            else if (k < 0.07f) r.ea = inf;
            else if (k < 0.08f) r.ea = std::numeric_limits<float>::quiet_NaN();
            else if (k < 0.09f) r.max_abs = std::numeric_limits<float>::denorm_min();
            else if (k < 0.10f) r.max_abs = std::numeric_limits<float>::max();
        }
        const int n = 1 + (int)(u(rng) * 31.99f), pub = (int)(u(rng) * (float)n);
        const Block a = run_block(rows, 0, pub, {});
        const Block b = run_block(rows, pub, n, a.ea8);
        for (int i = pub; i < n; i++) { adopted += b.sc[i].shared; total++; }
    }
    printf("shadow8_scale: random sweep: %ld of %ld rows adopted\n", adopted, total);
    CHECK(adopted > 0 && adopted < total);
}
}  // namespace

int main() {
    test_class_sets();
    test_special_rows();
    test_append_into_a_published_class();
    test_random_sweep();
    printf("shadow8_scale: ok\n");
    return 0;
}
