// shadow8_scale.h -- the SCALE RULE of the int8 shadow (index.hip, k_shadow8), as plain C++ that compiles for the host and for the
// device: which rows form a filter class, the class's shared scan-side term E, the cap, and whether a row adopts the shared scale.
// No HIP in here beyond the function qualifiers; tests/native/shadow8_scale_main.cpp drives this file alone on the CPU.
//
// The scan's int8 score of a row is dot_i32 * ea8[row] with ea8 = scale * ea. A lane of the 16x16 MFMA tile holds, of one 32-row
// block and one query column, the 8 rows {16h + 4kq + j}, all with row bit 2 = kq & 1: a subset of the 16 rows
// {8q + 4 * half + j} of the block with that row bit, the class k_group_bounds maximises over (Index::gb8). The filter's bound of
// such a site is max(0, max dot) * max(ea8 of the class) + max(eb of the class). Where every row of the class carries the SAME ea8
// the first term is bit for bit the maximum of the rows' own products (multiplying by one positive constant is monotone and
// rounds identically), so the bound is the site's exact maximum and the filter needs no per-row arithmetic.
//
// Rule for one class. A row's own scale is max|a| / 127 (0 for a row of zeros or one with a non-finite value). Its product is
// p = own * ea where both are finite and positive and so is p, otherwise 0. E = max of the class's products, where a row that a
// published shadow already holds contributes its ea8 as it stands (such a row is never rewritten: a search on another stream may
// be reading it). A row with p > 0 and E <= S8_CLASS_CAP * p adopts: it stores ea8 = E, the very bits, and is quantised with
// scale max(E / ea, own) -- never below its own scale, so no value leaves [-127, 127] before the clip. Every other row keeps its
// own scale and ea8 = own * ea: rows of zeros, rows with a non-finite value, removed rows (ea = 0) and rows the cap excludes. The
// cap only matters where ea does not follow the row's norm (inner product: a short row beside long ones would lose all its
// resolution); on cosine p is the row's peak over its norm, and a ratio above 2 costs the row more than one bit.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AK_S8_HD __host__ __device__ inline
#else
#define AK_S8_HD inline
#endif

namespace ak {

constexpr float S8_CLASS_CAP = 2.0f;      // R: a row adopts the class's scale up to this multiple of its own (one bit of resolution)
constexpr int S8_BLOCK = 32, S8_CLASS_ROWS = 16;

AK_S8_HD int s8_class_of(int row_in_block) { return (row_in_block >> 2) & 1; }
// member m (0..15) of class `half` of a block, as a row of the block: k_group_bounds' set
AK_S8_HD int s8_class_member(int half, int m) { return 8 * (m >> 2) + 4 * half + (m & 3); }

AK_S8_HD bool s8_pos_finite(float x) { return x > 0.f && x < INFINITY; }

// own scale of a row: max|a| / 127; 0 for a row with a non-finite value (its shadow is all zeros)
AK_S8_HD float s8_own_scale(float max_abs, bool non_finite) { return non_finite ? 0.f : max_abs / 127.f; }

// what a row still to be quantised contributes to its class's E; 0 = the row cannot adopt and contributes nothing
AK_S8_HD float s8_product(float own, float ea) {
    if (!s8_pos_finite(own) || !s8_pos_finite(ea)) return 0.f;
    const float p = own * ea;
    return s8_pos_finite(p) ? p : 0.f;
}

// what a row of a published shadow contributes: its ea8 as it stands
AK_S8_HD float s8_published(float ea8) { return s8_pos_finite(ea8) ? ea8 : 0.f; }

// E of a class from the contributions of its rows (rows past the end of the corpus contribute 0)
AK_S8_HD float s8_class_max(const float *p, int count) {
    float e = 0.f;
    for (int i = 0; i < count; i++) e = p[i] > e ? p[i] : e;
    return e;
}

struct S8Scale {
    float scale;      // the quantiser's: a8 = clip(round(a / scale)); 0 = an all-zero shadow row
    float ea8;        // the scan-side term stored for the row
    bool shared;      // the row adopted the class's E
};

AK_S8_HD S8Scale s8_row_scale(float own, float ea, float E) {
    const float p = s8_product(own, ea);
    if (p > 0.f && E >= p && E <= S8_CLASS_CAP * p) {
        const float s = E / ea;
        if (s8_pos_finite(s)) return {s > own ? s : own, E, true};
    }
    return {own, own * ea, false};
}

// E of the class `half` of one 32-row block from the block's 32 contributions (k_shadow8 keeps them in LDS)
AK_S8_HD float s8_block_class_max(const float *p_block, int half) {
    float cls[S8_CLASS_ROWS];
    for (int m = 0; m < S8_CLASS_ROWS; m++) cls[m] = p_block[s8_class_member(half, m)];
    return s8_class_max(cls, S8_CLASS_ROWS);
}

// the whole decision for row i of a block still to be quantised, from the block's own scales and contributions: what k_shadow8
// runs per row, and what tests/native/shadow8_scale_main.cpp runs for it on the host
AK_S8_HD S8Scale s8_block_row_scale(const float *own_block, const float *p_block, int i, float ea) {
    return s8_row_scale(own_block[i], ea, s8_block_class_max(p_block, s8_class_of(i)));
}

// the scale the scan applies to a row's integers, in double, for the measured rho: ea8 / ea for an adopting row (the stored
// bits, not the quantiser's rounded quotient), the own scale otherwise
AK_S8_HD double s8_applied_scale(const S8Scale &s, float ea) { return s.shared ? (double)s.ea8 / (double)ea : (double)s.scale; }

}  // namespace ak
