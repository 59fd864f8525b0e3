"""Float64 statements of what the float32 (`precision="f32"`) and split-bf16 (`precision="bf16x3"`) parity kernels compute, the bounds a
correct kernel must meet against them, and CPU emulations of the kernels' documented rounding schemes. Plain numpy, written from the
mathematics, not from the kernels; tests/kernel_refs.py (kr) supplies the shared pieces (bf16 conversion, LayerNorm, Worst).

NO TOLERANCE HERE IS PICKED OR MEASURED. e = 2^-24 is the unit round-off of float32, u = 2^-8 that of bf16 (8 significand bits, round
to nearest even: |fl(x) - x| <= u |x|). Every bound is a formula in e, u and absolute-value sums of the very inputs of the case.

THE SPLIT. x = hi + lo + rem with hi = bf16(x), lo = bf16(x - hi). x - hi has at most 16 significant bits and is exact in float32;
|x - hi| <= u |x|, so |lo| <= u |x| (1 + u) and |rem| = |(x - hi) - lo| <= u |x - hi| <= u^2 |x|. A product of two split numbers computed as
hi.hi + lo.hi + hi.lo leaves out   x w - (xh wh + xl wh + xh wl) = xl wl + xr w + (xh + xl) wr   exactly, of size at most
    u^2 (1 + u)^2 |x| |w| + u^2 |x| |w| + (1 + u^2) u^2 |x| |w|  <=  C_SPLIT |x| |w|,   C_SPLIT = 3 u^2 + 3 u^3 = 4.6e-5
(the code comment's "~4e-6 per product with random sign" is a typical value; this is the bound). The tests do not use the constant: they
use the identity, i.e. the absolute sums |xl| |wl|^T + |xr| |w|^T + |xh + xl| |wr|^T of the case's own halves (split_drop), which
test_parity_kernel_refs_cpu holds to be <= C_SPLIT |x| |W|^T on every case. Where an operand reaches the kernel already split (MODE
5 / 6, gemm_ln_x3: the operation is defined on hi + lo) only lo.lo is dropped: |xl| |wl|^T.

STRUCTURE OF EVERY [hi | lo] OUTPUT. hi is the round-to-nearest-even bf16 of the float32 value, bit for bit; lo the bf16 of value - hi
(exact in float32), bit for bit. Where the float32 value is itself an output (split_hilo, split_rows, the `out` of k3_embed and
k3_add_ln, the x32 of gemm_ln_x3) split_mismatch counts the elements that differ from that. Where it is not (ctx2 of the split attention,
MODE 6) hi + lo must meet the value bound widened by the remainder u^2 |value|, and |lo| must be at most half a bf16 step of hi
(lo_too_large). A float32 result below 2^-126 may be flushed to zero by the hardware: such an element may come back as zero; nothing
else is loosened for it.

float32 GEMM  y = x W^T + bias, one float32 accumulator per output, bias added last. With y_abs = |x| |W|^T + |bias|:
    epilogue 0    (K + 1) e y_abs                       (K products accumulated in any order, each addition rounded once, + the bias)
    epilogue 1    g = 0.5 y (1 + erf(y / sqrt 2)), |g'| <= 1.13:  1.13 (K + 1) e y_abs + 8 e |y|   -- the erf term: y / sqrt 2 rounded
                  (its effect on erf <= 0.5 e), erff within 4 ulp = 8 e |erf| <= 8 e (the HIP math API's stated error), 1 + erf rounded
                  (<= 2 e), the product rounded: 0.5 |y| (0.5 + 8 + 2) e + e |g| <= 6.25 e |y|, inside 8 e |y|
    epilogue 2    + residual, one addition:  (K + 1) e y_abs + e |y + R|
split-bf16 GEMM  the same with 3 K products of bf16 halves (exact in float32) accumulated:  (3 K + 1) e (1 + 2 u) y_abs + split_drop.
MODE 5  as the split GEMM on operands that arrive split: dropped = |xl| |wl|^T only. Columns >= nvalid keep what was there.
MODE 6  gelu(y) = y Phi(y) with Phi from the table gemm.hip documents: 384 cubic Hermite pieces of width 1 / 32 over [-6, 6) built from Phi
    and its density at the nodes, the end pieces held outside the range (phi_pieces, gelu_tab64: float64, from that description). Bound
    against the EXACT gelu:  1.13 dy + tab_dist(y) + eval(y) + u^2 |g|:  tab_dist = |gelu_tab64(y) - gelu64(y)| at that very point (the
    role erf_err plays in kernel_refs), eval the float32 evaluation: t = fma(y, 32, 192) rounded once (e |t|, i.e. e |t| / 32 in y, times the
    density), the four coefficients rounded to float32 and three fma (5 e sum |c_i|), the product with y (e |g|); u^2 |g| is the split's remainder.
gemm_ln_x3  LN(x W^T + bias + res): kr.gemm_ln_ref's dr with the split accumulation and lo.lo in it, kr.layernorm_bound without the bf16 store.

ATTENTION  out = P v, P = softmax(s) over the visible keys, s = q k^T / sqrt(hd) + bias[k - q]. k32m_attn works in base e (expf), k3_attn in
base 2 (q carries log2(e) / sqrt(hd), the table handed to it is the base-2 one, v_exp_f32). With L = |q| |k|_max / sqrt(hd) + |bias|_max
(Cauchy-Schwarz, natural units) a logit is hd products accumulated plus scale, mask / bias add and the subtraction of the running
maximum: |ds| <= (hd + 4) e L. In base e p = e^(s - m) moves by |ds| relatively; in base 2 the logit is log2(e) times larger and p = 2^(..)
moves by ln2 times its error: the same number. Numerator and row sum both: 2 (hd + 4) e L out_abs, out_abs = P |v|. Further:
    the exponential's stated error, 1 ulp = 2 e, numerator and row sum                            4 e out_abs
    the n-term sums of O and l (n = the keys walked, 32 per block), each product added on its own  2 n e out_abs
    the rescaling by alpha per key block (a product and alpha's own 1 ulp + rounded argument), O and l   6 nb e out_abs, nb = ceil(S / 32)
    1 / l and the product with it                                                                2 e |out|
No bf16 rounding of P or of the output appears: there is none. The split kernel accumulates 3 hd and 3 n products instead, and
drops the second-order terms of both products: in the scores max_k split_drop(q', k) / sqrt(hd)-scaled, through the exponential twice; in
P.V with p = ph + pl + pr, |pl| <= u (1 + u) p, |pr| <= u^2 p:  u (1 + u) P |vl| + u^2 P |v| + (1 + u) P |vr|.
A sequence with no visible key gives context rows of exact zeros; rows of masked queries must be finite (they are not compared).

ROW KERNELS  k32_embed / k3_embed: LN((word[id] + pos[p]) + type), ids out of range -> row 0; k32_add_ln / k3_add_ln: LN(y + r). kr.layernorm_bound
with dr = the float32 additions in front (e times each RESULT) and no bf16 store. k_pool<false>: the masked mean (or token 0), then x /
max(|x|, 1e-12): stack_kernel_refs' pooling bound with this kernel's tree (at most S + 8 additions; the weights are 0 / 1, the products exact)
and its L2 tail.

A comparison returns the worst err / bound and where (kr.Worst); a kernel passes at <= 1."""
import math

import numpy as np

try:
    from tests import kernel_refs as kr
except ImportError:          # imported by the worker script, whose directory is tests/ itself
    import kernel_refs as kr

E, U = kr.E32, kr.U
F = np.float32
C_SPLIT = 3.0 * U * U + 3.0 * U ** 3
TINY = 2.0 ** -126
LOG2E = 1.4426950408889634
L2_FLOOR = 1e-12


# ---- the split ---------------------------------------------------------------------------------------------------------------------------
def split_bits(x):
    """float32 x -> (hi bits, lo bits): hi = bf16(x), lo = bf16(x - hi)."""
    x = np.ascontiguousarray(x, F)
    hi = kr.bf16_bits(x)
    return hi, kr.bf16_bits(x - kr.bf16_value(hi))


def split3(x):
    """float32 x -> float64 (hi, lo, rem), hi + lo + rem == x exactly."""
    hb, lb = split_bits(x)
    h, l = kr.bf16_value(hb).astype(np.float64), kr.bf16_value(lb).astype(np.float64)
    return h, l, np.asarray(x, F).astype(np.float64) - h - l


def split_rows(x):
    """[rows][K] float32 -> [rows][2 K] bf16 bits [hi | lo]: the operand layout of MODE 5 / 6 and gemm_ln_x3."""
    hb, lb = split_bits(x)
    return np.concatenate([hb, lb], axis=-1)


def split_mismatch(value32, hi_bits, lo_bits):
    """Number of elements whose hi or lo is not the split of the float32 value, bit for bit (flush-to-zero below 2^-126 allowed)."""
    v = np.ascontiguousarray(value32, F)
    hb, lb = split_bits(v)
    hi_bits, lo_bits = np.asarray(hi_bits, np.uint16), np.asarray(lo_bits, np.uint16)
    d = np.abs(v.astype(np.float64) - kr.bf16_value(hb).astype(np.float64))
    bad_h = (hi_bits != hb) & ~((np.abs(v) < TINY) & ((hi_bits & 0x7FFF) == 0))
    bad_l = (lo_bits != lb) & ~((d < TINY) & ((lo_bits & 0x7FFF) == 0))
    return int((bad_h | bad_l).sum())


def lo_too_large(hi_bits, lo_bits):
    """Number of elements with |lo| above half a bf16 step of hi (hi = 0: lo must be below 2^-126)."""
    h = np.abs(kr.bf16_value(hi_bits).astype(np.float64))
    l = np.abs(kr.bf16_value(lo_bits).astype(np.float64))
    with np.errstate(divide="ignore"):
        step = np.where(h > 0, 2.0 ** (np.floor(np.log2(np.where(h > 0, h, 1.0))) - 7), 0.0)
    return int((l > np.maximum(0.5 * step, TINY)).sum())


def split_drop(x, w):
    """|xl| |wl|^T + |xr| |w|^T + |xh + xl| |wr|^T: what hi.hi + lo.hi + hi.lo leaves out of x w^T, as an absolute sum. x [T][K], w [N][K] float32."""
    xh, xl, xr = split3(x)
    wh, wl, wr = split3(w)
    return np.abs(xl) @ np.abs(wl).T + np.abs(xr) @ np.abs(np.asarray(w, np.float64)).T + np.abs(xh + xl) @ np.abs(wr).T


# ---- GEMM --------------------------------------------------------------------------------------------------------------------------------
def gemm_ref(x, w, bias):
    """(y, y_abs) in float64: y = x W^T + bias, y_abs = |x| |W|^T + |bias|."""
    return kr.gemm_ref(x, w, bias)


def epilogue(epi, y, dy, res=None):
    """(want, bound) of a parity GEMM's epilogue on y known to within dy: 0 as it is, 1 erf GELU, 2 + residual."""
    if epi == 0:
        return y, dy
    if epi == 1:
        return kr.gelu64(y), 1.13 * dy + 8.0 * E * np.abs(y)
    r = y + np.asarray(res, np.float64)
    return r, dy + E * np.abs(r)


def gemm_f32_expect(epi, x, w, bias, res=None):
    y, y_abs = gemm_ref(x, w, bias)
    return epilogue(epi, y, (x.shape[1] + 1) * E * y_abs, res)


def gemm_x3_expect(epi, x, w, bias, res=None):
    """launch_gemm_x3: x float32 (split in the kernel), w float32 (its halves made by split_hilo)."""
    y, y_abs = gemm_ref(x, w, bias)
    return epilogue(epi, y, (3 * x.shape[1] + 1) * E * (1.0 + 2.0 * U) * y_abs + split_drop(x, w), res)


def halves(rows2):
    """[rows][2 K] bf16 bits [hi | lo] -> float64 (hi, lo)."""
    K = rows2.shape[-1] // 2
    return kr.bf16_value(rows2[..., :K]).astype(np.float64), kr.bf16_value(rows2[..., K:]).astype(np.float64)


def gemm_x3w_pre(x2, w2, bias, bias_in_sum=True):
    """MODE 5 / 6 and gemm_ln_x3 before the epilogue: operands as [hi | lo] bf16 rows, the operation defined on hi + lo. (y, dy).
    bias_in_sum False: dy of the accumulation alone (gemm_ln_x3 charges the additions behind it by their results)."""
    xh, xl = halves(x2)
    wh, wl = halves(w2)
    y, y_abs = gemm_ref(xh + xl, wh + wl, bias)
    if not bias_in_sum:
        y_abs = y_abs - np.abs(np.asarray(bias, np.float64))
    return y, (3 * xh.shape[1] + 1) * E * (1.0 + 2.0 * U) * y_abs + np.abs(xl) @ np.abs(wl).T


# ---- the table GELU of MODE 6 ----------------------------------------------------------------------------------------------------------
PHI_N, PHI_LO, PHI_H = 384, -6.0, 1.0 / 32.0
PHI_TMAX = float(F(383.99997))


def Phi64(x):
    from scipy.special import erfc
    return 0.5 * erfc(-np.asarray(x, np.float64) / math.sqrt(2.0))


def phi_pieces():
    """[384][4] float64: piece i over [x0, x0 + h), x0 = -6 + i h, as c0 + c1 d + c2 d^2 + c3 d^3 in d = (x - x0) / h: the cubic Hermite
    interpolant of Phi with the density as its derivative at both nodes."""
    x0 = PHI_LO + PHI_H * np.arange(PHI_N)
    x1 = x0 + PHI_H
    dens = lambda x: np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    d, f0, f1 = Phi64(x1) - Phi64(x0), dens(x0), dens(x1)
    return np.stack([Phi64(x0), PHI_H * f0, 3.0 * d - PHI_H * (2.0 * f0 + f1), -2.0 * d + PHI_H * (f0 + f1)], axis=1)


_PIECES = None


def _pieces():
    global _PIECES
    if _PIECES is None:
        _PIECES = phi_pieces()
    return _PIECES


def gelu_tab64(x):
    """x Phi_table(x) in float64: the end pieces held outside [-6, 6)."""
    x = np.asarray(x, np.float64)
    t = np.clip(32.0 * x + 192.0, 0.0, PHI_TMAX)
    iv = np.floor(t).astype(np.int64)
    d = t - iv
    c = _pieces()[iv]
    return x * (((c[..., 3] * d + c[..., 2]) * d + c[..., 1]) * d + c[..., 0])


def _fma32(a, b, c):
    return (np.asarray(a, F).astype(np.float64) * np.asarray(b, F).astype(np.float64) + np.asarray(c, F).astype(np.float64)).astype(F)


def gelu_tab32(x):
    """The documented float32 evaluation: t = med3(fma(x, 32, 192), 0, 383.99997), piece and fraction from t, three fma, times x."""
    x = np.asarray(x, F)
    t = np.clip(_fma32(x, F(32), F(192)), F(0), F(PHI_TMAX))
    iv = t.astype(np.int32)
    d = (t - iv.astype(F)).astype(F)
    c = _pieces().astype(F)[iv]
    p = _fma32(_fma32(_fma32(c[..., 3], d, c[..., 2]), d, c[..., 1]), d, c[..., 0])
    return (x * p).astype(F)


def gelu_tab_bound(y, dy):
    """MODE 6's value bound against the exact GELU (module docstring)."""
    y = np.asarray(y, np.float64)
    g = kr.gelu64(y)
    t = np.clip(32.0 * y + 192.0, 0.0, PHI_TMAX)
    csum = np.abs(_pieces()[np.floor(t).astype(np.int64)]).sum(axis=-1)
    dens = np.exp(-0.5 * y * y) / math.sqrt(2.0 * math.pi)
    ev = np.abs(y) * (dens * E * t / 32.0 + 5.0 * E * csum) + E * np.abs(g)
    return g, 1.13 * dy + np.abs(gelu_tab64(y) - g) + ev + U * U * np.abs(g)


# ---- attention ---------------------------------------------------------------------------------------------------------------------------
def rel_dense(rel_row, S, flip=False):
    """bias[q][k] = row[REL_MID + k - q] (flip: the mutant that reads q - k)."""
    q = np.arange(S)[:, None]
    k = np.arange(S)[None, :]
    return np.asarray(rel_row, np.float64)[kr.REL_MID + (q - k if flip else k - q)]


def attn_probs(q, k, vis, bias, hd_scale):
    """P [S][S] float64 of one head: softmax over the visible keys of q k^T hd_scale + bias (natural units); zero rows where nothing is visible."""
    s = (np.asarray(q, np.float64) @ np.asarray(k, np.float64).T) * hd_scale
    if bias is not None:
        s = s + bias
    s = np.where(vis, s, -np.inf)
    m = s.max(axis=1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    p = np.exp(s - m)
    l = p.sum(axis=1, keepdims=True)
    return p / np.where(l > 0, l, 1.0)


def attn_expect(q, k, v, key_mask, bias, split, bias_max=0.0):
    """(out, bound) [S][hd] of one (sequence, head): q, k, v [S][hd] float32, key_mask [S] bool, bias dense [S][S] in natural units or None.
    split: the bound of k3_attn (three-term products), else k32m_attn's."""
    S, hd = q.shape
    vis = np.broadcast_to(np.asarray(key_mask, bool)[None, :], (S, S))
    P = attn_probs(q, k, vis, bias, 1.0 / math.sqrt(hd))
    v64 = np.asarray(v, np.float64)
    out, out_abs = P @ v64, P @ np.abs(v64)
    qn = np.sqrt((np.asarray(q, np.float64) ** 2).sum(axis=1))
    kn = math.sqrt(float((np.asarray(k, np.float64) ** 2).sum(axis=1).max()))
    L = qn * kn / math.sqrt(hd) + bias_max
    nb = -(-S // 32)
    n = 32 * nb
    m3 = 3 if split else 1
    f = E * (m3 * n + n + 6.0 * nb + 4.0 + 2.0 * (m3 * hd + 4) * L)
    bound = f[:, None] * out_abs + 2.0 * E * np.abs(out)
    if split:
        qs = (np.asarray(q, F) * (F(LOG2E) / np.sqrt(F(hd)))).astype(F)             # q as the kernel splits it: base 2, one rounding
        ds = split_drop(qs, np.asarray(k, F)).max(axis=1) / LOG2E                    # back in natural units
        vh, vl, vr = split3(v)
        bound = bound + 2.0 * ds[:, None] * out_abs + U * (1.0 + U) * (P @ np.abs(vl)) + U * U * out_abs + (1.0 + U) * (P @ np.abs(vr))
    return out, bound


# ---- row kernels -------------------------------------------------------------------------------------------------------------------------
def embed_rows(ids, posrow, word, pos, typ, vocab):
    """(r, dr): the float64 row (word[id] + pos[p]) + type and the bound of its two float32 additions; ids out of range read row 0."""
    ids = np.asarray(ids).copy()
    ids[(ids < 0) | (ids >= vocab)] = 0
    a = word[ids].astype(np.float64) + pos[posrow].astype(np.float64)
    r = a + typ.astype(np.float64)
    return r, E * np.abs(a) + E * np.abs(r)


def ln_expect(r, dr, gamma, beta, eps, **mut):
    """(out, bound) of a float32 LayerNorm of rows r known to within dr: no bf16 store."""
    out, parts = kr.layernorm_ref(r, gamma, beta, eps, **mut)
    return out, kr.layernorm_bound(r, dr, gamma, out, parts, False)


def pool_expect(x, mask, pooling, normalise, count_masked=False, cls_batch0=False):
    """k_pool<false>: x [B][S][H] float32, mask [B][S]; pooling 0 mean / 1 CLS. (want, bound) [B][H]. A sequence without a visible token has
    count max(0, 1e-9): zeros. The two flags are the mutants."""
    B, S, H = x.shape
    x64 = x.astype(np.float64)
    w = np.ones((B, S)) if count_masked else (np.asarray(mask) != 0).astype(np.float64)
    if pooling == 1:
        y = x64[np.zeros(B, int) if cls_batch0 else np.arange(B), 0]
        dy = np.zeros_like(y)
    else:
        cnt = np.maximum(w.sum(axis=1, keepdims=True), 1e-9)
        y = (w[:, :, None] * x64).sum(axis=1) / cnt
        dy = (S + 8) * E * (w[:, :, None] * np.abs(x64)).sum(axis=1) / cnt + 3.0 * E * np.abs(y)
    if not normalise:
        return y, dy
    nrm = np.sqrt((y * y).sum(axis=1, keepdims=True))
    s = 1.0 / np.maximum(nrm, L2_FLOOR)
    out = y * s
    yh = np.where(nrm > 0, np.abs(y) / np.where(nrm > 0, nrm, 1.0), 0.0)
    tree = 4 + 8                                     # <= 4 squares per thread, 8 halving steps over 256 threads
    free = s * (dy + yh * (yh * dy).sum(axis=1, keepdims=True)) + (0.5 * (tree + 1) + 3.0) * E * np.abs(out)
    floor = s * dy + 2.0 * E * np.abs(out)
    return out, np.where(nrm >= L2_FLOOR, free, floor)


# ---- emulations of the documented rounding schemes -----------------------------------------------------------------------------------------
def emu_epilogue(epi, acc, bias, res):
    from scipy.special import erf
    v = (acc + np.asarray(bias, F)).astype(F)
    if epi == 1:
        a = (v * F(0.70710678118654752)).astype(F)
        er = erf(a.astype(np.float64)).astype(F)                 # (a correctly rounded erff: inside the 4 ulp the bound allows)
        v = ((F(0.5) * v) * (F(1.0) + er)).astype(F)
    if epi == 2:
        v = (v + np.asarray(res, F)).astype(F)
    return v


def emu_gemm_f32(epi, x, w, bias, res=None, step=32):
    """k32m_gemm: one float32 chain over k ascending (here: float32 partial products of `step` k at a time, added in order)."""
    x, w = np.asarray(x, F), np.asarray(w, F)
    acc = np.zeros((x.shape[0], w.shape[0]), F)
    for k0 in range(0, x.shape[1], step):
        acc = (acc + x[:, k0:k0 + step] @ w[:, k0:k0 + step].T).astype(F)
    return emu_epilogue(epi, acc, bias, res)


def emu_three_term(xh, xl, wh, wl, step=16):
    """Three bf16 products per 16-k sub-step into one float32 accumulator: lo.hi, hi.lo, then hi.hi (float32 arrays holding bf16 values)."""
    acc = np.zeros((xh.shape[0], wh.shape[0]), F)
    for k0 in range(0, xh.shape[1], step):
        s = slice(k0, k0 + step)
        for a, b in ((xl, wh), (xh, wl), (xh, wh)):
            acc = (acc + a[:, s] @ b[:, s].T).astype(F)
    return acc


def emu_gemm_x3(epi, x, w, bias, res=None):
    xh, xl = (kr.bf16_value(b) for b in split_bits(x))
    wh, wl = (kr.bf16_value(b) for b in split_bits(w))
    return emu_epilogue(epi, emu_three_term(xh, xl, wh, wl), bias, res)


def emu_gemm_x3w(mode, x2, w2, bias):
    """MODE 5 -> float32 [T][N]; MODE 6 -> [T][2 N] bf16 bits."""
    K = x2.shape[1] // 2
    acc = emu_three_term(kr.bf16_value(x2[:, :K]), kr.bf16_value(x2[:, K:]), kr.bf16_value(w2[:, :K]), kr.bf16_value(w2[:, K:]), step=64)
    v = (acc + np.asarray(bias, F)).astype(F)
    return v if mode == 5 else split_rows(gelu_tab32(v))


def emu_attn(q, k, v, key_mask, bias, split):
    """32-key blocks, online softmax in float32, the row sum from the same p that feeds P.V; split: base 2 and both products three-term."""
    S, hd = q.shape
    q, k, v = np.asarray(q, F), np.asarray(k, F), np.asarray(v, F)
    sp = lambda a: tuple(kr.bf16_value(b) for b in split_bits(a))
    if split:
        qh, ql = sp((q * (F(LOG2E) / np.sqrt(F(hd)))).astype(F))
        kh, kl = sp(k)
        vh, vl = sp(v)
        ex = lambda a: np.exp2(a.astype(np.float64)).astype(F)
    else:
        ex = lambda a: np.exp(a.astype(np.float64)).astype(F)
    o = np.zeros((S, hd), F)
    m = np.full(S, -np.inf, F)
    l = np.zeros(S, F)
    km = np.asarray(key_mask, bool)
    with np.errstate(invalid="ignore"):
        for k0 in range(0, S, 32):
            s_ = slice(k0, min(k0 + 32, S))
            if split:
                sc = ((ql @ kh[s_].T + qh @ kl[s_].T).astype(F) + qh @ kh[s_].T).astype(F)
                if bias is not None:
                    sc = (sc + (bias[:, s_] * LOG2E).astype(F)).astype(F)
            else:
                sc = ((q @ k[s_].T).astype(F) * (F(1) / np.sqrt(F(hd)))).astype(F)
                if bias is not None:
                    sc = (sc + bias[:, s_].astype(F)).astype(F)
            sc = np.where(km[s_][None, :], sc, F(-np.inf))
            mn = np.maximum(m, sc.max(axis=1))
            mref = np.where(np.isfinite(mn), mn, F(0))
            alpha = np.where(np.isfinite(m), ex(m - mref), F(0))
            p = np.where(np.isfinite(sc), ex(sc - mref[:, None]), F(0))
            l = (l * alpha + p.sum(axis=1, dtype=F)).astype(F)
            if split:
                ph, pl = sp(p)
                pv = ((vl[s_].T @ ph.T + vh[s_].T @ pl.T).astype(F) + vh[s_].T @ ph.T).astype(F).T
            else:
                pv = p @ v[s_]
            o = (o * alpha[:, None] + pv).astype(F)
            m = mn
    inv = np.where(l > 0, F(1) / np.where(l > 0, l, F(1)), F(0))
    return (o * inv[:, None]).astype(F)


def emu_pool(x, mask, pooling, normalise):
    x = np.asarray(x, F)
    B, S, H = x.shape
    w = (np.asarray(mask) != 0).astype(F)
    if pooling == 1:
        y = x[:, 0].copy()
    else:
        cnt = np.maximum(w.sum(axis=1, dtype=F), F(1e-9))
        y = np.zeros((B, H), F)
        for s in range(S):
            y = (y + w[:, s:s + 1] * x[:, s]).astype(F)
        y = (y / cnt[:, None]).astype(F)
    if not normalise:
        return y
    nrm = np.maximum(np.sqrt((y * y).sum(axis=1, dtype=F)), F(L2_FLOOR))
    return (y / nrm[:, None]).astype(F)
