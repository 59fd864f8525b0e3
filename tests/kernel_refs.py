"""Float64 statements of the operations the encoder-side HIP kernels perform, the error bounds a bf16 kernel must meet against
them, and an emulation of the kernels' rounding scheme. Plain numpy, written from the mathematics, not from the kernels.

    attention    out = P v,  P = softmax_2(q k^T + bias) over the visible keys.   q carries log2(e) / sqrt(hd): the scale is the
                 producer's job (the QKV GEMM, MODE 0) and is tested there.
    gemm         y = x W^T + bias, then the epilogue of each mode.

THE BAR IS DERIVED. u = 2^-8 is the unit round-off of bf16 (8 significand bits, round to nearest even: |fl(x) - x| <= u |x|),
e = 2^-24 that of float32.

Attention. The kernels round twice on the data path: P to bf16 for the second MFMA and the context to bf16 on the way out; the row
sum is taken from the unrounded p. With out_abs = P |v|:
    P rounding          |sum_i dp_i v_i| / l <= u sum_i p_i |v_i| / l = u out_abs
    output rounding     u |ctx| = u |out| to first order
    float32 terms       a logit is a sum of hd products accumulated in float32 (plus the bias / mask add and the subtraction of the
                        running maximum): |ds| <= (hd + 4) e (|q| |k|_max + |bias|_max) by Cauchy-Schwarz. p = 2^(s - m) moves by
                        ln2 |ds| relatively, numerator and row sum both: 2 ln2 |ds| out_abs. The sums over n keys of O and of l,
                        each bounded as if every product were added on its own: 2 n e out_abs.
    bound = u (|out| + out_abs) + e (2 n + 2 ln2 (hd + 4) (|q| |k|_max + |bias|_max)) out_abs
The float32 part is 5-15 % of the whole at S = 8192 and for the spike probes, far less elsewhere.

GEMM. With y_abs = |x| |W|^T + |bias| the float32 accumulation over K products and the bias add give |dy| <= (K + 1) e y_abs =: e_pre.
Per mode (g' = the slope of the epilogue at that point; every bf16 store adds u |stored value|):
    MODE 2   float32 out                    e_pre
    MODE 0   q = bf16(y qscale)             qscale e_pre + (u + e) |y qscale|;   k, V^T = bf16(y): e_pre + u |y|
    MODE 1   bf16(gelu(y)), narrow tile     1.13 e_pre + 0.5 |y| erf_err(y / sqrt 2) + u |gelu(y)|    (|gelu'| <= 1.13; the kernel's erf is a
                                            documented polynomial: erf_err is its distance from the exact function at that point, in
                                            float64 on the CPU, plus the running error bound of its float32 Horner evaluation)
             wide tile: GELU from the table 1.13 e_pre + 1.02 (1.13 u |y| + u |gelu(y)|) + 2^-15: what
                                            test_gelu_table_of_the_fused_layer_kernel_is_the_exact_function proves about the lookup
    MODE 4   bf16(bf16(y) + res)            e_pre + u |y| + u |y + res| (1 + u)      (the GEMM output is rounded before the add)
    MODE 7   bf16(silu(g) up)               1.1 |up| e_pre(g) + |silu(g)| e_pre(up) + (|g| + 4) e |r| + u |r|   (|silu'| <= 1.1; the
                                            fast exponential: its argument g log2(e) is rounded in float32, |g| e relative in the result)
    MODE 8   bf16(gelu(a) g)                1.13 |g| e_pre(a) + |gelu(a)| e_pre(g) + 0.5 |a| |g| erf_err(a / sqrt 2) + u |r|
A comparison returns the worst err / bound and where it occurred; a kernel passes at <= 1.

LAYERNORM of a row r of n features: mu = mean r, var = mean (r - mu)^2 (biased, inside the root together with eps),
rstd = 1 / sqrt(var + eps), rh = (r - mu) rstd, out = gamma rh + beta. A perturbation dr of the row moves it, to first order, by
gamma rstd ((dr - mean dr) - rh mean(rh dr)) (d rstd = -rstd^2 mean(rh dr)):
    perturbation        |gamma| rstd (|dr| + mean |dr| + |rh| mean(|rh| |dr|))
    float32 statistics  the sum of n terms, each addition bounded on its own: |d mu| <= n e mean |r| -> |gamma| rstd n e mean |r|; the
                        centred squares ((n + 3) e relative in var, half of it in rstd) and the four operations of
                        (r - mu) rstd gamma + beta: (0.5 (n + 3) + 4) e |gamma rh| + e |out|
    bf16 store          u |out|
Every term but the last two carries rstd |r|-sized factors: a row whose mean is large against its standard deviation is bounded
(and computed) worse in proportion to |mean| / std, and a row of near-zero variance by 1 / sqrt(eps).
    gemm_ln    dr = (K + 1) e |x| |W|^T + e |bias + res| + e |r|: the accumulation, then bias + residual, then their sum (each
               float32 addition e times its RESULT: a row whose bias and residual cancel is not charged for their sizes); the
               residual itself is an input (float32 rows or bf16 rows: exact either way). The float32 output carries no u |out|.
    the fused layer  x <- LN2(z + W2 gelu(W1 z + b1) + b2), z = LN1(x + ctx Wo^T + bo): z leaves LayerNorm-1 as bf16 (the MFMA operand AND
               the residual of LayerNorm-2: both read the X registers) and gelu(h) enters the second product as bf16. Charging
               u |z| and u |gelu(h)| per element and carrying them through |W1|, the slope 1.13 and |W2| as absolute sums gives a
               bound of 3 against outputs of 0.7 (384 x 1536 terms that cannot all have the same sign): it sees nothing. So
               the bound is split by the triangle inequality: |kernel - out| <= |out~ - out| + |kernel - out~|, out~ the same
               formula evaluated in float64 WITH the kernels' documented roundings (z and gelu(h) rounded to bf16; for the role kernel
               k_ffn384r gelu by gelu_table.h's table, gelu_table64). The first term is a number, not an estimate: what those
               roundings do to this very row (never more than the absolute-sum propagation it replaces). The second is carried
               the usual way, but a rounding is monotone: the kernel's bf16 value, rounded from a float32 value within b of out~'s,
               lies between bf16(v - b) and bf16(v + b) -- dz = max |bf16(z +- b_LN1) - bf16(z)| is zero wherever no rounding
               boundary lies within b_LN1 (the float32 bound of LayerNorm-1) and one bf16 step where one does.
               dh = dz |W1|^T + e_pre;  polynomial kernels (k_ffn384w8's half tiles, the 4-wave generation):
               dg = max |bf16(g +- b_g) - bf16(g)|, b_g = 1.13 dh + 0.5 |h| erf_err;  table: dg = max |tab(h +- dh) - tab(h)|;
               dy = dg |W2|^T + e_pre; dr2 = dz + dy + e (|y| + |r2|) into the LayerNorm bound with a bf16 store.
    stand-alone LayerNorms  dr = e |r| when a residual is added (one float32 add), 0 otherwise.
LAZY LayerNorm (gemm.hip LZ). Between launches a row r travels as r~ = bf16(gamma (.) r) with its float32 (mean, 1 / std); the
consumer finishes LN(r) = rstd (r~ - mu gamma) + beta. The operation the tests hold it to is LN(r) of the UNROUNDED r with exact
statistics, so the rounding of r~ is the kernel's to answer for:
    |d LN(r)_k| <= rstd u |gamma_k r_k|       -- u |r| rstd, not u |LN(r)|: it grows with |mean| / std (FIRST CANCELLATION TERM)
                   + e rstd (3 |r~_k| + 4 |mu gamma_k|) + e |LN(r)_k|    (float32 statistics as given, rounded once: e each; two fma)
    MODE 0 / 1 (A operand)   out = rstd (acc - mu fold_c) + b':  rstd u (|gamma r| |W|^T) + rstd (K + 1) e (|r~| |W|^T)
                             + e (3 rstd |acc| + 4 rstd |mu| (|gamma| |W|^T) + 2 |out|)  [fold_c, b' as given, rounded to float32: inside the 4 and 2]
                             then the epilogue's own terms (q scale, table GELU, bf16 store) as for the plain modes
    MODE 4     r = x W^T + b + LN_prev(r_prev) (or + the bf16 rows as they are): dr = e_pre + |d LN_prev| + 2 e (y_abs + |res|);
               stored out_g (.) r, rounded once: |out_g| dr + (u + e) |out_g r|; the partial sums per 128-feature slice
               |d sum| <= sum dr + 128 e sum |r|,  |d sumsq| <= sum (2 |r| dr + dr^2) + 130 e sum (|r| + dr)^2
               (dr^2 kept: behind a near-constant residual row dr exceeds |r|)
    ln_finalize   one-pass variance from raw sums S1 = sum r, S2 = sum r^2 over nslot slices: mu = S1 / n, var = S2 / n - mu^2.
               |d mu| <= (nslot + 1) e |S1| / n;  |d var| <= (nslot + 2) e S2 / n + 2 |mu| |d mu| + 2 e mu^2  -- S2 / n = mean^2 + var, so
               relative to var this is e (mean^2 + var) / var (SECOND CANCELLATION TERM; with the n-term sums of the producing
               launch in front of it: e n (mean^2 + var) / var);  rstd is then bounded over the whole interval
               [max(var - d var, 0), var + d var] + eps (the kernel clamps a negative variance to 0), not to first order: for a
               near-constant row d var exceeds var + eps, and the bound says so;  + 2 e rstd for the root and the division
    fold_ln    K-term float32 sums: |d c| <= (K + 1) e |gamma| |W|^T, |d b'| <= (K + 2) e (|beta| |W|^T + |b|)
"""
import math

import numpy as np

U = 2.0 ** -8
E32 = 2.0 ** -24
LN2 = math.log(2.0)
REL_ROW, REL_MID = 2048, 1024   # layout of a head's relative-position bias row: distance d at REL_MID + d


# ---- number formats and layouts ----------------------------------------------------------------------------------------
def bf16_bits(x):
    """float -> bf16 bit patterns (uint16), round to nearest even."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    """bf16 bit patterns -> float32 values."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_value(bf16_bits(x))


def vt_pos(s):
    """Position of key s inside its V^T row: the keys of a group of 16 are stored [0-3, 8-11, 4-7, 12-15]."""
    s = np.asarray(s)
    return (s & ~12) | ((s & 4) << 1) | ((s & 8) >> 1)


def pack_token_major(bits):
    """[B][heads][S][hd] bf16 bits -> [B][S][heads * hd]."""
    B, h, S, hd = bits.shape
    return np.ascontiguousarray(bits.transpose(0, 2, 1, 3)).reshape(B, S, h * hd)


def pack_head_major(bits):
    """[B][heads][S][hd] bf16 bits as they are (a head's rows contiguous; the decoder's [B][heads][S][128] too)."""
    return np.ascontiguousarray(bits)


def pack_vt(bits, pos=None):
    """[B][heads][S][hd] bf16 bits -> V^T [B][heads * hd][S], key s of a row at pos[s] (vt_pos order)."""
    B, h, S, hd = bits.shape
    pos = vt_pos(np.arange(S)) if pos is None else np.asarray(pos)
    out = np.empty((B, h * hd, S), np.uint16)
    out[:, :, pos] = bits.transpose(0, 1, 3, 2).reshape(B, h * hd, S)
    return out


def unpack_vt(vt, pos=None):
    """V^T [B][H][S] bf16 bits in vt_pos order -> [B][S][H] bits."""
    S = vt.shape[-1]
    pos = vt_pos(np.arange(S)) if pos is None else np.asarray(pos)
    return np.ascontiguousarray(vt[:, :, pos].transpose(0, 2, 1))


# ---- visibility ----------------------------------------------------------------------------------------------------------
class Visibility:
    """Which keys a query sees: key_mask[k] and |q - k| <= window (window None: no band) and k <= q + diag when causal.
    `diag` moves the causal diagonal (0: the operation; the mutants use +1 / -1)."""

    def __init__(self, key_mask, window=None, causal=False, diag=0):
        self.key_mask = np.asarray(key_mask, dtype=bool)
        self.window, self.causal, self.diag = window, causal, diag

    def key_range(self, q_lo, q_hi):
        """A key interval outside which no query of [q_lo, q_hi) sees anything."""
        nz = np.flatnonzero(self.key_mask)
        if nz.size == 0:
            return 0, 0
        lo, hi = int(nz[0]), int(nz[-1]) + 1
        if self.window is not None:
            lo, hi = max(lo, q_lo - self.window), min(hi, q_hi + self.window)
        if self.causal:
            hi = min(hi, q_hi + self.diag)
        return lo, max(lo, hi)

    def block(self, q_lo, q_hi, k_lo, k_hi):
        q = np.arange(q_lo, q_hi)[:, None]
        k = np.arange(k_lo, k_hi)[None, :]
        vis = np.broadcast_to(self.key_mask[k_lo:k_hi][None, :], (q_hi - q_lo, k_hi - k_lo)).copy()
        if self.window is not None:
            vis &= np.abs(q - k) <= self.window
        if self.causal:
            vis &= k <= q + self.diag
        return vis

    def dense(self, S):
        return self.block(0, S, 0, len(self.key_mask))


def mask_right(S, n):
    return np.arange(S) < n


def mask_left(S, n):
    return np.arange(S) >= S - n


def mask_holes(S, n, rng):
    """n leading keys with about a tenth of them removed, one whole 32-key block among them when there is room; key 0 stays."""
    m = np.arange(S) < n
    m &= rng.random(S) >= 0.1
    if n >= 96:
        m[32:64] = False
    if n > 0:
        m[0] = True
    return m


def rel_bias_dense(rel_row, S):
    """MPNet's additive term rel[k - q] as a dense [S][S] matrix (rel_row: one head's row, distance d at REL_MID + d)."""
    q = np.arange(S)[:, None]
    k = np.arange(S)[None, :]
    return np.asarray(rel_row, dtype=np.float64)[REL_MID + k - q]


# ---- attention -------------------------------------------------------------------------------------------------------------
def attention_ref(q, k, v, visible, bias=None, chunk=512, scale=1.0):
    """(out, out_abs) for one head: q [Sq][hd], k / v [Sk][hd], visible a Visibility or a dense bool [Sq][Sk], bias dense [Sq][Sk]
    or None. float64 throughout. A query that sees no key gets zeros (its row is not part of any comparison)."""
    q = np.asarray(q, np.float64) * scale
    k = np.asarray(k, np.float64)
    v = np.asarray(v, np.float64)
    Sq, Sk = q.shape[0], k.shape[0]
    out = np.zeros((Sq, v.shape[1]))
    out_abs = np.zeros_like(out)
    for lo in range(0, Sq, chunk):
        hi = min(lo + chunk, Sq)
        if isinstance(visible, Visibility):
            k_lo, k_hi = visible.key_range(lo, hi)
            if k_hi <= k_lo:
                continue
            vis = visible.block(lo, hi, k_lo, k_hi)
        else:
            k_lo, k_hi, vis = 0, Sk, visible[lo:hi]
        s = q[lo:hi] @ k[k_lo:k_hi].T
        if bias is not None:
            s = s + bias[lo:hi, k_lo:k_hi]
        s = np.where(vis, s, -np.inf)
        m = s.max(axis=1)
        m = np.where(np.isfinite(m), m, 0.0)
        p = np.exp2(s - m[:, None])
        l = p.sum(axis=1)
        p /= np.where(l > 0, l, 1.0)[:, None]
        out[lo:hi] = p @ v[k_lo:k_hi]
        out_abs[lo:hi] = p @ np.abs(v[k_lo:k_hi])
    return out, out_abs


def attention_bound(q, k, out, out_abs, bias_max=0.0):
    """The derived bound (module docstring) per element of `out`; n = every key of the row."""
    q = np.asarray(q, np.float64)
    k = np.asarray(k, np.float64)
    hd, n = q.shape[1], k.shape[0]
    qn = np.sqrt((q * q).sum(axis=1))
    kn = math.sqrt(float((k * k).sum(axis=1).max())) if n else 0.0
    f32 = E32 * (2.0 * n + 2.0 * LN2 * (hd + 4) * (qn * kn + bias_max))
    return U * (np.abs(out) + out_abs) + f32[:, None] * out_abs


def attention_emulate(q, k, v, visible, bias=None):
    """The kernels' rounding scheme on the CPU: 32-key blocks, online softmax in float32, P rounded to bf16 for the second product,
    the row sum from the unrounded p, bf16 output. Blocks without a visible pair are skipped for the queries concerned (they leave
    the running maximum and sum unchanged either way). Returns float32 values that are bf16 numbers."""
    q = np.asarray(q, np.float32)
    k = np.asarray(k, np.float32)
    v = np.asarray(v, np.float32)
    Sq, Sk = q.shape[0], k.shape[0]
    vis_all = visible.dense(Sq) if isinstance(visible, Visibility) else np.asarray(visible)
    o = np.zeros((Sq, v.shape[1]), np.float32)
    m = np.full(Sq, -np.inf, np.float32)
    l = np.zeros(Sq, np.float32)
    with np.errstate(invalid="ignore"):
        for k0 in range(0, Sk, 32):
            vis = vis_all[:, k0:k0 + 32]
            if not vis.any():
                continue
            s = q @ k[k0:k0 + 32].T
            if bias is not None:
                s = s + bias[:, k0:k0 + 32].astype(np.float32)
            s = np.where(vis, s, np.float32(-np.inf))
            mn = np.maximum(m, s.max(axis=1))
            mref = np.where(np.isfinite(mn), mn, np.float32(0))
            alpha = np.exp2(m - mref).astype(np.float32)
            p = np.exp2(s - mref[:, None]).astype(np.float32)
            l = l * alpha + p.sum(axis=1, dtype=np.float32)
            o = o * alpha[:, None] + bf16_round(p) @ v[k0:k0 + 32]
            m = mn
    inv = np.where(l > 0, np.float32(1) / np.where(l > 0, l, np.float32(1)), np.float32(0))
    return bf16_round(o * inv[:, None])


# ---- comparison ------------------------------------------------------------------------------------------------------------
class Worst:
    """The worst err / bound seen so far and where: (case, batch row, head, token, feature)."""

    def __init__(self):
        self.ratio, self.where, self.n = 0.0, None, 0

    def add(self, got, want, bound, case, b=None, h=None, rows=None, col0=0):
        """got / want / bound [rows][features]; `rows` maps the first axis to token numbers (default: as they are)."""
        got = np.asarray(got, np.float64)
        assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
        if got.size == 0:
            return 0.0
        err = np.abs(got - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err > 0, err / bound, 0.0)
        r = np.where(np.isfinite(got), r, np.inf)      # a NaN / inf where a number is due is over any bound
        i = int(np.argmax(r))
        t, f = divmod(i, got.shape[1])
        worst = float(r.flat[i])
        self.n += got.size
        if worst > self.ratio or self.where is None:
            self.ratio = worst
            self.where = (case, b, h, int(rows[t]) if rows is not None else t, col0 + f, float(got.flat[i]), float(want.flat[i]), float(bound.flat[i]))
        return worst

    def __str__(self):
        if self.where is None:
            return "nothing compared"
        c, b, h, t, f, g, w, bd = self.where
        return f"worst err / bound {self.ratio:.3f} over {self.n} elements at case {c}, batch row {b}, head {h}, token {t}, feature {f}: got {g:.6g}, want {w:.6g}, bound {bd:.3g}"


# ---- GEMM and its epilogues -------------------------------------------------------------------------------------------------
def erf64(x):
    from scipy.special import erf
    return erf(np.asarray(x, np.float64))


def gelu64(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + erf64(x / math.sqrt(2.0)))


ERF_POLY = [-2.400035948e-09, 1.419115847e-07, -3.739696922e-06, 5.846631029e-05, -6.112857373e-04, 4.584099166e-03, -2.581433021e-02,
            1.118641943e-01, -3.757072389e-01, 1.128325701e+00]


def erf_poly(u):
    """The polynomial gemm.hip evaluates for erf(u), |u| clamped to 3.2 and the result to [-1, 1], in float64: what the approximation
    itself costs, apart from float32 rounding. Coefficients as documented in gemm.hip (degree 9 in u^2, times u)."""
    u = np.clip(np.asarray(u, np.float64), -3.2, 3.2)
    t = u * u
    p = np.full_like(u, ERF_POLY[0])
    for ci in ERF_POLY[1:]:
        p = p * t + ci
    return np.clip(p * u, -1.0, 1.0)


def erf_err(u):
    """|erf_poly(u) - erf(u)| plus the running error bound of the float32 evaluation (Horner, 9 fma steps and two products:
    (2 * 10 + 1) e sum_k |c_k| |u|^(2 k + 1); Higham, Accuracy and Stability of Numerical Algorithms, section 5.1)."""
    u = np.asarray(u, np.float64)
    uc = np.clip(np.abs(u), 0.0, 3.2)
    t = uc * uc
    p = np.full_like(uc, abs(ERF_POLY[0]))
    for ci in ERF_POLY[1:]:
        p = p * t + abs(ci)
    return np.abs(erf_poly(u) - erf64(u)) + 21.0 * E32 * p * uc


def gemm_ref(x, w, bias, drop_k=None):
    """(y, y_abs): y = x W^T + bias, y_abs = |x| |W|^T + |bias| in float64. x [T][K], w [N][K] (nn.Linear layout), bias [N]."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    bias = np.asarray(bias, np.float64)
    if drop_k is not None:                           # mutant: one k-slice left out
        x = x.copy()
        x[:, drop_k] = 0.0
    return x @ w.T + bias, np.abs(x) @ np.abs(w).T + np.abs(bias)


def e_pre(y_abs, K):
    return (K + 1) * E32 * y_abs


def epi_f32(y, y_abs, K):
    """MODE 2."""
    return y, e_pre(y_abs, K)


def epi_bf16(y, y_abs, K, scale=1.0):
    """A plain bf16 store of y * scale (MODE 0's q with scale = qscale, its k and V^T with scale = 1)."""
    r = y * scale
    return r, abs(scale) * e_pre(y_abs, K) + (U + (E32 if scale != 1.0 else 0.0)) * np.abs(r)


def epi_gelu(y, y_abs, K, table):
    """MODE 1: the polynomial erf on the narrow tile, the bf16 table on the wide one."""
    r = gelu64(y)
    if table:
        return r, 1.13 * e_pre(y_abs, K) + 1.02 * (1.13 * U * np.abs(y) + U * np.abs(r)) + 2.0 ** -15
    return r, 1.13 * e_pre(y_abs, K) + 0.5 * np.abs(y) * erf_err(y / math.sqrt(2.0)) + U * np.abs(r)


def epi_gelu_erff(y, y_abs, K):
    """gemm_skinny's GELU epilogue: 0.5 v (1 + erff(v / sqrt 2)) in float32 (the device library's erff: a few ulp; with the two
    products and the sum 8 e |y| covers it), one bf16 rounding."""
    r = gelu64(y)
    return r, 1.13 * e_pre(y_abs, K) + 8.0 * E32 * np.abs(y) + U * np.abs(r)


def epi_residual_bf16(y, y_abs, K, res):
    """MODE 4: the GEMM output rounded to bf16, the bf16 residual row added in float32, the sum rounded to bf16."""
    res = np.asarray(res, np.float64)
    r = y + res
    return r, e_pre(y_abs, K) + U * np.abs(y) + U * (1.0 + U) * np.abs(r)


def epi_swiglu(y, y_abs, K, swap=False):
    """MODE 7 over interleaved rows: column 2 j the gate, 2 j + 1 the up value; silu(gate) up, N / 2 columns."""
    g, up = (y[:, 1::2], y[:, 0::2]) if swap else (y[:, 0::2], y[:, 1::2])
    eg, eu = (e_pre(y_abs[:, 1::2], K), e_pre(y_abs[:, 0::2], K)) if swap else (e_pre(y_abs[:, 0::2], K), e_pre(y_abs[:, 1::2], K))
    sg = 1.0 / (1.0 + np.exp(-g))
    silu = g * sg
    r = silu * up
    return r, 1.1 * np.abs(up) * eg + np.abs(silu) * eu + (np.abs(g) + 4.0) * E32 * np.abs(r) + U * np.abs(r)


def epi_geglu(y, y_abs, K, swap=False):
    """MODE 8 over interleaved rows: column 2 j the GELU input a, 2 j + 1 the gate g; gelu(a) g, N / 2 columns."""
    a, g = (y[:, 1::2], y[:, 0::2]) if swap else (y[:, 0::2], y[:, 1::2])
    ea, eg = (e_pre(y_abs[:, 1::2], K), e_pre(y_abs[:, 0::2], K)) if swap else (e_pre(y_abs[:, 0::2], K), e_pre(y_abs[:, 1::2], K))
    ga = gelu64(a)
    r = ga * g
    return r, 1.13 * np.abs(g) * ea + np.abs(ga) * eg + 0.5 * np.abs(a) * np.abs(g) * erf_err(a / math.sqrt(2.0)) + U * np.abs(r)


def qkv_split(y, y_abs, K, H, qscale):
    """MODE 0: columns [0, H) -> q scaled, [H, 2 H) -> k, [2 H, 3 H) -> v (token-major values; the V^T layout is the packer's)."""
    q = epi_bf16(y[:, :H], y_abs[:, :H], K, qscale)
    k = epi_bf16(y[:, H:2 * H], y_abs[:, H:2 * H], K)
    v = epi_bf16(y[:, 2 * H:], y_abs[:, 2 * H:], K)
    return q, k, v


def gemm_emulate(x, w, bias):
    """A bf16-operand GEMM with float32 accumulation on the CPU (products of bf16 numbers are exact in float32; numpy adds them in
    float32 in its own order)."""
    return np.asarray(x, np.float32) @ np.asarray(w, np.float32).T + np.asarray(bias, np.float32)


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------
class LnParts:
    """mu [T][1], rstd [T][1], rh [T][n] of a LayerNorm; ratio [T] = |mean| / std of the rows (std without eps)."""

    def __init__(self, mu, var, rstd, rh):
        self.mu, self.var, self.rstd, self.rh = mu, var, rstd, rh
        with np.errstate(divide="ignore", invalid="ignore"):
            self.ratio = np.where(var[:, 0] > 0, np.abs(mu[:, 0]) / np.sqrt(var[:, 0]), np.inf)


def layernorm_ref(r, gamma, beta, eps, eps_mode="inside", ddof=0, stat_cols=None, stat_shift=0):
    """(out, LnParts): out = gamma (r - mu) / sqrt(var + eps) + beta per row of r [T][n], float64. The other arguments are the mutants:
    eps_mode 'dropped' | 'outside' (added to the root), ddof 1 (variance over n - 1), stat_cols (a bool [n]: features outside it are
    left out of both sums, still divided by n), stat_shift (the statistics of token t + shift)."""
    r = np.asarray(r, np.float64)
    gamma = np.asarray(gamma, np.float64)
    beta = np.asarray(beta, np.float64)
    n = r.shape[1]
    rs = r if stat_cols is None else r * stat_cols
    mu = rs.sum(axis=1, keepdims=True) / n
    c = (rs - mu) if stat_cols is None else (rs - mu) * stat_cols
    var = (c * c).sum(axis=1, keepdims=True) / (n - ddof)
    with np.errstate(divide="ignore"):
        if eps_mode == "inside":
            rstd = 1.0 / np.sqrt(var + eps)
        elif eps_mode == "outside":
            rstd = 1.0 / (np.sqrt(var) + eps)
        else:
            rstd = 1.0 / np.sqrt(var)
    if stat_shift:
        mu, rstd = np.roll(mu, -stat_shift, axis=0), np.roll(rstd, -stat_shift, axis=0)
    rh = (r - mu) * rstd
    return gamma * rh + beta, LnParts(mu, var, rstd, rh)


def layernorm_bound(r, dr, gamma, out, parts, bf16_store):
    """The LayerNorm bound of the module docstring for a row perturbed by at most dr (same shape as r, or a scalar)."""
    r = np.asarray(r, np.float64)
    n = r.shape[1]
    g = np.abs(np.asarray(gamma, np.float64))
    dr = np.broadcast_to(np.asarray(dr, np.float64), r.shape)
    rh = np.abs(parts.rh)
    pert = g * parts.rstd * (dr + dr.mean(axis=1, keepdims=True) + rh * (rh * dr).mean(axis=1, keepdims=True))
    f32 = g * parts.rstd * n * E32 * np.abs(r).mean(axis=1, keepdims=True) + g * rh * (0.5 * (n + 3) + 4.0) * E32 + E32 * np.abs(out)
    return pert + f32 + (U * np.abs(out) if bf16_store else 0.0)


def layernorm_emulate(r32, gamma, beta, eps):
    """The two-pass float32 LayerNorm every non-lazy kernel runs: r32 is the float32 row as the kernel holds it."""
    f = np.float32
    r32 = np.asarray(r32, f)
    n = f(r32.shape[1])
    mu = r32.sum(axis=1, keepdims=True, dtype=f) / n
    c = r32 - mu
    var = (c * c).sum(axis=1, keepdims=True, dtype=f) / n
    rstd = f(1) / np.sqrt(var + f(eps))
    return c * rstd * np.asarray(gamma, f) + np.asarray(beta, f)


def gemm_ln_ref(x, w, bias, res, gamma, beta, eps, **mut):
    """gemm_ln.hip: LN(x W^T + bias + res). Returns (out, bound of the float32 output, bound of the bf16 output, LnParts)."""
    y, y_abs = gemm_ref(x, w, bias)
    res = np.asarray(res, np.float64)
    bias = np.asarray(bias, np.float64)
    r = y + res
    dr = e_pre(y_abs - np.abs(bias), x.shape[1]) + E32 * (np.abs(bias + res) + np.abs(r))
    out, parts = layernorm_ref(r, gamma, beta, eps)
    b32 = layernorm_bound(r, dr, gamma, out, parts, False)
    return out, b32, b32 + U * np.abs(out), parts


def bf16_span(v, b):
    """(bf16(v), max |bf16(v') - bf16(v)| over float32 v' within b of v): rounding is monotone, so the ends of the interval decide."""
    v = np.asarray(v, np.float64)
    c = bf16_round(v.astype(np.float32)).astype(np.float64)
    hi = bf16_round((v + b).astype(np.float32)).astype(np.float64)
    lo = bf16_round((v - b).astype(np.float32)).astype(np.float64)
    return c, np.maximum(hi - c, c - lo)


def gelu_tanh64(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_table64(h):
    """The GELU-by-table of gelu_table.h as a function: h truncated towards zero to sign, exponent and 7 mantissa bits of an f16 (its
    subnormals below 2^-14), the entry bf16(gelu(midpoint of that bucket)). Finite |h| < 65504 only."""
    h = np.asarray(h, np.float64)
    a = np.abs(h)
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    step = np.where(a >= 2.0 ** -14, 2.0 ** (e - 7), 2.0 ** -21)
    mid = np.copysign((np.floor(a / step) + 0.5) * step, h)
    return bf16_round(gelu64(mid).astype(np.float32)).astype(np.float64)


def _ffn_eval(x, ctx, p, eps, scheme, mut=None):
    """The fused layer in float64. scheme None: the operation itself. 'poly' / 'table': with the kernels' roundings as part of it (z and
    gelu(h) to bf16; 'table': gelu_table64) and the bound against THAT (module docstring). Returns (out, bound or None, LnParts of LN2)."""
    f8 = lambda a: np.asarray(a, np.float64)
    x = f8(x)
    g1, be1, g2, be2 = f8(p["g1"]), f8(p["be1"]), f8(p["g2"]), f8(p["be2"])
    bo, b2 = f8(p["bo"]), f8(p["b2"])
    if mut == "gamma1_beta1_for_ln2":
        g2, be2 = g1, be1
    if mut == "bo_missing":
        bo = np.zeros_like(bo)
    if mut == "b2_missing":
        b2 = np.zeros_like(b2)
    dz = np.zeros_like(x)
    if ctx is not None:
        y1, y1_abs = gemm_ref(ctx, p["wo"], bo)
        r1 = y1 + (0.0 if mut == "residual1_not_added" else x)
        z, p1 = layernorm_ref(r1, g1, be1, eps)
        if scheme:
            dr1 = e_pre(y1_abs - np.abs(bo), x.shape[1]) + E32 * (np.abs(y1) + np.abs(r1))
            z, dz = bf16_span(z, layernorm_bound(r1, dr1, g1, z, p1, False))
    else:
        z = x
    w1, w2 = f8(p["w1"]), f8(p["w2"])
    h, h_abs = gemm_ref(z, w1, p["b1"])
    g = gelu_tanh64(h) if mut == "tanh_gelu" else gelu64(h)
    dg = None
    if scheme:
        dh = dz @ np.abs(w1).T + e_pre(h_abs, w1.shape[1])
        if scheme == "table":
            # the bucket of h' within dh of h: the table is monotone in the bucket except across GELU's minimum, where it is flat to a bf16 step
            g = gelu_table64(h)
            dg = np.maximum(np.abs(gelu_table64(h + dh) - g), np.abs(gelu_table64(h - dh) - g)) + np.where(np.abs(h + 0.7518) <= dh, 2.0 ** -9, 0.0)
        else:
            g, dg = bf16_span(g, 1.13 * dh + 0.5 * np.abs(h) * erf_err(h / math.sqrt(2.0)))
    gm = g
    if mut == "w2_k_chunks_swapped":          # features [32, 64) and [64, 96) of the intermediate meet each other's W2 columns
        gm = g.copy()
        gm[:, 32:64], gm[:, 64:96] = g[:, 64:96], g[:, 32:64]
    y2, y2_abs = gemm_ref(gm, w2, b2)
    if mut == "residual2_added_after_ln":
        out, p2 = layernorm_ref(y2, g2, be2, eps)
        return out + z, None, p2
    r2 = y2 + (0.0 if mut == "residual2_not_added" else z)
    out, p2 = layernorm_ref(r2, g2, be2, eps)
    if not scheme:
        return out, None, p2
    dr2 = dz + dg @ np.abs(w2).T + e_pre(y2_abs, w2.shape[1]) + E32 * (np.abs(y2) + np.abs(r2))
    return out, layernorm_bound(r2, dr2, g2, out, p2, True), p2


def ffn_layer_ref(x, ctx, p, eps, table, mut=None):
    """The fused layer of ffn.hip, x <- LN2(z + W2 gelu(W1 z + b1) + b2), z = LN1(x + ctx Wo^T + bo), in float64, and its bound (module
    docstring). x [T][384] the layer's input rows (bf16 values), ctx the attention output or None (then z = x: the feed-forward
    block alone); p: wo, bo, g1, be1, w1, b1, w2, b2, g2, be2. table: the role kernel's GELU by table (True) or the polynomial
    kernels'. mut: the name of a defect (tests/test_kernel_refs_cpu.py), applied to the operation; no bound then.
    Returns (out, bound, LnParts of LayerNorm-2)."""
    out, _, parts = _ffn_eval(x, ctx, p, eps, None, mut)
    if mut:
        return out, None, parts
    o16, b16, _ = _ffn_eval(x, ctx, p, eps, "table" if table else "poly")
    return out, np.abs(o16 - out) + b16, parts


def ffn_layer_emulate(x, ctx, p, eps, table):
    """The documented rounding scheme of the fused layer on the CPU: float32 GEMMs over bf16 operands, z and gelu(h) rounded to
    bf16 (table: the lookup), both LayerNorms two-pass in float32, bf16 out."""
    f = np.float32
    x = np.asarray(x, f)
    if ctx is not None:
        z = bf16_round(layernorm_emulate(gemm_emulate(ctx, p["wo"], p["bo"]) + x, p["g1"], p["be1"], eps))
    else:
        z = x
    h = gemm_emulate(z, p["w1"], p["b1"])
    g = gelu_table64(h).astype(f) if table else bf16_round(gelu64(h).astype(f))
    return bf16_round(layernorm_emulate(gemm_emulate(g, p["w2"], p["b2"]) + z, p["g2"], p["be2"], eps))


# ---- lazy LayerNorm --------------------------------------------------------------------------------------------------------
def lazy_rows(r, gamma):
    """What travels between the launches for rows r [T][n] (float64): r~ = bf16(gamma (.) r) as bits, and the float32 (mean, 1 / std)
    pairs are the caller's (stats_f32)."""
    return bf16_bits((np.asarray(gamma, np.float64) * r).astype(np.float32))


def stats_f32(parts):
    """[T][2] float32 (mean, 1 / std) from float64-exact statistics."""
    return np.concatenate([parts.mu, parts.rstd], axis=1).astype(np.float32)


def lazy_ln_bound(r, gamma, out, parts):
    """|rstd (r~ - mu gamma) + beta - LN(r)| for r~ = bf16(gamma r) and float32-rounded exact statistics (no store rounding)."""
    g = np.abs(np.asarray(gamma, np.float64))
    gr = g * np.abs(r)
    return parts.rstd * (U * gr + E32 * (3.0 * gr + 4.0 * np.abs(parts.mu) * g)) + E32 * np.abs(out)


def lazy_a_ref(r, gamma, beta, eps, w, bias, mut=None):
    """MODE 0 / 1 of launch_gemm_lazy before the epilogue: (y, dy, y_abs) with y = LN(r) W^T + b and dy the bound of
    rstd (acc - mu fold_c) + b' computed from r~ = bf16(gamma r) (module docstring). mut 'mu_fold_c_dropped'."""
    w8 = np.asarray(w, np.float64)
    g = np.asarray(gamma, np.float64)
    ln, parts = layernorm_ref(r, gamma, beta, eps)
    y = ln @ w8.T + np.asarray(bias, np.float64)
    if mut == "mu_fold_c_dropped":
        y = y + parts.rstd * parts.mu * (w8 @ g)[None, :]
    K = w8.shape[1]
    aw = np.abs(w8).T
    gr = np.abs(g * r)
    acc_abs = gr @ aw
    mu_c = np.abs(parts.mu) * (np.abs(g) @ aw)[None, :]
    b_abs = np.abs(np.asarray(beta, np.float64)) @ aw + np.abs(np.asarray(bias, np.float64))
    dy = parts.rstd * (U * acc_abs + (K + 1) * E32 * acc_abs) + E32 * (3.0 * parts.rstd * acc_abs + 4.0 * parts.rstd * mu_c + 2.0 * (np.abs(y) + b_abs))
    y_abs = parts.rstd * (acc_abs + mu_c) + b_abs
    return y, dy, y_abs, parts


def lazy_a_emulate(r, gamma, beta, eps, w, bias):
    """The lazy A-operand scheme in float32: bf16 r~, float32 statistics, fold_c and b' as float32, rstd (acc - mu c) + b'."""
    f = np.float32
    parts = layernorm_ref(r, gamma, beta, eps)[1]
    rt = bf16_value(lazy_rows(r, gamma))
    st = stats_f32(parts)
    c, bf = fold_ln_ref(w, gamma, beta, bias)[:2]
    acc = rt @ np.asarray(w, f).T
    return st[:, 1:2] * (acc - st[:, 0:1] * c.astype(f)) + bf.astype(f)


def lazy_mode4_ref(x, w, bias, out_g, res_rows=None, prev=None, mut=None):
    """MODE 4 of launch_gemm_lazy: r = x W^T + b + residual, the residual either bf16 rows as they are (res_rows) or
    LN_prev(r_prev) finished on the way (prev = (r_prev, gamma, beta, eps): the kernel reads bf16(gamma r_prev) and float32
    statistics). Returns (r, dr, stored = out_g (.) r, its bound). mut: 'res_b_dropped'."""
    y, y_abs = gemm_ref(x, w, bias)
    og = np.asarray(out_g, np.float64)
    if prev is not None:
        rp, g, b, eps = prev
        res, parts = layernorm_ref(rp, g, np.zeros_like(np.asarray(b, np.float64)) if mut == "res_b_dropped" else b, eps)
        dres = lazy_ln_bound(rp, g, res, parts)
    else:
        res, dres = np.asarray(res_rows, np.float64), 0.0
    r = y + res
    dr = e_pre(y_abs, x.shape[1]) + dres + 2.0 * E32 * (y_abs + np.abs(res))
    stored = og * r
    return r, dr, stored, np.abs(og) * dr + (U + E32) * np.abs(stored)


def slice_sums_ref(r, dr):
    """Partial sums [nslot][T][2] = (sum r, sum r^2) per 128-feature slice and their bounds."""
    T, n = r.shape
    rr = r.reshape(T, n // 128, 128)
    dd = np.broadcast_to(dr, r.shape).reshape(T, n // 128, 128)
    s = np.stack([rr.sum(axis=2), (rr * rr).sum(axis=2)], axis=2).transpose(1, 0, 2)
    b1 = dd.sum(axis=2) + 128 * E32 * np.abs(rr).sum(axis=2)
    b2 = (2.0 * np.abs(rr) * dd + dd * dd).sum(axis=2) + 130 * E32 * ((np.abs(rr) + dd) ** 2).sum(axis=2)
    return s, np.stack([b1, b2], axis=2).transpose(1, 0, 2)


def ln_finalize_ref(part, inv_h, eps, mut=None):
    """(mean, 1 / std) [T][2] from partial sums [nslot][T][2] (float32 values, taken as exact) and the bound of the one-pass float32
    evaluation (module docstring)."""
    p = np.asarray(part, np.float64)
    nslot = p.shape[0]
    s1, s2 = p[:, :, 0].sum(axis=0), p[:, :, 1].sum(axis=0)
    a1, a2 = np.abs(p[:, :, 0]).sum(axis=0), p[:, :, 1].sum(axis=0)
    mu = s1 * inv_h
    var = np.maximum(s2 * inv_h - mu * mu, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    dmu = (nslot + 1) * E32 * a1 * inv_h
    dvar = (nslot + 2) * E32 * a2 * inv_h + 2.0 * np.abs(mu) * dmu + 2.0 * E32 * mu * mu
    hi = 1.0 / np.sqrt(np.maximum(var - dvar, 0.0) + eps)
    drstd = np.maximum(hi - rstd, rstd - 1.0 / np.sqrt(var + dvar + eps)) + 2.0 * E32 * hi
    return np.stack([mu, rstd], axis=1), np.stack([dmu + E32 * np.abs(mu), drstd], axis=1)


def fold_ln_ref(w, gamma, beta, bias):
    """c = W gamma, b' = bias + W beta and their float32 summation bounds."""
    w8 = np.asarray(w, np.float64)
    g, b, bi = (np.asarray(a, np.float64) for a in (gamma, beta, bias))
    K = w8.shape[1]
    aw = np.abs(w8)
    return w8 @ g, bi + w8 @ b, (K + 1) * E32 * (aw @ np.abs(g)), (K + 2) * E32 * (aw @ np.abs(b) + np.abs(bi))
