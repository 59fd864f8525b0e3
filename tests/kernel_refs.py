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
