"""Float64 statement of what k_ll_rope (decoder128.hip) computes, the bound a float32 / bf16 kernel must meet against it, a float32 emulation in
the kernel's own order and the mutants the bound must see; in the manner of tests/stack_kernel_refs.py, whose RoPE bound this is without
the RMSNorm in front. Plain numpy, written from the mathematics.

    q'[d]      = (q[d] cos_p[d] - q[d + 64] sin_p[d]) s        d < 64, p = the token's position in its sequence, s = log2(e) / sqrt(128)
    q'[d + 64] = (q[d + 64] cos_p[d] + q[d] sin_p[d]) s
    k' likewise without s; v' = v. Layouts: q [B][nq][S][128], k / v [B][nkv][S][128].

Bound, with U = 2^-8 (bf16) and E = 2^-24 (float32): the inputs are bf16 (exact), the tables float32 as handed over (taken as exact).
Two products and their sum round once each: each product is off by E of itself, the sum by E of its result <= E (|x0 cos| + |x1 sin|)
(1 + E), together under 3 E mag, mag = |x0 cos| + |x1 sin|; q's scale is a float32 constant (the exact s rounded once: E s) and its
product one more rounding, 2 E |q'| <= 2 E mag s:
    d = (3 + 2 [q]) E mag s;   the bf16 store of a float32 value within d of the wanted one: U |want| + (1 + U) d   (store16).
v is a copy: bit for bit. Rows behind the outputs keep the sentinel.

Mean pooling with the final RMSNorm (k_ll_pool_part / k_ll_pool_fin), derived as tests/stack_kernel_refs.py derives the pools':
    y_t = x_t rs_t, rs_t = 1 / sqrt(mean x_t^2 + eps) per token t < n (the norm BEFORE the mean);  out = w (sum_t y_t) / n;  then the L2 tail.
    y_t: one wave per token sums 4 H / 256 squares per lane and six butterfly steps (tree = 4 H / 256 + 6); / H, + eps and rsqrtf as for
         any RMSNorm, one product: d_t = (0.5 (tree + 3) + 3) E |y_t|.
    sum: a wave adds its 16 tokens of a chunk in turn, the four wave partials and the chunk sums follow: tree_pool = 16 + 3 + chunks, on
         sum_t |y_t| (the rows alternate in sign, the sum cancels);  the weight, 1 / n and their products: 3 E |out|.
    L2:  stack_kernel_refs.l2_ref with the block tree H / 256 + 10 (a thread's H / 256 terms, six butterfly steps, four wave partials).
A row of length 0 is exact zeros; token rows at or past a length are NaN in the input and must not be read."""
import numpy as np

try:
    from tests import kernel_refs as kr
    from tests import llama_kernel_cases as lc
except ImportError:
    import kernel_refs as kr
    import llama_kernel_cases as lc

U, E = kr.U, kr.E32
F = np.float32
HD = lc.HD


def store16(want, d):
    return U * np.abs(want) + (1.0 + U) * d


def _split(c, inp):
    B, S, nq, nkv = c["B"], c["S"], c["nq"], c["nkv"]
    return inp["qkv"].reshape(B, S, nq + 2 * nkv, HD)


def rope_expect(c, inp, mut=None):
    """{q, k: ("bound", want, bound) in the output layout, v: ("exact", bits)}. mut: swap (cos / sin exchanged) | sign (rotate_half's
    sign) | pos (position off by one) | noscale (q scale missing)."""
    B, S, nq, nkv = c["B"], c["S"], c["nq"], c["nkv"]
    bits = _split(c, inp)
    x = kr.bf16_value(bits).astype(np.float64)
    pos = np.arange(S) + (1 if mut == "pos" else 0)
    cos, sin = inp["rc"].astype(np.float64)[pos][None, :, None, :], inp["rs"].astype(np.float64)[pos][None, :, None, :]
    if mut == "swap":
        cos, sin = sin, cos
    sg = -1.0 if mut == "sign" else 1.0
    out = {}
    for name, lo, n, scl in (("q", 0, nq, 1.0 if mut == "noscale" else c["qscale"]), ("k", nq, nkv, 1.0)):
        x0, x1 = x[:, :, lo:lo + n, :64], x[:, :, lo:lo + n, 64:]
        want = np.concatenate([x0 * cos - sg * x1 * sin, x1 * cos + sg * x0 * sin], -1) * scl
        mag = np.concatenate([np.abs(x0 * cos) + np.abs(x1 * sin), np.abs(x1 * cos) + np.abs(x0 * sin)], -1) * scl
        bound = store16(want, (3.0 + 2.0 * (name == "q")) * E * mag)
        out[name] = ("bound", np.ascontiguousarray(want.transpose(0, 2, 1, 3)), np.ascontiguousarray(bound.transpose(0, 2, 1, 3)))
    out["v"] = ("exact", np.ascontiguousarray(bits[:, :, nq + nkv:].transpose(0, 2, 1, 3)))
    return out


def rope_emulate(c, inp):
    """The kernel's float32 operations in its order; bf16 bits in the output layouts."""
    nq, nkv = c["nq"], c["nkv"]
    bits = _split(c, inp)
    x = kr.bf16_value(bits)
    cos, sin = inp["rc"][:c["S"]][None, :, None, :], inp["rs"][:c["S"]][None, :, None, :]
    out = {}
    for name, lo, n, scl in (("q", 0, nq, F(c["qscale"])), ("k", nq, nkv, None)):
        x0, x1 = x[:, :, lo:lo + n, :64], x[:, :, lo:lo + n, 64:]
        o0, o1 = x0 * cos - x1 * sin, x1 * cos + x0 * sin
        if scl is not None:
            o0, o1 = o0 * scl, o1 * scl
        out[name] = kr.bf16_bits(np.concatenate([o0, o1], -1).astype(F).transpose(0, 2, 1, 3))
    out["v"] = np.ascontiguousarray(bits[:, :, nq + nkv:].transpose(0, 2, 1, 3))
    return out


def compare(exp, got, worst, case):
    """Hold `got` {name: raw bits} to the expectation; returns the names of the exact outputs that differ."""
    bad = []
    for name, e in exp.items():
        g = np.asarray(got[name])
        if e[0] == "exact":
            if g.shape != e[1].shape or not np.array_equal(g, e[1]):
                bad.append(name)
            continue
        _, want, bound = e
        worst.add(kr.bf16_value(g).reshape(-1, HD), want.reshape(-1, HD), bound.reshape(-1, HD), f"{case}:{name}")
    return bad


def flagged(exp, mutant):
    """True when the mutant's wanted values, rounded to bf16 and taken as a kernel's output, miss `exp`."""
    got = {name: (kr.bf16_bits(m[1].astype(F)) if m[0] == "bound" else m[1]) for name, m in mutant.items()}
    w = kr.Worst()
    return bool(compare(exp, got, w, "mutant")) or w.ratio > 1.0


# ---- mean pooling with the final RMSNorm -------------------------------------------------------------------------------------------------
def pool_expect(c, inp, mut=None):
    """(want, bound) [B][H]. mut: norm_after (the norm of the mean instead of the mean of the norms) | div_S (the mean over S)."""
    from tests import stack_kernel_refs as sr
    H, S, eps = c["H"], c["S"], c["eps"]
    w = inp["w"].astype(np.float64)
    want, bound = np.zeros((c["B"], H)), np.zeros((c["B"], H))
    tree = 4 * (-(-H // 256)) + 6
    for b, n in enumerate(int(v) for v in inp["lens"]):
        if n <= 0:
            continue
        x = inp["x"][b, :n].astype(np.float64)
        if mut == "norm_after":
            m = x.mean(0)
            y, dy = m / np.sqrt((m * m).mean() + eps) * w, 0.0 * m
        else:
            yt = x / np.sqrt((x * x).mean(-1, keepdims=True) + eps)
            dt = (0.5 * (tree + 3) + 3.0) * E * np.abs(yt)
            used = -(-n // 64)
            y = yt.sum(0) * w / (S if mut == "div_S" else n)
            dy = np.abs(w) / n * (dt.sum(0) + (16 + 3 + used) * E * np.abs(yt).sum(0)) + 3.0 * E * np.abs(y)
        want[b], bound[b] = sr.l2_ref(y, dy, -(-H // 256) + 10, c["normalise"])
    return want, bound


def pool_emulate(c, inp):
    """The kernels' float32 operations in their order (stack_kernel_refs' wave, chunk and block sums)."""
    from tests import stack_kernel_refs as sr
    H = c["H"]
    out = np.zeros((c["B"], H), F)
    w = inp["w"].astype(F)
    for b, n in enumerate(int(v) for v in inp["lens"]):
        if n <= 0:
            continue
        x = inp["x"][b, :n]
        rs = sr._rsqrt32(sr._sumsq_wave(x, H, False) / F(H) + F(c["eps"]))
        y = sr.emu_pool_sum((x * rs).astype(F), n) * w * (F(1) / F(n))
        out[b] = sr.emu_l2(y, c["normalise"])
    return out
