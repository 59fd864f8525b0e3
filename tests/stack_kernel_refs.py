"""Float64 statements of what the small kernels of the pre-norm stacks compute (decoder128.hip, mbert.hip, gemma.hip), the bounds a
float32 / bf16 kernel must meet against them, float32 emulations in the kernels' summation order, and the mutants the bounds must see.
Plain numpy, written from the mathematics; nothing here goes through the library or the HF-based *_ref.py files.

THE BOUNDS ARE DERIVED, in the manner of tests/kernel_refs.py. U = 2^-8 (bf16), E = 2^-24 (float32) are the unit round-offs.

Summation trees. A float32 sum whose longest chain of additions has `tree` links is off by at most tree E sum |terms| (every addition
bounded on its own). The kernels sum a row of H features
    one wave per row   4 NJ products per lane (NJ = ceil(H / 256) float4 per lane), six butterfly steps:     tree_wave = 4 NJ + 6
    one block per row  NJ terms per thread, six butterfly steps, the four wave partials:                       tree_block = NJ + 10
A bf16 store of a float32 value v within d of the wanted value: |bf16(v) - want| <= U |v| + d <= U |want| + (1 + U) d.

RMSNorm  out = x rs w, rs = 1 / sqrt(mean x^2 + eps). The squares are rounded once each and summed (all terms positive: the sum is
    off by (tree + 1) E relative), / H and + eps round once each, rsqrtf is 1 ulp = 2 E: rs is off by (0.5 (tree + 3) + 2) E relative;
    the two products add 2 E:            d = c_rms E |out|,  c_rms = 0.5 (tree + 3) + 4
    a perturbation dx of the row moves it by at most |w| rs (dx + |xh| mean(|xh| dx)), xh = x rs  (d rs = -rs^3 mean(x dx)).
LayerNorm (weight only)  out = w (x - mu) rstd, two passes. kernel_refs.layernorm_bound with the summation tree in place of n:
    |d mu| <= tree E mean |x|  ->  |w| rstd tree E mean |x|;  the centred squares, / H, + eps, rsqrtf, and the three operations of
    (x - mu) rstd w:  (0.5 (tree + 3) + 5) E |out|.   Both ride on rstd |x|: a row of |mean| / std = r is bounded r times worse.
L2 tail  out = y sc, sc = 1 / max(|y|, 1e-12). With dy on y: sc (dy + |yh| sum(|yh| dy)), yh = y / |y|, plus the float32 work
    (sum of squares (tree_block + 1) E relative, half of it after the root; root, division, product): (0.5 (tree_block + 1) + 3) E |out|.
    Under the floor sc is the constant 1e12 (rounded once): sc dy + 2 E |out|.
Pooling  mean over n tokens of y_t: a wave adds its 16 tokens of a chunk in turn, the four wave partials and the chunk sums follow:
    tree_pool = 16 + 3 + chunks. The sum can cancel (the test's rows alternate in sign), so the bound rides on sum |y_t|:
    (sum_t d_t + tree_pool E sum_t |y_t|) / n, d_t the bound of y_t itself; 1 / n, the weight and their products add 3 E |out|.
RoPE  o0 = y0 cos - y1 sin, o1 = y1 cos + y0 sin on the float32 tables the launch is handed (taken as exact): two products and a sum,
    3 E (|y0 cos| + |y1 sin|); Qwen3: y = RMSNorm_head(x) (tree = 2 + 6: two products per lane) in front, c_rms E more, and q's scale 1 E.
Dense  out = sum_k W[n][k] x[k]: (tree_wave(K) + 1) E sum |W x|.
Exact (bit for bit): token_slot's lengths and mask, Qwen3's and Gemma's x32 at the embedding, every float32 add of the residual
stream, copies (v, normalise = 0 in k_gm_l2), 1 + w, zeros for rows of length 0, the sentinel wherever a kernel must not write.

An expectation is {output name: ("exact", array) | ("bound", want, bound)}; compare() holds raw kernel outputs, emulations and
mutants to it alike. bf16 outputs travel as uint16 bit patterns."""
import math

import numpy as np

try:
    from tests import kernel_refs as kr
    from tests import stack_kernel_cases as sc
except ImportError:
    import kernel_refs as kr
    import stack_kernel_cases as sc

U, E = kr.U, kr.E32
F = np.float32
ROPE_EPS = sc.ROPE_EPS
L2_FLOOR = 1e-12
POOL_CHUNK = 64


def tree_wave(H):
    return 4 * sc.nj(H) + 6


def tree_block(H):
    return sc.nj(H) + 10


def c_rms(tree):
    return 0.5 * (tree + 3) + 4.0


def store16(want, d):
    """bound of a bf16 store of a float32 value within d of `want`."""
    return U * np.abs(want) + (1.0 + U) * d


def bits32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- comparison ------------------------------------------------------------------------------------------------------------------------
def compare(exp, got, worst, case, need_all=True):
    """Hold `got` {name: raw array} to the expectation `exp`. Exact entries: bit for bit (returns the names that differ); bound entries
    go into `worst` (err / bound; a NaN is over any bound)."""
    bad = []
    for name, e in exp.items():
        if name not in got:
            assert not need_all, f"{case}: output {name} missing"
            continue
        g = np.asarray(got[name])
        if e[0] == "exact":
            w = np.asarray(e[1])
            same = g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize and np.array_equal(g.view(np.uint8), w.view(np.uint8))
            if not same:
                bad.append(name)
            continue
        _, want, bound = e
        if g.dtype == np.uint16:
            g = kr.bf16_value(g)
        g = g.reshape(want.shape)
        n = want.shape[-1] if want.ndim > 1 else want.size
        worst.add(g.reshape(-1, n), want.reshape(-1, n), bound.reshape(-1, n), f"{case}:{name}")
    return bad


def flagged(exp, mutant):
    """True when the mutant's expectation, taken as a kernel's output, misses `exp`: a bit mismatch, a NaN or err / bound > 1."""
    got = {name: m[1] for name, m in mutant.items()}
    w = kr.Worst()
    bad = compare(exp, got, w, "mutant", need_all=False)
    return bool(bad) or w.ratio > 1.0


# ---- norms -----------------------------------------------------------------------------------------------------------------------------
def rms_ref(x, w, eps, mut=None):
    """(out, rs) of an RMSNorm over the last axis in float64. mut: eps_outside | mean_256nj | w_shift."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    H = x.shape[-1]
    n = 256 * sc.nj(H) if mut == "mean_256nj" else H
    ms = (x * x).sum(-1, keepdims=True) / n
    with np.errstate(divide="ignore"):
        rs = 1.0 / (np.sqrt(ms) + eps) if mut == "eps_outside" else 1.0 / np.sqrt(ms + eps)
    if mut == "w_shift":
        w = np.roll(w, -4)                   # a lane multiplies by its neighbour's four weights
    return x * rs * w, rs


def rms_pert(x, rs, w, dx):
    xh = np.abs(x * rs)
    return np.abs(w) * rs * (dx + xh * (xh * dx).mean(-1, keepdims=True))


def ln_ref(x, w, eps, mut=None):
    """(out, mu, rstd, rh) of a weight-only LayerNorm in float64. mut: eps_outside | mean_256nj | w_shift | onepass (the variance as
    E[x^2] - mean^2 in float32)."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    H = x.shape[-1]
    n = 256 * sc.nj(H) if mut == "mean_256nj" else H
    mu = x.sum(-1, keepdims=True) / n
    var = ((x - mu) ** 2).sum(-1, keepdims=True) / n
    if mut == "onepass":
        x32 = x.astype(F)
        mu32 = x32.sum(-1, keepdims=True, dtype=F) / F(H)
        var = np.maximum((x32 * x32).sum(-1, keepdims=True, dtype=F) / F(H) - mu32 * mu32, F(0)).astype(np.float64)
        mu = mu32.astype(np.float64)
    with np.errstate(divide="ignore"):
        rstd = 1.0 / (np.sqrt(var) + eps) if mut == "eps_outside" else 1.0 / np.sqrt(var + eps)
    if mut == "w_shift":
        w = np.roll(w, -4)
    rh = (x - mu) * rstd
    return w * rh, mu, rstd, rh


def ln_bound(x, w, out, rstd, tree):
    return np.abs(w) * rstd * tree * E * np.abs(x).mean(-1, keepdims=True) + (0.5 * (tree + 3) + 5.0) * E * np.abs(out)


def l2_ref(y, dy, tree, normalise=1, mut=None):
    """(out, bound) of the L2 tail over the last axis of y (float64) known to within dy. mut: no_floor."""
    nrm = np.sqrt((y * y).sum(-1, keepdims=True))
    if not normalise:
        return y, dy + 0.0 * y
    with np.errstate(divide="ignore", invalid="ignore"):
        if mut == "no_floor":
            return y / nrm, None
        s = 1.0 / np.maximum(nrm, L2_FLOOR)
        out = y * s
        yh = np.where(nrm > 0, np.abs(y) / np.where(nrm > 0, nrm, 1.0), 0.0)
    free = s * (dy + yh * (yh * dy).sum(-1, keepdims=True)) + (0.5 * (tree + 1) + 3.0) * E * np.abs(out)
    floor = s * dy + 2.0 * E * np.abs(out)
    return out, np.where(nrm >= L2_FLOOR, free, floor)


# ---- float32 emulation pieces --------------------------------------------------------------------------------------------------------
_XOR = [np.arange(64) ^ off for off in (32, 16, 8, 4, 2, 1)]


def wave_sum32(v):
    """stack.h wave_sum over the last axis (64 lanes), in its order; every lane's result (all equal up to the order of each add)."""
    v = np.asarray(v, F)
    for ix in _XOR:
        v = v + v[..., ix]
    return v


def _lanes(x, H):
    """[..., H] -> [..., NJ, 64, 4] as a wave holds a row: feature lane * 4 + j * 256 + e; zeros past H."""
    n = sc.nj(H) * 256
    xp = np.zeros(x.shape[:-1] + (n,), F)
    xp[..., :H] = x
    return xp.reshape(x.shape[:-1] + (n // 256, 64, 4))


def _sumsq_wave(x, H, paired):
    l = _lanes(x, H)
    sq = l * l
    t = (sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3]) if paired else ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]
    ss = np.zeros(t.shape[:-2] + (64,), F)
    for j in range(t.shape[-2]):
        ss = ss + t[..., j, :]
    return wave_sum32(ss)[..., :1]


def _rsqrt32(v):
    return (F(1) / np.sqrt(np.asarray(v, F))).astype(F)


def emu_rms(x, w, eps, paired):
    """RMSNorm of float32 rows by one wave per row (k_dec_*: the four squares left to right; k_gm_*: in pairs)."""
    x = np.asarray(x, F)
    H = x.shape[-1]
    rs = _rsqrt32(_sumsq_wave(x, H, paired) / F(H) + F(eps))
    return x * rs * np.asarray(w, F)


def emu_ln_stats(x, eps):
    """mb_row_stats: (mean, rstd) of float32 rows by one wave per row."""
    x = np.asarray(x, F)
    H = x.shape[-1]
    l = _lanes(x, H)
    t = (l[..., 0] + l[..., 1]) + (l[..., 2] + l[..., 3])
    s = np.zeros(t.shape[:-2] + (64,), F)
    for j in range(t.shape[-2]):
        s = s + t[..., j, :]
    mean = wave_sum32(s)[..., :1] / F(H)
    valid = _lanes(np.ones_like(x), H)
    c = (l - mean[..., None, None]) * valid
    sq = c * c
    t = (sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3])
    q = np.zeros(t.shape[:-2] + (64,), F)
    for j in range(t.shape[-2]):
        q = q + t[..., j, :]
    return mean, _rsqrt32(wave_sum32(q)[..., :1] / F(H) + F(eps))


def emu_ln(x, w, eps):
    mean, rstd = emu_ln_stats(x, eps)
    return (np.asarray(x, F) - mean) * rstd * np.asarray(w, F)


def _block_sum(v):
    """Sum over the last axis by a 256-thread block: thread tid takes features tid + 256 j in turn, wave_sum per wave, the four wave
    partials in wave order."""
    v = np.asarray(v, F)
    D = v.shape[-1]
    n = -(-D // 256) * 256
    vp = np.zeros(v.shape[:-1] + (n,), F)
    vp[..., :D] = v
    vp = vp.reshape(v.shape[:-1] + (n // 256, 4, 64))
    s = np.zeros(vp.shape[:-3] + (4, 64), F)
    for j in range(vp.shape[-3]):
        s = s + vp[..., j, :, :]
    r = wave_sum32(s)[..., 0]
    return (((r[..., 0] + r[..., 1]) + r[..., 2]) + r[..., 3])[..., None]


def emu_l2(y, normalise):
    y = np.asarray(y, F)
    if not normalise:
        return y * F(1)
    return y * (F(1) / np.maximum(np.sqrt(_block_sum(y * y)), F(L2_FLOOR)))


def emu_pool_sum(y, n):
    """Chunk sums of the first n token rows y [n][H] (float32) in pool_part's order, then added in chunk order (stage 2)."""
    H = y.shape[-1]
    tot = np.zeros(H, F)
    for c0 in range(0, n, POOL_CHUNK):
        blk = np.zeros((POOL_CHUNK, H), F)
        blk[:min(n, c0 + POOL_CHUNK) - c0] = y[c0:min(n, c0 + POOL_CHUNK)]
        blk = blk.reshape(16, 4, H)
        a = np.zeros((4, H), F)
        for i in range(16):
            a = a + blk[i]
        tot = tot + (((a[0] + a[1]) + a[2]) + a[3])
    return tot


# ---- embedding kernels -------------------------------------------------------------------------------------------------------------------
def token_slots(c, inp, mut=None):
    """(ids [B][S] as the table is read, lens_out [B], mask [B][S]). mut: stray_id (a stray id read as it is: here some other row than 0)
    | len_unclamped."""
    B, S, V = c["B"], c["S"], c["vocab"]
    raw = inp["lens"][:, 0].astype(np.int64)
    lens = raw if mut == "len_unclamped" else np.clip(raw, 0, S)
    sq = np.arange(S)[None, :]
    inside = sq < lens[:, None]
    ids = np.where(inside, inp["ids"][:, :S].astype(np.int64), 0)
    stray = (ids < 0) | (ids >= V)
    ids = np.where(stray, np.abs(ids) % (V - 1) + 1 if mut == "stray_id" else 0, ids)
    return ids, lens.astype(np.int32), inside.astype(np.int32)


def embed_expect(c, inp, mut=None):
    B, S, H, fam = c["B"], c["S"], c["H"], c["fam"]
    ids, lens, mask = token_slots(c, inp, mut)
    rows = kr.bf16_value(inp["emb"])[ids.reshape(-1)]                                  # [B S][H] float32
    out = {"lens": ("exact", lens), "x32_guard": ("exact", np.full((sc.GUARD, H), sc.SENT, F)),
           "h16_guard": ("exact", kr.bf16_bits(np.full((sc.GUARD, H), sc.SENT, F)))}
    tree = tree_wave(H)
    w = inp["w"].astype(np.float64)
    if fam == "mb":
        out["mask"] = ("exact", mask.reshape(-1))
        want, mu, rstd, rh = ln_ref(rows, w, c["eps"], mut)
        d = ln_bound(rows.astype(np.float64), w, want, rstd, tree)
        out["x32"] = ("bound", want, d)
        out["h16"] = ("bound", want, store16(want, d))
        return out
    x32 = rows if fam == "dec" else rows * np.sqrt(F(H))                               # one float32 multiply by float32 sqrt(H)
    out["x32"] = ("exact", x32.astype(F))
    want, _ = rms_ref(x32, w, c["eps"], mut)
    out["h16"] = ("bound", want, store16(want, c_rms(tree) * E * np.abs(want)))
    return out


def embed_emulate(c, inp):
    H, fam = c["H"], c["fam"]
    ids, lens, mask = token_slots(c, inp)
    rows = kr.bf16_value(inp["emb"])[ids.reshape(-1)]
    if fam == "mb":
        x = emu_ln(rows, inp["w"], c["eps"])
        return {"lens": lens, "mask": mask.reshape(-1), "x32": x, "h16": kr.bf16_bits(x)}
    x32 = rows if fam == "dec" else rows * np.sqrt(F(H))
    return {"lens": lens, "x32": x32.astype(F), "h16": kr.bf16_bits(emu_rms(x32, inp["w"], c["eps"], paired=fam == "gm"))}


# ---- add + norm kernels ------------------------------------------------------------------------------------------------------------------
def addnorm_expect(c, inp, mut=None):
    """Qwen3 / ModernBERT: x32 <- float32(x + y) bit for bit, h16 the norm of THAT row. Gemma: x32 <- x + RMSNorm(y; w_post) at its
    bound, then RMSNorm(x32; w) of the float64 row with that bound carried through as a perturbation; `out32`: float32 rows."""
    T, H, fam, form, eps = c["T"], c["H"], c["fam"], c["form"], c["eps"]
    tree = tree_wave(H)
    sent32, sent16 = np.full((sc.GUARD, H), sc.SENT, F), kr.bf16_bits(np.full((sc.GUARD, H), sc.SENT, F))
    out = {"x32_guard": ("exact", sent32)}
    w = inp["w"].astype(np.float64)
    if fam != "gm":
        r = inp["x"] + inp["y"]                                                        # float32
        out["x32"] = ("exact", r)
        if form == "add":
            out["h16"] = ("exact", kr.bf16_bits(np.full((T + sc.GUARD, H), sc.SENT, F)))
            return out
        out["h16_guard"] = ("exact", sent16)
        if fam == "dec":
            want, _ = rms_ref(r, w, eps, mut)
            d = c_rms(tree) * E * np.abs(want)
        else:
            want, mu, rstd, rh = ln_ref(r, w, eps, mut)
            d = ln_bound(r.astype(np.float64), w, want, rstd, tree)
        out["h16"] = ("bound", want, store16(want, d))
        return out
    wp = inp["w_post"].astype(np.float64)
    n1, _ = rms_ref(inp["y"], wp, eps, mut)
    xn = inp["x"].astype(np.float64) + n1
    dx = c_rms(tree) * E * np.abs(n1) + E * np.abs(xn)
    out["x32"] = ("bound", xn, dx)
    want, rs = rms_ref(xn, w, eps, mut)
    d = rms_pert(xn, rs, w, dx) + c_rms(tree) * E * np.abs(want)
    if form == "out32":
        out["y32"] = ("bound", want, d)
        out["y32_guard"] = ("exact", sent32)
    else:
        out["h16"] = ("bound", want, store16(want, d))
        out["h16_guard"] = ("exact", sent16)
    return out


def addnorm_emulate(c, inp):
    fam, form, eps = c["fam"], c["form"], c["eps"]
    if fam != "gm":
        r = inp["x"] + inp["y"]
        if form == "add":
            return {"x32": r}
        h = emu_rms(r, inp["w"], eps, paired=False) if fam == "dec" else emu_ln(r, inp["w"], eps)
        return {"x32": r, "h16": kr.bf16_bits(h)}
    xn = inp["x"] + emu_rms(inp["y"], inp["w_post"], eps, paired=True)
    o = emu_rms(xn, inp["w"], eps, paired=True)
    return {"x32": xn, "y32": o} if form == "out32" else {"x32": xn, "h16": kr.bf16_bits(o)}


# ---- RoPE ------------------------------------------------------------------------------------------------------------------------------------
def _rotate(y, cos, sin, hd, mut=None):
    """y [..., hd] at tables broadcastable to [..., hd / 2] -> (rotated, |y0 cos| + |y1 sin| magnitudes). mut: sign | partner."""
    h = hd // 2
    y0, y1 = y[..., :h], y[..., h:]
    if mut == "partner":                    # the partner at d + hd / 4 instead of d + hd / 2
        y1 = y[..., hd // 4:hd // 4 + h]
    sg = -1.0 if mut == "sign" else 1.0
    want = np.concatenate([y0 * cos - sg * y1 * sin, y1 * cos + sg * y0 * sin], -1)
    mag = np.concatenate([np.abs(y0 * cos) + np.abs(y1 * sin), np.abs(y1 * cos) + np.abs(y0 * sin)], -1)
    return want, mag


def _positions(c, mut):
    B, S = c["B"], c["S"]
    t = np.arange(B * S)
    return (t if mut == "pos_t" else t % S).reshape(B, S)


def rope_expect(c, inp, rc, rs, mut=None):
    """rc / rs: the float32 tables the launch is handed, [>= S][hd / 2] ([>= B S] for the pos_t mutant)."""
    B, S, hd = c["B"], c["S"], c["hd"]
    pos = _positions(c, mut)
    cos, sin = np.asarray(rc, np.float64)[pos], np.asarray(rs, np.float64)[pos]        # [B][S][hd / 2]
    guard = ("exact", kr.bf16_bits(np.full((1, hd), sc.SENT, F)))
    if c["fam"] == "mb":
        H = c["H"]
        out = {}
        for name in ("q", "k"):
            x = kr.bf16_value(inp[name]).astype(np.float64).reshape(B, S, H // hd, hd)
            want, mag = _rotate(x, cos[:, :, None, :], sin[:, :, None, :], hd, mut)
            out[name] = ("bound", want.reshape(B * S, H), None if mag is None else store16(want, 3.0 * E * mag).reshape(B * S, H))
            out[name + "_guard"] = ("exact", kr.bf16_bits(np.full((sc.GUARD, H), sc.SENT, F)))
        return out
    nq, nkv = c["nq"], c["nkv"]
    x = kr.bf16_value(inp["qkv"]).astype(np.float64).reshape(B, S, nq + 2 * nkv, hd)
    out = {}
    crope = c_rms(2 + 6) + 3.0
    for name, lo, n, wn, scl in (("q", 0, nq, inp["qn"], c["qscale"]), ("k", nq, nkv, inp["kn"], 1.0)):
        if mut == "scale_k":
            scl = 1.0 if name == "q" else c["qscale"]
        y, _ = rms_ref(x[:, :, lo:lo + n], wn, ROPE_EPS)
        want, mag = _rotate(y, cos[:, :, None, :], sin[:, :, None, :], hd, mut)
        want = want * scl
        bound = None if mag is None else store16(want, (crope + (1.0 if name == "q" else 0.0)) * E * mag * scl)
        out[name] = ("bound", want.transpose(0, 2, 1, 3), None if bound is None else bound.transpose(0, 2, 1, 3))
        out[name + "_guard"] = guard
    out["v"] = ("exact", np.ascontiguousarray(inp["qkv"].reshape(B, S, nq + 2 * nkv, hd)[:, :, nq + nkv:].transpose(0, 2, 1, 3)))
    out["v_guard"] = guard
    return out


def rope_emulate(c, inp, rc, rs):
    B, S, hd = c["B"], c["S"], c["hd"]
    pos = _positions(c, None)
    cos, sin = np.asarray(rc, F)[pos][:, :, None, :], np.asarray(rs, F)[pos][:, :, None, :]
    h = hd // 2
    if c["fam"] == "mb":
        out = {}
        for name in ("q", "k"):
            x = kr.bf16_value(inp[name]).reshape(B, S, c["H"] // hd, hd)
            x0, x1 = x[..., :h], x[..., h:]
            out[name] = kr.bf16_bits(np.concatenate([x0 * cos - x1 * sin, x1 * cos + x0 * sin], -1)).reshape(B * S, c["H"])
        return out
    nq, nkv = c["nq"], c["nkv"]
    x = kr.bf16_value(inp["qkv"]).reshape(B, S, nq + 2 * nkv, hd)
    out = {}
    for name, lo, n, wn, scl in (("q", 0, nq, inp["qn"], F(c["qscale"])), ("k", nq, nkv, inp["kn"], None)):
        xs = x[:, :, lo:lo + n]
        x0, x1 = xs[..., :h], xs[..., h:]
        rsq = _rsqrt32(wave_sum32(x0 * x0 + x1 * x1)[..., :1] * F(1.0 / hd) + F(ROPE_EPS))
        y0, y1 = x0 * rsq * wn[:h], x1 * rsq * wn[h:]
        o0, o1 = y0 * cos - y1 * sin, y1 * cos + y0 * sin
        if scl is not None:
            o0, o1 = o0 * scl, o1 * scl
        out[name] = kr.bf16_bits(np.concatenate([o0, o1], -1).transpose(0, 2, 1, 3))
    out["v"] = np.ascontiguousarray(inp["qkv"].reshape(B, S, nq + 2 * nkv, hd)[:, :, nq + nkv:].transpose(0, 2, 1, 3))
    return out


# ---- pooling -------------------------------------------------------------------------------------------------------------------------------------
def pool_expect(c, inp, mode, mut=None):
    """One pooling launch (sc.pool_modes) -> {"out": ...}: per batch row either exact zeros (length 0) or (want, bound) -- stacked
    into one bound entry whose zero rows have bound 0. mut: n_plus_1 | n_ceil64 | div_S | cls_1 | last_len | no_floor | onepass |
    eps_outside | mean_256nj | w_shift."""
    name, pooling, normalise = mode
    fam, S, H, eps = c["fam"], c["S"], c["H"], c["eps"]
    x, w = inp["x"], inp["w"].astype(np.float64)
    B = x.shape[0]
    want, bound = np.zeros((B, H)), np.zeros((B, H))
    norm_mut = mut if mut in ("onepass", "eps_outside", "mean_256nj", "w_shift") else None
    l2_mut = mut if mut == "no_floor" else None
    for b, n in enumerate(int(v) for v in inp["lens"]):
        if n <= 0:
            continue
        if fam == "dec":
            t = n if mut == "last_len" else n - 1
            row = x[b, min(t, S - 1)] if t < S else np.full(H, np.nan, F)
            y, _ = rms_ref(row, w, eps, norm_mut)
            dy = c_rms(tree_block(H)) * E * np.abs(y)
        else:
            cnt = 1 if pooling == 1 else n
            first = 1 if (mut == "cls_1" and pooling == 1) else 0
            m = cnt + 1 if mut == "n_plus_1" else (-(-cnt // 64) * 64 if mut == "n_ceil64" else cnt)
            rows = np.full((m, H), np.nan)
            avail = x[b, first:min(first + m, S)].astype(np.float64)
            rows[:avail.shape[0]] = avail
            used = -(-cnt // POOL_CHUNK)
            if fam == "mb":
                yt, mu, rstd, rh = ln_ref(rows, np.ones(H), eps, norm_mut)
                dt = ln_bound(rows, np.ones(H), yt, rstd, tree_wave(H))
                wv = np.roll(w, -4) if norm_mut == "w_shift" else w
            else:
                yt, dt, wv = rows, np.zeros_like(rows), np.ones(H)
            div = S if mut == "div_S" else cnt
            y = yt.sum(0) * wv / div
            dy = np.abs(wv) / cnt * (dt.sum(0) + (16 + 3 + used) * E * np.abs(yt).sum(0)) + 3.0 * E * np.abs(y)
        if normalise is None:
            want[b], bound[b] = y, dy
        else:
            o, bd = l2_ref(y, dy, tree_block(H), normalise, l2_mut)
            want[b], bound[b] = o, (0.0 if bd is None else bd)
    return {"out": ("bound", want, bound), "out_guard": ("exact", np.full((1, H), sc.SENT, F))}


def pool_emulate(c, inp, mode):
    name, pooling, normalise = mode
    fam, S, H, eps = c["fam"], c["S"], c["H"], c["eps"]
    x, w = inp["x"], inp["w"].astype(F)
    out = np.zeros((x.shape[0], H), F)
    for b, n in enumerate(int(v) for v in inp["lens"]):
        if n <= 0:
            continue
        if fam == "dec":
            row = x[b, n - 1]
            rs = _rsqrt32(_block_sum(row * row) / F(H) + F(eps))
            y = row * rs * w
        else:
            cnt = 1 if pooling == 1 else n
            rows = x[b, :cnt]
            if fam == "mb":
                mean, rstd = emu_ln_stats(rows, eps)
                rows = (rows - mean) * rstd
            y = emu_pool_sum(rows, cnt)
            y = y * w * (F(1) / F(cnt)) if fam == "mb" else y * (F(1) / F(cnt))
        out[b] = y if normalise is None else emu_l2(y, normalise)
    return {"out": out}


# ---- dense, L2, fold -----------------------------------------------------------------------------------------------------------------------------
def dense_expect(c, inp, mut=None):
    x, w = inp["x"].astype(np.float64), inp["w"].astype(np.float64)
    N, K = c["N"], c["K"]
    if mut == "stride_N":                   # row n read at W + n N
        ix = (np.arange(N)[:, None] * N + np.arange(K)[None, :]) % (N * K)
        w = w.reshape(-1)[ix]
    want = x @ w.T
    return {"out": ("bound", want, (tree_wave(K) + 1) * E * (np.abs(x) @ np.abs(w).T)), "out_guard": ("exact", np.full((1, 8), sc.SENT, F))}


def dense_emulate(c, inp):
    x, w = inp["x"], inp["w"]
    K = c["K"]
    p = _lanes(w, K)[None] * _lanes(x, K)[:, None]                                     # [B][N][NJ][64][4]
    t = (p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])
    s = np.zeros(t.shape[:-2] + (64,), F)
    for j in range(t.shape[-2]):
        s = s + t[..., j, :]
    return {"out": wave_sum32(s)[..., 0]}


def l2_expect(c, inp, mut=None):
    x = inp["x"]
    if not c["normalise"]:
        return {"out": ("exact", x)}
    want, bound = l2_ref(x.astype(np.float64), 0.0, tree_block(c["D"]), 1, mut)
    return {"out": ("bound", want, np.zeros_like(want) if bound is None else bound)}


def l2_emulate(c, inp):
    return {"out": emu_l2(inp["x"], c["normalise"])}


def fold_expect(inp):
    return {"out": ("exact", F(1) + inp["w"]), "out_guard": ("exact", np.full(8, sc.SENT, F))}


# ---- k_gemm MODE 3 -------------------------------------------------------------------------------------------------------------------------------
def gemm3_expect(c, inp, drop_k=None):
    y, y_abs = kr.gemm_ref(kr.bf16_value(inp["x"]), kr.bf16_value(inp["w"]), inp["bias"], drop_k=drop_k)
    return {"out": ("bound",) + kr.epi_bf16(y, y_abs, c["K"])}
