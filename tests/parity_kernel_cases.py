"""The cases of the parity-mode kernel tests (tests/test_parity_kernels_gpu.py), their inputs and the checks of their outputs. The GPU
worker (tests/parity_kernel_worker.py), the float64 references in the parent and the CPU proofs (tests/test_parity_kernel_refs_cpu.py:
emulations inside, mutants outside) call the same builders and the same checks, so they see the same numbers and the same bar.

Inputs carry full float32 mantissas (normal deviates cast to float32): the lo half of every split is non-zero nearly everywhere.
Outputs are lists of named raw arrays, as the worker stores them; a check takes such a dict whoever made it.

GEMM input classes: `random` (x ~ N(0, 1), W ~ N(0, 0.05), bias ~ N(0, 0.1)); `gelu` (the same with the pre-activation spread over
[-8, 8] by the bias: the table's end pieces and erf's tails); `cancel` (columns in pairs whose hi halves are equal and opposite in x and
equal in W while the lo halves differ: hi.hi sums to exactly zero, the result is made of lo.hi and hi.lo terms alone; K <= 64, where
those terms stand clear of the accumulation bound); `onehot` (one non-zero per X row at k = (3 t + 1) % K and per W row at k = (5 n + 2) % K:
every output is the bias plus at most a single product, so a permutation of k, of rows or of tiles shows at a bound of a few e).
Attention: q, k, v ~ N(0, 1) with the logit spread alternating between flat and peaked from one (sequence, head) to the next, plus spike
probes (a key whose logit dominates its query's row and whose v row is distinctive) on the last visible key, the first key past it and
the key in front of the first visible one. The lengths of a case's sequences are taken in turn from kernel_cases.lengths_for(S); a batch of
12 holds them all, the smaller batches the issue asks for (B . heads in {1, 3, 8, 9, 24}) a rotating part of them."""
import math
import zlib

import numpy as np

try:
    from tests import kernel_cases as kc
    from tests import kernel_refs as kr
    from tests import parity_kernel_refs as pr
except ImportError:          # imported by the worker script, whose directory is tests/ itself
    import kernel_cases as kc
    import kernel_refs as kr
    import parity_kernel_refs as pr

F = np.float32
SENT = 12288.0               # prefilled where a kernel must not write
SENT16 = int(kr.bf16_bits(np.array([SENT], F))[0])
PAD_ROWS = 3                 # rows of the output allocation past T: must come back untouched


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _step16(h):
    """One bf16 step at the bf16 value h."""
    h = np.abs(np.asarray(h, np.float64))
    return 2.0 ** (np.floor(np.log2(np.where(h > 0, h, 1.0))) - 7)


# ---- launch_gemm_f32 / launch_gemm_x3 ----------------------------------------------------------------------------------------------------
def gemm_cases():
    """(T, N, K, epilogue, ldc / N, col0 / N, class). T = 1056 is nine token tiles (the second lap of the XCD order), K = 32 one K-step."""
    rows = [(1, 128, 32, 0, 1, 0, "random"), (31, 128, 64, 1, 1, 0, "gelu"), (128, 384, 384, 0, 3, 1, "random"), (129, 128, 384, 2, 1, 0, "random"),
            (129, 384, 64, 0, 3, 2, "onehot"), (1056, 384, 32, 0, 1, 0, "onehot"), (1056, 128, 384, 1, 1, 0, "gelu"), (1056, 384, 64, 2, 3, 0, "random"),
            (128, 128, 64, 2, 1, 0, "cancel"), (31, 384, 1536, 0, 3, 0, "random"), (129, 128, 32, 0, 1, 0, "cancel"), (128, 384, 64, 1, 1, 0, "gelu"),
            (1, 384, 384, 2, 3, 1, "onehot"), (31, 128, 32, 1, 1, 0, "gelu"), (129, 128, 1536, 2, 3, 2, "random"), (1056, 128, 64, 0, 3, 1, "cancel")]
    return [dict(T=T, N=N, K=K, epi=e, ldc=l * N, col0=c0 * N, cls=cls, name=f"g_T{T}_N{N}_K{K}_e{e}_ld{l}_c{c0}_{cls}") for T, N, K, e, l, c0, cls in rows]


def gemm_refused():
    """Shapes the launchers refuse: the error code, no launch."""
    return [dict(T=4, N=192, K=32), dict(T=4, N=128, K=48)]


def onehot_k(c):
    return (3 * np.arange(c["T"]) + 1) % c["K"], (5 * np.arange(c["N"]) + 2) % c["K"]


def gemm_inputs(c):
    """x [T][K] (exactly T rows, as the product allocates it), w [N][K], bias [N], res [T][ldc] (epilogue 2: in Y's layout), float32."""
    rng = _rng(c["name"])
    T, N, K, cls = c["T"], c["N"], c["K"], c["cls"]
    if cls == "cancel":
        x0 = rng.standard_normal((T, K // 2))
        w0 = rng.standard_normal((N, K // 2)) * 0.05
        xb, wb = kr.bf16_round(x0.astype(F)).astype(np.float64), kr.bf16_round(w0.astype(F)).astype(np.float64)
        x, w = np.empty((T, K)), np.empty((N, K))
        x[:, 0::2], x[:, 1::2] = x0, -xb + rng.uniform(-0.24, 0.24, xb.shape) * _step16(xb)
        w[:, 0::2], w[:, 1::2] = w0, wb + rng.uniform(-0.24, 0.24, wb.shape) * _step16(wb)
        x, w = x.astype(F), w.astype(F)
        bias = (1e-3 * rng.standard_normal(N)).astype(F)
    elif cls == "onehot":
        kx, kw = onehot_k(c)
        x, w = np.zeros((T, K), F), np.zeros((N, K), F)
        x[np.arange(T), kx] = (rng.standard_normal(T) + np.where(rng.random(T) < 0.5, 2.0, -2.0)).astype(F)
        w[np.arange(N), kw] = (rng.standard_normal(N) + np.where(rng.random(N) < 0.5, 2.0, -2.0)).astype(F)
        bias = (0.1 * rng.standard_normal(N)).astype(F)
    else:
        x = rng.standard_normal((T, K)).astype(F)
        w = (rng.standard_normal((N, K)) * 0.05).astype(F)
        bias = (0.1 * rng.standard_normal(N)).astype(F)
        if cls == "gelu":
            x, w = (x * F(0.25)).astype(F), (w * F(10.0 / math.sqrt(K))).astype(F)      # products of std 0.125 around ...
            bias = rng.permutation(np.linspace(-8.0, 8.0, N)).astype(F)       # ... pre-activations spread over [-8, 8]
    res = rng.standard_normal((T, c["ldc"])).astype(F) if c["epi"] == 2 else None
    return dict(x=x, w=w, bias=bias, res=res)


def gemm_res_block(c, inp):
    return None if inp["res"] is None else inp["res"][:, c["col0"]:c["col0"] + c["N"]]


def gemm_place(c, vals, col0=None):
    """An output allocation [T + PAD_ROWS][ldc] of sentinels with vals [T][N] at column col0 (default: the case's)."""
    col0 = c["col0"] if col0 is None else col0
    Y = np.full((c["T"] + PAD_ROWS, c["ldc"]), SENT, F)
    Y[:c["T"], col0:col0 + c["N"]] = vals
    return Y


def gemm_check(c, Y, want, bound, worst):
    """Y: the whole allocation as it came back. The block against (want, bound); returns the number of sentinels that were overwritten."""
    T, N, c0 = c["T"], c["N"], c["col0"]
    keep = np.ones(Y.shape, bool)
    keep[:T, c0:c0 + N] = False
    worst.add(Y[:T, c0:c0 + N], want, bound, c["name"], col0=c0)
    return int((Y[keep] != F(SENT)).sum())


# ---- launch_gemm_x3w (MODE 5 / 6) ----------------------------------------------------------------------------------------------------------
def x3w_cases(child="default"):
    """default: the launcher's own tile choice -- narrow at the small shapes, both sides of its threshold at K' = 64 (16 x 16 = 256 wide
    tiles at (4096, 4096); 15 x 17 = 255 at (3840, 4352): narrow), and 10 x 26 = 260 narrow tiles at (2560, 3328): a workgroup of the
    256-workgroup grid walks a second tile. wide: the same small shapes under AK_GEMM_BN=256 (N % 256 == 0 only)."""
    small = [(256, 128, 64, 0), (512, 384, 128, 0), (256, 512, 384, 384), (512, 512, 64, 512), (256, 1280, 64, 1152), (256, 512, 128, 448)]
    out = []
    for T, N, K1, nv in small:
        if child == "wide" and N % 256:
            continue
        for mode in (5, 6):
            if mode == 6 and nv not in (0, N):
                continue
            out.append(dict(T=T, N=N, K1=K1, nvalid=nv, mode=mode))
    if child == "default":
        out += [dict(T=4096, N=4096, K1=64, nvalid=0, mode=5), dict(T=3840, N=4352, K1=64, nvalid=0, mode=5),
                dict(T=4096, N=4096, K1=64, nvalid=0, mode=6), dict(T=2560, N=3328, K1=64, nvalid=0, mode=5)]
    for c in out:
        c.update(child=child, cls="gelu" if c["mode"] == 6 else "random", name=f"x3w_{child}_m{c['mode']}_T{c['T']}_N{c['N']}_K{c['K1']}_v{c['nvalid']}")
    return out


def x3w_selection(c):
    """launch_gemm_x3w's rule (gemm.hip), restated: (wide tile?, tiles, workgroups). The wide tile needs N % 256 == 0 and at least 256
    tiles of 256 x 256, or AK_GEMM_BN=256 with N % 256 == 0; at most 256 persistent workgroups."""
    wide = c["N"] % 256 == 0 and (c["T"] // 256) * (c["N"] // 256) >= 256
    if c["child"] == "wide" and c["N"] % 256 == 0:
        wide = True
    tiles = (c["T"] // 256) * (c["N"] // (256 if wide else 128))
    return wide, tiles, min(tiles, 256)


def x3w_nvalid(c):
    return c["nvalid"] if 0 < c["nvalid"] <= c["N"] else c["N"]


def x3w_inputs(c):
    """x2 [T][2 K'], w2 [N][2 K'] bf16 bits [hi | lo] of float32 operands, bias [N]."""
    g = gemm_inputs(dict(T=c["T"], N=c["N"], K=c["K1"], cls=c["cls"], epi=0, ldc=c["N"], name=c["name"]))
    return dict(x2=pr.split_rows(g["x"]), w2=pr.split_rows(g["w"]), bias=g["bias"])


def x3w_check(c, out, inp, worst):
    """MODE 5: out [T][N] float32, columns >= nvalid still the sentinel. MODE 6: out [T][2 N] bf16 bits: hi + lo against the table bound, |lo|
    within half a step of hi. Returns the number of structural violations."""
    y, dy = pr.gemm_x3w_pre(inp["x2"], inp["w2"], inp["bias"])
    N, nv = c["N"], x3w_nvalid(c)
    if c["mode"] == 5:
        worst.add(out[:, :nv], y[:, :nv], dy[:, :nv], c["name"])
        return int((out[:, nv:] != F(SENT)).sum())
    g, bound = pr.gelu_tab_bound(y, dy)
    hi, lo = out[:, :N], out[:, N:]
    worst.add(kr.bf16_value(hi).astype(np.float64) + kr.bf16_value(lo).astype(np.float64), g, bound, c["name"])
    return pr.lo_too_large(hi, lo)


# ---- launch_gemm_ln_x3 ---------------------------------------------------------------------------------------------------------------------
def gemm_ln_x3_cases():
    out = [dict(T=256, K1=384), dict(T=512, K1=1536), dict(T=512, K1=384), dict(T=256, K1=1536)]
    for i, c in enumerate(out):
        c.update(eps=(1e-12, 1e-5)[i % 2], name=f"gemmln3_T{c['T']}_K{c['K1']}")
    return out


def gemm_ln_x3_inputs(c):
    """kernel_cases.gemm_ln_inputs' row classes (offset rows of |mean| / std ~ 0, 4, 32 and the near-constant row) on float32 operands."""
    rng = _rng(c["name"])
    T, K, H = c["T"], c["K1"], kc.LN_H
    x = rng.standard_normal((T, K)).astype(F)
    w = (rng.standard_normal((H, K)) * (1.0 / math.sqrt(K))).astype(F)
    bias = (0.1 * rng.standard_normal(H)).astype(F)
    g, b = ln_params(rng, H)
    res = rng.standard_normal((T, H)) * 2.0 + kc.row_offsets(T, 2.5)
    x[kc.flat_row(T)] = 0.0
    res[kc.flat_row(T)] = 2.0 ** -10 + 2.0 ** -22 * rng.integers(-3, 4, H) - bias.astype(np.float64)
    return dict(x2=pr.split_rows(x), w2=pr.split_rows(w), bias=bias, res=res.astype(F), gamma=g, beta=b)


def gemm_ln_x3_expect(c, inp, **mut):
    """kr.gemm_ln_ref's dr on split operands: the accumulation (the bias is not part of it), then bias + residual, then their sum -- each
    float32 addition e times its RESULT."""
    y, dy = pr.gemm_x3w_pre(inp["x2"], inp["w2"], inp["bias"], bias_in_sum=False)
    res, bias = inp["res"].astype(np.float64), inp["bias"].astype(np.float64)
    r = y + res
    dr = dy + pr.E * (np.abs(bias + res) + np.abs(r))
    return pr.ln_expect(r, dr, inp["gamma"], inp["beta"], c["eps"], **mut)


# ---- attention -------------------------------------------------------------------------------------------------------------------------------
def attn_cases():
    """(hd, S, B, heads, mask, rel). B . heads in {1, 3, 8, 9, 24}: the grid is padded to eights, group 8 is the first of the second lap.
    One case at H = 384: the split launcher's rows are then 1152 -> 1280 floats, as the padded QKV projection of hidden 384 writes them."""
    rows = [(32, 1, 1, 1, "right", 0), (64, 31, 3, 1, "right", 1), (32, 32, 4, 2, "left", 0), (64, 33, 3, 3, "holes", 1), (32, 96, 12, 2, "right", 1),
            (64, 128, 1, 3, "left", 0), (32, 129, 4, 2, "holes", 0), (64, 160, 3, 3, "right", 1), (64, 512, 1, 1, "holes", 1), (32, 512, 3, 3, "left", 1),
            (64, 96, 12, 2, "fullmask", 0), (32, 160, 8, 1, "fullmask", 1), (64, 129, 4, 6, "right", 0), (32, 31, 1, 3, "holes", 1),
            (64, 96, 3, 3, "left", 1)]
    return [dict(hd=hd, S=S, B=B, heads=h, mask=m, rel=bool(r), name=f"a_hd{hd}_S{S}_B{B}_h{h}_{m}_rel{r}") for hd, S, B, h, m, r in rows]


ATTN_LAUNCHERS = ("f32", "x3", "x3_split")
SPLIT_LDQ_PAD = 128          # the split launcher's qkv rows: ldq = 3 H + 128 (1152 -> 1280 at H = 384)


def attn_inputs(c):
    """qkv [B * S][3 H] float32, mask [B][S] bool, rel [heads][REL_ROW] float32 (natural units) or None."""
    rng = _rng(c["name"])
    hd, S, B, heads = c["hd"], c["S"], c["B"], c["heads"]
    H = heads * hd
    lens = kc.lengths_for(S)
    start = zlib.crc32(c["name"].encode()) % len(lens)
    q = rng.standard_normal((B, heads, S, hd))
    k = rng.standard_normal((B, heads, S, hd))
    v = rng.standard_normal((B, heads, S, hd))
    mask = np.zeros((B, S), bool)
    for b in range(B):
        n = lens[(start + b) % len(lens)] if b else (S - 1 if S > 2 else S)          # (row 0: a long one, whatever the rotation gives the rest)
        if c["mask"] == "fullmask":
            n = 0 if b == B // 2 else max(n, 1)
            mask[b] = kr.mask_right(S, n)
        elif c["mask"] == "left":
            n = max(1, min(n, S - 32)) if S > 32 else max(n, 1)          # S > 32: the first key block fully masked
            mask[b] = kr.mask_left(S, n)
        elif c["mask"] == "holes":
            mask[b] = kr.mask_holes(S, max(n, 1), rng)
        else:
            mask[b] = kr.mask_right(S, max(n, 1))
        sig = np.where((b + np.arange(heads)) % 2 == 0, 0.5, 1.6)
        q[b] *= sig[:, None, None]
        vis = np.flatnonzero(mask[b])
        if vis.size == 0:
            continue
        first, last = int(vis[0]), int(vis[-1])
        pairs = [(last, last), (first, last + 1), (last, first - 1), ((first + last) // 2, S - 1), (first, (first + last) // 2)]
        for i, (qi, kj) in enumerate(pairs):
            if not (0 <= kj < S):
                continue
            h = (i + b) % heads
            qv = q[b, h, qi]
            k[b, h, kj] = qv * (10.0 * math.sqrt(hd) / max(float(qv @ qv), 1e-12))      # natural logit 10 against its query
            v[b, h, kj] = kc._probe_v(i, hd) * (1.0 + 0.01 * rng.standard_normal(hd))      # (distinctive, and no bf16 number: its lo half counts)
    pack = lambda a: a.transpose(0, 2, 1, 3).reshape(B * S, H)
    qkv = np.concatenate([pack(q), pack(k), pack(v)], axis=1).astype(F)
    rel = None
    if c["rel"]:
        rel = np.zeros((heads, kr.REL_ROW), F)
        d = np.arange(-kr.REL_MID, kr.REL_ROW - kr.REL_MID)
        inside = np.abs(d) < S
        rel[:, inside] = (rng.standard_normal((heads, int(inside.sum()))) * np.where(rng.random((heads, int(inside.sum()))) < 0.1, 3.0, 0.7)).astype(F)
    return dict(qkv=qkv, mask=mask, rel=rel)


def attn_rel_base2(rel):
    """The table the base-2 kernels are handed: rel log2(e), rounded to float32 (as k_rel_table makes it)."""
    return (rel * F(pr.LOG2E)).astype(F)


def attn_head(c, inp, b, h):
    S, hd, H = c["S"], c["hd"], c["heads"] * c["hd"]
    rows = inp["qkv"][b * S:(b + 1) * S]
    return rows[:, h * hd:(h + 1) * hd], rows[:, H + h * hd:H + (h + 1) * hd], rows[:, 2 * H + h * hd:2 * H + (h + 1) * hd]


def attn_bias(c, inp, h, launcher, flip=False):
    """(dense bias in natural units as the launcher's table states it, its largest magnitude) or (None, 0)."""
    if inp["rel"] is None:
        return None, 0.0
    row = inp["rel"][h].astype(np.float64) if launcher == "f32" else attn_rel_base2(inp["rel"])[h].astype(np.float64) / pr.LOG2E
    return pr.rel_dense(row, c["S"], flip), float(np.abs(row).max())


def attn_values(c, launcher, out):
    """The launcher's raw output -> float64 [B * S][H] values (+ structural violations of the split form)."""
    H = c["heads"] * c["hd"]
    if launcher != "x3_split":
        return np.asarray(out, np.float64), 0
    hi, lo = out[:, :H], out[:, H:]
    return kr.bf16_value(hi).astype(np.float64) + kr.bf16_value(lo).astype(np.float64), pr.lo_too_large(hi, lo)


def attn_check(c, inp, launcher, out, worst, ref=None):
    """Every row of a visible query of every (sequence, head) against the float64 reference; a sequence without a visible key: exact zeros;
    every other row finite. Returns the number of violations of those two and of the [hi | lo] structure."""
    S, hd, B, heads = c["S"], c["hd"], c["B"], c["heads"]
    vals, bad = attn_values(c, launcher, out)
    split = launcher != "f32"
    for b in range(B):
        m = inp["mask"][b]
        rows = vals[b * S:(b + 1) * S]
        if not m.any():
            bad += int((rows != 0).sum())
            continue
        bad += int((~np.isfinite(rows[~m])).sum())
        valid = np.flatnonzero(m)
        for h in range(heads):
            key = (c["name"], launcher, b, h)
            if ref is not None and key in ref:
                want, bound = ref[key]
            else:
                qh, kh, vh = attn_head(c, inp, b, h)
                bias, bmax = attn_bias(c, inp, h, launcher)
                want, bound = pr.attn_expect(qh, kh, vh, m, bias, split, bmax)
                if launcher == "x3_split":
                    bound = bound + pr.U * pr.U * np.abs(want)
                want, bound = want[valid], bound[valid]
                if ref is not None:
                    ref[key] = (want, bound)
            worst.add(rows[valid, h * hd:(h + 1) * hd], want, bound, c["name"], b, h, rows=valid)
    return bad


# ---- row kernels ---------------------------------------------------------------------------------------------------------------------------
VOCAB, NPOS = 50, 40


def ln_params(rng, H):
    """kernel_cases.ln_params at any H >= 128: gamma ~ N(1, 0.3) with three entries exactly 0 and three negative, beta ~ N(0, 0.5), float32."""
    g = (1.0 + 0.3 * rng.standard_normal(H)).astype(F)
    g[[3, H // 5, H - 56]] = 0.0
    neg = [5, H // 3, H - 1]
    g[neg] = -np.abs(g[neg])
    return g, (0.5 * rng.standard_normal(H)).astype(F)


def embed_cases():
    """(T, S, H, posid). ids out of range (negative, = vocab, far above) among them."""
    rows = [(1, 1, 128, 0), (3, 3, 384, 1), (4, 2, 768, 0), (5, 5, 1024, 1), (257, 32, 384, 0), (257, 257, 128, 1)]
    return [dict(T=T, S=S, H=H, posid=bool(p), eps=(1e-12, 1e-5)[i % 2], name=f"emb_T{T}_S{S}_H{H}_p{p}") for i, (T, S, H, p) in enumerate(rows)]


def embed_inputs(c):
    rng = _rng(c["name"])
    T, H = c["T"], c["H"]
    ids = rng.integers(0, VOCAB, T).astype(np.int32)
    ids[::5] = np.array([-1, VOCAB, 10 ** 9, -2 ** 31, VOCAB + 7])[np.arange(len(ids[::5])) % 5]
    if T > 1:
        ids[1] = 7
    g, b = ln_params(rng, H)
    posid = rng.integers(0, NPOS, T).astype(np.int32) if c["posid"] else None
    return dict(ids=ids, posid=posid, word=rng.standard_normal((VOCAB, H)).astype(F), pos=(0.5 * rng.standard_normal((max(NPOS, c["S"]), H))).astype(F),
                type=(0.3 * rng.standard_normal(H) + 0.5).astype(F), gamma=g, beta=b)


def embed_expect(c, inp, **mut):
    posrow = inp["posid"] if inp["posid"] is not None else np.arange(c["T"]) % c["S"]
    r, dr = pr.embed_rows(inp["ids"], posrow, inp["word"], inp["pos"], inp["type"], VOCAB)
    return pr.ln_expect(r, dr, inp["gamma"], inp["beta"], c["eps"], **mut)


def add_ln_cases():
    """(T, H, ldy - H, r). r: none | sep (a second buffer) | inplace (out is r). ldy > H is the split launcher's only; the float32 one reads rows of H."""
    rows = [(1, 128, 0, "sep"), (3, 384, 128, "inplace"), (4, 768, 0, "none"), (5, 1024, 256, "sep"), (257, 384, 0, "inplace"), (257, 128, 128, "none")]
    return [dict(T=T, H=H, pad=p, r=r, eps=(1e-12, 1e-5)[i % 2], name=f"ln_T{T}_H{H}_p{p}_{r}") for i, (T, H, p, r) in enumerate(rows)]


def add_ln_inputs(c):
    rng = _rng(c["name"])
    T, H = c["T"], c["H"]
    g, b = ln_params(rng, H)
    y = (rng.standard_normal((T, H)) * 1.5 + kc.row_offsets(T, 2.0)).astype(F)
    r = None if c["r"] == "none" else (rng.standard_normal((T, H)) * 2.0).astype(F)
    if T >= 3:                                       # a near-constant row (variance 2e-13, below BERT's eps): eps decides its scale
        y[kc.flat_row(T)] = (2.0 ** -10 + 2.0 ** -22 * rng.integers(-3, 4, H)).astype(F)
        if r is not None:
            r[kc.flat_row(T)] = 0.0
    return dict(y=y, r=r, gamma=g, beta=b)


def add_ln_expect(c, inp, no_residual=False, **mut):
    y = inp["y"].astype(np.float64)
    if inp["r"] is None or no_residual:
        return pr.ln_expect(y, 0.0, inp["gamma"], inp["beta"], c["eps"], **mut)
    r = y + inp["r"].astype(np.float64)
    return pr.ln_expect(r, pr.E * np.abs(r), inp["gamma"], inp["beta"], c["eps"], **mut)


def split_out_check(name, out32, out2, want, bound, worst):
    """A row kernel's float32 rows against the bound, and its [hi | lo] rows against those float32 rows bit for bit. Returns the mismatches."""
    H = out32.shape[1]
    worst.add(out32, want, bound, name)
    return pr.split_mismatch(out32, out2[:, :H], out2[:, H:])


def pool_cases():
    """(B, S, H): each with mean / CLS x normalise 0 / 1. Sequences: full, one visible token, holes, none visible, two tokens that cancel."""
    return [dict(B=5, S=S, H=H, name=f"pool_S{S}_H{H}") for S, H in ((33, 128), (96, 384), (257, 768), (512, 1024))]


POOL_MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]     # (pooling: 0 mean / 1 CLS -- the library's AK_POOL_MEAN / AK_POOL_CLS, normalise)


def pool_inputs(c):
    rng = _rng(c["name"])
    B, S, H = c["B"], c["S"], c["H"]
    x = rng.standard_normal((B, S, H)).astype(F)
    mask = np.zeros((B, S), np.int32)
    mask[0] = 1
    mask[1, S // 2] = 1
    mask[2] = rng.random(S) < 0.6
    mask[2, 0] = 0
    mask[4, [1, S - 1]] = 1
    x[4, S - 1] = -x[4, 1]                           # the pooled vector is exactly zero: the 1e-12 floor
    x[3, 0] = 0.0                                    # no visible token; CLS reads a zero row: the floor again
    return dict(x=x, mask=mask)


def pool_zero_rows(pooling):
    """Sequences whose output is exact zeros in any order of additions: no visible token (mean: 0 / 1e-9; CLS: token 0 is a zero row), and,
    for the mean, two visible rows x and -x (their sum is exact, zeros add exactly) -- 0 / max(0, 1e-12) = 0: the floor, not 0 / 0."""
    return [3] if pooling == 1 else [3, 4]


def split_cases():
    """split_hilo over n elements, split_rows over [rows][K]."""
    return [dict(kind="hilo", n=n, name=f"hilo_{n}") for n in (1, 255, 257, 128 * 384 + 3)] + \
           [dict(kind="rows", rows=r, K=K, name=f"rows_{r}_{K}") for r, K in ((1, 4), (3, 384), (257, 132), (64, 1536))]


def split_inputs(c):
    rng = _rng(c["name"])
    n = c["n"] if c["kind"] == "hilo" else c["rows"] * c["K"]
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 3, n)).astype(F)
    x[:: 17] = kr.bf16_round(x[:: 17])               # values that are bf16 numbers: lo = 0
    x[3:: 29] = 0.0
    return x if c["kind"] == "hilo" else x.reshape(c["rows"], c["K"])
