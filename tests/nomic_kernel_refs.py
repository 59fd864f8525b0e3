"""Cases, inputs, float64 statements, derived bounds, float32 emulations and mutants of NomicBERT's three row kernels (csrc/nomic.hip:
k_nb_embed, k_nb_add_ln, k_nb_pool_part + k_nb_pool_fin), one launch each through ak_kts_nb_*: family `nb` of tests/test_stack_kernels_gpu.py. Plain numpy, written from the mathematics,
on the conventions of tests/stack_kernel_refs.py (its module docstring derives the pieces used here: the summation trees, store16, the
LayerNorm bound, the pooling bound, the L2 tail); nothing here goes through the library or tests/nomic_ref.py.

U = 2^-8 (bf16), E = 2^-24 (float32). What is new against the ModernBERT kernels:

LayerNorm with a bias of a SUM  out = g (r - mu) rstd + b, r = a + c the one float32 add in front (embedding: bf16 word row + float32
    type row; add + norm: x32 + y32). The float64 statement takes r = a + c exactly; the kernel's r is within dr = E |r| of it. A
    perturbation dr of the row moves g rh by |g| rstd (dr + mean dr + |rh| mean(|rh| dr)) (kernel_refs.layernorm_bound); the
    float32 LayerNorm of the row it holds adds stack_kernel_refs.ln_bound on g rh (mean tree, centred squares, rsqrtf, the three
    products); the add of b rounds once: E |out|.
        d = |g| rstd (dr + mean dr + |rh| mean(|rh| dr)) + ln_bound(r, g, g rh, rstd, tree_wave(H)) + E |out|
    x32 (float32) is held to d, h16 = bf16(x32) to U |want| + (1 + U) d.
Pooling  the identity per token: stack_kernel_refs.pool_expect's statement for a family without a per-token norm and without a weight,
    with the L2 tail and cls pooling: (tree_pool E sum_t |x_t|) / n + 3 E |y|, then l2_ref.
Exact (bit for bit): token_slot's lengths and mask, zeros for rows of length 0, the sentinel behind every buffer.

An expectation is {output name: ("exact", array) | ("bound", want, bound)}; stack_kernel_refs.compare / flagged hold kernel outputs,
emulations and mutants to it. Mutants: onepass (variance as E[x^2] - mean^2), no_bias (the LayerNorm bias dropped), y_alone (LayerNorm
of y without the residual), type_1 (token-type row 1), cls_1 (cls reading token 1), div_S (mean divided by S), no_writeback (x32 left
holding the sum, as k_mb_add_ln leaves it)."""
import zlib

import numpy as np

try:
    from tests import kernel_cases as kc
    from tests import kernel_refs as kr
    from tests import stack_kernel_cases as sc
    from tests import stack_kernel_refs as sr
except ImportError:          # imported by the worker script, whose directory is tests/ itself
    import kernel_cases as kc
    import kernel_refs as kr
    import stack_kernel_cases as sc
    import stack_kernel_refs as sr

U, E, F = sr.U, sr.E, np.float32
HS = sc.HS                   # 128, 256, 384, 640, 768, 1024: idle lanes, full and partial NJ
SS = (32, 96, 192)
VOCAB, TYPES = sc.VOCAB, 2
GUARD, SENT, SENT_I = sc.GUARD, sc.SENT, sc.SENT_I
EPS = (1e-12, 1e-5)          # the model's eps and one at which eps decides sooner


def _rng(c, salt=""):
    return np.random.default_rng(zlib.crc32((c["name"] + salt).encode()))


def raw_lens(S):
    """Lengths from {S, S - 1, 65, 1, 0} and, for the clamp, one negative and one past S (65 is past S = 32, too)."""
    return np.array([-3, 0, 1, 65, S - 1, S, S + 5], np.int32)


# ---- cases and inputs ------------------------------------------------------------------------------------------------------------
def embed_cases():
    """k_nb_embed<NJ>: B = 7 rows at S = 32, 96 and 192, ld_ids > S, lens_stride = 2, every hidden size."""
    out = []
    for H in HS:
        for S in SS:
            out.append(dict(fam="nb", H=H, S=S, B=7, ld_ids=S + 7, lens_stride=2, vocab=VOCAB, eps=EPS[len(out) % 2], name=f"embed_nb_H{H}_S{S}"))
    return out


def embed_inputs(c):
    """As stack_kernel_cases.embed_inputs (stray ids inside the length, garbage past it and behind S, table rows of very different
    size and |mean| / std, one all-zero row) plus the float32 token-type table [2][H], its two rows different, and a LayerNorm
    weight and bias from kernel_cases.ln_params."""
    rng = _rng(c)
    B, S, H, ld, V = c["B"], c["S"], c["H"], c["ld_ids"], c["vocab"]
    raw = raw_lens(S)
    lens = np.full((B, c["lens_stride"]), 77777, np.int32)
    lens[:, 0] = raw
    ids = rng.integers(1, V, (B, ld)).astype(np.int32)
    junk = np.array([-7, V, V + 1, 10 ** 6, 2 ** 31 - 1, -2 ** 31, 5, V - 1], np.int64)
    for b in range(B):
        n = min(max(int(raw[b]), 0), S)
        ids[b, n:] = rng.choice(junk, size=ld - n).astype(np.int32)
    ids[4, 1], ids[5, 2], ids[6, 3], ids[5, 5], ids[6, 0] = -1, V, 2 ** 30, 11, V - 1
    sig = sc._scales(rng, V)
    off = np.array(kc.CLASSES, np.float64)[np.arange(V) % 3][:, None] * sig * np.where(np.arange(V) % 2, -1.0, 1.0)[:, None]
    emb = rng.standard_normal((V, H)) * sig + off
    emb[11] = 0.0
    typ = (0.5 * rng.standard_normal((TYPES, H))).astype(F)
    (g, b), = kc.ln_params(rng, max(H, 256), 1)
    return dict(ids=ids, lens=lens, emb=kr.bf16_bits(emb.astype(F)), type=typ, g=g[:H].copy(), b=b[:H].copy())


def addnorm_cases():
    """k_nb_add_ln<NJ>: T in {1, 5, 127, 384} (1, 1, 3 and 0 waves of the last workgroup with a row), every hidden size."""
    out = []
    for H in HS:
        for T in (1, 5, 127, 384):
            out.append(dict(fam="nb", H=H, T=T, eps=EPS[len(out) % 2], name=f"addnorm_nb_H{H}_T{T}"))
    return out


def addnorm_inputs(c):
    """stack_kernel_cases.addnorm_inputs' rows for the LayerNorm family (row scales 2^-6 .. 2^6, the |mean| / std classes in y, an
    all-zero row, a row of a few units of 2^-22) with a LayerNorm weight and bias."""
    base = sc.addnorm_inputs(dict(c, fam="mb"))
    rng = _rng(c, "ln")
    (g, b), = kc.ln_params(rng, max(c["H"], 256), 1)
    return dict(x=base["x"], y=base["y"], g=g[:c["H"]].copy(), b=b[:c["H"]].copy())


def pool_lens(S):
    return {192: [192, 191, 129, 65, 64, 63, 1, 0], 96: [96, 95, 65, 64, 63, 1, 0], 32: [32, 31, 1, 0]}[S]


def pool_cases():
    """k_nb_pool_part + k_nb_pool_fin: every hidden size at S = 192 with the chunk edges 63 / 64 / 65 among the lengths; S = 96 and
    S = 32 (a single chunk) at H = 384 and 768; the S = 192 launch's row of 129 tokens alone at S = 2048 (`twin`)."""
    out = []
    for H in HS:
        out.append(dict(H=H, S=192, lens=pool_lens(192), name=f"pool_nb_H{H}_S192"))
    for H in (384, 768):
        for S in (96, 32):
            out.append(dict(H=H, S=S, lens=pool_lens(S), name=f"pool_nb_H{H}_S{S}"))
    out.append(dict(H=768, S=2048, lens=[129], twin="pool_nb_H768_S192", name="pool_nb_H768_twin"))
    for c in out:
        c.update(fam="nb", eps=0.0)
    return out


TWIN_ROW = pool_lens(192).index(129)
POOL_MODES = [("mean_n1", 0, 1), ("mean_n0", 0, 0), ("cls_n1", 1, 1), ("cls_n0", 1, 0)]


def pool_inputs(c):
    """x [B][S][H] float32: token t of row b is (-1)^t (a_b + noise), so a pooled mean is small against the sum of magnitudes. Token
    rows at or past the length are NaN."""
    if "twin" in c:
        src = pool_inputs(next(b for b in pool_cases() if b["name"] == c["twin"]))
        x = np.full((1, c["S"], c["H"]), np.nan, F)
        x[0, :192] = src["x"][TWIN_ROW]
        return dict(x=x, lens=np.array(c["lens"], np.int32), w=src["w"])
    rng = _rng(c)
    B, S, H = len(c["lens"]), c["S"], c["H"]
    x = np.empty((B, S, H), F)
    sign = np.where(np.arange(S) % 2, -1.0, 1.0)[:, None]
    for b, n in enumerate(c["lens"]):
        sig = 2.0 ** int(rng.integers(-6, 7))
        a = rng.standard_normal(H) * sig
        xb = (sign * (a[None, :] + 0.25 * sig * rng.standard_normal((S, H)))).astype(F)
        xb[n:] = np.nan
        x[b] = xb
    return dict(x=x, lens=np.array(c["lens"], np.int32), w=np.ones(H, F))      # (w: pool_expect's signature; the model has no weight here)


# ---- LayerNorm with a bias of a sum ----------------------------------------------------------------------------------------------
def ln_sum_expect(a, c, g, b, eps, mut=None):
    """(want, d) of out = LayerNorm(a + c; g, b) in float64 for a kernel that forms r = a + c in one float32 add. mut: onepass |
    no_bias | y_alone (the LayerNorm of c alone)."""
    a, c = np.asarray(a, np.float64), np.asarray(c, np.float64)
    g, b = np.asarray(g, np.float64), np.asarray(b, np.float64)
    r = c if mut == "y_alone" else a + c
    H = r.shape[-1]
    grh, mu, rstd, rh = sr.ln_ref(r, g, eps, "onepass" if mut == "onepass" else None)
    want = grh if mut == "no_bias" else grh + b
    dr = E * np.abs(r)
    arh = np.abs(rh)
    pert = np.abs(g) * rstd * (dr + dr.mean(-1, keepdims=True) + arh * (arh * dr).mean(-1, keepdims=True))
    return want, pert + sr.ln_bound(r, g, grh, rstd, sr.tree_wave(H)) + E * np.abs(want)


def emu_ln_sum(a, c, g, b, eps):
    """The kernels' float32 arithmetic: r = a + c, mb_row_stats' two passes in wave order, (r - mean) rstd g + b."""
    r = np.asarray(a, F) + np.asarray(c, F)
    mean, rstd = sr.emu_ln_stats(r, eps)
    return (r - mean) * rstd * np.asarray(g, F) + np.asarray(b, F)


def _guards(H):
    return {"x32_guard": ("exact", np.full((GUARD, H), SENT, F)), "h16_guard": ("exact", kr.bf16_bits(np.full((GUARD, H), SENT, F)))}


def embed_expect(c, inp, mut=None):
    """mut: onepass | no_bias | type_1 | stray_id | len_unclamped."""
    H = c["H"]
    ids, lens, mask = sr.token_slots(c, inp, mut if mut in ("stray_id", "len_unclamped") else None)
    rows = kr.bf16_value(inp["emb"])[ids.reshape(-1)]
    typ = inp["type"][1 if mut == "type_1" else 0]
    want, d = ln_sum_expect(rows, np.broadcast_to(typ, rows.shape), inp["g"], inp["b"], c["eps"], mut)
    out = {"lens": ("exact", lens), "mask": ("exact", mask.reshape(-1)), "x32": ("bound", want, d), "h16": ("bound", want, sr.store16(want, d))}
    out.update(_guards(H))
    return out


def embed_emulate(c, inp):
    ids, lens, mask = sr.token_slots(c, inp)
    rows = kr.bf16_value(inp["emb"])[ids.reshape(-1)]
    x = emu_ln_sum(rows, np.broadcast_to(inp["type"][0], rows.shape), inp["g"], inp["b"], c["eps"])
    return {"lens": lens, "mask": mask.reshape(-1), "x32": x, "h16": kr.bf16_bits(x)}


def addnorm_expect(c, inp, mut=None):
    """x32 <- LayerNorm(x + y; g, b) in float32, h16 = bf16 of it. mut: onepass | no_bias | y_alone | no_writeback (x32 keeps the sum)."""
    want, d = ln_sum_expect(inp["x"], inp["y"], inp["g"], inp["b"], c["eps"], mut)
    x_want = inp["x"].astype(np.float64) + inp["y"].astype(np.float64) if mut == "no_writeback" else want
    out = {"x32": ("bound", x_want, d), "h16": ("bound", want, sr.store16(want, d))}
    out.update(_guards(c["H"]))
    return out


def addnorm_emulate(c, inp):
    x = emu_ln_sum(inp["x"], inp["y"], inp["g"], inp["b"], c["eps"])
    return {"x32": x, "h16": kr.bf16_bits(x)}


def pool_expect(c, inp, mode, mut=None):
    """stack_kernel_refs.pool_expect for a family with the identity per token and no weight. mut: cls_1 | div_S | n_plus_1 | n_ceil64."""
    return sr.pool_expect(c, inp, mode, mut)


def pool_emulate(c, inp, mode):
    return sr.pool_emulate(c, inp, mode)
