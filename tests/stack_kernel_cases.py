"""Cases and inputs of tests/test_stack_kernels_gpu.py, shared by the parent (float64 references), the child (launches) and the CPU
suite (tests/test_stack_kernels_cpu.py): the small kernels of the pre-norm stacks -- decoder128.hip (Qwen3, `dec`), mbert.hip (ModernBERT,
`mb`), gemma.hip (EmbeddingGemma, `gm`) -- and k_gemm MODE 3, one launch each, in the manner of tests/gemma_kernel_cases.py. Everything
comes from a seed (the case's name); the shapes are the smallest at which each kernel can still go wrong."""
import math
import zlib

import numpy as np

try:
    from tests import kernel_cases as kc
    from tests import kernel_refs as kr
except ImportError:          # imported by the worker script, whose directory is tests/ itself
    import kernel_cases as kc
    import kernel_refs as kr

# hidden sizes of every row kernel: lanes 32 .. 63 idle; full NJ = 1; NJ = 2 with the second slice half filled; NJ = 3 partial; full
# NJ = 3; full NJ = 4; and, Qwen3 only (its kernels loop past 1024, the library sets no cap), Qwen3-Embedding-4B's 2560
HS = (128, 256, 384, 640, 768, 1024)
DEC_H = 2560
FAMS = ("dec", "mb", "gm")
VOCAB = 97
SENT = kc.SENTINEL           # float32- and bf16-exact: prefilled where a kernel must not write
SENT_I = -123456789
GUARD = 4                    # sentinel rows behind every row buffer (one workgroup of the row kernels)


def hs(fam):
    return HS + (DEC_H,) if fam == "dec" else HS


def nj(H):
    return -(-H // 256)


def _rng(c, salt=""):
    return np.random.default_rng(zlib.crc32((c["name"] + salt).encode()))


def _eps(i):
    return (1e-6, 1e-5)[i % 2]


def _scales(rng, n):
    return np.exp2(rng.integers(-6, 7, (n, 1))).astype(np.float64)


def weights(rng, H, n=1):
    """n norm weights from kernel_cases.ln_params (zeros and negatives among them); H = 128: the first 128 of a 256-wide draw."""
    return [g[:H].copy() for g, _ in kc.ln_params(rng, max(H, 256), n)]


# ---- embedding kernels (token_slot) ----------------------------------------------------------------------------------------------
def embed_cases():
    """k_dec_embed / k_mb_embed / k_gm_embed: B = 6 rows at S = 32 and 96, ld_ids > S, lens_stride = 2."""
    out = []
    for fam in FAMS:
        for H in hs(fam):
            for S in (32, 96):
                out.append(dict(fam=fam, H=H, S=S, B=6, ld_ids=S + 7, lens_stride=2, vocab=VOCAB, eps=_eps(len(out)),
                                name=f"embed_{fam}_H{H}_S{S}"))
    return out


def embed_inputs(c):
    """Lengths {-3, 0, 1, S - 1, S, S + 5}; inside the length one negative id, one id == vocab, one far past it (and the id of an
    all-zero table row); past the length and in the columns behind S garbage, out-of-range ids among it. The table: rows of very
    different size, the three |mean| / std classes by row number (ModernBERT's LayerNorm sees them), row 11 zero."""
    rng = _rng(c)
    B, S, H, ld, V = c["B"], c["S"], c["H"], c["ld_ids"], c["vocab"]
    raw = np.array([-3, 0, 1, S - 1, S, S + 5], np.int32)
    lens = np.full((B, c["lens_stride"]), 77777, np.int32)
    lens[:, 0] = raw
    ids = rng.integers(1, V, (B, ld)).astype(np.int32)
    junk = np.array([-7, V, V + 1, 10 ** 6, 2 ** 31 - 1, -2 ** 31, 5, V - 1], np.int64)
    for b in range(B):
        n = min(max(int(raw[b]), 0), S)
        ids[b, n:] = rng.choice(junk, size=ld - n).astype(np.int32)
    ids[3, 1], ids[4, 2], ids[5, 3], ids[4, 5], ids[5, 0] = -1, V, 2 ** 30, 11, V - 1
    sig = _scales(rng, V)
    off = np.array(kc.CLASSES, np.float64)[np.arange(V) % 3][:, None] * sig * np.where(np.arange(V) % 2, -1.0, 1.0)[:, None]
    emb = rng.standard_normal((V, H)) * sig + off
    emb[11] = 0.0
    g, = weights(rng, H)
    return dict(ids=ids, lens=lens, emb=kr.bf16_bits(emb.astype(np.float32)), w=g)


# ---- add + norm kernels ------------------------------------------------------------------------------------------------------------
def addnorm_cases():
    """k_dec_add_rmsnorm, k_mb_add_ln<NJ>, k_gm_norm_add_norm<NJ>: T in {1, 5, 127, 512} (1, 1, 3 and 0 waves of the last workgroup
    with a row). form `norm`: the add and the norm; `add`: w == NULL (T = 5); Gemma `h16` and `out32` (out32 aliasing y32: the
    final norm)."""
    out = []
    for fam in FAMS:
        for H in hs(fam):
            for T in (1, 5, 127, 512):
                forms = ("h16", "out32") if fam == "gm" else (("norm", "add") if T == 5 else ("norm",))
                for form in forms:
                    out.append(dict(fam=fam, H=H, T=T, form=form, eps=_eps(len(out)), name=f"addnorm_{fam}_{form}_H{H}_T{T}"))
    return out


def zero_row(T):
    return kc.flat_row(T) if T > 2 else None


def tiny_row(T):
    return kc.flat_row(T) + 1 if T > 2 and kc.flat_row(T) + 1 < T else None


def addnorm_inputs(c):
    """As kernel_cases.layernorm_inputs: x N(0, 1) and y N(0, 2) at row scales 2^-6 .. 2^6, a few rows 64 times larger, for the
    LayerNorm kernel the class offset of the token in y; one all-zero row and one row of a few units of 2^-22 (eps decides);
    weights from ln_params (zeros and negatives among them)."""
    rng = _rng(c)
    T, H = c["T"], c["H"]
    sc = _scales(rng, T)
    x = rng.standard_normal((T, H)) * sc
    x[rng.choice(T, size=max(1, T // 64), replace=False)] *= 64.0
    y = rng.standard_normal((T, H)) * 2.0 * sc
    if c["fam"] == "mb":
        y += kc.row_offsets(T, 2.3) * sc
    if zero_row(T) is not None:
        x[zero_row(T)] = y[zero_row(T)] = 0.0
    if tiny_row(T) is not None:
        x[tiny_row(T)] = 2.0 ** -22 * rng.integers(-3, 4, H)
        y[tiny_row(T)] = 0.0
    g1, g2 = weights(rng, H, 2)
    return dict(x=x.astype(np.float32), y=y.astype(np.float32), w=g1, w_post=g2)


# ---- RoPE ---------------------------------------------------------------------------------------------------------------------------
DEC_HD, MB_HD = 128, 64
ROPE_EPS = 1e-6


def rope_cases():
    """k_dec_qk_rope: (nq, nkv) in {(1, 1), (2, 1), (4, 1), (3, 3)} -- 3, 4, 6 and 9 head slots over four waves -- at B = 2, S = 64
    and B = 3, S = 32 (the position restarts per row), and B = 1, S = 8192 (the last table row). k_mb_rope in place at H in
    {128, 384, 768}, the same B / S pairs, and S = 8192 at H = 128. Thetas: Qwen3's 1e6, ModernBERT's global 160000 / local 10000."""
    out = []
    for nq, nkv in ((1, 1), (2, 1), (4, 1), (3, 3)):
        for B, S in ((2, 64), (3, 32)):
            out.append(dict(fam="dec", B=B, S=S, nq=nq, nkv=nkv))
    out.append(dict(fam="dec", B=1, S=8192, nq=1, nkv=1))
    for H in (128, 384, 768):
        for B, S in ((2, 64), (3, 32)):
            out.append(dict(fam="mb", B=B, S=S, H=H))
    out.append(dict(fam="mb", B=1, S=8192, H=128))
    for i, c in enumerate(out):
        if c["fam"] == "dec":
            c.update(theta=1e6, hd=DEC_HD, qscale=math.log2(math.e) / math.sqrt(128.0), name=f"rope_dec_B{c['B']}_S{c['S']}_q{c['nq']}_kv{c['nkv']}")
        else:
            c.update(theta=(160000.0, 10000.0)[i % 2], hd=MB_HD, name=f"rope_mb_B{c['B']}_S{c['S']}_H{c['H']}")
    return out


def rope_inputs(c):
    """Head rows of very different size, one all-zero head; the head-norm weights N(1, 0.3)."""
    rng = _rng(c)
    T = c["B"] * c["S"]
    if c["fam"] == "dec":
        slots = c["nq"] + 2 * c["nkv"]
        x = rng.standard_normal((T, slots, DEC_HD), dtype=np.float32) * np.exp2(rng.integers(-6, 6, (T, slots, 1))).astype(np.float32)
        x[T // 2, 0] = 0.0
        qn = (1.0 + 0.3 * rng.standard_normal(DEC_HD)).astype(np.float32)
        kn = (1.0 + 0.3 * rng.standard_normal(DEC_HD)).astype(np.float32)
        return dict(qkv=kr.bf16_bits(x), qn=qn, kn=kn)
    heads = c["H"] // MB_HD
    x = rng.standard_normal((2, T, heads, MB_HD), dtype=np.float32) * np.exp2(rng.integers(-6, 6, (2, T, heads, 1))).astype(np.float32)
    x[0, T // 2, 0] = 0.0
    return dict(q=kr.bf16_bits(x[0]).reshape(T, c["H"]), k=kr.bf16_bits(x[1]).reshape(T, c["H"]))


# ---- pooling -------------------------------------------------------------------------------------------------------------------------
LENS192 = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192)
TWIN_ROW = LENS192.index(129)            # the row given a second time, alone at S = 2048
STEEP = (1, 3)                           # lengths whose token rows have |mean| / std = 512 (float32 rows can)


def pool_cases():
    """k_dec_pool; k_mb_pool_part + k_mb_pool_fin; k_gm_pool_part + k_gm_pool_fin. Per family and hidden size one launch at S = 192
    with every length of LENS192 as a batch row, and one at S = 2048 with the S = 192 launch's row of length 129 alone (`twin`);
    per family S = 32 (a single chunk) and S = 2048 with lengths {2048, 1985}."""
    out = []
    for fam in FAMS:
        for H in hs(fam):
            out.append(dict(fam=fam, H=H, S=192, lens=list(LENS192), name=f"pool_{fam}_H{H}_S192"))
            out.append(dict(fam=fam, H=H, S=2048, lens=[129], twin=f"pool_{fam}_H{H}_S192", name=f"pool_{fam}_H{H}_twin"))
        out.append(dict(fam=fam, H=384, S=32, lens=[0, 1, 31, 32], name=f"pool_{fam}_H384_S32"))
        out.append(dict(fam=fam, H=768, S=2048, lens=[2048, 1985], name=f"pool_{fam}_H768_S2048"))
    for i, c in enumerate(out):
        c["eps"] = _eps(i)
        if "twin" in c:
            c["eps"] = out[i - 1]["eps"]
    return out


def pool_modes(c):
    """The launches on one case's input: (suffix, pooling, normalise)."""
    if c["fam"] == "dec":
        return [("last_n1", None, 1), ("last_n0", None, 0)]
    if c["fam"] == "gm":
        return [("mean", 0, None)]
    return [("mean_n1", 0, 1), ("mean_n0", 0, 0), ("cls_n1", 1, 1), ("cls_n0", 1, 0)]


def pool_inputs(c):
    """x [B][S][H] float32. Token t of row b is (-1)^t (a_b + noise) plus, for the LayerNorm family, the token's class offset: the rows
    alternate in sign, so a pooled mean is small against the sum of magnitudes. Token rows at or past the length are NaN; for the
    last-token pool every row but the pooled one. Lengths in STEEP: |mean| / std = 512. The last token of the length-2 row is zero."""
    if "twin" in c:
        base = next(b for b in pool_cases() if b["name"] == c["twin"])
        src = pool_inputs(base)
        x = np.full((1, c["S"], c["H"]), np.nan, np.float32)
        x[0, :192] = src["x"][TWIN_ROW]
        return dict(x=x, lens=np.array(c["lens"], np.int32), w=src["w"])
    rng = _rng(c)
    B, S, H = len(c["lens"]), c["S"], c["H"]
    x = np.empty((B, S, H), np.float32)
    sign = np.where(np.arange(S) % 2, -1.0, 1.0)[:, None]
    for b, n in enumerate(c["lens"]):
        sig = 2.0 ** int(rng.integers(-6, 7))
        a = rng.standard_normal(H) * sig
        rows = a[None, :] + 0.25 * sig * rng.standard_normal((S, H))
        if c["fam"] == "mb":
            rows += kc.row_offsets(S, sig) if n not in STEEP else 512.0 * sig
        xb = (sign * rows).astype(np.float32)
        if n == 2:
            xb[1] = 0.0
        xb[n:] = np.nan
        if c["fam"] == "dec" and n > 0:
            xb[:n - 1] = np.nan
        x[b] = xb
    g, = weights(rng, H)
    return dict(x=x, lens=np.array(c["lens"], np.int32), w=g)


# ---- dense, L2, fold -------------------------------------------------------------------------------------------------------------------
def dense_cases():
    """k_gm_dense: N in {4, 7, 768} (7: the n >= N guard), K in {128, 768, 3072}, B = 3."""
    return [dict(N=N, K=K, B=3, name=f"dense_N{N}_K{K}") for N in (4, 7, 768) for K in (128, 768, 3072)]


def dense_inputs(c):
    rng = _rng(c)
    x = rng.standard_normal((c["B"], c["K"])) * np.where(np.arange(c["K"]) % 2, -1.0, 1.0)
    w = rng.standard_normal((c["N"], c["K"])) / math.sqrt(c["K"])
    w[::3, 1::2] = w[::3, 0::2]          # against the alternating sign of x: sums that nearly cancel
    return dict(x=x.astype(np.float32), w=w.astype(np.float32))


def l2_cases():
    """k_gm_l2 at D in {128, 256, 768, 1000}, normalise on and off."""
    return [dict(D=D, normalise=nm, B=5, name=f"l2_D{D}_n{nm}") for D in (128, 256, 768, 1000) for nm in (1, 0)]


def l2_inputs(c):
    """Rows: N(0, 1); all zero; magnitude 2^-50 (under the 1e-12 floor: the scale is 1e12; its squares are normal numbers); N(0, 2^10);
    N(0, 2^-6) alternating in sign."""
    rng = np.random.default_rng(zlib.crc32(f"l2_D{c['D']}".encode()))          # the same rows with normalise on and off
    x = rng.standard_normal((5, c["D"]))
    x[1] = 0.0
    x[2] = 2.0 ** -50 * np.sign(x[2]) * (1.0 + 0.25 * rng.random(c["D"]))
    x[3] *= 2.0 ** 10
    x[4] *= 2.0 ** -6
    return dict(x=x.astype(np.float32))


FOLD_N = 1000


def fold_inputs():
    return dict(w=np.random.default_rng(zlib.crc32(b"fold1p")).standard_normal(FOLD_N).astype(np.float32))


# ---- k_gemm MODE 3 -----------------------------------------------------------------------------------------------------------------------
def gemm3_cases():
    """launch_gemm(3): the narrow tile at T = 512; the wide phased tile and the wide in-step loop (K < 192) at the T for which the
    launcher itself picks the wide tile."""
    def wide_T(N):
        return 256 * math.ceil(256 / (N // 256))
    out = [dict(T=512, N=640, K=128, tile="narrow"), dict(T=512, N=1152, K=1024, tile="narrow"),
           dict(T=wide_T(4096), N=4096, K=1024, tile="wide"), dict(T=wide_T(1024), N=1024, K=64, tile="wide")]
    for c in out:
        c.update(mode=3, name=f"gemm_m3_{c['tile']}_T{c['T']}_N{c['N']}_K{c['K']}")
    return out
