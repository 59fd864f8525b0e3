"""The cases of the kernel-level tests (tests/test_kernels_gpu.py) and their inputs, built from a seed: the GPU worker
(tests/kernel_worker.py), the float64 references in the parent and the mutant tests on the CPU (tests/test_kernel_refs_cpu.py) all call
the same builders, so they see the same numbers.

Attention inputs: random bf16 q, k, v -- the logit spread alternates between flat (0.3) and peaked (3.0, base-2 domain) from one
(batch row, head) to the next -- plus SPIKE PROBES: a key whose logit against one chosen query dominates the row (2^14 against
the typical key) and whose v row is distinctive, placed at distance exactly w and w + 1 from first / last queries of a wave, a
workgroup and the row, on the causal diagonal and one past it, on the last real key and the first pad key, in a mask's holes. An
off-by-one in a band, a diagonal or a length then shows as an O(1) error, not as a statistical one. Pad rows of q, k and v hold
random finite numbers like the real rows: a pad key that is attended shows, a pad query must still come out finite.
Every valid query keeps at least one visible key (itself) and lengths lie in [0, S]: no case is outside its launcher's contract.
"""
import math
import zlib

import numpy as np

try:
    from tests import kernel_refs as kr
except ImportError:          # imported by the worker script, whose directory is tests/ itself
    import kernel_refs as kr

SPIKE = 14.0                 # base-2 logit of a probe key against its query
FLAT, PEAKED = 0.3, 3.0


def lengths_for(S):
    return sorted({n for n in (0, 1, 31, 32, 33, 127, 128, 129, S - 33, S - 1, S) if 0 <= n <= S})


def _seed(name):
    return zlib.crc32(name.encode())


# ---- case lists ------------------------------------------------------------------------------------------------------------------
def window_cases():
    """launch_attn_window. Every window at S = 544 and S = 2048, the small S at the windows around one and two 32-key blocks and at
    the three ways of saying `no band`, S = 8192 at w in {1, 64, 200, none}; every length in every case; heads 1, 2 and 16."""
    every = lambda S: [1, 2, 31, 32, 33, 63, 64, 65, 95, 127, 128, 129, 200, S - 1, S, -1]
    out = []
    for S, heads in ((544, 2), (2048, 1)):
        out += [dict(kernel="window", S=S, heads=heads, window=w) for w in every(S)]
    for i, S in enumerate((32, 64, 96, 128, 160, 512)):
        for w in (1, 2, 31, 32, 33, 64, S - 1, S, -1):
            out.append(dict(kernel="window", S=S, heads=(1, 2, 16)[i % 3], window=w))
    # S = 8192: all 16 heads are compared under a band (the reference is cheap there); without one the reference of a full row is
    # 13 GFLOP per head in float64, so that case runs 2 heads and compares both
    out += [dict(kernel="window", S=8192, heads=16, window=64), dict(kernel="window", S=8192, heads=2, window=1),
            dict(kernel="window", S=8192, heads=2, window=200), dict(kernel="window", S=8192, heads=2, window=-1)]
    for c in out:
        c.update(hd=64, mask="right", name=f"window_S{c['S']}_h{c['heads']}_w{c['window']}")
    return out


def long_cases():
    """launch_attn_long: right-padded at every S; one mask with holes and one left-padded (the kernel reads `mask` per key while
    `rowlen` bounds the walk)."""
    out = [dict(kernel="long", S=S, heads=2, mask="right") for S in (544, 1024, 4128, 8192)]
    out += [dict(kernel="long", S=1024, heads=2, mask="holes"), dict(kernel="long", S=4128, heads=1, mask="left"),
            dict(kernel="long", S=544, heads=16, mask="holes")]
    for c in out:
        c.update(hd=64, window=-1, name=f"long_S{c['S']}_h{c['heads']}_{c['mask']}")
    return out


def attn_cases():
    """launch_attn: S in {32, 64, 96, 256, 512} (4 / 8 / 16 waves), head size 32 token-major and head-major and head size 64, the three
    mask kinds, without the bias and with it at n_rel = S and n_rel = 512 (one value at S = 512): the full product."""
    out = []
    for S in (32, 64, 96, 256, 512):
        for hd, layout, heads in ((32, "token", 3), (32, "head", 3), (64, "token", 2)):
            for mask in ("right", "holes", "left"):
                for n_rel in sorted({0, S, 512}):
                    out.append(dict(kernel="attn", S=S, heads=heads, hd=hd, layout=layout, mask=mask, n_rel=n_rel, window=-1,
                                    name=f"attn_S{S}_hd{hd}{layout[0]}_{mask}_rel{n_rel}"))
    return out


def causal_cases():
    """launch_attn_causal: every (nq, nkv) at every S. At S = 8192 with 32 query heads the float64 reference of all heads is
    unaffordable beside the rest of the file (6 GFLOP per head and full row, three such rows): that case compares every row of the
    first and the last query head. (6, 2) is G = 3: three waves (192 threads, which do not divide the 512-chunk staging loop), at one
    key block, at the diagonal plus one block below and at several row blocks, with a neighbouring kv head for the GQA-map probe."""
    out = []
    for nq, nkv in ((1, 1), (2, 1), (4, 1), (16, 8), (32, 8), (6, 2)):
        for S in (32, 64, 256, 2048, 8192) if nq != 6 else (32, 64, 256):
            c = dict(kernel="causal", S=S, nq=nq, nkv=nkv, heads=nq, hd=128, mask="right", window=-1, name=f"causal_q{nq}_kv{nkv}_S{S}")
            if S == 8192 and nq >= 32:
                c["check_heads"] = [0, nq - 1]
            out.append(c)
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _mask_row(kind, S, n, rng):
    if kind == "right":
        return kr.mask_right(S, n)
    if kind == "left":
        return kr.mask_left(S, n)
    return kr.mask_holes(S, n, rng)


def effective_window(case):
    """None when the launcher runs without a band (window < 0 or >= S), else the half-width."""
    w = case.get("window", -1)
    return None if w < 0 or w >= case["S"] else w


def _probe_pairs(case, mask, b):
    """(query, key) pairs to spike in batch row b; the order rotates with b so that pairs that collide on a key in one row get their
    turn in another."""
    S = case["S"]
    valid = np.flatnonzero(mask)
    if valid.size == 0:
        return []
    first, last = int(valid[0]), int(valid[-1])
    qs = [first, first + 31, first + 32, first + 63, first + 64, first + 127, first + 128, first + 255, first + 256, last, last - 1, last - 31, last - 32,
          (first + last) // 2]
    pairs = []
    w = effective_window(case)
    if case["kernel"] == "causal":
        for q in qs:
            pairs += [(q, q), (q, q + 1)]
    elif w is not None:
        for q in qs:
            pairs += [(q, q + w), (q, q + w + 1), (q, q - w), (q, q - w - 1)]
        pairs += [(last, last + 1), (last - w + 1, last + 1)]
    else:
        for q in qs:
            pairs += [(q, last), (q, last + 1), (q, first - 1), (q, first)]
    holes = np.flatnonzero(~mask[first:last + 1]) + first
    if holes.size:                                          # a mask's holes: the first one, one of the whole-block hole, the last one
        pairs += [(first, int(holes[0])), (last, int(holes[len(holes) // 2])), (last, int(holes[-1]))]
    pairs = [(q, k) for q, k in pairs if 0 <= q < S and 0 <= k < S and mask[q]]
    r = b % len(pairs) if pairs else 0
    return pairs[r:] + pairs[:r]


def _probe_v(i, hd):
    d = np.arange(hd)
    return np.where(((d * (2 * i + 3)) >> 2) & 1, 3.0, -3.0).astype(np.float32) * (1.0 + 0.25 * (i % 3))


def attn_inputs(case):
    """q, k, v as bf16 bits in the logical layout [B][heads][S][hd] (causal: k, v [B][nkv][S][128]), mask [B][S] bool, rowlen [B]
    (one past the last real key), rel [heads][REL_ROW] float32 or None."""
    S, hd = case["S"], case["hd"]
    hq = case["heads"]
    hk = case.get("nkv", hq)
    G = hq // hk
    lens = lengths_for(S)
    B = len(lens)
    rng = np.random.default_rng(_seed(case["name"]))
    q = np.empty((B, hq, S, hd), np.uint16)
    k = np.empty((B, hk, S, hd), np.uint16)
    v = np.empty((B, hk, S, hd), np.uint16)
    mask = np.zeros((B, S), bool)
    rowlen = np.zeros(B, np.int32)
    for b, n in enumerate(lens):
        mask[b] = _mask_row(case["mask"], S, n, rng)
        nz = np.flatnonzero(mask[b])
        rowlen[b] = nz[-1] + 1 if nz.size else 0
        sigma = np.where((b + np.arange(hq)) % 2 == 0, FLAT, PEAKED).astype(np.float32) / math.sqrt(hd)
        qb = kr.bf16_round(rng.standard_normal((hq, S, hd), dtype=np.float32) * sigma[:, None, None])
        kb = rng.standard_normal((hk, S, hd), dtype=np.float32)
        vb = rng.standard_normal((hk, S, hd), dtype=np.float32)
        taken = set()
        for i, (qi, kj) in enumerate(_probe_pairs(case, mask[b], b)):
            h = i % hq
            g = h // G
            if (g, kj) in taken:
                continue
            taken.add((g, kj))
            qv = qb[h, qi].astype(np.float64)
            kb[g, kj] = (qv * (SPIKE / max(float(qv @ qv), 1e-12))).astype(np.float32)
            vb[g, kj] = _probe_v(i, hd)
        q[b], k[b], v[b] = kr.bf16_bits(qb), kr.bf16_bits(kb), kr.bf16_bits(vb)
    rel = None
    if case.get("n_rel"):
        # per-distance bias, base-2 domain, N(0, 2) inside |d| < n_rel and zero outside; not symmetric in d
        rel = np.zeros((hq, kr.REL_ROW), np.float32)
        d = np.arange(-kr.REL_MID, kr.REL_ROW - kr.REL_MID)
        inside = np.abs(d) < case["n_rel"]
        rel[:, inside] = rng.standard_normal((hq, int(inside.sum())), dtype=np.float32) * 2.0
    return dict(q=q, k=k, v=v, mask=mask, rowlen=rowlen, rel=rel, lens=np.array(lens, np.int32))


def visibility(case, mask_row):
    return kr.Visibility(mask_row, window=effective_window(case), causal=case["kernel"] == "causal")


def head_slices(case, inp, b, h):
    """float32 values q [S][hd], k, v of query head h (its kv head under grouped-query attention: h // G)."""
    g = h // (case["heads"] // case.get("nkv", case["heads"]))
    return kr.bf16_value(inp["q"][b, h]), kr.bf16_value(inp["k"][b, g]), kr.bf16_value(inp["v"][b, g])


def check_attention(case, inp, ctx_bits, worst, ref=None):
    """Every valid query row of every head (or of case['check_heads']) of ctx [B][S][heads * hd] against the float64 reference;
    every other row must be finite. `ref`: a dict that caches (out, bound) per (b, h) across kernels run on the same inputs."""
    S, hd, hq = case["S"], case["hd"], case["heads"]
    ctx = kr.bf16_value(ctx_bits).reshape(len(inp["lens"]), S, hq * hd)
    for b in range(ctx.shape[0]):
        valid = np.flatnonzero(inp["mask"][b])
        pad = np.ones(S, bool)
        pad[valid] = False
        assert np.isfinite(ctx[b][pad]).all(), f"{case['name']}: batch row {b} has a non-finite pad row"
        if valid.size == 0:
            continue
        n = int(inp["rowlen"][b])
        vis = visibility(case, inp["mask"][b])
        for h in case.get("check_heads", range(hq)):
            if ref is not None and (b, h) in ref:
                out, bound = ref[(b, h)]
            else:
                qh, kh, vh = head_slices(case, inp, b, h)
                bias = kr.rel_bias_dense(inp["rel"][h], S)[:n] if inp["rel"] is not None else None
                out, out_abs = kr.attention_ref(qh[:n], kh, vh, vis, bias)
                bound = kr.attention_bound(qh[:n], kh, out, out_abs, float(np.abs(inp["rel"][h]).max()) if inp["rel"] is not None else 0.0)
                out, bound = out[valid], bound[valid]
                if ref is not None:
                    ref[(b, h)] = (out, bound)
            worst.add(ctx[b, valid, h * hd:(h + 1) * hd], out, bound, case["name"], b, h, rows=valid)


# ---- GEMM ------------------------------------------------------------------------------------------------------------------------
def gemm_cases():
    """launch_gemm. Each mode on the narrow tile (T = 512) and at a T for which the launcher itself picks the wide tile
    ((T / 256) (N / 256) >= 256, N % 256 == 0); the K list spread over them (192 is where the phased loop of the wide tile starts: K = 64
    and 128 run its in-step loop); MODE 8 at the padded 2 I = 5376 and at an N that is a multiple of 128 only; MODE 0 at H % 256 == 0
    (narrow and wide) and != 0, with a batch whose real tokens end before the padded T."""
    def wide_T(N):
        return 256 * math.ceil(256 / (N // 256))
    out = []
    narrow = [(0, 1152, 384), (0, 768, 64), (1, 384, 128), (1, 1536, 1152), (2, 384, 192), (2, 128, 4096), (4, 640, 768), (4, 384, 2688),
              (7, 512, 1024), (7, 1280, 64), (8, 640, 384), (8, 5376, 192)]
    for mode, N, K in narrow:
        out.append(dict(mode=mode, T=512, N=N, K=K, tile="narrow"))
    wide = [(0, 768, 768), (0, 3072, 128), (1, 3072, 768), (1, 1024, 64), (2, 768, 3072), (2, 1024, 128), (4, 768, 192), (4, 1024, 1024),
            (7, 2048, 1024), (7, 6144, 64), (8, 5376, 1152), (8, 2304, 768)]
    for mode, N, K in wide:
        out.append(dict(mode=mode, T=wide_T(N), N=N, K=K, tile="wide"))
    out.append(dict(mode=2, T=wide_T(768), N=768, K=4096, tile="wide"))
    out.append(dict(mode=1, T=wide_T(1536), N=1536, K=2688, tile="wide"))
    for c in out:
        if c["mode"] == 0:
            c["H"] = c["N"] // 3
            c["S"] = 128
            c["ldo"] = c["T"] - 160            # the last 160 padded token rows have no V^T slot (one whole sequence and a 32-token block)
        c["name"] = f"gemm_m{c['mode']}_{c['tile']}_T{c['T']}_N{c['N']}_K{c['K']}"
    return out


def gemm_tile_is_wide(c):
    """The launcher's own rule (gemm.hip launch_gemm), restated so that the case list can be checked against its intent on the CPU."""
    wide = c["N"] % 256 == 0 and (c["T"] // 256) * (c["N"] // 256) >= 256 and (c["mode"] != 0 or c["H"] % 256 == 0)
    if c["mode"] == 8 and c["K"] < 192:
        wide = False
    return wide


def qscale(c):
    return math.log2(math.e) / 8.0               # log2(e) / sqrt(64): what the encoder hands MODE 0 at head size 64


SENTINEL = 12288.0           # bf16-exact; prefilled where a kernel must not write


def vt_expected(c, v_want, v_bound, pos=None, ldo=None):
    """The V^T buffer [T / S][H][S] of a QKV case from token-major v [T][H]: key s of a sequence at pos[s] (vt_pos order), the
    sentinel (bound 0) in the slots of the padded tokens t >= ldo."""
    S, H, T = c["S"], c["H"], c["T"]
    ldo = c["ldo"] if ldo is None else ldo
    pos = kr.vt_pos(np.arange(S)) if pos is None else pos
    want = np.full((T // S, H, S), SENTINEL)
    bound = np.zeros_like(want)
    real = (np.arange(T) < ldo).reshape(T // S, S)
    vw = v_want.reshape(T // S, S, H).transpose(0, 2, 1)
    vb = v_bound.reshape(T // S, S, H).transpose(0, 2, 1)
    for b in range(T // S):
        r = np.flatnonzero(real[b])
        want[b][:, pos[r]] = vw[b][:, r]
        bound[b][:, pos[r]] = vb[b][:, r]
    return want, bound


def gemm_expect(c, inp, y, y_abs):
    """{output name: (want, bound)} of one launch_gemm case from the float64 product, token-major (MODE 0: q, k, v)."""
    K, mode = c["K"], c["mode"]
    if mode == 0:
        q, k, v = kr.qkv_split(y, y_abs, K, c["H"], qscale(c))
        return {"q": q, "k": k, "v": v}
    if mode == 1:
        return {"out": kr.epi_gelu(y, y_abs, K, table=c["tile"] == "wide")}
    if mode == 2:
        return {"out": kr.epi_f32(y, y_abs, K)}
    if mode == 4:
        return {"out": kr.epi_residual_bf16(y, y_abs, K, kr.bf16_value(inp["res"]))}
    if mode == 7:
        return {"out": kr.epi_swiglu(y, y_abs, K)}
    return {"out": kr.epi_geglu(y, y_abs, K)}


def gemm_inputs(c):
    """x [T][K], w [N][K] as bf16 bits, bias [N] float32, res [T][N] bf16 bits (MODE 4). A few rows of x are 64 times larger and
    the weights of some columns nearly cancel against them, so that y is small where y_abs is large."""
    rng = np.random.default_rng(_seed(c["name"]))
    T, N, K = c["T"], c["N"], c["K"]
    x = rng.standard_normal((T, K), dtype=np.float32)
    big = rng.choice(T, size=max(2, T // 64), replace=False)
    x[big] *= 64.0
    w = rng.standard_normal((N, K), dtype=np.float32) / np.float32(math.sqrt(K))
    w[::7, 1::2] = -w[::7, 0::2]               # with x[big, 1::2] = x[big, 0::2] below: exact cancellation pairs in the float64 sum
    x[big[::2], 1::2] = x[big[::2], 0::2]
    bias = rng.standard_normal(N, dtype=np.float32)
    out = dict(x=kr.bf16_bits(x), w=kr.bf16_bits(w), bias=bias)
    if c["mode"] == 4:
        out["res"] = kr.bf16_bits(rng.standard_normal((T, N), dtype=np.float32) * 2.0)
    return out


def skinny_cases():
    out = []
    for rows in (32, 64):
        for K in (384, 1024):          # the 4-wave (K < 1024) and the 8-wave branch
            out.append(dict(kind="f32", rows=rows, N=384, K=K))
            out.append(dict(kind="gelu", rows=rows, N=1536, K=K))
            out.append(dict(kind="qkv", rows=rows, N=3 * 384, K=K, H=384, S=32, Treal=rows - 32 if rows > 32 else rows))
    for c in out:
        c.update(T=c["rows"], mode=-1, name=f"skinny_{c['kind']}_r{c['rows']}_K{c['K']}")
    return out


# ---- the LayerNorm-fused kernels ---------------------------------------------------------------------------------------------------
LN_H = 384
CLASSES = (0, 4, 32)         # |mean| / std of the rows, about: token t is of class CLASSES[t % 3]


def ln_params(rng, H, n=1):
    """n (gamma, beta) pairs: gamma ~ N(1, 0.3) with a few entries exactly 0 and a few negative, beta ~ N(0, 0.5), float32."""
    out = []
    for i in range(n):
        g = (1.0 + 0.3 * rng.standard_normal(H)).astype(np.float32)
        g[[3 + i, 77 + i, H - 56 - i]] = 0.0
        neg = [5 + i, 130 + i, H - 1 - i]
        g[neg] = -np.abs(g[neg])
        out.append((g, (0.5 * rng.standard_normal(H)).astype(np.float32)))
    return out


def row_offsets(T, sigma):
    """Per-token offsets that put token t at |mean| / std of about CLASSES[t % 3] for rows of standard deviation sigma."""
    return (np.array(CLASSES, np.float64)[np.arange(T) % 3] * sigma)[:, None] * np.where(np.arange(T) % 2, -1.0, 1.0)[:, None]


def ratio_class(ratio):
    """0 / 1 / 2: the class of a row by its |mean| / std (< 2, < 16, the rest)."""
    return (np.asarray(ratio) >= 2.0).astype(int) + (np.asarray(ratio) >= 16.0).astype(int)


def flat_row(T):
    return T // 2 + 1        # the row of near-zero variance


def gemm_ln_cases():
    """launch_gemm_ln: every K-step count around the 4-slot ring (K / 32 = 1, 2, 3, 4, 5) and the product's two, one tile and
    three, both residual forms; 257 tiles, the first count at which a workgroup of the 256-workgroup grid runs a second tile. eps
    alternates between BERT's 1e-12 and 1e-5."""
    out = [dict(T=T, K=K, res=res) for K in (32, 64, 96, 128, 160, 384, 1536) for T in (128, 384) for res in ("f32", "bf16")]
    out += [dict(T=257 * 128, K=384, res=res) for res in ("f32", "bf16")]
    for i, c in enumerate(out):
        c.update(N=LN_H, mode=-1, eps=(1e-12, 1e-5)[(i // 2) % 2], name=f"gemmln_{c['res']}_T{c['T']}_K{c['K']}")
    return out


def gemm_ln_tiles_per_workgroup(c):
    """launch_gemm_ln's grid rule (gemm_ln.hip), restated: 128-token tiles over at most 256 persistent workgroups."""
    ntiles = c["T"] // 128
    return -(-ntiles // min(ntiles, 256))


def gemm_ln_inputs(c):
    """gemm_inputs' x, w, bias at N = 384 (large rows, cancellation pairs) plus gamma, beta and the residual rows: N(0, 2) plus the
    class offset of the token; the flat row has x = 0 and res = 2^-10 + a few units of 2^-22 - bias, so that bias + res is constant up to that and the residual's
    format (float32: a variance of 2e-13, a fifth of BERT's eps; bf16: 2e-6, eps-dominated at eps = 1e-5)."""
    inp = gemm_inputs(c)
    rng = np.random.default_rng(_seed(c["name"] + "/ln"))
    T = c["T"]
    (g, b), = ln_params(rng, LN_H)
    res = rng.standard_normal((T, LN_H)) * 2.0 + row_offsets(T, 2.5)
    x = kr.bf16_value(inp["x"]).copy()
    x[flat_row(T)] = 0.0
    res[flat_row(T)] = 2.0 ** -10 + 2.0 ** -22 * rng.integers(-3, 4, LN_H) - inp["bias"].astype(np.float64)
    res = res.astype(np.float32)
    inp.update(x=kr.bf16_bits(x), gamma=g, beta=b, res=kr.bf16_round(res) if c["res"] == "bf16" else res)
    return inp


# stand-alone LayerNorms of encoder.hip: (kernel, input rows, residual, float32 output too) as the forward pass combines them
LN_FORMS = [("layernorm", "f32", "f32", True), ("layernorm", "f32", "bf16", False), ("layernorm", "bf16", None, False),
            ("layernorm16", "bf16", None, False), ("ln_apply16", "lazy", None, False)]


def layernorm_cases():
    """k_layernorm (4 rows per workgroup: T = 1, 5, 127, 512 leave 1, 1, 3, 0 waves of the last workgroup with a row),
    k_layernorm16 (2 rows per wave), k_ln_apply16 (one 8-feature run per lane) at H = 384, 768, 1024."""
    out = []
    for H in (384, 768, 1024):
        for T in (1, 5, 127, 512):
            for kern, xin, res, y32 in LN_FORMS:
                out.append(dict(kernel=kern, H=H, T=T, xin=xin, res=res, y32=y32, eps=1e-12 if H != 768 else 1e-5,
                                name=f"{kern}_{xin}_{res}_H{H}_T{T}"))
    return out


def layernorm_inputs(c):
    """x: N(0, 1) rows with a few 64 times larger; res: N(0, 2) plus the class offset (without a residual the offset goes into x);
    the flat row is a few units of 2^-22 (its variance a fifth of BERT's eps); `lazy`: the true rows r in float64, what travels is kr.lazy_rows / kr.stats_f32."""
    rng = np.random.default_rng(_seed(c["name"]))
    T, H = c["T"], c["H"]
    (g, b), = ln_params(rng, H)
    x = rng.standard_normal((T, H))
    x[rng.choice(T, size=max(1, T // 64), replace=False)] *= 64.0
    res = None
    if c["res"]:
        res = rng.standard_normal((T, H)) * 2.0 + row_offsets(T, 2.3)
    else:
        x = x + row_offsets(T, 1.0)
    if T > 2:
        x[flat_row(T)] = 2.0 ** -22 * rng.integers(-3, 4, H)          # bf16-exact, variance 2e-13: eps decides
        if res is not None:
            res[flat_row(T)] = 0.0
    rnd = {"f32": lambda a: a.astype(np.float32), "bf16": lambda a: kr.bf16_round(a.astype(np.float32)), "lazy": lambda a: a}
    return dict(x=rnd[c["xin"]](x), res=None if res is None else rnd[c["res"]](res), gamma=g, beta=b)


def qkv384_cases(forced=False):
    """launch_qkv384: S = 32, 128, 512 at one and three 128-token tiles (S = 512: the two smallest Tpad a sequence fits), all rows real
    and the last S + 32 rows padding (where that leaves a token), token- and head-major; Tpad = 258 * 128, where the launcher
    itself picks k_qkv384<2>. forced: the cases of the child that runs under AK_QKV_TG=2 (256 tokens per workgroup at Tpad = 256)."""
    out = []
    shapes = [(256, 32), (256, 128)] if forced else [(128, 32), (384, 32), (128, 128), (384, 128), (512, 512), (1024, 512), (258 * 128, 128)]
    for Tpad, S in shapes:
        for T in sorted({Tpad, Tpad - S - 32}):
            if T <= 0:
                continue
            for hm in (0, 1):
                out.append(dict(T=Tpad, Treal=T, S=S, H=LN_H, N=3 * LN_H, K=LN_H, mode=0, head_major=hm, tg=2 if forced else qkv384_tg(Tpad),
                                name=f"qkv384{'_tg2' if forced else ''}_T{Tpad}_S{S}_real{T}_{'head' if hm else 'token'}"))
    return out


def qkv384_tg(Tpad):
    """launch_qkv384's own rule (ffn.hip), restated: 32 tokens per wave once there are more 128-token tiles than CUs."""
    return 2 if Tpad % 256 == 0 and Tpad // 128 > 256 else 1


def qscale32():
    return math.log2(math.e) / math.sqrt(32.0)          # the hidden-384 path: 12 heads of 32


def head_major_expected(c, want, bound):
    """Token-major [Tpad][384] -> [Tpad / S][12][S][32] with the sentinel (bound 0) in the rows of tokens >= Treal."""
    Tp, S = c["T"], c["S"]
    real = (np.arange(Tp) < c["Treal"])[:, None]
    w = np.where(real, want, SENTINEL).reshape(Tp // S, S, 12, 32).transpose(0, 2, 1, 3)
    b = np.where(real, bound, 0.0).reshape(Tp // S, S, 12, 32).transpose(0, 2, 1, 3)
    return np.ascontiguousarray(w).reshape(-1, 32), np.ascontiguousarray(b).reshape(-1, 32)


def ffn384_cases(child="default"):
    """launch_ffn384. default: with the fused out-projection at I = 64 (the smallest ffn_fused_supported takes) and 1536, T = 128,
    256, 384 (the half-tile kernel k_ffn384w8<true, 4> by the launcher's own rule) and T = 129 * 128, the first T at which it
    launches the role kernel k_ffn384r; the ctx-less form at T = 256. nwv8 (AK_FFN_NWV=8): the role kernel at T = 128, 384.
    w4 (AK_FFN_W8=0): the 4-wave generation, ctx-less, T = 256."""
    if child == "default":
        out = [dict(T=T, I=I, ctx=True) for I in (64, 1536) for T in (128, 256, 384)]
        out += [dict(T=129 * 128, I=1536, ctx=True), dict(T=256, I=1536, ctx=False)]
    elif child == "nwv8":
        out = [dict(T=T, I=1536, ctx=True) for T in (128, 384)]
    else:
        out = [dict(T=256, I=1536, ctx=False)]
    for c in out:
        c.update(kernel=ffn384_kernel(c, child), eps=1e-12, name=f"ffn384_{child}_T{c['T']}_I{c['I']}_{'ctx' if c['ctx'] else 'noctx'}")
    return out


def ffn384_kernel(c, child="default"):
    """launch_ffn384's selection (ffn.hip), restated: half tiles while 2 ntiles <= 256 (AK_FFN_NWV forces), else the role kernel."""
    if child == "w4":
        return "k_ffn384"
    half = child != "nwv8" and 2 * (c["T"] // 128) <= 256
    if not c["ctx"]:
        return "k_ffn384w8<false, 4>" if half else "k_ffn384w8<false>"
    return "k_ffn384w8<true, 4>" if half else "k_ffn384r"


def ffn384_table_gelu(c):
    return c["kernel"] == "k_ffn384r"


def ffn384_inputs(c):
    """The layer's input rows x (N(0, 1) plus the class offset: LayerNorm-1 sees rows of every class), the attention output ctx
    (gemm_inputs' large rows and cancellation pairs against Wo), weights N(0, 1 / K), every bias and two (gamma, beta) pairs."""
    rng = np.random.default_rng(_seed(c["name"]))
    T, I, H = c["T"], c["I"], LN_H
    a = gemm_inputs(dict(name=c["name"] + "/wo", T=T, N=H, K=H, mode=-1))
    (g1, be1), (g2, be2) = ln_params(rng, H, 2)
    x = rng.standard_normal((T, H)) * 1.5 + row_offsets(T, 2.0)
    x[flat_row(T)] = 0.125
    w1 = rng.standard_normal((I, H), dtype=np.float32) / np.float32(math.sqrt(H))
    w2 = rng.standard_normal((H, I), dtype=np.float32) / np.float32(math.sqrt(I))
    b1 = rng.standard_normal(I, dtype=np.float32)
    p = dict(wo=kr.bf16_value(a["w"]), bo=a["bias"], g1=g1, be1=be1, w1=kr.bf16_round(w1), b1=b1,
             w2=kr.bf16_round(w2), b2=rng.standard_normal(H, dtype=np.float32), g2=g2, be2=be2)
    return dict(x=kr.bf16_round(x.astype(np.float32)), ctx=kr.bf16_value(a["x"]) if c["ctx"] else None, p=p)


def compare_rows(T, tile, seed):
    """The token rows a large case is compared on: whole tiles -- the first, the last, those on either side of the 127 / 128 and
    255 / 256 tile boundaries (the grid and selection thresholds) and eight seeded random ones; every row at T <= 1024."""
    if T <= 1024:
        return np.arange(T)
    nt = T // tile
    rng = np.random.default_rng(seed)
    tiles = {0, nt - 1} | {t for t in (126, 127, 128, 129, 254, 255, 256, 257) if t < nt} | set(rng.choice(nt, size=8, replace=False).tolist())
    return np.concatenate([np.arange(t * tile, (t + 1) * tile) for t in sorted(tiles)])


def lazy_cases(forced=True):
    """launch_gemm_lazy. forced (the child under AK_ENC_LAZYLN=2), T = 256: MODE 0 and 1 at bge-base's shapes and at the smallest K the
    tile takes beside 192, MODE 4 with the residual finished on the way (res_stats) and added as it is. Not forced: MODE 4 at
    N = 768, T = 43 * 256, the first T at which gemm_lazy_supported says yes by itself (43 * 3 = 129 >= LAZY_MIN_TILES = 128)."""
    out = []
    if forced:
        out += [dict(mode=0, T=256, N=N, K=K) for N, K in ((2304, 768), (768, 256))]
        out += [dict(mode=1, T=256, N=N, K=K) for N, K in ((3072, 768), (1024, 256))]
        out += [dict(mode=4, T=256, N=N, K=K, res_stats=rs) for N, K in ((768, 768), (768, 3072), (256, 192)) for rs in (True, False)]
    else:
        out += [dict(mode=4, T=43 * 256, N=768, K=768, res_stats=True)]
    for c in out:
        c.update(eps=1e-12, name=f"lazy_m{c['mode']}_T{c['T']}_N{c['N']}_K{c['K']}" + ("" if c["mode"] != 4 else "_stats" if c["res_stats"] else "_plain"))
        if c["mode"] == 0:
            c.update(H=c["N"] // 3, S=128, ldo=c["T"] - 160, tile="wide")
    return out


def lazy_tile_selected(c, forced):
    """launch_gemm_lazy's shape rule (gemm.hip), restated: the wide phased tile, and at least LAZY_MIN_TILES = 128 of them unless forced."""
    ok = c["T"] % 256 == 0 and c["N"] % 256 == 0 and c["K"] % 64 == 0 and c["K"] >= 192 and (c["mode"] != 0 or c["H"] % 256 == 0)
    return ok and (forced or (c["T"] // 256) * (c["N"] // 256) >= 128)


def lazy_inputs(c):
    """MODE 0 / 1: the true rows r [T][K] (N(0, 1.5) plus class offsets, large rows, a flat row), their LayerNorm's gamma / beta, W, b.
    MODE 4: x (gemm_inputs), W, b, the gamma the output is scaled by and the residual: true rows r_prev with gamma / beta of their
    LayerNorm (res_stats) or plain bf16 rows."""
    rng = np.random.default_rng(_seed(c["name"]))
    T, N, K = c["T"], c["N"], c["K"]
    a = gemm_inputs(dict(name=c["name"] + "/gemm", T=T, N=N, K=K, mode=-1))
    out = dict(w=kr.bf16_value(a["w"]), bias=a["bias"])
    if c["mode"] != 4:
        (g, b), = ln_params(rng, K)
        r = kr.bf16_value(a["x"]).astype(np.float64) * 1.5 + row_offsets(T, 1.5)
        r[flat_row(T)] = 0.125
        out.update(r=r, gamma=g, beta=b)
        return out
    (g, b), (og, _) = ln_params(rng, N, 2)
    rp = rng.standard_normal((T, N)) * 2.0 + row_offsets(T, 2.0)
    rp[rng.choice(T, size=max(2, T // 64), replace=False)] *= 64.0
    rp[flat_row(T)] = 0.125
    out.update(x=kr.bf16_value(a["x"]), out_g=og, r_prev=rp, gamma=g, beta=b, res_rows=kr.bf16_round(rp.astype(np.float32)))
    return out


def ln_finalize_cases():
    return [dict(nslot=n, T=T, eps=1e-12 if n != 6 else 1e-5, name=f"lnfin_n{n}_T{T}") for n in (2, 3, 6, 8) for T in (1, 255, 256, 11008)]


def ln_finalize_inputs(c):
    """Partial sums [nslot][T][2] (float32) of rows of every class, large rows and a constant row among them."""
    rng = np.random.default_rng(_seed(c["name"]))
    T, n = c["T"], c["nslot"] * 128
    r = rng.standard_normal((T, n)) * 2.0 + row_offsets(T, 2.0)
    r[rng.choice(T, size=max(1, T // 64), replace=False)] *= 64.0
    if T > 2:
        r[flat_row(T)] = 0.125
    return kr.slice_sums_ref(r, 0.0)[0].astype(np.float32)


def fold_ln_cases():
    return [dict(N=N, K=K, name=f"fold_N{N}_K{K}") for N, K in ((2304, 768), (768, 256), (3072, 768), (1024, 256), (768, 3072), (256, 192))]


def fold_ln_inputs(c):
    rng = np.random.default_rng(_seed(c["name"]))
    (g, b), = ln_params(rng, c["K"])
    w = kr.bf16_round(rng.standard_normal((c["N"], c["K"]), dtype=np.float32) / np.float32(math.sqrt(c["K"])))
    return dict(w=w, gamma=g, beta=b, bias=rng.standard_normal(c["N"], dtype=np.float32))


# ---- what the LayerNorm-fused cases expect ------------------------------------------------------------------------------------------
def ln_rows(c, inp):
    """(r, dr, lazy) of a stand-alone LayerNorm case: the float64 pre-norm row and the bound of the kernel's own add."""
    x = np.asarray(inp["x"], np.float64)
    if inp["res"] is None:
        return x, 0.0
    r = x + inp["res"].astype(np.float64)
    return r, kr.E32 * np.abs(r)


def layernorm_expect(c, inp):
    """(out, bound32, bound16, parts) of a stand-alone LayerNorm case."""
    r, dr = ln_rows(c, inp)
    out, parts = kr.layernorm_ref(r, inp["gamma"], inp["beta"], c["eps"])
    if c["xin"] == "lazy":
        b = kr.lazy_ln_bound(r, inp["gamma"], out, parts)
        return out, b, b + kr.U * np.abs(out), parts
    b32 = kr.layernorm_bound(r, dr, inp["gamma"], out, parts, False)
    return out, b32, b32 + kr.U * np.abs(out), parts


def qkv384_expect(c, inp):
    """{q, k: (want, bound) in the case's layout, vt: (want, bound)} of a launch_qkv384 case."""
    y, y_abs = kr.gemm_ref(kr.bf16_value(inp["x"]), kr.bf16_value(inp["w"]), inp["bias"])
    return qkv384_layout(c, *kr.qkv_split(y, y_abs, c["K"], c["H"], qscale32()))


def qkv384_layout(c, q, k, v):
    out = {"vt": tuple(a.reshape(-1, c["S"]) for a in vt_expected(c, *v, ldo=c["Treal"]))}
    for name, (want, bound) in (("q", q), ("k", k)):
        out[name] = head_major_expected(c, want, bound) if c["head_major"] else (want, bound)
    return out


def lazy_expect(c, inp):
    """{output: (want, bound)} of a launch_gemm_lazy case and the LnParts that class its rows."""
    if c["mode"] != 4:
        y, dy, y_abs, parts = kr.lazy_a_ref(inp["r"], inp["gamma"], inp["beta"], c["eps"], inp["w"], inp["bias"])
        return lazy_epilogue(c, y, dy), parts
    prev = (inp["r_prev"], inp["gamma"], inp["beta"], c["eps"]) if c["res_stats"] else None
    r, dr, stored, bound = kr.lazy_mode4_ref(inp["x"], inp["w"], inp["bias"], inp["out_g"], res_rows=inp["res_rows"], prev=prev)
    sums, sb = kr.slice_sums_ref(r, dr)
    return {"out": (stored, bound), "stats": (sums.reshape(-1, 2), sb.reshape(-1, 2))}, kr.layernorm_ref(r, inp["out_g"], 0.0 * inp["out_g"], c["eps"])[1]


def lazy_epilogue(c, y, dy):
    """The epilogues of MODE 0 (q scaled, k, v: bf16 stores) and MODE 1 (table GELU of the wide tile) over a pre-epilogue bound dy."""
    if c["mode"] == 1:
        g = kr.gelu64(y)
        return {"out": (g, 1.13 * dy + 1.02 * (1.13 * kr.U * np.abs(y) + kr.U * np.abs(g)) + 2.0 ** -15)}
    H, s = c["H"], qscale(c)
    q = (y[:, :H] * s, s * dy[:, :H] + (kr.U + kr.E32) * np.abs(y[:, :H] * s))
    return {"q": q, "k": (y[:, H:2 * H], dy[:, H:2 * H] + kr.U * np.abs(y[:, H:2 * H])), "v": (y[:, 2 * H:], dy[:, 2 * H:] + kr.U * np.abs(y[:, 2 * H:]))}
