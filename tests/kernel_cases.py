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
    first and the last query head."""
    out = []
    for nq, nkv in ((1, 1), (2, 1), (4, 1), (16, 8), (32, 8)):
        for S in (32, 64, 256, 2048, 8192):
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
