"""The cases of the Mistral / Llama kernel-level tests (tests/test_llama_kernels_gpu.py) and their inputs, built from a seed, in the
manner of tests/kernel_cases.py: the GPU worker (tests/llama_kernel_worker.py), the float64 references in the parent and the mutant
tests on the CPU (tests/test_llama_cpu.py) all call the same builders, so they see the same numbers.

Attention (launch_attn_causal with CausalAttnArgs::window = w): key <= query and query - key <= w - 1, which is
kernel_refs.Visibility(causal=True, window=w - 1). Inputs as kernel_cases.attn_inputs builds them (random bf16 q, k, v, flat and peaked
logit spreads, pad rows random and finite) with SPIKE PROBES of this mask: a key at distance w - 1 (visible) and w (hidden) from the
first / last queries of a wave, a workgroup and the row; on the diagonal and one past it (for the last real query that is the first
pad key); and a visible key of the NEIGHBOURING kv head spiked against a query of this one (a wrong grouped-query map sees it).
Every case runs the five lengths S, S - 1, a mid-block one, 1 and 0.
Bidirectional cases (CausalAttnArgs::bidirectional: every key below the row's length, the window ignored) spike a key ABOVE the diagonal
(it must be seen), the last real and the first pad key, key 0 and a key of the neighbouring kv head.

k_ll_rope: q | k | v rows of every G at S = 32, 96, 192, two sequences, tables of theta 1e4 as float32. The mean pool: pool_cases."""
import math

import numpy as np

try:
    from tests import kernel_cases as kc
    from tests import kernel_refs as kr
except ImportError:          # imported by the worker script, whose directory is tests/ itself
    import kernel_cases as kc
    import kernel_refs as kr

HD = 128
GROUPS = {1: (2, 2), 2: (4, 2), 3: (6, 2), 4: (8, 2)}       # G -> (nq, nkv): two kv heads, so that a neighbouring one exists
WINDOWS = (1, 31, 32, 33, 64, 100)
SENT = kc.SENTINEL
GUARD = 3                    # rows behind an output that must keep the sentinel


def lengths_for(S):
    return [S, S - 1, (S // 2 // 32) * 32 + 13, 1, 0]


def attn_cases():
    """G in {1, 2, 3, 4} x S in {96, 160} x every window; S = 32, 64 (one and two key blocks; w = 100 >= S hides nothing) and 288 (nine
    blocks, nine workgroups per kv head) at G = 4; S = 2048 at G = 4 with w = 1000 (a band
    edge that is not a multiple of 32, 33 of 64 blocks walked by the last workgroup)."""
    out = []
    for G in (1, 2, 3, 4):
        for S in (96, 160):
            out += [dict(G=G, S=S, window=w) for w in WINDOWS]
    for S in (32, 64, 288):
        out += [dict(G=4, S=S, window=w) for w in (31, 100)]
    out.append(dict(G=4, S=2048, window=1000))
    # bidirectional (every key below the length; the window argument is ignored): the same G x S, and S = 2048 once
    for G in (1, 2, 3, 4):
        out += [dict(G=G, S=S, window=0, bidir=True) for S in (96, 160)]
    out.append(dict(G=4, S=2048, window=0, bidir=True))
    for c in out:
        nq, nkv = GROUPS[c["G"]]
        c.setdefault("bidir", False)
        tag = "bidir" if c["bidir"] else f"w{c['window']}"
        c.update(kernel="causal", nq=nq, nkv=nkv, heads=nq, hd=HD, name=f"llattn_g{c['G']}_S{c['S']}_{tag}")
    return out


def equal_cases():
    """Two of kernel_cases.causal_cases, run through launch_attn_causal as Qwen3 calls it and through the window argument at 0: bit for bit."""
    want = {"causal_q6_kv2_S64", "causal_q16_kv8_S256"}
    return [c for c in kc.causal_cases() if c["name"] in want]


def _probe_pairs(case, n, b):
    """(query, key, other_head) triples to spike in a row of length n; the order rotates with b."""
    S, w = case["S"], case["window"]
    if n <= 0:
        return []
    last = n - 1
    if case.get("bidir"):
        # a key ABOVE the diagonal (it must be seen), the last real key and the first pad key, key 0, the neighbouring kv head
        qs = [0, 31, 32, 63, 64, last, last - 1, last - 32, last // 2]
        pairs = []
        for q in qs:
            pairs += [(q, q + 1, False), (q, last, False), (q, last + 1, False), (q, min(q + 33, last), False), (q, 0, False)]
        pairs += [(0, last, True), (last // 2, min(last // 2 + 1, last), True)]
        pairs = [(q, k, o) for q, k, o in pairs if 0 <= q < n and 0 <= k < S]
        r = b % len(pairs) if pairs else 0
        return pairs[r:] + pairs[:r]
    qs = [0, 31, 32, 63, 64, 127, 128, last, last - 1, last - 31, last - 32, last // 2, w - 1, w, w + 31, w + 32]
    pairs = []
    for q in qs:
        pairs += [(q, q - (w - 1), False), (q, q - w, False), (q, q, False), (q, q + 1, False)]
    pairs += [(last, max(last - (w - 1), 0), True), (last // 2, last // 2, True)]
    pairs = [(q, k, o) for q, k, o in pairs if 0 <= q < n and 0 <= k < S]
    r = b % len(pairs) if pairs else 0
    return pairs[r:] + pairs[:r]


def attn_inputs(case):
    """q [B][nq][S][128], k, v [B][nkv][S][128] as bf16 bits, lens [B], mask [B][S]."""
    S, hq, hk = case["S"], case["nq"], case["nkv"]
    G = hq // hk
    lens = lengths_for(S)
    B = len(lens)
    rng = np.random.default_rng(kc._seed(case["name"]))
    q = np.empty((B, hq, S, HD), np.uint16)
    k = np.empty((B, hk, S, HD), np.uint16)
    v = np.empty((B, hk, S, HD), np.uint16)
    for b, n in enumerate(lens):
        sigma = np.where((b + np.arange(hq)) % 2 == 0, kc.FLAT, kc.PEAKED).astype(np.float32) / math.sqrt(HD)
        qb = kr.bf16_round(rng.standard_normal((hq, S, HD), dtype=np.float32) * sigma[:, None, None])
        kb = rng.standard_normal((hk, S, HD), dtype=np.float32)
        vb = rng.standard_normal((hk, S, HD), dtype=np.float32)
        taken = set()
        for i, (qi, kj, other) in enumerate(_probe_pairs(case, n, b)):
            h = i % hq
            g = h // G
            if other:
                g = (g + 1) % hk
            if (g, kj) in taken:
                continue
            taken.add((g, kj))
            qv = qb[h, qi].astype(np.float64)
            kb[g, kj] = (qv * (kc.SPIKE / max(float(qv @ qv), 1e-12))).astype(np.float32)
            vb[g, kj] = kc._probe_v(i, HD)
        q[b], k[b], v[b] = kr.bf16_bits(qb), kr.bf16_bits(kb), kr.bf16_bits(vb)
    lens = np.array(lens, np.int32)
    return dict(q=q, k=k, v=v, lens=lens, mask=np.arange(S)[None, :] < lens[:, None])


def visibility(case, mask_row, dw=0, diag=0, pad=0):
    """The operation (dw = diag = pad = 0) and the off-by-one mutants: window w + dw, the diagonal moved by diag; bidirectional cases: the
    key mask moved by pad (+1: the first pad key attended, -1: the last real key dropped)."""
    if case.get("bidir"):
        n = int(np.asarray(mask_row).sum())
        return kr.Visibility(np.arange(len(mask_row)) < n + pad)
    return kr.Visibility(mask_row, window=case["window"] - 1 + dw, causal=True, diag=diag)


def coarse_visibility(case, n):
    """The mutant that masks the band by whole 32 x 32 blocks only (per-pair band mask forgotten; the diagonal is kept)."""
    S, W = case["S"], case["window"] - 1
    q = np.arange(n)[:, None]
    k = np.arange(S)[None, :]
    lo = np.maximum(q // 32 * 32 - W, 0) // 32 * 32          # first key of the first block any query of the wave reaches
    return (k <= q) & (k >= lo)


def check_attention(case, inp, ctx_bits, worst, vis_of=None):
    """Every valid query row of every head of ctx [B][S][nq * 128] against the float64 reference at attention_bound; every row at or
    past a length must be exactly zero. vis_of(b, n): another visibility (the mutants)."""
    S, hq, G = case["S"], case["nq"], case["nq"] // case["nkv"]
    ctx = kr.bf16_value(ctx_bits).reshape(len(inp["lens"]), S, hq * HD)
    for b, n in enumerate(int(x) for x in inp["lens"]):
        assert np.array_equal(ctx[b, n:], np.zeros_like(ctx[b, n:])), f"{case['name']}: batch row {b} has a non-zero row at or past its length"
        if n == 0:
            continue
        for h in range(hq):
            qh, kh, vh = kr.bf16_value(inp["q"][b, h]), kr.bf16_value(inp["k"][b, h // G]), kr.bf16_value(inp["v"][b, h // G])
            vis = vis_of(b, n) if vis_of else visibility(case, inp["mask"][b])
            out, out_abs = kr.attention_ref(qh[:n], kh, vh, vis)
            bound = kr.attention_bound(qh[:n], kh, out, out_abs)
            worst.add(ctx[b, :n, h * HD:(h + 1) * HD], out, bound, case["name"], b, h)


# ---- k_ll_rope ---------------------------------------------------------------------------------------------------------------------
def rope_cases():
    out = []
    for G, (nq, nkv) in GROUPS.items():
        for S in (32, 96, 192):
            out.append(dict(G=G, nq=nq, nkv=nkv, S=S, B=2, qscale=math.log2(math.e) / math.sqrt(HD), name=f"llrope_g{G}_S{S}"))
    return out


def rope_table(n_pos, theta=1e4):
    """float32 cos / sin [n_pos][64] of HF's default rotary embedding (float32 angle = float32 position x float32 frequency)."""
    inv = (1.0 / theta ** (np.arange(0, HD, 2, dtype=np.float64) / HD)).astype(np.float32)
    ang = np.arange(n_pos, dtype=np.float32)[:, None] * inv[None, :]
    return np.cos(ang.astype(np.float64)).astype(np.float32), np.sin(ang.astype(np.float64)).astype(np.float32)


def rope_inputs(case):
    """qkv [B * S][(nq + 2 nkv) 128] bf16 bits: N(0, 1) with a few rows 64 times larger; tables one position longer than S (the
    position-off-by-one mutant reads it)."""
    rng = np.random.default_rng(kc._seed(case["name"]))
    T, slots = case["B"] * case["S"], case["nq"] + 2 * case["nkv"]
    x = rng.standard_normal((T, slots * HD), dtype=np.float32)
    x[rng.choice(T, size=max(2, T // 32), replace=False)] *= 64.0
    rc, rs = rope_table(case["S"] + 1)
    return dict(qkv=kr.bf16_bits(x), rc=rc, rs=rs)


# ---- mean pooling with the final RMSNorm (k_ll_pool_part / k_ll_pool_fin) ------------------------------------------------------------------
POOL_EPS = 1e-5
POOL_H = (256, 1152, 4096)   # one column slice; 1024 + 128 (two slices, the second narrow); four full slices (the models' width)


def pool_cases():
    """S = 192 / 96 / 32 at every width with the chunk edges 63 / 64 / 65 among the lengths, normalised and not; and the 129-token row
    alone at S = 2048 (H = 4096), which must equal itself in the S = 192 batch bit for bit."""
    out = []
    for H in POOL_H:
        for S, lens in ((192, (192, 129, 65, 64, 63, 1, 0)), (96, (96, 65, 64, 63, 0)), (32, (32, 31, 1))):
            for normalise in (1, 0):
                out.append(dict(H=H, S=S, lens=lens, normalise=normalise, name=f"llpool_H{H}_S{S}_n{normalise}"))
    out.append(dict(H=4096, S=2048, lens=(129,), normalise=1, name="llpool_H4096_S2048_n1", alone=True))
    for c in out:
        c.update(B=len(c["lens"]), eps=POOL_EPS)
    return out


def pool_inputs(c):
    """x [B][S][H] float32: rows N(0, 1) alternating in sign from token to token plus a common offset (the mean cancels), a few 64 times
    larger; every token row at or past a length is NaN (it must not be read); w ~ N(1, 0.3). The `alone` case holds the 129-token row of
    the S = 192, H = 4096 batch."""
    if c.get("alone"):
        src = [k for k in pool_cases() if k["name"] == "llpool_H4096_S192_n1"][0]
        inp = pool_inputs(src)
        x = np.full((1, c["S"], c["H"]), np.nan, np.float32)
        x[0, :129] = inp["x"][1, :129]
        return dict(x=x, w=inp["w"], lens=np.array([129], np.int32))
    rng = np.random.default_rng(kc._seed(f"llpool_H{c['H']}_S{c['S']}"))
    B, S, H = c["B"], c["S"], c["H"]
    x = rng.standard_normal((B, S, H)).astype(np.float32) * np.where(np.arange(S) % 2, -1.0, 1.0)[None, :, None].astype(np.float32)
    x += rng.standard_normal((1, 1, H)).astype(np.float32) * 0.5
    x[:, ::7] *= 64.0
    for b, n in enumerate(c["lens"]):
        x[b, n:] = np.nan
    return dict(x=x, w=(1.0 + 0.3 * rng.standard_normal(H)).astype(np.float32), lens=np.array(c["lens"], np.int32))
