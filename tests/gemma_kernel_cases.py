"""Cases and inputs of tests/test_gemma_kernels_gpu.py, shared by the parent (references) and the child (launches): launch_attn_gqa one
launch at a time and k_gm_qk_norm_rope, in the manner of tests/kernel_cases.py, whose probes, Visibility and comparison are reused."""
import math
import zlib

import numpy as np

try:
    from tests import kernel_cases as kc
    from tests import kernel_refs as kr
except ImportError:          # imported by the worker script, whose directory is tests/ itself
    import kernel_cases as kc
    import kernel_refs as kr

HD = 256
WINDOWS = (0, 1, 16, 32, 33, 256)            # 0 = global
HEADS = {1: (2, 2), 2: (4, 2), 3: (3, 1), 4: (4, 1)}      # G -> (nq, nkv)


def lens_of(S, i):
    """Three of the five length classes {S, S - 1, mid-block, 1, 0} per case, rotating with the case number: B = 3."""
    five = [S, S - 1, max(1, S // 2 + 13 if S > 32 else 17), 1, 0]
    return [five[(i + j) % 5] for j in (0, 2, 3)] if i % 2 else [five[(i + j) % 5] for j in (0, 1, 2)]


def gqa_cases():
    """launch_attn_gqa: the smallest shapes at which the kernel can go wrong. Every half-window x every G at S = 96 and 160 (three and
    five key blocks: bands inside one block, across two, past the row); S = 32 and 64 (one and two blocks: a single row block per
    workgroup at G = 3 / 4, a workgroup wider than the row at G = 1 / 2); S = 288 and 544 (the half-window 256 clipped by the row and
    not); S = 2048 (the longest row: 64 key blocks, the band walk of the model's own window) at G = 3 and one case per other G."""
    out, i = [], 0
    for S in (96, 160):
        for w in WINDOWS:
            for G in (1, 2, 3, 4):
                out.append((S, w, G, HEADS[G]))
    for S in (32, 64):
        for j, w in enumerate(WINDOWS[:5]):
            out.append((S, w, 1 + (j + S // 32) % 4, None))
    for S in (288, 544):
        for j, w in enumerate(WINDOWS):
            out.append((S, w, 1 + (j + S // 32) % 4, None))
    out += [(544, 256, 3, (6, 2)), (2048, 0, 3, None), (2048, 256, 3, None), (2048, 33, 1, None), (2048, 1, 2, None), (2048, 256, 4, None),
            (2048, 32, 3, None), (2048, 16, 4, None)]
    cases = []
    for i, (S, w, G, heads) in enumerate(out):
        nq, nkv = heads or HEADS[G]
        cases.append(dict(kernel="gqa", S=S, half_window=w, window=w if w > 0 else -1, nq=nq, nkv=nkv, heads=nq, hd=HD, mask="right",
                          lens=lens_of(S, i), name=f"gqa_S{S}_w{w}_q{nq}_kv{nkv}"))
    return cases


def family(case):
    return "S<=64" if case["S"] <= 64 else ("S=96,160" if case["S"] <= 160 else ("S=288,544" if case["S"] <= 544 else "S=2048"))


def gqa_inputs(case):
    """kernel_cases.attn_inputs for this kernel: q [B][nq][S][256], k / v [B][nkv][S][256] as bf16 bits, mask / rowlen / lens; the
    probes of kernel_cases._probe_pairs (a large score at distance w and w + 1 on both sides, on the last real key and the first pad
    key) and, with more than one kv head, the same spike planted on a VISIBLE key of the neighbouring kv head (a kernel that maps a
    query head to the wrong kv head meets it)."""
    S, hq, hk = case["S"], case["nq"], case["nkv"]
    G = hq // hk
    lens = case["lens"]
    B = len(lens)
    rng = np.random.default_rng(zlib.crc32(case["name"].encode()))
    q = np.empty((B, hq, S, HD), np.uint16)
    k = np.empty((B, hk, S, HD), np.uint16)
    v = np.empty((B, hk, S, HD), np.uint16)
    mask = np.zeros((B, S), bool)
    for b, n in enumerate(lens):
        mask[b] = kr.mask_right(S, n)
        sigma = np.where((b + np.arange(hq)) % 2 == 0, kc.FLAT, kc.PEAKED).astype(np.float32) / math.sqrt(HD)
        qb = kr.bf16_round(rng.standard_normal((hq, S, HD), dtype=np.float32) * sigma[:, None, None])
        kb = rng.standard_normal((hk, S, HD), dtype=np.float32)
        vb = rng.standard_normal((hk, S, HD), dtype=np.float32)
        taken = set()
        for i, (qi, kj) in enumerate(kc._probe_pairs(case, mask[b], b)):
            h = i % hq
            g = h // G
            if (g, kj) in taken:
                continue
            taken.add((g, kj))
            qv = qb[h, qi].astype(np.float64)
            spike = (qv * (kc.SPIKE / max(float(qv @ qv), 1e-12))).astype(np.float32)
            kb[g, kj] = spike
            vb[g, kj] = kc._probe_v(i, HD)
            g2 = (g + 1) % hk
            if hk > 1 and i % 3 == 0 and (g2, qi) not in taken:      # the neighbouring kv head, on the query's own position (always visible)
                taken.add((g2, qi))
                kb[g2, qi] = spike
                vb[g2, qi] = kc._probe_v(i + 1, HD)
        q[b], k[b], v[b] = kr.bf16_bits(qb), kr.bf16_bits(kb), kr.bf16_bits(vb)
    return dict(q=q, k=k, v=v, mask=mask, rowlen=np.array(lens, np.int32), rel=None, lens=np.array(lens, np.int32))


# ---- k_gm_qk_norm_rope -----------------------------------------------------------------------------------------------------------
ROPE_CASES = [dict(name="rope_B2_S64_q3_kv1", B=2, S=64, nq=3, nkv=1, theta=1e4, qscale=math.log2(math.e) / math.sqrt(128.0)),
              dict(name="rope_B1_S2048_q4_kv2", B=1, S=2048, nq=4, nkv=2, theta=1e6, qscale=math.log2(math.e) / 16.0),
              dict(name="rope_B3_S32_q2_kv2", B=3, S=32, nq=2, nkv=2, theta=1e6, qscale=1.0)]
ROPE_EPS = 1e-6


def rope_inputs(c):
    rng = np.random.default_rng(zlib.crc32(c["name"].encode()))
    slots = c["nq"] + 2 * c["nkv"]
    T = c["B"] * c["S"]
    # rows of very different size (the RMSNorm must take them all), one all-zero head
    x = rng.standard_normal((T, slots, HD), dtype=np.float32) * np.exp2(rng.integers(-6, 6, (T, slots, 1))).astype(np.float32)
    x[T // 2, 0] = 0.0
    qn = (1.0 + 0.3 * rng.standard_normal(HD)).astype(np.float32)      # the folded weights 1 + w
    kn = (1.0 + 0.3 * rng.standard_normal(HD)).astype(np.float32)
    return dict(qkv=kr.bf16_bits(x), qn=qn, kn=kn)


def rope_expect(c, inp, rc, rs):
    """float64 statement of the launch on the float32 tables rc / rs [n_pos][128] it is given -> {name: (want, bound)}; q / k
    [B][heads][S][256]. The bound: one bf16 store, U |want|, plus the float32 work in front of it: the sum of 256 squares (256 E32
    relative on the sum, half of it on its inverse root), the mean / eps / rsqrt steps, and four roundings per product term --
    (256 / 2 + 12) E32 on |x0' cos| + |x1' sin|."""
    B, S, nq, nkv = c["B"], c["S"], c["nq"], c["nkv"]
    x = kr.bf16_value(inp["qkv"]).astype(np.float64).reshape(B, S, nq + 2 * nkv, HD)
    cos, sin = np.asarray(rc, np.float64)[:S], np.asarray(rs, np.float64)[:S]
    out = {}
    for name, lo, n, wn, sc in (("q", 0, nq, inp["qn"], c["qscale"]), ("k", nq, nkv, inp["kn"], 1.0)):
        xs = x[:, :, lo:lo + n]                                                   # [B][S][n][256]
        y = xs / np.sqrt((xs * xs).mean(-1, keepdims=True) + ROPE_EPS) * wn.astype(np.float64)
        y0, y1 = y[..., :128], y[..., 128:]
        cc, ss = cos[None, :, None, :], sin[None, :, None, :]
        want = np.concatenate([y0 * cc - y1 * ss, y1 * cc + y0 * ss], -1) * sc
        mag = np.concatenate([np.abs(y0 * cc) + np.abs(y1 * ss), np.abs(y1 * cc) + np.abs(y0 * ss)], -1) * sc
        bound = kr.U * np.abs(want) + (HD / 2 + 12) * kr.E32 * mag
        out[name] = (want.transpose(0, 2, 1, 3), bound.transpose(0, 2, 1, 3))
    out["v"] = x[:, :, nq + nkv:].transpose(0, 2, 1, 3)                           # exact copies
    return out


# ---- k_gemm MODE 9 (tanh GeGLU) ------------------------------------------------------------------------------------------------------
# the narrow tile (the fixtures' shapes; N a multiple of 128 only) and a T at which the launcher's own rule takes the wide phased tile
# at the model's gate / up shape: (T / 256) (N / 256) >= 256
GEGLU_CASES = [dict(mode=9, T=512, N=768, K=384, tile="narrow"), dict(mode=9, T=512, N=640, K=192, tile="narrow"),
               dict(mode=9, T=256 * math.ceil(256 / 9), N=2304, K=768, tile="wide")]
for _c in GEGLU_CASES:
    _c["name"] = f"geglu_tanh_{_c['tile']}_T{_c['T']}_N{_c['N']}_K{_c['K']}"


def epi_geglu_tanh(y, y_abs, K):
    """MODE 9 over interleaved rows: column 2 j the GELU input a, 2 j + 1 the gate g; gelu_tanh(a) g, N / 2 columns. The bound, in the
    manner of kernel_refs.epi_geglu: the GEMM's error on a through the GELU's slope (<= 1.13) and on g through |gelu(a)|; the float32
    epilogue a g / (1 + exp(-2 u)): u carries <= 5 roundings, so exp's argument is off by 5 e |2u| and exp(-2u) by (7 |2u| + 2) e
    relative; through 1 / (1 + x) that is at most 7 e absolute on the sigmoid at any u (|2u| e^-|2u| <= 0.37), plus the product and
    the quotient: 8 e |a| |g|; then one bf16 store."""
    a, g = y[:, 0::2], y[:, 1::2]
    ea, eg = kr.e_pre(y_abs[:, 0::2], K), kr.e_pre(y_abs[:, 1::2], K)
    ga = kr.gelu_tanh64(a)
    r = ga * g
    return r, 1.13 * np.abs(g) * ea + np.abs(ga) * eg + 8.0 * kr.E32 * np.abs(a) * np.abs(g) + kr.U * np.abs(r)
