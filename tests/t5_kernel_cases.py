"""Cases, inputs and float64 expectations of the T5 kernel tests (tests/test_t5_kernels_gpu.py; the child tests/t5_kernel_worker.py
runs the launches): launch_attn_relbias (k_attn_long_relbias) through ak_kts_t5_attn and k_gemm MODE 10 through
ak_kts_t5_gemm_relu.

Attention. The operation is kernel_refs.attention_ref with the dense bias tab[h][clamp(key - query, -D, D) + D] (base-2 domain, like
q); the bound is kernel_refs.attention_bound as ak_kt_attn_window's, with the bias inside the score magnitude: bias_max = max |tab[h]|
(the float32 add of the bias to the score is one of the (hd + 4) roundings the bound charges on |q| |k|_max + |bias|_max).
The table is random and NOT symmetric in key - query, so a mirrored gather cannot pass.

ReLU. r = max(y, 0) is 1-Lipschitz: |max(y', 0) - max(y, 0)| <= |y' - y| <= e_pre, plus the bf16 store u |r| (kernel_refs' GEMM
bound for a plain bf16 output, with r in place of y)."""
import zlib

import numpy as np

try:
    from tests import kernel_refs as kr
except ImportError:          # imported by the worker script, whose directory is tests/ itself
    import kernel_refs as kr

HD = 64
GUARD = 4                    # token rows behind every output buffer, prefilled, that no launch may touch
SENT = 12288.0               # bf16-exact

# name -> S, heads, D, lens. S = 128 at D = 8: the workgroup's four waves meet far-left, far-right and mixed key blocks; S = 704 at
# D = 128: far blocks on both sides of more than one workgroup; a row of length 0 writes zero context rows
ATTN_CASES = [
    dict(name="S32", S=32, heads=2, D=128, lens=[32, 5]),
    dict(name="S160", S=160, heads=2, D=128, lens=[129, 33, 1]),
    dict(name="S128_D8", S=128, heads=2, D=8, lens=[128, 97]),
    dict(name="S704", S=704, heads=2, D=128, lens=[704, 641]),
    dict(name="len0", S=64, heads=1, D=128, lens=[0, 40]),
]
EQUAL_CASES = ["S160", "S704"]             # an all-zero table against ak_kt_attn_window at window -1, bit for bit

# T = 256, N in {256, 512}, K in {128, 768}. Child "relu": the narrow tile (two column tiles are far below one per CU). Child
# "relu_wide" runs with AK_GEMM_BN=256, the launcher's A/B switch: at K = 768 the wide phased tile, at K = 128 (below the phased loop's
# 192) the launcher stays on the narrow tile -- MODE 10 has no other instantiation
RELU_CASES = [dict(name=f"relu_N{N}_K{K}", mode=10, T=256, N=N, K=K) for N in (256, 512) for K in (128, 768)]


def relu_tile(c, forced_wide):
    """The launcher's rule (gemm.hip launch_gemm) restated."""
    wide = c["N"] % 256 == 0 and ((c["T"] // 256) * (c["N"] // 256) >= 256 or forced_wide)
    return "wide" if wide and c["K"] >= 192 else "narrow"


def _seed(name):
    return zlib.crc32(("t5:" + name).encode())


def attn_inputs(c):
    """q, k, v as bf16 bits [B][heads][S][64], mask [B][S] bool (right-padded), lens, tab [heads][2 D + 1] float32 (base-2 domain,
    N(0, 2), asymmetric). q at two widths of the score distribution, as kernel_cases.attn_inputs draws it."""
    S, heads, D, lens = c["S"], c["heads"], c["D"], c["lens"]
    B = len(lens)
    rng = np.random.default_rng(_seed(c["name"]))
    sigma = np.where(np.arange(heads) % 2 == 0, 0.3, 3.0).astype(np.float32) / 8.0
    q = kr.bf16_bits(rng.standard_normal((B, heads, S, HD), dtype=np.float32) * sigma[None, :, None, None])
    k = kr.bf16_bits(rng.standard_normal((B, heads, S, HD), dtype=np.float32))
    v = kr.bf16_bits(rng.standard_normal((B, heads, S, HD), dtype=np.float32))
    mask = np.arange(S)[None, :] < np.asarray(lens)[:, None]
    tab = (rng.standard_normal((heads, 2 * D + 1), dtype=np.float32) * 2.0).astype(np.float32)
    return dict(q=q, k=k, v=v, mask=mask, lens=np.asarray(lens, np.int32), tab=tab)


def bias_dense(tab_row, S, D):
    """tab[clamp(key - query, -D, D) + D] as [S queries][S keys], float64."""
    d = np.arange(S)[None, :] - np.arange(S)[:, None]
    return np.asarray(tab_row, np.float64)[np.clip(d, -D, D) + D]


def attn_check(c, inp, ctx_bits, worst, tab=None):
    """Every valid query row of every head of ctx [B][S][heads * 64] against float64 with table `tab` (default: the case's own)."""
    S, heads, D = c["S"], c["heads"], c["D"]
    tab = inp["tab"] if tab is None else tab
    ctx = kr.bf16_value(ctx_bits).reshape(len(c["lens"]), S, heads * HD)
    for b, n in enumerate(c["lens"]):
        if n == 0:
            continue
        vis = kr.Visibility(inp["mask"][b])
        for h in range(heads):
            qh, kh, vh = (kr.bf16_value(inp[x][b, h]) for x in ("q", "k", "v"))
            out, out_abs = kr.attention_ref(qh[:n], kh, vh, vis, bias_dense(tab[h], S, D)[:n])
            bound = kr.attention_bound(qh[:n], kh, out, out_abs, float(np.abs(tab[h]).max()))
            worst.add(ctx[b, :n, h * HD:(h + 1) * HD], out, bound, c["name"], b, h)


def epi_relu(y, y_abs, K):
    r = np.maximum(y, 0.0)
    return r, kr.e_pre(y_abs, K) + kr.U * np.abs(r)
