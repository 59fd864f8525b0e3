"""The cases of the Qwen2 kernel-level tests (tests/test_qwen2_kernels_gpu.py) and their inputs, built from a seed, in the manner of
tests/llama_kernel_cases.py: the GPU worker (tests/qwen2_kernel_worker.py), the float64 references in the parent and the mutant tests on
the CPU (tests/test_qwen2_cpu.py) all call the same builders, so they see the same numbers.

Attention (launch_attn_causal_split: a kv group of G = 5 .. 8 query heads split over P = 2 workgroups of GP = ceil(G / 2) waves, wave w
of part p computing head p * GP + w of the group). Inputs as llama_kernel_cases.attn_inputs builds them (random bf16 q, k, v, flat and
peaked logit spreads, pad rows random and finite) with SPIKE PROBES: the diagonal and one past it; the last real key and the first pad
key; key 0; a key above the diagonal (bidirectional cases: it must be seen; causal ones: it must not); a visible key of the NEIGHBOURING
kv head spiked against a query of this one (a wrong grouped-query map, or a surplus wave's head index running into the next group, sees
it); and a key spiked against the query of the head at the SAME wave slot of the OTHER part of the group (a part whose head base is
forgotten computes that head's output in this head's place). Lengths per case: S, 0, S - 1, 1, a mid-block one, S -- a full row directly
behind an empty and behind a 1-token row, so that the stray store of a surplus wave (G = 5, 7) lands on a row that is compared.

k_gemm MODE 3 with a real bias: the two QKV shapes of the released models, bias N(0, 2) with a few entries at +-64."""
import math

import numpy as np

try:
    from tests import kernel_cases as kc
    from tests import kernel_refs as kr
    from tests import llama_kernel_cases as lc
except ImportError:          # imported by the worker script, whose directory is tests/ itself
    import kernel_cases as kc
    import kernel_refs as kr
    import llama_kernel_cases as lc

HD = 128
GROUPS = {5: (10, 2), 6: (12, 2), 7: (14, 2), 8: (16, 2)}      # G -> (nq, nkv): two kv heads, so that a neighbouring one exists
SENT = kc.SENTINEL
GUARD = 3                    # token rows behind ctx that must keep the sentinel


def parts(G):
    """(P, GP): workgroups per kv group and waves per workgroup, as attn_causal_body.h computes them."""
    P = (G + 3) // 4
    return P, (G + P - 1) // P


def lengths_for(S):
    return [S, 0, S - 1, 1, (S // 2 // 32) * 32 + 13, S]


def attn_cases():
    """G in {5, 6, 7, 8} x S in {96, 160} x {causal, bidirectional}; G = 7 and G = 5 at S = 32, 64 (one and two key blocks) and 288 (nine
    workgroups per part); G = 7 at S = 2048 once causal and once bidirectional."""
    out = []
    for G in (5, 6, 7, 8):
        for S in (96, 160):
            out += [dict(G=G, S=S, bidir=b) for b in (False, True)]
    for G in (7, 5):
        for S in (32, 64, 288):
            out += [dict(G=G, S=S, bidir=b) for b in (False, True)]
    out += [dict(G=7, S=2048, bidir=False), dict(G=7, S=2048, bidir=True)]
    for c in out:
        nq, nkv = GROUPS[c["G"]]
        c.update(kernel="causal", nq=nq, nkv=nkv, heads=nq, hd=HD, window=0, name=f"q2attn_g{c['G']}_S{c['S']}_{'bidir' if c['bidir'] else 'causal'}")
    return out


def equal_cases():
    """launch_attn_causal as it was: llama_kernel_cases.equal_cases() (G = 2 and 3) and a G = 4 case of kernel_cases.causal_cases()."""
    return lc.equal_cases() + [c for c in kc.causal_cases() if c["name"] == "causal_q32_kv8_S64"]


OWN, NEIGHBOUR, OTHER_PART = 0, 1, 2


def _probe_pairs(case, n, b):
    """(query, key, kind) triples to spike in a row of length n; the order rotates with b."""
    S = case["S"]
    if n <= 0:
        return []
    last = n - 1
    qs = [0, 31, 32, 63, 64, last, last - 1, last - 31, last - 32, last // 2]
    pairs = []
    for q in qs:
        pairs += [(q, q, OWN), (q, q + 1, OWN), (q, last, OWN), (q, last + 1, OWN), (q, 0, OWN), (q, min(q + 33, last), OWN)]
    pairs += [(last, max(last - 3, 0), NEIGHBOUR), (last // 2, last // 2, NEIGHBOUR), (last, max(last - 5, 0), OTHER_PART),
              (last // 2, max(last // 2 - 1, 0), OTHER_PART), (min(33, last), min(2, last), OTHER_PART)]
    pairs = [(q, k, o) for q, k, o in pairs if 0 <= q < n and 0 <= k < S]
    r = b % len(pairs)
    return pairs[r:] + pairs[:r]


def attn_inputs(case):
    """q [B][nq][S][128], k, v [B][nkv][S][128] as bf16 bits, lens [B], mask [B][S]."""
    S, hq, hk = case["S"], case["nq"], case["nkv"]
    G = hq // hk
    GP = parts(G)[1]
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
        for i, (qi, kj, kind) in enumerate(_probe_pairs(case, n, b)):
            h = i % hq
            g = h // G
            if kind == NEIGHBOUR:
                g = (g + 1) % hk
            elif kind == OTHER_PART:                           # the head at the same wave slot of the group's other part, where it exists
                other = (1 - (h % G) // GP) * GP + (h % G) % GP
                if other < G:
                    h = g * G + other
            if (g, kj) in taken:
                continue
            taken.add((g, kj))
            qv = qb[h, qi].astype(np.float64)
            kb[g, kj] = (qv * (kc.SPIKE / max(float(qv @ qv), 1e-12))).astype(np.float32)
            vb[g, kj] = kc._probe_v(i, HD)
        q[b], k[b], v[b] = kr.bf16_bits(qb), kr.bf16_bits(kb), kr.bf16_bits(vb)
    lens = np.array(lens, np.int32)
    return dict(q=q, k=k, v=v, lens=lens, mask=np.arange(S)[None, :] < lens[:, None])


def visibility(case, mask_row, diag=0, pad=0):
    """The operation (diag = pad = 0) and the off-by-one mutants: the causal diagonal moved by diag; bidirectional cases: the key mask
    moved by pad (+1: the first pad key attended, -1: the last real key dropped)."""
    if case["bidir"]:
        n = int(np.asarray(mask_row).sum())
        return kr.Visibility(np.arange(len(mask_row)) < n + pad)
    return kr.Visibility(mask_row, causal=True, diag=diag)


def check_attention(case, inp, ctx_bits, worst, vis_of=None):
    """llama_kernel_cases.check_attention under this file's visibility: every valid query row of every head of ctx [B][S][nq * 128]
    against the float64 reference at attention_bound; every row at or past a length exactly zero."""
    lc.check_attention(case, inp, ctx_bits, worst, vis_of or (lambda b, n: visibility(case, inp["mask"][b])))


# ---- k_gemm MODE 3 with the q | k | v bias ------------------------------------------------------------------------------------------
def gemm_cases():
    """(T, N, K): the QKV projection of Qwen2-7B (N = (28 + 8) 128, K = 3584) and of Qwen2-1.5B (N = (12 + 4) 128, K = 1536), 512 tokens."""
    out = [dict(T=512, N=4608, K=3584), dict(T=512, N=2048, K=1536)]
    for c in out:
        c.update(mode=3, name=f"q2gemm_T{c['T']}_N{c['N']}_K{c['K']}")
    return out


def gemm_inputs(c):
    """kernel_cases.gemm_inputs with the bias a q | k | v bias would be: N(0, 2), a few entries at +-64."""
    inp = kc.gemm_inputs(c)
    rng = np.random.default_rng(kc._seed(c["name"] + ":bias"))
    bias = (2.0 * rng.standard_normal(c["N"])).astype(np.float32)
    at = rng.choice(c["N"], size=8, replace=False)
    bias[at] = np.where(np.arange(8) % 2 == 0, 64.0, -64.0).astype(np.float32)
    inp["bias"] = bias
    return inp


def gemm_expect(c, inp, bias=None):
    """(want, bound) of the bf16 output: float64 x W^T + bias at kernel_refs' GEMM bound (epi_bf16). bias: another one (the mutants)."""
    y, y_abs = kr.gemm_ref(kr.bf16_value(inp["x"]), kr.bf16_value(inp["w"]), inp["bias"] if bias is None else bias)
    return kr.epi_bf16(y, y_abs, c["K"])
