"""GPU suite of the EmbeddingGemma kernels, launch by launch, in the manner of tests/test_kernels_gpu.py: launch_attn_gqa (head size
256, grouped queries, optional band) ONE launch at a time through ak_ktg_attn_gqa, and k_gm_qk_norm_rope through ak_ktg_qk_norm_rope,
in child processes on libarchi_hip_dbg.so (tests/gemma_kernel_worker.py; each case once, nothing is run again after a failure).

Attention is compared with kernel_refs.attention_ref in float64, element by element over every valid query row of every head, at
kernel_refs.attention_bound (the derived u (|out| + P |v|) bound; err / bound <= 1); rows past a length must be finite. The probes
are kernel_cases._probe_pairs' (a large score at distance w and w + 1 on both sides, on the last real key and the first pad key) plus
a spike on a key of the neighbouring kv head (tests/gemma_kernel_cases.py). Each test prints its worst err / bound (-s)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import gemma_kernel_cases as gc
from tests import kernel_cases as kc
from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_DEAD = []                   # a child that ended badly: nothing more is started on the GPU from this file
_RES = {}


def _child(tmp_path_factory, group):
    if group in _RES:
        return _RES[group]
    out = str(tmp_path_factory.mktemp("gemma_kernels") / f"{group}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AK_")}
    env["ARCHI_HIP_DBG"] = "1"
    t0 = time.time()
    assert not _DEAD, f"not started: child {_DEAD[0]} ended badly before"
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "gemma_kernel_worker.py"), group, out], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=300)
    except subprocess.TimeoutExpired:
        _DEAD.append(group)
        raise
    if p.returncode != 0:
        _DEAD.append(group)
    assert p.returncode == 0, f"{group}: exit {p.returncode}\n" + p.stderr.decode("utf-8", "replace")[-3000:]
    print(f"child {group}: {time.time() - t0:.0f} s")
    _RES[group] = np.load(out)
    return _RES[group]


@pytest.mark.parametrize("fam", ["S<=64", "S=96,160", "S=288,544", "S=2048"])
def test_launch_attn_gqa(tmp_path_factory, fam):
    """k_attn_gqa<G, WIN> at G = 1 .. 4, half-windows {global, 1, 16, 32, 33, 256}, S from one key block to 64, lengths {S, S - 1,
    mid-block, 1, 0}: every valid query row of every head against float64 at the derived bound."""
    res = _child(tmp_path_factory, "gqa")
    worst = kr.Worst()
    seen = set()
    for case in gc.gqa_cases():
        if gc.family(case) != fam:
            continue
        seen.add((case["nq"] // case["nkv"], case["half_window"]))
        kc.check_attention(case, gc.gqa_inputs(case), res[case["name"]], worst)
    print(f"attn_gqa {fam}: {worst}")
    assert worst.n > 0 and worst.ratio <= 1.0, str(worst)
    if fam == "S=96,160":
        assert seen == {(G, w) for G in (1, 2, 3, 4) for w in gc.WINDOWS}


def test_rows_past_the_length_are_zero(tmp_path_factory):
    """Query rows at or past a row's length: zero context rows (the prefill was NaN), also where the whole row is empty."""
    res = _child(tmp_path_factory, "gqa")
    n = 0
    for case in gc.gqa_cases():
        if case["S"] > 544:
            continue
        ctx = res[case["name"]]
        for b, ln in enumerate(case["lens"]):
            assert not ctx[b, ln:].any(), (case["name"], b)
            n += ctx[b, ln:].size
    assert n > 0


def test_qk_norm_rope(tmp_path_factory):
    """k_gm_qk_norm_rope against its float64 statement on the float32 tables it is handed: per-head RMSNorm, rotate_half RoPE, the q
    scale; q and k head-major at U |stored| plus the float32 terms, v transposed in vt_pos order bit for bit."""
    res = _child(tmp_path_factory, "rope")
    worst = kr.Worst()
    for c in gc.ROPE_CASES:
        inp = gc.rope_inputs(c)
        e = gc.rope_expect(c, inp, res[c["name"] + ":rc"], res[c["name"] + ":rs"])
        for name in ("q", "k"):
            want, bound = e[name]
            got = kr.bf16_value(res[c["name"] + ":" + name])
            worst.add(got.reshape(-1, gc.HD), want.reshape(-1, gc.HD), bound.reshape(-1, gc.HD), c["name"] + ":" + name)
        B, S, nkv = c["B"], c["S"], c["nkv"]
        vt = kr.unpack_vt(res[c["name"] + ":vt"])                                  # [B][S][nkv * 256] bits
        want_v = kr.bf16_bits(e["v"].astype(np.float32)).transpose(0, 2, 1, 3).reshape(B, S, nkv * gc.HD)
        assert np.array_equal(vt, want_v), c["name"] + ": V^T is not a transposed copy"
    print(f"qk_norm_rope: {worst}")
    assert worst.n > 0 and worst.ratio <= 1.0, str(worst)


def test_gemm_tanh_geglu_on_both_tiles(tmp_path_factory):
    """k_gemm MODE 9 through ak_ktg_gemm_geglu_tanh (ak_kt_gemm keeps refusing the mode): the narrow tile and, at the model's gate / up
    shape with enough tokens, the wide phased tile the launcher picks itself; every output element against float64."""
    res = _child(tmp_path_factory, "geglu")
    for c in gc.GEGLU_CASES:
        assert kc.gemm_tile_is_wide(dict(c, mode=8)) == (c["tile"] == "wide")              # (MODE 9 follows MODE 8's rule)
        inp = kc.gemm_inputs(c)
        y, y_abs = kr.gemm_ref(kr.bf16_value(inp["x"]), kr.bf16_value(inp["w"]), inp["bias"])
        worst = kr.Worst()
        worst.add(kr.bf16_value(res[c["name"]]), *gc.epi_geglu_tanh(y, y_abs, c["K"]), c["name"])
        print(f"gemm MODE 9 {c['tile']}: {worst}")
        assert worst.n > 0 and worst.ratio <= 1.0, str(worst)
