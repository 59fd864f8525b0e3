"""Kernel-level GPU tests of the Mistral / Llama family (decoder128.hip, the window argument of attn_causal.hip), ONE launch at a time through
the ak_kts_ll_* wrappers, in child processes on their own timeouts (tests/llama_kernel_worker.py), in the manner of
tests/test_stack_kernels_gpu.py. A child that ends badly stops every later start from this file.

Attention: every valid query row of every head against kernel_refs.attention_ref at attention_bound (err / bound <= 1: derived, not
tuned); rows at or past a length exactly zero. Cases and probes: tests/llama_kernel_cases.py. The plain causal mode through the new
argument (window 0) equals launch_attn_causal's output bit for bit on two of the existing causal cases.
k_ll_rope and the mean pool: tests/llama_kernel_refs.py's float64 statements and bounds; v bit for bit; the rows behind every output keep the sentinel."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import kernel_refs as kr
from tests import llama_kernel_cases as lc
from tests import llama_kernel_refs as lr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_DEAD = []                   # a child that ended badly: nothing more is started on the GPU from this file
_RES = {}


def _child(tmp_path_factory, group):
    if group in _RES:
        return _RES[group]
    out = str(tmp_path_factory.mktemp("llama_kernels") / f"{group}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AK_")}
    env["ARCHI_HIP_DBG"] = "1"
    t0 = time.time()
    assert not _DEAD, f"not started: child {_DEAD[0]} ended badly before"
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "llama_kernel_worker.py"), group, out], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=180)
    except subprocess.TimeoutExpired:
        _DEAD.append(group)
        raise
    if p.returncode != 0:
        _DEAD.append(group)
    assert p.returncode == 0, f"{group}: exit {p.returncode}\n" + p.stderr.decode("utf-8", "replace")[-3000:]
    print(f"child {group}: {time.time() - t0:.0f} s")
    _RES[group] = np.load(out)
    return _RES[group]


@pytest.mark.parametrize("G", (1, 2, 3, 4))
def test_window_attention(tmp_path_factory, G):
    """k_attn_causal_band and k_attn_bidir at G query heads per kv head: S = 96, 160 at w in {1, 31, 32, 33, 64, 100} and bidirectional;
    G = 4 also S = 32, 64, 288 and S = 2048 at w = 1000 and bidirectional; lengths S, S - 1, mid-block, 1, 0 in every case."""
    res = _child(tmp_path_factory, "attn")
    worst = kr.Worst()
    cases = [c for c in lc.attn_cases() if c["G"] == G]
    for case in cases:
        lc.check_attention(case, lc.attn_inputs(case), res[case["name"]], worst)
    print(f"window attention G = {G}, {len(cases)} cases: {worst}")
    assert worst.n > 0 and worst.ratio <= 1.0, str(worst)
    wb = kr.Worst()
    for case in (c for c in cases if c["bidir"]):
        lc.check_attention(case, lc.attn_inputs(case), res[case["name"]], wb)
    print(f"  of which bidirectional: {wb}")


def test_plain_causal_through_the_window_argument_is_bit_equal(tmp_path_factory):
    res = _child(tmp_path_factory, "equal")
    cases = lc.equal_cases()
    assert len(cases) == 2
    for case in cases:
        a, b = res[case["name"] + ":qwen3"], res[case["name"] + ":window0"]
        assert a.shape == b.shape and np.array_equal(a, b), case["name"]


def test_ll_rope(tmp_path_factory):
    """k_ll_rope at the (nq, nkv) of G = 1 .. 4, S = 32, 96, 192, two sequences."""
    res = _child(tmp_path_factory, "rope")
    worst, bad = kr.Worst(), []
    guard = kr.bf16_bits(np.full((lc.GUARD, lc.HD), lc.SENT, np.float32))
    for c in lc.rope_cases():
        got = {n: res[f"{c['name']}:{n}"] for n in ("q", "k", "v")}
        bad += [f"{c['name']}:{n}" for n in lr.compare(lr.rope_expect(c, lc.rope_inputs(c)), got, worst, c["name"])]
        bad += [f"{c['name']}:{n}_guard" for n in ("q", "k", "v") if not np.array_equal(res[f"{c['name']}:{n}_guard"], guard)]
    print(f"k_ll_rope: {worst}")
    assert not bad, f"not bit for bit: {bad[:8]}"
    assert worst.n > 0 and worst.ratio <= 1.0, str(worst)


def test_ll_mean_pool(tmp_path_factory):
    """k_ll_pool_part / k_ll_pool_fin at H = 256, 1152 and 4096 (one, two and four column slices), S = 192 / 96 / 32 with the chunk edges
    63 / 64 / 65 among the lengths, normalised and not; token rows past a length are NaN and must not be read; a row of length 0 is exact
    zeros; the row behind the output keeps the sentinel; the 129-token row alone at S = 2048 equals itself in the S = 192 batch bit for bit."""
    res = _child(tmp_path_factory, "pool")
    worst = kr.Worst()
    for c in lc.pool_cases():
        inp = lc.pool_inputs(c)
        got = res[c["name"]]
        want, bound = lr.pool_expect(c, inp)
        assert np.array_equal(got[c["B"]], np.full(c["H"], lc.SENT, np.float32)), c["name"]
        for b, n in enumerate(c["lens"]):
            if n == 0:
                assert np.array_equal(got[b].view(np.uint32), np.zeros(c["H"], np.uint32)), (c["name"], b)
        worst.add(got[:c["B"]], want, bound, c["name"])
    print(f"k_ll_pool: {worst}")
    assert worst.n > 0 and worst.ratio <= 1.0, str(worst)
    assert np.array_equal(res["llpool_H4096_S2048_n1"][0].view(np.uint32), res["llpool_H4096_S192_n1"][1].view(np.uint32))
