"""Kernel-level GPU tests of the Qwen2 family (the split mapping of attn_causal.hip, k_gemm MODE 3 with a real bias), ONE launch at a
time through ak_kts_q2_attn / ak_kts_gemm_bf16, in child processes on their own timeouts (tests/qwen2_kernel_worker.py), in the manner
of tests/test_llama_kernels_gpu.py. A child that ends badly stops every later start from this file.

Attention: every valid query row of every head against kernel_refs.attention_ref at attention_bound (err / bound <= 1: derived, not
tuned); rows at or past a length exactly zero; the rows behind ctx keep the sentinel. Cases and probes: tests/qwen2_kernel_cases.py.
launch_attn_causal at G = 2 and G = 4 still gives what it gave through both of its wrappers, bit for bit, and holds its own reference.
The QKV GEMM with a bias N(0, 2) and entries at +-64: every output element against float64 at kernel_refs' GEMM bound."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import kernel_cases as kc
from tests import kernel_refs as kr
from tests import qwen2_kernel_cases as qc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_DEAD = []                   # a child that ended badly: nothing more is started on the GPU from this file
_RES = {}


def _child(tmp_path_factory, group):
    if group in _RES:
        return _RES[group]
    out = str(tmp_path_factory.mktemp("qwen2_kernels") / f"{group}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AK_")}
    env["ARCHI_HIP_DBG"] = "1"
    t0 = time.time()
    assert not _DEAD, f"not started: child {_DEAD[0]} ended badly before"
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "qwen2_kernel_worker.py"), group, out], env=env, stdout=subprocess.PIPE,
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


def _hold(res, cases, what):
    worst = kr.Worst()
    guard = kr.bf16_bits(np.full((qc.GUARD, cases[0]["nq"] * qc.HD), qc.SENT, np.float32))
    for case in cases:
        assert np.array_equal(res[case["name"] + ":guard"], guard), f"{case['name']}: the rows behind ctx were written"
        qc.check_attention(case, qc.attn_inputs(case), res[case["name"]], worst)
    print(f"{what}, {len(cases)} cases: {worst}")
    assert worst.n > 0 and worst.ratio <= 1.0, str(worst)


@pytest.mark.parametrize("G", (5, 6, 7, 8))
def test_split_attention(tmp_path_factory, G):
    """k_attn_causal_gs and k_attn_bidir_gs at G query heads per kv head (parts 3 + 2, 3 + 3, 4 + 3, 4 + 4): S = 96, 160; G = 5 and 7
    also S = 32, 64, 288; lengths S, 0, S - 1, 1, mid-block, S in every case."""
    res = _child(tmp_path_factory, "attn")
    _hold(res, [c for c in qc.attn_cases() if c["G"] == G and c["S"] < 2048], f"split attention G = {G}")


def test_split_attention_at_2048(tmp_path_factory):
    """G = 7 at S = 2048 (64 key blocks, 64 workgroups per part), causal and bidirectional."""
    res = _child(tmp_path_factory, "attn_long")
    cases = [c for c in qc.attn_cases() if c["S"] >= 2048]
    assert [(c["G"], c["bidir"]) for c in cases] == [(7, False), (7, True)]
    _hold(res, cases, "split attention S = 2048")


def test_unsplit_launcher_is_what_it_was(tmp_path_factory):
    """launch_attn_causal at G = 2, 3 and 4 (llama_kernel_cases.equal_cases() and one G = 4 case): both wrappers bit for bit, and inside
    the bound of the reference the existing causal test holds them to."""
    res = _child(tmp_path_factory, "equal")
    cases = qc.equal_cases()
    assert sorted(c["nq"] // c["nkv"] for c in cases) == [2, 3, 4]
    worst = kr.Worst()
    for case in cases:
        a, b = res[case["name"] + ":qwen3"], res[case["name"] + ":window0"]
        assert a.shape == b.shape and np.array_equal(a, b), case["name"]
        kc.check_attention(case, kc.attn_inputs(case), a, worst)
    print(f"launch_attn_causal, G = 2, 3, 4: {worst}")
    assert worst.n > 0 and worst.ratio <= 1.0, str(worst)


def test_qkv_gemm_with_a_real_bias(tmp_path_factory):
    """k_gemm MODE 3 at the QKV shapes of Qwen2-7B and Qwen2-1.5B with the bias operand no pre-norm stack fed before."""
    res = _child(tmp_path_factory, "gemm")
    worst = kr.Worst()
    for c in qc.gemm_cases():
        inp = qc.gemm_inputs(c)
        want, bound = qc.gemm_expect(c, inp)
        assert np.array_equal(res[c["name"] + ":guard"], kr.bf16_bits(np.full((qc.GUARD, c["N"]), qc.SENT, np.float32))), c["name"]
        worst.add(kr.bf16_value(res[c["name"]]), want, bound, c["name"])
    print(f"QKV GEMM with bias: {worst}")
    assert worst.n > 0 and worst.ratio <= 1.0, str(worst)
