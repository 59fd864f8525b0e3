"""GPU suite of the two kernels the T5 path adds, launch by launch in the manner of tests/test_kernels_gpu.py: k_attn_long_relbias
(the clamped relative bias) ONE launch at a time through ak_kts_t5_attn and k_gemm MODE 10 (ReLU) through ak_kts_t5_gemm_relu, in child
processes on libarchi_hip_dbg.so (tests/t5_kernel_worker.py; each case once, nothing is run again after a failure).

Every valid query row of every head, and every GEMM output element, against float64 at the derived bounds of tests/t5_kernel_cases.py
(err / bound <= 1; each test prints its worst, -s). In the same file: the mirrored table is over the bound (the test can see the
direction of key - query), and an all-zero table reproduces ak_kt_attn_window's output at window -1 bit for bit."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import kernel_cases as kc
from tests import kernel_refs as kr
from tests import t5_kernel_cases as tc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_DEAD = []                   # a child that ended badly: nothing more is started on the GPU from this file
_RES = {}


def _child(tmp_path_factory, group):
    if group in _RES:
        return _RES[group]
    out = str(tmp_path_factory.mktemp("t5_kernels") / f"{group}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AK_")}
    env["ARCHI_HIP_DBG"] = "1"
    if group == "relu_wide":
        env["AK_GEMM_BN"] = "256"
    t0 = time.time()
    assert not _DEAD, f"not started: child {_DEAD[0]} ended badly before"
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "t5_kernel_worker.py"), group, out], env=env, stdout=subprocess.PIPE,
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


@pytest.mark.parametrize("name", [c["name"] for c in tc.ATTN_CASES])
def test_biased_attention_against_float64(tmp_path_factory, name):
    res = _child(tmp_path_factory, "attn")
    c = next(c for c in tc.ATTN_CASES if c["name"] == name)
    inp = tc.attn_inputs(c)
    ctx = res[name]
    worst = kr.Worst()
    tc.attn_check(c, inp, ctx, worst)
    print(f"t5 attention {name}: {worst}")
    assert worst.n > 0 and worst.ratio <= 1.0, str(worst)
    for b, n in enumerate(c["lens"]):             # past a length: finite rows; zero rows in every 128-query block wholly past it
        assert np.isfinite(kr.bf16_value(ctx[b, n:])).all(), (name, b)
        assert not ctx[b, (n + 127) // 128 * 128:].any(), (name, b)
    assert (res[name + ":guard"] == kr.bf16_bits(np.float32(tc.SENT))).all()
    # the mutant: the same launch held to the float64 operation with the table mirrored in key - query
    mirrored = kr.Worst()
    tc.attn_check(c, inp, ctx, mirrored, tab=np.ascontiguousarray(inp["tab"][:, ::-1]))
    print(f"t5 attention {name}, against the mirrored table: err / bound {mirrored.ratio:.1f}")
    assert mirrored.ratio > 1.0


def test_case_list_is_what_the_issue_asks():
    by = {c["name"]: c for c in tc.ATTN_CASES}
    assert (by["S32"]["S"], by["S160"]["S"], by["S160"]["lens"]) == (32, 160, [129, 33, 1])
    assert (by["S128_D8"]["S"], by["S128_D8"]["D"], by["S704"]["S"], by["S704"]["D"]) == (128, 8, 704, 128)
    assert any(0 in c["lens"] for c in tc.ATTN_CASES)
    assert sorted((c["T"], c["N"], c["K"]) for c in tc.RELU_CASES) == [(256, N, K) for N in (256, 512) for K in (128, 768)]
    assert {tc.relu_tile(c, False) for c in tc.RELU_CASES} == {"narrow"}
    assert sorted(c["K"] for c in tc.RELU_CASES if tc.relu_tile(c, True) == "wide") == [768, 768]
    for c in tc.ATTN_CASES:
        tab = tc.attn_inputs(c)["tab"]
        assert np.abs(tab - tab[:, ::-1]).max() > 1.0                            # asymmetric


@pytest.mark.parametrize("name", tc.EQUAL_CASES)
def test_zero_table_is_the_unbiased_kernel_bit_for_bit(tmp_path_factory, name):
    res = _child(tmp_path_factory, "equal")
    assert np.array_equal(res[name + ":zero_table"], res[name + ":window"])
    assert not (res[name + ":window"] == kr.bf16_bits(np.float32(tc.SENT))).all()


@pytest.mark.parametrize("group", ["relu", "relu_wide"])
def test_gemm_relu_against_float64(tmp_path_factory, group):
    res = _child(tmp_path_factory, group)
    for c in tc.RELU_CASES:
        inp = kc.gemm_inputs(c)
        y, y_abs = kr.gemm_ref(kr.bf16_value(inp["x"]), kr.bf16_value(inp["w"]), inp["bias"])
        neg = float((y < 0).mean())
        assert 0.4 <= neg <= 0.6, neg                                            # about half the outputs are clipped
        got = kr.bf16_value(res[c["name"]])
        worst = kr.Worst()
        worst.add(got, *tc.epi_relu(y, y_abs, c["K"]), c["name"])
        print(f"gemm MODE 10 {c['name']} ({tc.relu_tile(c, group == 'relu_wide')} tile), {neg:.0%} negative: {worst}")
        assert worst.n == c["T"] * c["N"] and worst.ratio <= 1.0, str(worst)
        assert (got >= 0).all() and (res[c["name"] + ":guard"] == kr.bf16_bits(np.float32(tc.SENT))).all()
