"""Child of tests/test_qwen2_kernels_gpu.py, in the manner of tests/llama_kernel_worker.py: runs every case of one group through its
single-launch wrapper (libarchi_hip_dbg.so; the parent sets ARCHI_HIP_DBG=1), each case ONCE, and writes the raw outputs to one .npz. The
float64 references are the parent's work. Any launcher error or HIP error ends the process with a non-zero status. Every output buffer
is prefilled: the sentinel everywhere (ctx: the kernel must write every row below S, zeros at or past a length), GUARD token rows behind it.

    qwen2_kernel_worker.py <group> <out.npz>      group: attn | attn_long | equal | gemm"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from tests import kernel_cases as kc  # noqa: E402
from tests import kernel_refs as kr  # noqa: E402
from tests import qwen2_kernel_cases as qc  # noqa: E402
from tests.kernel_worker import NAN_BITS, _check, _dev, _full16, _host16, _ptr  # noqa: E402

SENT16 = int(kr.bf16_bits(np.float32(qc.SENT)).reshape(-1)[0])


def run_attn(lib, res, long=False):
    for case in qc.attn_cases():
        if (case["S"] >= 2048) != long:
            continue
        inp = qc.attn_inputs(case)
        B, S, width = len(inp["lens"]), case["S"], case["nq"] * qc.HD
        q, k, v, lens = _dev(inp["q"]), _dev(inp["k"]), _dev(inp["v"]), _dev(inp["lens"])
        ctx = _full16((B * S + qc.GUARD, width), SENT16)
        _check(lib, lib.ak_kts_q2_attn(_ptr(q), _ptr(k), _ptr(v), _ptr(lens), _ptr(ctx), B, S, case["nq"], case["nkv"], int(case["bidir"]), None), case["name"])
        h = _host16(ctx)
        res[case["name"]] = h[:B * S].reshape(B, S, width)
        res[case["name"] + ":guard"] = h[B * S:]


def run_equal(lib, res):
    """launch_attn_causal as Qwen3 calls it (ak_kt_attn_causal) and through ak_kts_ll_attn at window 0: G = 2 and G = 4, untouched."""
    for case in qc.equal_cases():
        inp = kc.attn_inputs(case)
        B, S = len(inp["lens"]), case["S"]
        q, k, v, lens = _dev(inp["q"]), _dev(inp["k"]), _dev(inp["v"]), _dev(inp["lens"].astype(np.int32))
        a, b = (_full16((B, S, case["nq"] * qc.HD), NAN_BITS) for _ in range(2))
        _check(lib, lib.ak_kt_attn_causal(_ptr(q), _ptr(k), _ptr(v), _ptr(lens), _ptr(a), B, S, case["nq"], case["nkv"], None), case["name"])
        _check(lib, lib.ak_kts_ll_attn(_ptr(q), _ptr(k), _ptr(v), _ptr(lens), _ptr(b), B, S, case["nq"], case["nkv"], 0, 0, None), case["name"])
        res[case["name"] + ":qwen3"], res[case["name"] + ":window0"] = _host16(a), _host16(b)


def run_gemm(lib, res):
    for c in qc.gemm_cases():
        inp = qc.gemm_inputs(c)
        x, w, bias = _dev(inp["x"]), _dev(inp["w"]), _dev(inp["bias"])
        out = _full16((c["T"] + qc.GUARD, c["N"]), SENT16)
        _check(lib, lib.ak_kts_gemm_bf16(_ptr(x), _ptr(w), _ptr(bias), c["T"], c["N"], c["K"], _ptr(out), None), c["name"])
        h = _host16(out)
        res[c["name"]], res[c["name"] + ":guard"] = h[:c["T"]], h[c["T"]:]


def main():
    group, out = sys.argv[1], sys.argv[2]
    from archi_amd import _lib
    lib = _lib.init(0)
    assert _lib.is_dbg_library(), "the single-launch wrappers live in libarchi_hip_dbg.so (ARCHI_HIP_DBG=1)"
    res = {}
    {"attn": run_attn, "attn_long": lambda l, r: run_attn(l, r, long=True), "equal": run_equal, "gemm": run_gemm}[group](lib, res)
    np.savez(out, **res)


if __name__ == "__main__":
    main()
