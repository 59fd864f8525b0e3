"""Child of tests/test_t5_kernels_gpu.py, in the manner of tests/qwen2_kernel_worker.py: runs every case of one group through its
single-launch wrapper (libarchi_hip_dbg.so; the parent sets ARCHI_HIP_DBG=1), each case ONCE, and writes the raw outputs to one .npz.
The float64 references are the parent's work. Any launcher error or HIP error ends the process with a non-zero status. Every output
buffer is prefilled with a sentinel, GUARD token rows behind it.

    t5_kernel_worker.py <group> <out.npz>      group: attn | equal | relu | relu_wide (the parent sets AK_GEMM_BN=256 for the last)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from tests import kernel_cases as kc  # noqa: E402
from tests import kernel_refs as kr  # noqa: E402
from tests import t5_kernel_cases as tc  # noqa: E402
from tests.kernel_worker import _check, _dev, _full16, _host16, _ptr  # noqa: E402

SENT16 = int(kr.bf16_bits(np.float32(tc.SENT)).reshape(-1)[0])


def _attn_buffers(c, inp):
    B, S, H = len(c["lens"]), c["S"], c["heads"] * tc.HD
    q, k = _dev(kr.pack_token_major(inp["q"])), _dev(kr.pack_token_major(inp["k"]))
    vt = _dev(kr.pack_vt(inp["v"]))
    return B, S, H, q, k, vt, _dev(inp["mask"].astype(np.int32)), _dev(inp["lens"])


def run_attn(lib, res):
    for c in tc.ATTN_CASES:
        inp = tc.attn_inputs(c)
        B, S, H, q, k, vt, mask, lens = _attn_buffers(c, inp)
        tab = _dev(inp["tab"])
        ctx = _full16((B * S + tc.GUARD, H), SENT16)
        _check(lib, lib.ak_kts_t5_attn(_ptr(q), _ptr(k), _ptr(vt), _ptr(mask), _ptr(lens), _ptr(ctx), B, S, H, c["heads"], 0, 0, _ptr(tab),
                                       c["D"], None), c["name"])
        h = _host16(ctx)
        res[c["name"]], res[c["name"] + ":guard"] = h[:B * S].reshape(B, S, H), h[B * S:]


def run_equal(lib, res):
    """The biased kernel on an all-zero table and the un-biased one (ak_kt_attn_window, window -1) on the same inputs."""
    for c in (c for c in tc.ATTN_CASES if c["name"] in tc.EQUAL_CASES):
        inp = tc.attn_inputs(c)
        B, S, H, q, k, vt, mask, lens = _attn_buffers(c, inp)
        tab = _dev(np.zeros_like(inp["tab"]))
        a, b = (_full16((B * S, H), SENT16) for _ in range(2))
        _check(lib, lib.ak_kts_t5_attn(_ptr(q), _ptr(k), _ptr(vt), _ptr(mask), _ptr(lens), _ptr(a), B, S, H, c["heads"], 0, 0, _ptr(tab), c["D"],
                                       None), c["name"])
        _check(lib, lib.ak_kt_attn_window(_ptr(q), _ptr(k), _ptr(vt), _ptr(mask), _ptr(lens), _ptr(b), B, S, H, c["heads"], 0, 0, -1, None),
               c["name"])
        res[c["name"] + ":zero_table"], res[c["name"] + ":window"] = _host16(a), _host16(b)


def run_relu(lib, res):
    for c in tc.RELU_CASES:
        inp = kc.gemm_inputs(c)
        x, w, bias = _dev(inp["x"]), _dev(inp["w"]), _dev(inp["bias"])
        out = _full16((c["T"] + tc.GUARD, c["N"]), SENT16)
        _check(lib, lib.ak_kts_t5_gemm_relu(_ptr(x), _ptr(w), _ptr(bias), c["T"], c["N"], c["K"], _ptr(out), None), c["name"])
        h = _host16(out)
        res[c["name"]], res[c["name"] + ":guard"] = h[:c["T"]], h[c["T"]:]


def main():
    group, out = sys.argv[1], sys.argv[2]
    from archi_amd import _lib
    lib = _lib.init(0)
    assert _lib.is_dbg_library(), "the single-launch wrappers live in libarchi_hip_dbg.so (ARCHI_HIP_DBG=1)"
    assert (os.environ.get("AK_GEMM_BN") == "256") == (group == "relu_wide")
    res = {}
    {"attn": run_attn, "equal": run_equal, "relu": run_relu, "relu_wide": run_relu}[group](lib, res)
    np.savez(out, **res)


if __name__ == "__main__":
    main()
