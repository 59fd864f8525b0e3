"""Child of tests/test_llama_kernels_gpu.py, in the manner of tests/stack_kernel_worker.py: runs every case of one group through its
ak_kts_ll_* wrapper (libarchi_hip_dbg.so; the parent sets ARCHI_HIP_DBG=1), each case ONCE, and writes the raw outputs to one .npz. The
float64 references are the parent's work. Any launcher error or HIP error ends the process with a non-zero status. Every output buffer
is prefilled: bf16 NaN where the kernel must write, the sentinel where it must not.

    llama_kernel_worker.py <group> <out.npz>      group: attn | equal | rope | pool"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from tests import kernel_cases as kc  # noqa: E402
from tests import kernel_refs as kr  # noqa: E402
from tests import llama_kernel_cases as lc  # noqa: E402
from tests.kernel_worker import NAN_BITS, _check, _dev, _full16, _host16, _ptr  # noqa: E402

SENT16 = int(kr.bf16_bits(np.float32(lc.SENT)).reshape(-1)[0])


def run_attn(lib, res):
    for case in lc.attn_cases():
        inp = lc.attn_inputs(case)
        B, S = len(inp["lens"]), case["S"]
        q, k, v, lens = _dev(inp["q"]), _dev(inp["k"]), _dev(inp["v"]), _dev(inp["lens"])
        ctx = _full16((B, S, case["nq"] * lc.HD), NAN_BITS)
        _check(lib, lib.ak_kts_ll_attn(_ptr(q), _ptr(k), _ptr(v), _ptr(lens), _ptr(ctx), B, S, case["nq"], case["nkv"], case["window"], int(case["bidir"]), None),
               case["name"])
        res[case["name"]] = _host16(ctx)


def run_equal(lib, res):
    """launch_attn_causal as Qwen3 calls it (ak_kt_attn_causal) and through the window argument at 0 on the same inputs."""
    for case in lc.equal_cases():
        inp = kc.attn_inputs(case)
        B, S = len(inp["lens"]), case["S"]
        q, k, v, lens = _dev(inp["q"]), _dev(inp["k"]), _dev(inp["v"]), _dev(inp["lens"].astype(np.int32))
        a, b = (_full16((B, S, case["nq"] * lc.HD), NAN_BITS) for _ in range(2))
        _check(lib, lib.ak_kt_attn_causal(_ptr(q), _ptr(k), _ptr(v), _ptr(lens), _ptr(a), B, S, case["nq"], case["nkv"], None), case["name"])
        _check(lib, lib.ak_kts_ll_attn(_ptr(q), _ptr(k), _ptr(v), _ptr(lens), _ptr(b), B, S, case["nq"], case["nkv"], 0, 0, None), case["name"])
        res[case["name"] + ":qwen3"], res[case["name"] + ":window0"] = _host16(a), _host16(b)


def run_rope(lib, res):
    for c in lc.rope_cases():
        inp = lc.rope_inputs(c)
        B, S, nq, nkv = c["B"], c["S"], c["nq"], c["nkv"]
        qkv, rc, rs = _dev(inp["qkv"]), _dev(inp["rc"]), _dev(inp["rs"])
        outs = {}
        for name, heads in (("q", nq), ("k", nkv), ("v", nkv)):
            a = np.full((B * heads * S + lc.GUARD, lc.HD), SENT16, np.uint16)
            a[:B * heads * S] = NAN_BITS
            outs[name] = _dev(a)
        _check(lib, lib.ak_kts_ll_rope(_ptr(qkv), B, S, nq, nkv, _ptr(rc), _ptr(rs), ctypes.c_float(c["qscale"]), _ptr(outs["q"]), _ptr(outs["k"]),
                                       _ptr(outs["v"]), None), c["name"])
        for name, heads in (("q", nq), ("k", nkv), ("v", nkv)):
            h = _host16(outs[name])
            res[f"{c['name']}:{name}"] = h[:B * heads * S].reshape(B, heads, S, lc.HD)
            res[f"{c['name']}:{name}_guard"] = h[B * heads * S:]


def run_pool(lib, res):
    for c in lc.pool_cases():
        inp = lc.pool_inputs(c)
        B, S, H = c["B"], c["S"], c["H"]
        x, w, lens = _dev(inp["x"]), _dev(inp["w"]), _dev(inp["lens"])
        part = _dev(np.full((B * -(-S // 64), H), np.nan, np.float32))
        out = np.full((B + 1, H), lc.SENT, np.float32)
        out[:B] = np.nan
        out = _dev(out)
        _check(lib, lib.ak_kts_ll_pool(_ptr(x), _ptr(lens), B, S, H, _ptr(w), ctypes.c_float(c["eps"]), c["normalise"], _ptr(part), _ptr(out), None),
               c["name"])
        res[c["name"]] = out.cpu().numpy()


def main():
    group, out = sys.argv[1], sys.argv[2]
    from archi_amd import _lib
    lib = _lib.init(0)
    assert _lib.is_dbg_library(), "the single-launch wrappers live in libarchi_hip_dbg.so (ARCHI_HIP_DBG=1)"
    res = {}
    {"attn": run_attn, "equal": run_equal, "rope": run_rope, "pool": run_pool}[group](lib, res)
    np.savez(out, **res)


if __name__ == "__main__":
    main()
