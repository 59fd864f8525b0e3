"""Child of tests/test_gemma_kernels_gpu.py, in the manner of tests/kernel_worker.py: runs every case of one group through its
ak_ktg_* wrapper (libarchi_hip_dbg.so; the parent sets ARCHI_HIP_DBG=1), each case ONCE, and writes the raw outputs to one .npz. The
float64 references are the parent's work. Any launcher error or HIP error ends the process with a non-zero status.

    gemma_kernel_worker.py <group> <out.npz>      group: gqa | rope | geglu"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from tests import gemma_kernel_cases as gc  # noqa: E402
from tests import kernel_refs as kr  # noqa: E402
from tests.kernel_worker import NAN_BITS, _check, _dev, _full16, _host16, _ptr  # noqa: E402


def run_gqa(lib, res):
    for case in gc.gqa_cases():
        inp = gc.gqa_inputs(case)
        B, S, nq, nkv = len(inp["lens"]), case["S"], case["nq"], case["nkv"]
        q, k = _dev(kr.pack_head_major(inp["q"])), _dev(kr.pack_head_major(inp["k"]))
        vt = _dev(kr.pack_vt(inp["v"]))                    # [B][nkv * 256][S], vt_pos order
        lens = _dev(inp["lens"].astype(np.int32))
        ctx = _full16((B, S, nq * gc.HD), NAN_BITS)
        _check(lib, lib.ak_ktg_attn_gqa(_ptr(q), _ptr(k), _ptr(vt), _ptr(lens), _ptr(ctx), B, S, nq, nkv, case["half_window"], None), case["name"])
        res[case["name"]] = _host16(ctx)


def run_rope(lib, res):
    for c in gc.ROPE_CASES:
        inp = gc.rope_inputs(c)
        B, S, nq, nkv = c["B"], c["S"], c["nq"], c["nkv"]
        rc, rs = np.empty((S, 128), np.float32), np.empty((S, 128), np.float32)
        assert lib.ak_decoder_rope_table(ctypes.c_float(c["theta"]), gc.HD, S, rc.ctypes.data, rs.ctypes.data) == 0
        qkv, qn, kn, drc, drs = _dev(inp["qkv"]), _dev(inp["qn"]), _dev(inp["kn"]), _dev(rc), _dev(rs)
        q, k, vt = _full16((B, nq, S, gc.HD), NAN_BITS), _full16((B, nkv, S, gc.HD), NAN_BITS), _full16((B, nkv * gc.HD, S), NAN_BITS)
        _check(lib, lib.ak_ktg_qk_norm_rope(_ptr(qkv), B, S, nq, nkv, _ptr(qn), _ptr(kn), gc.ROPE_EPS, _ptr(drc), _ptr(drs), c["qscale"],
                                            _ptr(q), _ptr(k), _ptr(vt), None), c["name"])
        res[c["name"] + ":q"], res[c["name"] + ":k"], res[c["name"] + ":vt"] = _host16(q), _host16(k), _host16(vt)
        res[c["name"] + ":rc"], res[c["name"] + ":rs"] = rc, rs


def run_geglu(lib, res):
    from tests import kernel_cases as kc
    for c in gc.GEGLU_CASES:
        inp = kc.gemm_inputs(c)
        x, w, bias = _dev(inp["x"]), _dev(inp["w"]), _dev(inp["bias"])
        out = _full16((c["T"], c["N"] // 2), NAN_BITS)
        _check(lib, lib.ak_ktg_gemm_geglu_tanh(_ptr(x), _ptr(w), _ptr(bias), c["T"], c["N"], c["K"], _ptr(out), None), c["name"])
        res[c["name"]] = _host16(out)


def main(group, out):
    from archi_amd import _lib
    lib = _lib.init(0)
    assert _lib.is_dbg_library(), "the kernel-test entry points live in libarchi_hip_dbg.so (ARCHI_HIP_DBG=1)"
    res = {"dbg": np.array(1)}
    {"gqa": run_gqa, "rope": run_rope, "geglu": run_geglu}[group](lib, res)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
