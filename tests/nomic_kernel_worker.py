"""Child of tests/test_nomic_kernels_gpu.py, in the manner of tests/stack_kernel_worker.py: runs every case of one group through its
ak_ktn_* wrapper (libarchi_hip_dbg.so; the parent sets ARCHI_HIP_DBG=1), each case ONCE, and writes the raw outputs to one .npz
("<case>:<output>"). The float64 references are the parent's work. Any launcher error or HIP error ends the process with a non-zero
status. Every output buffer is prefilled: NaN where the kernel must write, the sentinel where it must not.

    nomic_kernel_worker.py <group> <out.npz>      group: embed | addnorm | pool"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from tests import nomic_kernel_refs as nk  # noqa: E402
from tests.kernel_worker import _check, _dev, _host16, _ptr  # noqa: E402
from tests.stack_kernel_worker import SENT16, _buf16, _buf32, _f, _host  # noqa: E402

G = nk.GUARD


def run_embed(lib, res):
    for c in nk.embed_cases():
        inp = nk.embed_inputs(c)
        B, S, H, T, n = c["B"], c["S"], c["H"], c["B"] * c["S"], c["name"]
        ids, lens, emb, typ, g, b = (_dev(inp[k]) for k in ("ids", "lens", "emb", "type", "g", "b"))
        x32, h16 = _buf32(T + G, H, T), _buf16(T + G, H, T)
        lens_out = _dev(np.full(B, nk.SENT_I, np.int32))
        mask = _dev(np.full(T + G, nk.SENT_I, np.int32))
        _check(lib, lib.ak_ktn_embed(_ptr(ids), c["ld_ids"], _ptr(lens), c["lens_stride"], B, S, H, c["vocab"], _ptr(emb), _ptr(typ), _ptr(g),
                                     _ptr(b), _f(c["eps"]), _ptr(x32), _ptr(h16), _ptr(mask), _ptr(lens_out), None), n)
        m = _host(mask)
        assert (m[T:] == nk.SENT_I).all(), n + ": mask written past B * S"
        x, h = _host(x32), _host16(h16)
        res[n + ":mask"], res[n + ":lens"] = m[:T], _host(lens_out)
        res[n + ":x32"], res[n + ":x32_guard"], res[n + ":h16"], res[n + ":h16_guard"] = x[:T], x[T:], h[:T], h[T:]


def run_addnorm(lib, res):
    for c in nk.addnorm_cases():
        inp = nk.addnorm_inputs(c)
        T, H, n = c["T"], c["H"], c["name"]
        x32, y32 = _buf32(T + G, H, T), _buf32(T + G, H, T)
        x32[:T] = _dev(inp["x"])
        y32[:T] = _dev(inp["y"])
        h16 = _buf16(T + G, H, T)
        g, b = _dev(inp["g"]), _dev(inp["b"])
        _check(lib, lib.ak_ktn_add_ln(_ptr(x32), _ptr(y32), T, H, _ptr(g), _ptr(b), _f(c["eps"]), _ptr(h16), None), n)
        x, y, h = _host(x32), _host(y32), _host16(h16)
        assert np.array_equal(y[:T].view(np.uint32), inp["y"].view(np.uint32)) and (y[T:] == nk.SENT).all(), n + ": y32 written"
        res[n + ":x32"], res[n + ":x32_guard"], res[n + ":h16"], res[n + ":h16_guard"] = x[:T], x[T:], h[:T], h[T:]


def run_pool(lib, res):
    for c in nk.pool_cases():
        inp = nk.pool_inputs(c)
        B, S, H, n = len(c["lens"]), c["S"], c["H"], c["name"]
        x, lens = _dev(inp["x"]), _dev(inp["lens"])
        nch = -(-S // 64)
        for suffix, pooling, normalise in nk.POOL_MODES:
            out = _buf32(B + 1, H, B)
            part = _buf32(B * nch + 1, H, B * nch)
            _check(lib, lib.ak_ktn_pool(_ptr(x), _ptr(lens), B, S, H, pooling, normalise, _ptr(part), _ptr(out), None), n + ":" + suffix)
            o = _host(out)
            res[f"{n}:{suffix}:out"], res[f"{n}:{suffix}:out_guard"] = o[:B], o[B:]
            assert (_host(part)[-1] == nk.SENT).all(), n + ": part written past its end"


def main(group, out):
    from archi_amd import _lib
    lib = _lib.init(0)
    assert _lib.is_dbg_library(), "the kernel-test entry points live in libarchi_hip_dbg.so (ARCHI_HIP_DBG=1)"
    res = {"dbg": np.array(1)}
    {"embed": run_embed, "addnorm": run_addnorm, "pool": run_pool}[group](lib, res)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
