"""Child of tests/test_stack_kernels_gpu.py, in the manner of tests/gemma_kernel_worker.py: runs every case of one group through its
ak_kts_* wrapper (libarchi_hip_dbg.so; the parent sets ARCHI_HIP_DBG=1), each case ONCE, and writes the raw outputs to one .npz
("<case>:<output>"); NomicBERT's cases (tests/nomic_kernel_refs.py, family `nb`) run in the embed, addnorm and pool groups behind the
other families'. The float64 references are the parent's work. Any launcher error or HIP error ends the process with a non-zero
status. Every output buffer is prefilled: NaN where the kernel must write, the sentinel where it must not.

    stack_kernel_worker.py <group> <out.npz>      group: embed | addnorm | rope | pool | tail | gemm3"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from tests import kernel_cases as kc  # noqa: E402
from tests import kernel_refs as kr  # noqa: E402
from tests import nomic_kernel_refs as nk  # noqa: E402
from tests import stack_kernel_cases as sc  # noqa: E402
from tests.kernel_worker import NAN_BITS, _check, _dev, _host16, _ptr  # noqa: E402

SENT16 = int(kr.bf16_bits(np.float32(sc.SENT)).reshape(-1)[0])
G = sc.GUARD


def _buf32(rows, H, real, fill=np.nan):
    """[rows][H] float32 on the device: `fill` in the first `real` rows, the sentinel behind them."""
    a = np.full((rows, H), sc.SENT, np.float32)
    a[:real] = fill
    return _dev(a)


def _buf16(rows, H, real, bits=NAN_BITS):
    a = np.full((rows, H), SENT16, np.uint16)
    a[:real] = bits
    return _dev(a)


def _f(v):
    return ctypes.c_float(v)


def _host(t):
    return t.cpu().numpy()


def run_embed(lib, res):
    for c in sc.embed_cases() + nk.embed_cases():
        inp = nk.embed_inputs(c) if c["fam"] == "nb" else sc.embed_inputs(c)
        B, S, H, T = c["B"], c["S"], c["H"], c["B"] * c["S"]
        ids, lens, emb = _dev(inp["ids"]), _dev(inp["lens"]), _dev(inp["emb"])
        norm = [_dev(inp[k]) for k in (("type", "g", "b") if c["fam"] == "nb" else ("w",))]      # the table and norm operands behind emb
        x32, h16 = _buf32(T + G, H, T), _buf16(T + G, H, T)
        lens_out = _dev(np.full(B, sc.SENT_I, np.int32))
        head = (_ptr(ids), c["ld_ids"], _ptr(lens), c["lens_stride"], B, S, H, c["vocab"], _ptr(emb), *map(_ptr, norm), _f(c["eps"]), _ptr(x32),
                _ptr(h16))
        n = c["name"]
        if c["fam"] in ("mb", "nb"):
            mask = _dev(np.full(T + G, sc.SENT_I, np.int32))
            _check(lib, getattr(lib, f"ak_kts_{c['fam']}_embed")(*head, _ptr(mask), _ptr(lens_out), None), n)
            m = _host(mask)
            assert (m[T:] == sc.SENT_I).all(), n + ": mask written past B * S"
            res[n + ":mask"] = m[:T]
        else:
            _check(lib, getattr(lib, f"ak_kts_{c['fam']}_embed")(*head, _ptr(lens_out), None), n)
        x, h = _host(x32), _host16(h16)
        res[n + ":x32"], res[n + ":x32_guard"], res[n + ":h16"], res[n + ":h16_guard"] = x[:T], x[T:], h[:T], h[T:]
        res[n + ":lens"] = _host(lens_out)


def run_addnorm(lib, res):
    for c in sc.addnorm_cases() + nk.addnorm_cases():
        fam, n = c["fam"], c["name"]
        inp = nk.addnorm_inputs(c) if fam == "nb" else sc.addnorm_inputs(c)
        T, H, form = c["T"], c["H"], c.get("form", "norm")
        x32, y32 = _buf32(T + G, H, T), _buf32(T + G, H, T)
        x32[:T] = _dev(inp["x"])
        y32[:T] = _dev(inp["y"])
        h16 = _buf16(T + G, H, 0 if form in ("add", "out32") else T)
        if fam == "nb":
            g, b = _dev(inp["g"]), _dev(inp["b"])
            _check(lib, lib.ak_kts_nb_add_ln(_ptr(x32), _ptr(y32), T, H, _ptr(g), _ptr(b), _f(c["eps"]), _ptr(h16), None), n)
        elif fam == "gm":
            w, wp = _dev(inp["w"]), _dev(inp["w_post"])
            _check(lib, lib.ak_kts_gm_norm_add_norm(_ptr(x32), _ptr(y32), T, H, _ptr(wp), _ptr(w), _f(c["eps"]), _ptr(h16),
                                                    _ptr(y32) if form == "out32" else None, None), n)
        else:
            w = _dev(inp["w"])
            fn = lib.ak_kts_dec_add_rmsnorm if fam == "dec" else lib.ak_kts_mb_add_ln
            _check(lib, fn(_ptr(x32), _ptr(y32), T, H, None if form == "add" else _ptr(w), _f(c["eps"]), _ptr(h16), None), n)
        x, y, h = _host(x32), _host(y32), _host16(h16)
        if fam == "nb":
            assert np.array_equal(y[:T].view(np.uint32), inp["y"].view(np.uint32)) and (y[T:] == nk.SENT).all(), n + ": y32 written"
        res[n + ":x32"], res[n + ":x32_guard"] = x[:T], x[T:]
        if form == "add":
            res[n + ":h16"] = h
        elif form == "out32":
            res[n + ":y32"], res[n + ":y32_guard"] = y[:T], y[T:]
            assert (h == SENT16).all(), n + ": h16 written in the float32 form"
        else:
            res[n + ":h16"], res[n + ":h16_guard"] = h[:T], h[T:]


def rope_tables(lib, c, n_pos=None):
    """The float32 tables of ak_decoder_rope_table at the case's theta and head size (host only)."""
    n_pos = n_pos or c["S"]
    rc, rs = np.empty((n_pos, c["hd"] // 2), np.float32), np.empty((n_pos, c["hd"] // 2), np.float32)
    assert lib.ak_decoder_rope_table(ctypes.c_float(c["theta"]), c["hd"], n_pos, rc.ctypes.data, rs.ctypes.data) == 0
    return rc, rs


def run_rope(lib, res):
    for c in sc.rope_cases():
        inp = sc.rope_inputs(c)
        B, S, hd, n = c["B"], c["S"], c["hd"], c["name"]
        T = B * S
        rc, rs = rope_tables(lib, c)
        drc, drs = _dev(rc), _dev(rs)
        res[n + ":rc"], res[n + ":rs"] = rc, rs
        if c["fam"] == "mb":
            H = c["H"]
            q, k = _buf16(T + G, H, T), _buf16(T + G, H, T)
            q[:T] = _dev(inp["q"])
            k[:T] = _dev(inp["k"])
            _check(lib, lib.ak_kts_mb_rope(_ptr(q), _ptr(k), T, S, H, _ptr(drc), _ptr(drs), None), n)
            for name, t in (("q", q), ("k", k)):
                h = _host16(t)
                res[f"{n}:{name}"], res[f"{n}:{name}_guard"] = h[:T], h[T:]
            continue
        nq, nkv = c["nq"], c["nkv"]
        qkv, qn, kn = _dev(inp["qkv"]), _dev(inp["qn"]), _dev(inp["kn"])
        q, k, v = _buf16(B * nq * S + 1, hd, B * nq * S), _buf16(B * nkv * S + 1, hd, B * nkv * S), _buf16(B * nkv * S + 1, hd, B * nkv * S)
        _check(lib, lib.ak_kts_dec_qk_rope(_ptr(qkv), B, S, nq, nkv, _ptr(qn), _ptr(kn), _f(sc.ROPE_EPS), _ptr(drc), _ptr(drs), _f(c["qscale"]),
                                           _ptr(q), _ptr(k), _ptr(v), None), n)
        for name, t, heads in (("q", q, nq), ("k", k, nkv), ("v", v, nkv)):
            h = _host16(t)
            res[f"{n}:{name}"], res[f"{n}:{name}_guard"] = h[:-1].reshape(B, heads, S, hd), h[-1:]


def run_pool(lib, res):
    for c in sc.pool_cases() + nk.pool_cases():
        inp = nk.pool_inputs(c) if c["fam"] == "nb" else sc.pool_inputs(c)
        B, S, H, fam, n = len(c["lens"]), c["S"], c["H"], c["fam"], c["name"]
        x, lens, w = _dev(inp["x"]), _dev(inp["lens"]), _dev(inp["w"])
        nch = -(-S // 64)
        for suffix, pooling, normalise in (nk.POOL_MODES if fam == "nb" else sc.pool_modes(c)):
            out = _buf32(B + 1, H, B)
            part = _buf32(B * nch + 1, H, B * nch)
            if fam == "dec":
                rc = lib.ak_kts_dec_pool(_ptr(x), _ptr(lens), B, S, H, _ptr(w), _f(c["eps"]), normalise, _ptr(out), None)
            elif fam == "mb":
                rc = lib.ak_kts_mb_pool(_ptr(x), _ptr(lens), B, S, H, _f(c["eps"]), _ptr(w), pooling, normalise, _ptr(part), _ptr(out), None)
            elif fam == "nb":
                rc = lib.ak_kts_nb_pool(_ptr(x), _ptr(lens), B, S, H, pooling, normalise, _ptr(part), _ptr(out), None)
            else:
                rc = lib.ak_kts_gm_pool(_ptr(x), _ptr(lens), B, S, H, _ptr(part), _ptr(out), None)
            _check(lib, rc, n + ":" + suffix)
            o = _host(out)
            res[f"{n}:{suffix}:out"], res[f"{n}:{suffix}:out_guard"] = o[:B], o[B:]
            assert (_host(part)[-1] == sc.SENT).all(), n + ": part written past its end"


def run_tail(lib, res):
    for c in sc.dense_cases():
        inp = sc.dense_inputs(c)
        B, N, K, n = c["B"], c["N"], c["K"], c["name"]
        x, w = _dev(inp["x"]), _dev(inp["w"])
        out = _dev(np.concatenate([np.full(B * N, np.nan, np.float32), np.full(8, sc.SENT, np.float32)]))
        _check(lib, lib.ak_kts_gm_dense(_ptr(x), _ptr(w), B, N, K, _ptr(out), None), n)
        o = _host(out)
        res[n + ":out"], res[n + ":out_guard"] = o[:B * N].reshape(B, N), o[B * N:].reshape(1, 8)
    for c in sc.l2_cases():
        inp = sc.l2_inputs(c)
        x = _dev(inp["x"])
        out = _buf32(c["B"], c["D"], c["B"])
        _check(lib, lib.ak_kts_gm_l2(_ptr(x), c["B"], c["D"], c["normalise"], _ptr(out), None), c["name"])
        res[c["name"] + ":out"] = _host(out)
    w = _dev(sc.fold_inputs()["w"])
    out = _dev(np.concatenate([np.full(sc.FOLD_N, np.nan, np.float32), np.full(8, sc.SENT, np.float32)]))
    _check(lib, lib.ak_kts_gm_fold1p(_ptr(w), sc.FOLD_N, _ptr(out), None), "fold1p")
    o = _host(out)
    res["fold1p:out"], res["fold1p:out_guard"] = o[:sc.FOLD_N], o[sc.FOLD_N:]


def run_gemm3(lib, res):
    from tests.kernel_worker import _full16
    for c in sc.gemm3_cases():
        inp = kc.gemm_inputs(c)
        x, w, bias = _dev(inp["x"]), _dev(inp["w"]), _dev(inp["bias"])
        out = _full16((c["T"], c["N"]), NAN_BITS)
        _check(lib, lib.ak_kts_gemm_bf16(_ptr(x), _ptr(w), _ptr(bias), c["T"], c["N"], c["K"], _ptr(out), None), c["name"])
        res[c["name"] + ":out"] = _host16(out)


def main(group, out):
    from archi_amd import _lib
    lib = _lib.init(0)
    assert _lib.is_dbg_library(), "the kernel-test entry points live in libarchi_hip_dbg.so (ARCHI_HIP_DBG=1)"
    res = {"dbg": np.array(1)}
    {"embed": run_embed, "addnorm": run_addnorm, "rope": run_rope, "pool": run_pool, "tail": run_tail, "gemm3": run_gemm3}[group](lib, res)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
