"""Child of tests/test_parity_kernels_gpu.py: runs every case of one group through its ak_ktp_* wrapper (libarchi_hip_dbg.so; the parent
sets ARCHI_HIP_DBG=1 and, for the wide-tile child of launch_gemm_x3w, AK_GEMM_BN=256), each case ONCE, and writes the raw outputs to one
.npz. The float64 references are the parent's work. A launcher error or a HIP error ends the process with a non-zero status, except
where a case asks for the error code: that code is what is stored.

    parity_kernel_worker.py <group> <out.npz>      group: gemm | attn | rows | x3w | x3w_wide"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from tests import parity_kernel_cases as pc  # noqa: E402
from tests import parity_kernel_refs as pr  # noqa: E402
from tests.kernel_worker import _check, _dev, _full16, _host16  # noqa: E402


def _p(t):
    return None if t is None else t.data_ptr()


def _f32(shape, value):
    import torch
    return torch.full(shape, value, dtype=torch.float32, device="cuda")


def run_gemm(lib, res):
    for c in pc.gemm_cases():
        inp = pc.gemm_inputs(c)
        T, N, K, epi = c["T"], c["N"], c["K"], c["epi"]
        x, w, bias = _dev(inp["x"]), _dev(inp["w"]), _dev(inp["bias"])
        r = _dev(inp["res"]) if inp["res"] is not None else None
        whi, wlo = (_dev(b) for b in pr.split_bits(inp["w"]))
        for which in ("f32", "x3"):
            y = _f32((T + pc.PAD_ROWS, c["ldc"]), pc.SENT)
            if which == "f32":
                rc = lib.ak_ktp_gemm_f32(epi, _p(x), _p(w), _p(bias), _p(r), T, N, K, _p(y), c["ldc"], c["col0"], None)
            else:
                rc = lib.ak_ktp_gemm_x3(epi, _p(x), _p(whi), _p(wlo), _p(bias), _p(r), T, N, K, _p(y), c["ldc"], c["col0"], None)
            _check(lib, rc, f"{c['name']} ({which})")
            res[f"{c['name']}:{which}"] = y.cpu().numpy()
        if epi != 2:                                  # the scalar kernel the comment of k32m_gemm names as its cross-check
            y = _f32((T, N), pc.SENT)
            _check(lib, lib.ak_ktp_gemm_f32_scalar(epi, _p(x), _p(w), _p(bias), T, N, K, _p(y), None), c["name"] + " (scalar)")
            res[c["name"] + ":scalar"] = y.cpu().numpy()
    for i, c in enumerate(pc.gemm_refused()):
        T, N, K = c["T"], c["N"], c["K"]
        x, w, bias, y = _f32((T, K), 0.0), _f32((N, K), 0.0), _f32((N,), 0.0), _f32((T, N), pc.SENT)
        w16 = _full16((N, K), 0)
        res[f"refused{i}:f32"] = np.array(lib.ak_ktp_gemm_f32(0, _p(x), _p(w), _p(bias), None, T, N, K, _p(y), N, 0, None))
        res[f"refused{i}:x3"] = np.array(lib.ak_ktp_gemm_x3(0, _p(x), _p(w16), _p(w16), _p(bias), None, T, N, K, _p(y), N, 0, None))
        res[f"refused{i}:y"] = y.cpu().numpy()


def run_attn(lib, res):
    import torch
    for c in pc.attn_cases():
        inp = pc.attn_inputs(c)
        B, S, heads, H = c["B"], c["S"], c["heads"], c["heads"] * c["hd"]
        qkv, mask = _dev(inp["qkv"]), _dev(inp["mask"].astype(np.int32))
        rel = _dev(inp["rel"]) if inp["rel"] is not None else None
        rel2 = _dev(pc.attn_rel_base2(inp["rel"])) if inp["rel"] is not None else None
        ctx = _f32((B * S, H), float("nan"))
        _check(lib, lib.ak_ktp_attn_f32(_p(qkv), _p(mask), B, S, H, heads, _p(ctx), _p(rel), None), c["name"] + " (f32)")
        res[c["name"] + ":f32"] = ctx.cpu().numpy()
        ctx = _f32((B * S, H), float("nan"))
        _check(lib, lib.ak_ktp_attn_x3(_p(qkv), _p(mask), B, S, H, heads, _p(ctx), _p(rel2), None), c["name"] + " (x3)")
        res[c["name"] + ":x3"] = ctx.cpu().numpy()
        ldq = 3 * H + pc.SPLIT_LDQ_PAD                # wider rows, the padding never read: NaN there
        wide = _f32((B * S, ldq), float("nan"))
        wide[:, :3 * H] = qkv
        ctx2 = _full16((B * S, 2 * H), 0x7FC0)
        _check(lib, lib.ak_ktp_attn_x3_split(_p(wide), ldq, _p(mask), B, S, H, heads, _p(ctx2), _p(rel2), None), c["name"] + " (x3_split)")
        res[c["name"] + ":x3_split"] = _host16(ctx2)
    # head size 48: the launchers' own error code
    qkv, mask, ctx, ctx2 = _f32((32, 3 * 96), 0.0), torch.ones((1, 32), dtype=torch.int32, device="cuda"), _f32((32, 96), pc.SENT), _full16((32, 192), pc.SENT16)
    res["hd48:f32"] = np.array(lib.ak_ktp_attn_f32(_p(qkv), _p(mask), 1, 32, 96, 2, _p(ctx), None, None))
    res["hd48:x3"] = np.array(lib.ak_ktp_attn_x3(_p(qkv), _p(mask), 1, 32, 96, 2, _p(ctx), None, None))
    res["hd48:x3_split"] = np.array(lib.ak_ktp_attn_x3_split(_p(qkv), 3 * 96, _p(mask), 1, 32, 96, 2, _p(ctx2), None, None))
    torch.cuda.synchronize()
    res["hd48:ctx"], res["hd48:ctx2"] = ctx.cpu().numpy(), _host16(ctx2)


def run_rows(lib, res):
    for c in pc.split_cases():
        x = pc.split_inputs(c)
        xd = _dev(x)
        if c["kind"] == "hilo":
            hi, lo = _full16((c["n"] + 8,), pc.SENT16), _full16((c["n"] + 8,), pc.SENT16)
            _check(lib, lib.ak_ktp_split_hilo(_p(xd), c["n"], _p(hi), _p(lo), None), c["name"])
            res[c["name"] + ":hi"], res[c["name"] + ":lo"] = _host16(hi), _host16(lo)
        else:
            out = _full16((c["rows"] + 1, 2 * c["K"]), pc.SENT16)
            _check(lib, lib.ak_ktp_split_rows(_p(xd), c["rows"], c["K"], _p(out), None), c["name"])
            res[c["name"]] = _host16(out)
    for c in pc.embed_cases():
        inp = pc.embed_inputs(c)
        T, H = c["T"], c["H"]
        d = {k: _dev(inp[k]) for k in ("ids", "word", "pos", "type", "gamma", "beta")}
        posid = _dev(inp["posid"]) if inp["posid"] is not None else None
        out = _f32((T + 1, H), pc.SENT)
        _check(lib, lib.ak_ktp_embed_f32(_p(d["ids"]), T, c["S"], H, pc.VOCAB, _p(d["word"]), _p(d["pos"]), _p(d["type"]), _p(d["gamma"]), _p(d["beta"]),
                                         c["eps"], _p(out), _p(posid), None), c["name"] + " (f32)")
        res[c["name"] + ":f32"] = out.cpu().numpy()
        out, out2 = _f32((T + 1, H), pc.SENT), _full16((T + 1, 2 * H), pc.SENT16)
        _check(lib, lib.ak_ktp_embed_split(_p(d["ids"]), T, c["S"], H, pc.VOCAB, _p(d["word"]), _p(d["pos"]), _p(d["type"]), _p(d["gamma"]), _p(d["beta"]),
                                           c["eps"], _p(out), _p(out2), _p(posid), None), c["name"] + " (split)")
        res[c["name"] + ":out"], res[c["name"] + ":out2"] = out.cpu().numpy(), _host16(out2)
    for c in pc.add_ln_cases():
        inp = pc.add_ln_inputs(c)
        T, H, ldy = c["T"], c["H"], c["H"] + c["pad"]
        g, b = _dev(inp["gamma"]), _dev(inp["beta"])
        # the float32 launch: rows of H, in place over y when the case says so (forward_f32 writes the LayerNorm into x, its residual)
        y = _dev(inp["y"])
        r = _dev(inp["r"]) if inp["r"] is not None else None
        out = r if c["r"] == "inplace" else _f32((T + 1, H), pc.SENT)
        _check(lib, lib.ak_ktp_add_ln_f32(_p(y), _p(r), T, H, _p(g), _p(b), c["eps"], _p(out), None), c["name"] + " (f32)")
        res[c["name"] + ":f32"] = out.cpu().numpy()
        # the split launch: y rows of ldy floats (NaN in the padding), r rows of H
        yw = _f32((T, ldy), float("nan"))
        yw[:, :H] = _dev(inp["y"])
        r = _dev(inp["r"]) if inp["r"] is not None else None
        out = r if c["r"] == "inplace" else _f32((T + 1, H), pc.SENT)
        out2 = _full16((T + 1, 2 * H), pc.SENT16)
        _check(lib, lib.ak_ktp_add_ln_split(_p(yw), ldy, _p(r), T, H, _p(g), _p(b), c["eps"], _p(out), _p(out2), None), c["name"] + " (split)")
        res[c["name"] + ":out"], res[c["name"] + ":out2"] = out.cpu().numpy(), _host16(out2)
    for c in pc.pool_cases():
        inp = pc.pool_inputs(c)
        x, mask = _dev(inp["x"]), _dev(inp["mask"])
        for pooling, normalise in pc.POOL_MODES:
            out = _f32((c["B"] + 1, c["H"]), pc.SENT)
            _check(lib, lib.ak_ktp_pool_f32(_p(x), _p(mask), c["B"], c["S"], c["H"], pooling, normalise, _p(out), None), c["name"])
            res[f"{c['name']}:{pooling}{normalise}"] = out.cpu().numpy()
    for c in pc.gemm_ln_x3_cases():
        inp = pc.gemm_ln_x3_inputs(c)
        d = {k: _dev(inp[k]) for k in ("x2", "w2", "bias", "gamma", "beta", "res")}
        x16 = _full16((c["T"], 2 * 384), 0x7FC0)
        _check(lib, lib.ak_ktp_gemm_ln_x3(_p(d["x2"]), _p(d["w2"]), _p(d["bias"]), _p(d["gamma"]), _p(d["beta"]), _p(d["res"]), _p(x16), c["T"], c["K1"],
                                          c["eps"], None), c["name"])
        res[c["name"] + ":x32"], res[c["name"] + ":x16"] = d["res"].cpu().numpy(), _host16(x16)


def run_x3w(lib, res, child):
    for c in pc.x3w_cases(child):
        inp = pc.x3w_inputs(c)
        T, N = c["T"], c["N"]
        x2, w2, bias = _dev(inp["x2"]), _dev(inp["w2"]), _dev(inp["bias"])
        if c["mode"] == 5:
            out = _f32((T, N), pc.SENT)
            _check(lib, lib.ak_ktp_gemm_x3w(5, _p(x2), _p(w2), _p(bias), T, N, c["K1"], _p(out), None, c["nvalid"], None), c["name"])
            res[c["name"]] = out.cpu().numpy()
        else:
            out = _full16((T, 2 * N), 0x7FC0)
            _check(lib, lib.ak_ktp_gemm_x3w(6, _p(x2), _p(w2), _p(bias), T, N, c["K1"], None, _p(out), c["nvalid"], None), c["name"])
            res[c["name"]] = _host16(out)


def main(group, out):
    from archi_amd import _lib
    lib = _lib.init(0)
    assert _lib.is_dbg_library(), "the kernel-test entry points live in libarchi_hip_dbg.so (ARCHI_HIP_DBG=1)"
    res = {"dbg": np.array(1)}
    if group == "gemm":
        run_gemm(lib, res)
    elif group == "attn":
        run_attn(lib, res)
    elif group == "rows":
        run_rows(lib, res)
    elif group in ("x3w", "x3w_wide"):
        run_x3w(lib, res, "wide" if group == "x3w_wide" else "default")
    else:
        raise SystemExit(f"unknown group {group}")
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
