"""Child of tests/test_kernels_gpu.py: runs every case of one group through its ak_kt_* wrapper (libarchi_hip_dbg.so; the parent sets
ARCHI_HIP_DBG=1 and, for the A/B alternates of launch_attn, AK_ATTN_STREAM), each case ONCE, and writes the raw outputs to one .npz.
The float64 references are the parent's work. Any launcher error or HIP error ends the process with a non-zero status.

    kernel_worker.py <group> <out.npz>      group: window | long | attn | causal | gemm | skinny | lnfused | lnfused_forced | lnfused_w4 | identity

`identity` is the odd one: one fixture forward each of the BERT encoder, the decoder and ModernBERT through whichever library the
environment selects (the parent runs it under both and compares bit for bit)."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from tests import kernel_cases as kc  # noqa: E402
from tests import kernel_refs as kr  # noqa: E402

NAN_BITS = 0x7FC0            # outputs are prefilled with bf16 NaN: a row the kernel does not write cannot pass for finite


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _host16(t):
    return t.cpu().numpy().view(np.uint16)


def _full16(shape, bits):
    import torch
    return torch.full(shape, int(np.asarray(bits, np.uint16).reshape(-1).view(np.int16)[0]), dtype=torch.int16, device="cuda")


def _check(lib, rc, what):
    from archi_amd import _lib
    import torch
    _lib.check(rc, what)
    torch.cuda.synchronize()


def run_attention(lib, group, res):
    import torch
    cases = {"window": kc.window_cases, "long": kc.long_cases, "attn": kc.attn_cases, "causal": kc.causal_cases}[group]()
    default_selection = not os.environ.get("AK_ATTN_STREAM")
    for case in cases:
        inp = kc.attn_inputs(case)
        B, S, hd, heads = len(inp["lens"]), case["S"], case["hd"], case["heads"]
        H = heads * hd
        pos = np.array([lib.ak_kt_vt_pos(s) for s in range(S)])
        ctx = _full16((B, S, H), NAN_BITS)
        if group == "causal":
            q, k, v = _dev(kr.pack_head_major(inp["q"])), _dev(kr.pack_head_major(inp["k"])), _dev(kr.pack_head_major(inp["v"]))
            lens = _dev(inp["lens"].astype(np.int32))
            _check(lib, lib.ak_kt_attn_causal(_ptr(q), _ptr(k), _ptr(v), _ptr(lens), _ptr(ctx), B, S, case["nq"], case["nkv"], None), case["name"])
            res[case["name"]] = _host16(ctx)
            continue
        if case.get("layout") == "head":
            q, k, ld, hs = _dev(kr.pack_head_major(inp["q"])), _dev(kr.pack_head_major(inp["k"])), hd, S * hd
        else:
            q, k, ld, hs = _dev(kr.pack_token_major(inp["q"])), _dev(kr.pack_token_major(inp["k"])), 0, 0
        vt = _dev(kr.pack_vt(inp["v"], pos))
        mask = _dev(inp["mask"].astype(np.int32))
        rowlen = _dev(inp["rowlen"].astype(np.int32))
        if group == "window":
            rc = lib.ak_kt_attn_window(_ptr(q), _ptr(k), _ptr(vt), _ptr(mask), _ptr(rowlen), _ptr(ctx), B, S, H, heads, ld, hs, case["window"], None)
        elif group == "long":
            rc = lib.ak_kt_attn_long(_ptr(q), _ptr(k), _ptr(vt), _ptr(mask), _ptr(rowlen), _ptr(ctx), B, S, H, heads, ld, hs, None)
        else:
            rel = _dev(inp["rel"]) if inp["rel"] is not None else None
            maskf = torch.empty((B, S), dtype=torch.float32, device="cuda")
            blk = torch.zeros(B, dtype=torch.int32, device="cuda")
            rc = lib.ak_kt_attn(_ptr(q), _ptr(k), _ptr(vt), _ptr(mask), _ptr(ctx), B, S, H, heads, ld, hs, _ptr(rel), _ptr(maskf), _ptr(blk), 0, None)
            if rc == 0 and default_selection:           # ... and once more without the prepared mask: the unstreamed k_attn
                _check(lib, rc, case["name"])
                res[case["name"]] = _host16(ctx)
                ctx = _full16((B, S, H), NAN_BITS)
                rc = lib.ak_kt_attn(_ptr(q), _ptr(k), _ptr(vt), _ptr(mask), _ptr(ctx), B, S, H, heads, ld, hs, _ptr(rel), None, None, 1, None)
                _check(lib, rc, case["name"] + " (unstreamed)")
                res[case["name"] + "|unstreamed"] = _host16(ctx)
                continue
        _check(lib, rc, case["name"])
        res[case["name"]] = _host16(ctx)


def run_gemm(lib, res):
    import torch
    from archi_amd._lib import AkKtGemm
    for c in kc.gemm_cases():
        inp = kc.gemm_inputs(c)
        T, N, K, mode = c["T"], c["N"], c["K"], c["mode"]
        x, w, bias = _dev(inp["x"]), _dev(inp["w"]), _dev(inp["bias"])
        g = AkKtGemm()
        g.X, g.W, g.bias, g.T, g.N, g.K = x.data_ptr(), w.data_ptr(), bias.data_ptr(), T, N, K
        keep = {}
        if mode == 0:
            H, S = c["H"], c["S"]
            keep = dict(q=_full16((T, H), NAN_BITS), k=_full16((T, H), NAN_BITS), vt=_full16((T // S, H, S), kr.bf16_bits(np.float32(kc.SENTINEL))))
            g.q, g.k, g.vt, g.H, g.S, g.qscale, g.ldo = keep["q"].data_ptr(), keep["k"].data_ptr(), keep["vt"].data_ptr(), H, S, kc.qscale(c), c["ldo"]
        elif mode == 2:
            keep = dict(out=torch.full((T, N), float("nan"), dtype=torch.float32, device="cuda"))
            g.out_f32 = keep["out"].data_ptr()
        else:
            ldo = N // 2 if mode in (7, 8) else N
            keep = dict(out=_full16((T, ldo), NAN_BITS))
            g.out_bf16, g.ldo = keep["out"].data_ptr(), ldo
            if mode == 4:
                res16 = _dev(inp["res"])
                g.res16 = res16.data_ptr()
        _check(lib, lib.ak_kt_gemm(mode, ctypes.byref(g), None), c["name"])
        for name, t in keep.items():
            res[f"{c['name']}:{name}"] = t.cpu().numpy() if t.dtype == torch.float32 else _host16(t)


def run_skinny(lib, res):
    import torch
    for c in kc.skinny_cases():
        inp = kc.gemm_inputs(c)
        rows, N, K = c["rows"], c["N"], c["K"]
        x, w, bias = _dev(inp["x"]), _dev(inp["w"]), _dev(inp["bias"])
        if c["kind"] == "f32":
            out = torch.full((rows, N), float("nan"), dtype=torch.float32, device="cuda")
            _check(lib, lib.ak_kt_gemm_skinny(_ptr(x), _ptr(w), _ptr(bias), rows, N, K, _ptr(out), None, 0, None), c["name"])
            res[c["name"] + ":out"] = out.cpu().numpy()
        elif c["kind"] == "gelu":
            out = _full16((rows, N), NAN_BITS)
            _check(lib, lib.ak_kt_gemm_skinny(_ptr(x), _ptr(w), _ptr(bias), rows, N, K, None, _ptr(out), N, None), c["name"])
            res[c["name"] + ":out"] = _host16(out)
        else:
            H, S = c["H"], c["S"]
            q, k = _full16((rows, H), NAN_BITS), _full16((rows, H), NAN_BITS)
            vt = _full16((rows // S, H, S), kr.bf16_bits(np.float32(kc.SENTINEL)))
            _check(lib, lib.ak_kt_gemm_skinny_qkv(_ptr(x), _ptr(w), _ptr(bias), rows, H, K, _ptr(q), _ptr(k), _ptr(vt), S, c["Treal"],
                                                  kc.qscale(c), None), c["name"])
            res[c["name"] + ":q"], res[c["name"] + ":k"], res[c["name"] + ":vt"] = _host16(q), _host16(k), _host16(vt)


def _f32(shape, value=float("nan")):
    import torch
    return torch.full(shape, value, dtype=torch.float32, device="cuda")


def _sentinel16(shape):
    return _full16(shape, kr.bf16_bits(np.float32(kc.SENTINEL)))


def run_gemm_ln(lib, res):
    for c in kc.gemm_ln_cases():
        inp = kc.gemm_ln_inputs(c)
        T, K = c["T"], c["K"]
        x, w, bias, g, b = _dev(inp["x"]), _dev(inp["w"]), _dev(inp["bias"]), _dev(inp["gamma"]), _dev(inp["beta"])
        if c["res"] == "f32":
            x32, x16 = _dev(inp["res"]), _full16((T, kc.LN_H), NAN_BITS)
        else:
            x32, x16 = None, _dev(kr.bf16_bits(inp["res"]))
        _check(lib, lib.ak_kt_gemm_ln(_ptr(x), _ptr(w), _ptr(bias), _ptr(g), _ptr(b), _ptr(x32), _ptr(x16), T, K, c["eps"], None), c["name"])
        res[c["name"] + ":x16"] = _host16(x16)
        if x32 is not None:
            res[c["name"] + ":x32"] = x32.cpu().numpy()


def run_layernorms(lib, res):
    """The stand-alone LayerNorm launches with the buffers aliased the way the forward pass aliases them, ln_finalize, fold_ln."""
    for c in kc.layernorm_cases():
        inp = kc.layernorm_inputs(c)
        T, H = c["T"], c["H"]
        g, b = _dev(inp["gamma"]), _dev(inp["beta"])
        if c["kernel"] == "ln_apply16":
            parts = kr.layernorm_ref(inp["x"], inp["gamma"], inp["beta"], c["eps"])[1]
            rt, st, y16 = _dev(kr.lazy_rows(inp["x"], inp["gamma"])), _dev(kr.stats_f32(parts)), _full16((T, H), NAN_BITS)
            _check(lib, lib.ak_kt_ln_apply16(_ptr(rt), _ptr(st), _ptr(g), _ptr(b), T, H, _ptr(y16), None), c["name"])
        elif c["kernel"] == "layernorm16":
            x16, y16 = _dev(kr.bf16_bits(inp["x"])), _full16((T, H), NAN_BITS)
            _check(lib, lib.ak_kt_layernorm16(_ptr(x16), _ptr(g), _ptr(b), T, H, c["eps"], _ptr(y16), None), c["name"])
        elif c["xin"] == "bf16":          # bf16 GEMM output in, no residual, bf16 out
            x16, y16 = _dev(kr.bf16_bits(inp["x"])), _full16((T, H), NAN_BITS)
            _check(lib, lib.ak_kt_layernorm(_ptr(x16), None, None, _ptr(g), _ptr(b), T, H, c["eps"], None, _ptr(y16), _ptr(x16), None), c["name"])
        elif c["res"] == "f32":           # float32 residual stream, in place, and its bf16 copy
            x, x32, y16 = _dev(inp["x"]), _dev(inp["res"]), _full16((T, H), NAN_BITS)
            _check(lib, lib.ak_kt_layernorm(_ptr(x), _ptr(x32), None, _ptr(g), _ptr(b), T, H, c["eps"], _ptr(x32), _ptr(y16), None, None), c["name"])
            res[c["name"] + ":y32"] = x32.cpu().numpy()
        else:                             # bf16 residual stream, in place
            x, y16 = _dev(inp["x"]), _dev(kr.bf16_bits(inp["res"]))
            _check(lib, lib.ak_kt_layernorm(_ptr(x), None, _ptr(y16), _ptr(g), _ptr(b), T, H, c["eps"], None, _ptr(y16), None, None), c["name"])
        res[c["name"] + ":y16"] = _host16(y16)
    for c in kc.ln_finalize_cases():
        part, out = _dev(kc.ln_finalize_inputs(c)), _f32((c["T"], 2))
        _check(lib, lib.ak_kt_ln_finalize(_ptr(part), c["nslot"], c["T"], 1.0 / (128 * c["nslot"]), c["eps"], _ptr(out), None), c["name"])
        res[c["name"]] = out.cpu().numpy()
    for c in kc.fold_ln_cases():
        inp = kc.fold_ln_inputs(c)
        w, g, b, bias = _dev(kr.bf16_bits(inp["w"])), _dev(inp["gamma"]), _dev(inp["beta"]), _dev(inp["bias"])
        cc, bf = _f32((c["N"],)), _f32((c["N"],))
        _check(lib, lib.ak_kt_fold_ln(_ptr(w), _ptr(g), _ptr(b), _ptr(bias), c["N"], c["K"], _ptr(cc), _ptr(bf), None), c["name"])
        res[c["name"] + ":c"], res[c["name"] + ":bf"] = cc.cpu().numpy(), bf.cpu().numpy()


def run_qkv384(lib, res, forced):
    import torch
    wbuf = torch.zeros(int(lib.ak_kt_qkv384_weight_bytes()), dtype=torch.uint8, device="cuda")
    for c in kc.qkv384_cases(forced):
        inp = kc.gemm_inputs(c)
        Tp, S, H = c["T"], c["S"], c["H"]
        x, w, bias = _dev(inp["x"]), _dev(inp["w"]), _dev(inp["bias"])
        q, k, vt = _sentinel16((Tp, H)), _sentinel16((Tp, H)), _sentinel16((Tp // S, H, S))
        _check(lib, lib.ak_kt_qkv384(_ptr(x), _ptr(w), _ptr(bias), _ptr(wbuf), _ptr(q), _ptr(k), _ptr(vt), Tp, c["Treal"], S, kc.qscale32(),
                                     c["head_major"], None), c["name"])
        res[c["name"] + ":q"], res[c["name"] + ":k"], res[c["name"] + ":vt"] = _host16(q), _host16(k), _host16(vt)


def run_ffn384(lib, res, child):
    import torch
    for c in kc.ffn384_cases(child):
        inp = kc.ffn384_inputs(c)
        p = inp["p"]
        bits = lambda a: _dev(kr.bf16_bits(a))
        x16 = bits(inp["x"])
        ctx = bits(inp["ctx"]) if c["ctx"] else None
        wo, w1, w2 = bits(p["wo"]), bits(p["w1"]), bits(p["w2"])
        v = {n: _dev(p[n]) for n in ("bo", "g1", "be1", "b1", "b2", "g2", "be2")}
        wbuf = torch.zeros(int(lib.ak_kt_ffn384_weight_bytes(c["I"])), dtype=torch.uint8, device="cuda")
        rc = lib.ak_kt_ffn384(_ptr(x16), _ptr(wo), _ptr(w1), _ptr(w2), _ptr(v["b1"]), _ptr(v["b2"]), _ptr(v["g2"]), _ptr(v["be2"]), _ptr(ctx),
                              _ptr(v["bo"]), _ptr(v["g1"]), _ptr(v["be1"]), _ptr(wbuf), c["T"], c["I"], c["eps"], None)
        _check(lib, rc, c["name"])
        res[c["name"]] = _host16(x16)


def run_lazy(lib, res, forced):
    from archi_amd._lib import AkKtGemmLazy
    for c in kc.lazy_cases(forced):
        inp = kc.lazy_inputs(c)
        T, N, K = c["T"], c["N"], c["K"]
        g = AkKtGemmLazy()
        w = _dev(kr.bf16_bits(inp["w"]))
        g.W, g.T, g.N, g.K, g.eps = w.data_ptr(), T, N, K, c["eps"]
        keep = {}
        if c["mode"] != 4:
            parts = kr.layernorm_ref(inp["r"], inp["gamma"], inp["beta"], c["eps"])[1]
            cc, bf = kr.fold_ln_ref(inp["w"], inp["gamma"], inp["beta"], inp["bias"])[:2]
            hold = [_dev(kr.lazy_rows(inp["r"], inp["gamma"])), _dev(bf.astype(np.float32)), _dev(cc.astype(np.float32)), _dev(kr.stats_f32(parts))]
            g.X, g.bias, g.fold_c, g.a_stats = (t.data_ptr() for t in hold)
            g.nslot, g.inv_h = K // 128, 1.0 / K
            if c["mode"] == 0:
                H, S = c["H"], c["S"]
                keep = dict(q=_full16((T, H), NAN_BITS), k=_full16((T, H), NAN_BITS), vt=_sentinel16((T // S, H, S)))
                g.q, g.k, g.vt, g.H, g.S, g.qscale, g.ldo = keep["q"].data_ptr(), keep["k"].data_ptr(), keep["vt"].data_ptr(), H, S, kc.qscale(c), c["ldo"]
            else:
                keep = dict(out=_full16((T, N), NAN_BITS))
                g.out_bf16, g.ldo = keep["out"].data_ptr(), N
        else:
            keep = dict(out=_full16((T, N), NAN_BITS), stats=_f32((N // 128, T, 2)))
            hold = [_dev(kr.bf16_bits(inp["x"])), _dev(inp["bias"]), _dev(inp["out_g"])]
            g.X, g.bias, g.out_g = (t.data_ptr() for t in hold)
            g.out_bf16, g.ldo, g.out_stats, g.nslot, g.inv_h = keep["out"].data_ptr(), N, keep["stats"].data_ptr(), N // 128, 1.0 / N
            if c["res_stats"]:
                parts = kr.layernorm_ref(inp["r_prev"], inp["gamma"], inp["beta"], c["eps"])[1]
                hold += [_dev(kr.lazy_rows(inp["r_prev"], inp["gamma"])), _dev(kr.stats_f32(parts)), _dev(inp["gamma"]), _dev(inp["beta"])]
                g.res16, g.res_stats, g.res_g, g.res_b = (t.data_ptr() for t in hold[3:])
            else:
                hold.append(_dev(kr.bf16_bits(inp["res_rows"])))
                g.res16 = hold[3].data_ptr()
        _check(lib, lib.ak_kt_gemm_lazy(c["mode"], ctypes.byref(g), None), c["name"])
        for name, t in keep.items():
            res[f"{c['name']}:{name}"] = t.cpu().numpy() if name == "stats" else _host16(t)


def run_identity(res):
    golden = os.path.join(HERE, "golden")
    from oracle import encoder_oracle as eo
    from archi_amd.encoder import HipEncoder
    f = np.load(os.path.join(golden, "encoder_bge_B2_S64_cls.npz"))
    vocab, H, L, heads, I, max_pos, _ = eo.SHAPES[str(f["shape"])]
    enc = HipEncoder(vocab, H, L, heads, I, max_pos, eo.synth_weights(str(f["shape"]), seed=int(f["weight_seed"])), device=0)
    res["bert"] = enc.forward(f["ids"], f["mask"], pooling=str(f["pooling"]), normalise=True).cpu().numpy()
    enc.close()
    from archi_amd.decoder import QWEN3_SHAPES, HipDecoder, random_qwen3_weights
    z = np.load(os.path.join(golden, "decoder_g2_B5_S96.npz"))
    dec = HipDecoder(QWEN3_SHAPES[str(z["shape"])], random_qwen3_weights(str(z["shape"]), seed=int(z["seed"])), device=0)
    res["decoder"] = dec.forward(z["ids"], z["lens"]).cpu().numpy()
    dec.close()
    from archi_amd.modernbert import HipModernBert, random_modernbert_weights
    from tests.golden.make_modernbert_fixtures import load
    c = load("mix_mean")
    m = HipModernBert(c["shape_name"], random_modernbert_weights(c["shape_name"], seed=c["seed"], std=c["std"]), device=0)
    res["modernbert_mix_mean"] = m.forward(c["ids"], c["lens"], pooling=c["pooling"]).cpu().numpy()
    m.close()


def main(group, out):
    from archi_amd import _lib
    lib = _lib.init(0)
    res = {"dbg": np.array(int(_lib.is_dbg_library()))}
    if group == "identity":
        run_identity(res)
    else:
        assert _lib.is_dbg_library(), "the kernel-test entry points live in libarchi_hip_dbg.so (ARCHI_HIP_DBG=1)"
        if group == "gemm":
            run_gemm(lib, res)
        elif group == "lnfused":                 # every LayerNorm-fused family by the launchers' own selection
            run_gemm_ln(lib, res)
            run_layernorms(lib, res)
            run_qkv384(lib, res, False)
            run_ffn384(lib, res, "default")
            run_lazy(lib, res, False)
        elif group == "lnfused_forced":          # under AK_FFN_NWV=8 AK_QKV_TG=2 AK_ENC_LAZYLN=2 (the parent sets them)
            run_qkv384(lib, res, True)
            run_ffn384(lib, res, "nwv8")
            run_lazy(lib, res, True)
        elif group == "lnfused_w4":              # under AK_FFN_W8=0: the 4-wave generation of the feed-forward kernel
            run_ffn384(lib, res, "w4")
        elif group == "skinny":
            run_skinny(lib, res)
        else:
            run_attention(lib, group, res)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
