"""Child of tests/test_kernels_gpu.py: runs every case of one group through its ak_kt_* wrapper (libarchi_hip_dbg.so; the parent sets
ARCHI_HIP_DBG=1 and, for the A/B alternates of launch_attn, AK_ATTN_STREAM), each case ONCE, and writes the raw outputs to one .npz.
The float64 references are the parent's work. Any launcher error or HIP error ends the process with a non-zero status.

    kernel_worker.py <group> <out.npz>      group: window | long | attn | causal | gemm | skinny | identity

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
        elif group == "skinny":
            run_skinny(lib, res)
        else:
            run_attention(lib, group, res)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
