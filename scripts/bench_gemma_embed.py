"""EmbeddingGemma on the HIP Gemma encoder (archi_amd.gemma.HipGemma), seeded weights of the google/embeddinggemma-300m shape at
128 x 512 and at 32 x 2048; per workload, TWICE in the same call, ms per forward and chunks/s (HIP events after warm-up), algorithmic
TFLOP/s and share of the 2.5 PF bf16 peak; beside them in the same run transformers Gemma3TextModel bf16 + SDPA on the same GPU and ids
(the yardstick: the HIP forward must not be slower) and the bge-base forward at 128 x 512 (the project's flagship encoder on the same
token count); the per-launch time of ONE sliding and ONE full launch_attn_gqa at 32 x 2048 (a child process on the dbg library, whose
ak_ktg_attn_gqa wrapper calls the launcher the forward pass calls) with the kernel's share of peak; then a check of the timed outputs
against float32 Gemma3TextModel on the CPU on sampled rows of the 512-token workload (exit status 1 on a mismatch or when the HIP
forward is slower than the vendor stack). Prints ONE JSON line.

Algorithmic flops per token and layer: 2 H (NQ + 2 NKV) + 2 NQ H + 6 H I for the GEMMs (NQ = 3 x 256, NKV = 256: 8.45 MFLOP) plus
4 NQ keys for attention, keys = S in a full layer and the keys inside |q - k| <= 256 (averaged over the row) in a sliding layer.

    python scripts/bench_gemma_embed.py [--iters 5] [--no-baseline] [--no-check] [--only g512,g2048] [--out profiles/gemma_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAME = "google/embeddinggemma-300m"
BGE = "BAAI/bge-base-en-v1.5"
PEAK_TFLOPS = 2500.0
WORKLOADS = {"g512": (128, 512), "g2048": (32, 2048)}


def visible_keys(S, w):
    """Mean number of keys a query of a full S-token row sees in a sliding layer (|q - k| <= w)."""
    q = np.arange(S)
    return float((np.minimum(S - 1, q + w) - np.maximum(0, q - w) + 1).mean())


def flops(shape, n_chunks, S):
    """(total, attention share, gemm flops per token and layer) of one forward over n_chunks full rows of S tokens."""
    H, L, nq, nkv, hd, I, window, types = shape[1], shape[2], shape[3], shape[4], shape[5], shape[6], shape[11], shape[13]
    gemm = 2 * H * (nq + 2 * nkv) * hd + 2 * nq * hd * H + 6 * H * I
    att = sum(4 * nq * hd * (S if t else visible_keys(S, window // 2)) for t in types)
    tot = n_chunks * S * (L * gemm + att)
    return tot, n_chunks * S * att / tot, gemm


def bge_flops(n_chunks, S, H, I, L):
    return n_chunks * L * (2 * S * (4 * H * H + 2 * H * I) + 4 * S * S * H)


def timed(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(iters):
        ev0.record()
        fn()
        ev1.record()
        ev1.synchronize()
        ms.append(ev0.elapsed_time(ev1))
    return float(np.median(ms)), ms


def attn_child(iters):
    """One launch_attn_gqa at a time on random operands, B = 32, S = 2048, 3 query heads on 1 kv head: the full launch and the
    sliding one (half-window 256). Runs in a process that loaded the dbg library."""
    import ctypes
    import torch
    from archi_amd import _lib
    lib = _lib.init(0)
    assert _lib.is_dbg_library()
    B, S, nq, nkv, hd, w = 32, 2048, 3, 1, 256, 256
    g = torch.Generator(device="cuda").manual_seed(0)
    q = (torch.randn((B, nq, S, hd), device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    k = torch.randn((B, nkv, S, hd), device="cuda", generator=g).to(torch.bfloat16)
    vt = torch.randn((B, nkv, hd, S), device="cuda", generator=g).to(torch.bfloat16)
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
    ctx = torch.empty((B, S, nq * hd), dtype=torch.bfloat16, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    out = {"B": B, "S": S, "q_heads": nq, "kv_heads": nkv, "half_window": w}
    for name, hw in (("full", 0), ("sliding", w)):
        def launch():
            _lib.check(lib.ak_ktg_attn_gqa(P(q), P(k), P(vt), P(lens), P(ctx), B, S, nq, nkv, hw, None), "ak_ktg_attn_gqa")
        ms, _ = timed(launch, iters, 2)
        keys = S if hw == 0 else visible_keys(S, hw)
        fl = 4.0 * nq * hd * keys * B * S
        out[name + "_ms"] = round(ms, 4)
        out[name + "_peak_share"] = round(fl / ms / 1e9 / PEAK_TFLOPS, 4)
    out["sliding_over_full"] = round(out["sliding_ms"] / out["full_ms"], 3)
    out["key_blocks_walked_ratio_derived"] = round(((128 + 2 * w) / 32 + 1) / (S / 32), 3)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--check-rows", type=int, default=2)
    ap.add_argument("--no-baseline", action="store_true", help="skip transformers bf16 + SDPA and the bge-base forward")
    ap.add_argument("--no-check", action="store_true", help="skip the float32 CPU check (kernel-trace runs)")
    ap.add_argument("--no-attn", action="store_true", help="skip the per-launch attention child")
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--attn-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.attn_child:
        return attn_child(args.iters)
    import torch
    from archi_amd.encoder import MODEL_SHAPES, HipEncoder, random_init_weights
    from archi_amd.gemma import GEMMA_SHAPES, HipGemma, random_gemma_weights
    from tests.gemma_ref import cos_gap, dense_matrices, hf_model, reference_embed
    res = {"bench": "gemma_embed", "precision": "bf16", "shape": NAME, "runs": []}
    ok = True
    shape = GEMMA_SHAPES[NAME]
    w = random_gemma_weights(shape, seed=args.seed)
    enc = HipGemma(shape, w, device=0)
    dev = enc._dev
    checks = []
    for key in args.only.split(","):
        B, S = WORKLOADS[key]
        ids = np.random.default_rng(args.seed + S).integers(3, shape[0], (B, S)).astype(np.int32)
        st = torch.from_numpy(np.concatenate([ids, np.full((B, 1), S, np.int32)], 1)).to(dev).contiguous()
        out = torch.empty((B, enc.out_dim), dtype=torch.float32, device=dev)
        fwd = lambda: enc.forward_lens(st, B, S, out)
        run1, all1 = timed(fwd, args.iters, args.warmup)
        run2, all2 = timed(fwd, args.iters, 0)
        hip_ms = min(run1, run2)
        fl, att_share, gemm_tok = flops(shape, B, S)
        run = {"workload": key, "chunks": B, "tokens": S, "hip_ms_run1": round(run1, 3), "hip_ms_run2": round(run2, 3),
               "hip_ms_all": [round(x, 3) for x in all1 + all2], "gemm_mflop_per_token_layer": round(gemm_tok / 1e6, 2),
               "attention_flop_share": round(att_share, 3), "chunks_per_s": round(B / hip_ms * 1e3, 1),
               "tflops": round(fl / hip_ms / 1e9, 1), "peak_share": round(fl / hip_ms / 1e9 / PEAK_TFLOPS, 4)}
        if key == "g512" and not args.no_baseline:
            bv, bH, bL, bheads, bI, bpos = MODEL_SHAPES[BGE][:6]
            bge = HipEncoder(bv, bH, bL, bheads, bI, bpos, random_init_weights(bv, bH, bL, bI, bpos, seed=args.seed), device=0)
            stage = torch.from_numpy(np.concatenate([np.minimum(ids, bv - 1), np.full((B, 1), S, np.int32)], 1)).to(dev).contiguous()
            out_b = torch.empty((B, bH), dtype=torch.float32, device=dev)
            bge_ms, _ = timed(lambda: bge.forward_lens(stage, B, S, out_b), args.iters, args.warmup)
            run["bge_base_ms"] = round(bge_ms, 3)
            run["bge_base_peak_share"] = round(bge_flops(B, S, bH, bI, bL) / bge_ms / 1e9 / PEAK_TFLOPS, 4)
            run["ratio_vs_bge_base"] = round(hip_ms / bge_ms, 3)
            bge.close()
            del bge
        if not args.no_baseline:
            model = hf_model(shape, w)
            model.config._attn_implementation = "sdpa"
            model = model.to(device=dev, dtype=torch.bfloat16)
            dense = [d.to(dev) for d in dense_matrices(shape, w)]
            t_ids = torch.from_numpy(ids).long().to(dev)
            mask = torch.ones_like(t_ids)

            def base():
                with torch.no_grad():
                    e = model(input_ids=t_ids, attention_mask=mask).last_hidden_state.float().mean(1)
                    for d in dense:
                        e = e @ d.T
                    return torch.nn.functional.normalize(e, dim=-1)
            base_ms, _ = timed(base, args.iters, args.warmup)
            run["torch_bf16_sdpa_ms"] = round(base_ms, 3)
            run["speedup_vs_torch"] = round(base_ms / hip_ms, 2)
            ok = ok and hip_ms <= base_ms
            del model
            torch.cuda.empty_cache()
        fwd()
        got = out.cpu().numpy()
        ok = ok and bool(np.isfinite(got).all())
        if S == 512 and not args.no_check:
            checks.append((key, ids, got))
        res["runs"].append(run)
    enc.close()
    del enc
    torch.cuda.empty_cache()
    if not args.no_attn:
        # a fresh child on the dbg library (the single-launch wrapper lives there); this process has released its buffers
        env = dict(os.environ, ARCHI_HIP_DBG="1")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--attn-child", "--iters", str(max(args.iters, 10))], env=env,
                           stdout=subprocess.PIPE, timeout=300)
        ok = ok and p.returncode == 0
        if p.returncode == 0:
            res["attention_launch"] = json.loads(p.stdout.decode().strip().splitlines()[-1])
    n = args.check_rows
    res["check"] = []
    for key, ids, got in checks:
        want = reference_embed(hf_model(shape, w), ids[:n], [ids.shape[1]] * n, dense_matrices(shape, w))
        gap = float(cos_gap(got[:n], want).max())
        res["check"].append({"workload": key, "rows": n, "max_1_minus_cos": gap, "max_abs": float(np.abs(got[:n] - want).max())})
        ok = ok and gap <= 1e-3
    res["check_ok"] = ok
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
