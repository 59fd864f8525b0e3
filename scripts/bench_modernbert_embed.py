"""ModernBERT embedders on the HIP ModernBERT encoder (archi_amd.modernbert.HipModernBert), seeded weights: the ModernBERT-base shape at
128 x 512 and at 8 x 8192 (one workload on each side of the point where the sliding layers' window starts to pay), the large shape at
128 x 512; per workload, TWICE in the same call, ms per forward and chunks/s (HIP events after warm-up), algorithmic TFLOP/s and share of
the 2.5 PF bf16 peak; beside them in the same run the bge-base forward at 128 x 512 (the project's flagship encoder on the same token
count) and transformers ModernBertModel bf16 + SDPA on the same GPU and ids; then a check of the timed outputs against float32
ModernBertModel on the CPU on sampled rows of the 512-token workloads (exit status 1 on a mismatch; the 8192-token rows are checked by
tests/test_modernbert_gpu.py on a small shape). Prints ONE JSON line.

Algorithmic flops per token and layer: 2 (4 H^2 + 3 H I) for the GEMMs (Wqkv 3 H^2, Wo H^2, Wi 2 H I, mlp.Wo H I; base: 10.03 MFLOP)
plus 4 H keys for attention, keys = S in a global layer and the keys inside |q - k| <= 64 (averaged over the row) in a sliding layer:
only work the model needs is counted, so a kernel that walks key blocks outside the window gets no credit for it.

    python scripts/bench_modernbert_embed.py [--iters 5] [--no-baseline] [--no-check] [--only base512,base8192,large512]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BASE = "nomic-ai/modernbert-embed-base"
LARGE = "lightonai/modernbert-embed-large"
BGE = "BAAI/bge-base-en-v1.5"
PEAK_TFLOPS = 2500.0
WORKLOADS = {"base512": (BASE, 128, 512), "base8192": (BASE, 8, 8192), "large512": (LARGE, 128, 512)}


def visible_keys(S, w):
    """Mean number of keys a query of a full S-token row sees in a sliding layer (|q - k| <= w)."""
    q = np.arange(S)
    return float((np.minimum(S - 1, q + w) - np.maximum(0, q - w) + 1).mean())


def flops(shape, n_chunks, S):
    """(total, attention share, gemm flops per token and layer) of one forward over n_chunks full rows of S tokens."""
    H, L, I, local, types = shape[1], shape[2], shape[4], shape[9], shape[10]
    gemm = 2 * (4 * H * H + 3 * H * I)
    att = sum(4 * H * (S if t else visible_keys(S, local // 2)) for t in types)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--check-rows", type=int, default=2)
    ap.add_argument("--no-baseline", action="store_true", help="skip transformers bf16 + SDPA and the bge-base forward")
    ap.add_argument("--no-check", action="store_true", help="skip the float32 CPU check (kernel-trace runs)")
    ap.add_argument("--only", default=",".join(WORKLOADS))
    args = ap.parse_args()
    import torch
    from archi_amd.encoder import MODEL_SHAPES, HipEncoder, random_init_weights
    from archi_amd.modernbert import MODERNBERT_SHAPES, HipModernBert, random_modernbert_weights
    from tests.modernbert_ref import cos_gap, hf_model, reference_embed
    res = {"bench": "modernbert_embed", "precision": "bf16", "runs": []}
    ok = True
    dev = None
    checks, weights = [], {}
    for key in args.only.split(","):
        name, B, S = WORKLOADS[key]
        shape = MODERNBERT_SHAPES[name]
        if name not in weights:
            weights = {name: random_modernbert_weights(shape, seed=args.seed)}
        w = weights[name]
        enc = HipModernBert(shape, w, device=0)
        dev = enc._dev
        H = shape[1]
        ids = np.random.default_rng(args.seed + S).integers(3, shape[0], (B, S)).astype(np.int32)
        st = torch.from_numpy(np.concatenate([ids, np.full((B, 1), S, np.int32)], 1)).to(dev).contiguous()
        out = torch.empty((B, H), dtype=torch.float32, device=dev)
        fwd = lambda: enc.forward_lens(st, B, S, out, pooling="mean")
        run1, all1 = timed(fwd, args.iters, args.warmup)
        run2, all2 = timed(fwd, args.iters, 0)
        hip_ms = min(run1, run2)
        fl, att_share, gemm_tok = flops(shape, B, S)
        run = {"workload": key, "shape": name, "chunks": B, "tokens": S, "hip_ms_run1": round(run1, 3), "hip_ms_run2": round(run2, 3),
               "hip_ms_all": [round(x, 3) for x in all1 + all2], "gemm_mflop_per_token_layer": round(gemm_tok / 1e6, 2),
               "attention_flop_share": round(att_share, 3), "chunks_per_s": round(B / hip_ms * 1e3, 1),
               "tflops": round(fl / hip_ms / 1e9, 1), "peak_share": round(fl / hip_ms / 1e9 / PEAK_TFLOPS, 4)}
        if key == "base512" and not args.no_baseline:
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
            t_ids = torch.from_numpy(ids).long().to(dev)
            mask = torch.ones_like(t_ids)

            def base():
                with torch.no_grad():
                    h = model(input_ids=t_ids, attention_mask=mask).last_hidden_state
                    return torch.nn.functional.normalize(h.float().mean(1), dim=-1)
            base_ms, _ = timed(base, args.iters, args.warmup)
            run["torch_bf16_sdpa_ms"] = round(base_ms, 3)
            run["speedup_vs_torch"] = round(base_ms / hip_ms, 2)
            del model
            torch.cuda.empty_cache()
        fwd()
        got = out.cpu().numpy()
        ok = ok and bool(np.isfinite(got).all())
        enc.close()
        del enc
        torch.cuda.empty_cache()
        if S == 512 and not args.no_check:
            checks.append((key, shape, w, ids, got))
        res["runs"].append(run)
    del weights
    # float32 CPU check of sampled rows of the timed outputs (a row's embedding does not depend on its neighbours)
    n = args.check_rows
    res["check"] = []
    for key, shape, w, ids, got in checks:
        want = reference_embed(hf_model(shape, w), ids[:n], [ids.shape[1]] * n, "mean")
        gap = float(cos_gap(got[:n], want).max())
        res["check"].append({"workload": key, "rows": n, "max_1_minus_cos": gap, "max_abs": float(np.abs(got[:n] - want).max())})
        ok = ok and gap <= 1e-3
    res["check_ok"] = ok
    print(json.dumps(res))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
