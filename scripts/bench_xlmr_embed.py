"""XLM-RoBERTa embedders on the HIP encoder with positions from the ids (archi_amd.encoder.HipEncoder, positions_from_ids), seeded
weights: the multilingual-e5-base shape at 128 x 512 against the same-run bge-base forward (the same GEMM and attention kernels on the
same shapes: the ratio is the cost of the positions pass), the bge-m3 shape (hidden 1024, 24 layers) at 128 x 512 and at 8 x 8192 (the
long-row attention kernel, csrc/attn_long.hip: one workload on each side of the S = 512 kernel choice); per workload ms per forward and
chunks/s (HIP events after warm-up), TFLOP/s and share of the 2.5 PF bf16 peak, transformers XLMRobertaModel bf16 + SDPA on the same
GPU and ids, then a check of sampled rows of the 512-token workloads against float32 XLMRobertaModel on the CPU (exit status 1 on a
mismatch; the 8192-token rows are checked by tests/test_xlmr_gpu.py on a small shape). Prints ONE JSON line.

    python scripts/bench_xlmr_embed.py [--iters 5] [--no-baseline]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

E5 = "intfloat/multilingual-e5-base"
M3 = "BAAI/bge-m3"
BGE = "BAAI/bge-base-en-v1.5"
PEAK_TFLOPS = 2500.0
EPS = 1e-5
PAD = 1


def flops(n_chunks, S, H, I, L):
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


def hf_bf16(shape_name, w, dev):
    import torch
    from transformers import XLMRobertaModel
    from archi_amd.encoder import XLMR_SHAPES, xlmr_hf_state_dict
    from tests.xlmr_ref import hf_config
    shape = XLMR_SHAPES[shape_name]
    cfg = hf_config(shape)
    cfg._attn_implementation = "sdpa"
    model = XLMRobertaModel(cfg, add_pooling_layer=False).eval()
    model.load_state_dict(xlmr_hf_state_dict(w, shape[2]), strict=False)
    return model.to(device=dev, dtype=torch.bfloat16), model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--check-rows", type=int, default=2)
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    import torch
    from archi_amd.encoder import MODEL_SHAPES, XLMR_SHAPES, HipEncoder, random_init_weights, random_xlmr_weights
    res = {"bench": "xlmr_embed", "precision": "bf16", "runs": []}
    ok = True
    B, S = 128, 512
    rng = np.random.default_rng(args.seed + S)
    ids = rng.integers(4, 250002, (B, S)).astype(np.int32)
    long_ids = rng.integers(4, 250002, (8, 8192)).astype(np.int32)
    bv, bH, bL, bheads, bI, bpos = MODEL_SHAPES[BGE][:6]
    bge = HipEncoder(bv, bH, bL, bheads, bI, bpos, random_init_weights(bv, bH, bL, bI, bpos, seed=args.seed), device=0)
    dev = bge._dev
    stage = torch.from_numpy(np.concatenate([np.minimum(ids, bv - 1), np.full((B, 1), S, np.int32)], 1)).to(dev).contiguous()
    out_b = torch.empty((B, bH), dtype=torch.float32, device=dev)
    checks = []
    weights = {}
    for name, wl in ((E5, ids), (M3, ids), (M3, long_ids)):
        B, S = wl.shape
        vocab, H, L, heads, I, max_pos = XLMR_SHAPES[name][:6]
        if name not in weights:
            weights = {name: random_xlmr_weights(name, seed=args.seed)}
        w = weights[name]
        enc = HipEncoder(vocab, H, L, heads, I, max_pos, w, ln_eps=EPS, device=0, positions_from_ids=PAD)
        st = torch.from_numpy(np.concatenate([wl, np.full((B, 1), S, np.int32)], 1)).to(dev).contiguous()
        out = torch.empty((B, H), dtype=torch.float32, device=dev)
        hip_ms, hip_all = timed(lambda: enc.forward_lens(st, B, S, out), args.iters, args.warmup)
        enc.forward_lens(st, B, S, out)
        fl = flops(B, S, H, I, L)
        run = {"shape": name, "chunks": B, "tokens": S, "hip_ms": round(hip_ms, 3), "hip_ms_all": [round(x, 3) for x in hip_all],
               "attention_flop_share": round(4 * S * S * H / (2 * S * (4 * H * H + 2 * H * I) + 4 * S * S * H), 3),
               "chunks_per_s": round(B / hip_ms * 1e3, 1), "tflops": round(fl / hip_ms / 1e9, 1),
               "peak_share": round(fl / hip_ms / 1e9 / PEAK_TFLOPS, 3)}
        if name == E5:
            bge_ms, _ = timed(lambda: bge.forward_lens(stage, B, S, out_b), args.iters, args.warmup)
            run["bge_base_ms"] = round(bge_ms, 3)
            run["ratio_vs_bge_base"] = round(hip_ms / bge_ms, 3)
        if not args.no_baseline:
            model, _ = hf_bf16(name, w, dev)
            t_ids = torch.from_numpy(wl).long().to(dev)
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
        got = out.cpu().numpy()
        ok = ok and bool(np.isfinite(got).all())
        enc.close()
        del enc
        torch.cuda.empty_cache()
        if S == 512:
            checks.append((name, w, got))
        res["runs"].append(run)
    del weights
    bge.close()
    # float32 CPU check of sampled rows (a row's embedding does not depend on its neighbours; mean pooling as forward_lens above)
    from transformers import XLMRobertaModel
    from archi_amd.encoder import xlmr_hf_state_dict
    from tests.xlmr_ref import hf_config, hf_embed
    n = args.check_rows
    res["check"] = []
    for name, w, got in checks:
        shape = XLMR_SHAPES[name]
        cfg = hf_config(shape)
        cfg._attn_implementation = "eager"
        model = XLMRobertaModel(cfg, add_pooling_layer=False).eval()
        model.load_state_dict(xlmr_hf_state_dict(w, shape[2]), strict=False)
        want = hf_embed(model, ids[:n], np.ones_like(ids[:n]), pooling="mean")
        cos = (got[:n] * want).sum(1) / (np.linalg.norm(got[:n], axis=1) * np.linalg.norm(want, axis=1))
        res["check"].append({"shape": name, "rows": n, "max_1_minus_cos": float(1 - cos.min()),
                             "max_abs": float(np.abs(got[:n] - want).max())})
        ok = ok and bool(1 - cos.min() <= 1e-3)
        del model
    res["check_ok"] = ok
    print(json.dumps(res))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
