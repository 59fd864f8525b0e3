"""Qwen3-Embedding-0.6B on the HIP decoder (archi_amd.decoder.HipDecoder), seeded weights: chunks/s at 256 chunks x 256 tokens
timed with HIP events after warm-up, achieved TFLOP/s and share of the 2.5 PF bf16 peak, a same-run PyTorch-ROCm baseline
(transformers Qwen3Model in bf16 with SDPA on the same GPU and ids), embed_query p50 latency, and an embedding check against
float32 Qwen3Model on the CPU (exit status 1 on a mismatch). Prints ONE JSON line.

    python scripts/bench_qwen3_embed.py [--chunks 256] [--tokens 256] [--iters 5] [--no-baseline]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPE = "Qwen/Qwen3-Embedding-0.6B"
PEAK_TFLOPS = 2500.0


def flops(n_chunks, L):
    gemm = 2 * 28 * (1024 * 4096 + 2048 * 1024 + 1024 * 6144 + 3072 * 1024)      # 0.881 GFLOP per token
    return n_chunks * (gemm * L + 28 * 4096 * L * (L + 1))


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
    ap.add_argument("--chunks", type=int, default=256)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--check-rows", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    import torch
    from archi_amd.decoder import QWEN3_SHAPES, HipDecoder, random_qwen3_weights
    shape = QWEN3_SHAPES[SHAPE]
    w = random_qwen3_weights(shape, seed=args.seed)
    dec = HipDecoder(shape, w, device=0)
    dev = dec._dev
    B, S = args.chunks, args.tokens
    rng = np.random.default_rng(args.seed)
    ids = rng.integers(0, shape[0], (B, S)).astype(np.int32)
    stage = torch.from_numpy(np.concatenate([ids, np.full((B, 1), S, np.int32)], 1)).to(dev).contiguous()
    out = torch.empty((B, dec.hidden), dtype=torch.float32, device=dev)
    hip_ms, hip_all = timed(lambda: dec.forward_lens(stage, B, S, out), args.iters, args.warmup)
    fl = flops(B, S)
    res = {"bench": "qwen3_embed", "shape": SHAPE, "chunks": B, "tokens": S, "hip_ms": round(hip_ms, 3),
           "hip_ms_all": [round(x, 3) for x in hip_all], "chunks_per_s": round(B / hip_ms * 1e3, 1),
           "tflops": round(fl / hip_ms / 1e9, 1), "peak_share": round(fl / hip_ms / 1e9 / PEAK_TFLOPS, 3),
           "gflop_per_forward": round(fl / 1e9, 1)}
    hip_out = out.cpu().numpy()

    # embed_query: one row of 24 tokens, host ids in, host row out (what embed_query pays)
    q_ids = ids[:1, :24]
    lat = []
    for i in range(60):
        t0 = time.perf_counter()
        dec.forward(q_ids, [24]).cpu()
        if i >= 10:
            lat.append((time.perf_counter() - t0) * 1e3)
    res["embed_query_p50_ms"] = round(float(np.median(lat)), 3)

    from tests.decoder_ref import hf_model, reference
    if not args.no_baseline:
        model = hf_model(SHAPE, w, attn="sdpa").to(device=dev, dtype=torch.bfloat16)
        t_ids = torch.from_numpy(ids).long().to(dev)
        mask = torch.ones_like(t_ids)

        def base():
            with torch.no_grad():
                h = model(input_ids=t_ids, attention_mask=mask).last_hidden_state[:, -1]
                return torch.nn.functional.normalize(h.float(), dim=-1)
        base_ms, _ = timed(base, args.iters, args.warmup)
        res["torch_bf16_sdpa_ms"] = round(base_ms, 3)
        res["torch_chunks_per_s"] = round(B / base_ms * 1e3, 1)
        res["speedup_vs_torch"] = round(base_ms / hip_ms, 2)
        del model
        torch.cuda.empty_cache()

    n = args.check_rows
    want = reference(hf_model(SHAPE, w), ids[:n], np.full(n, S))
    got = hip_out[:n]
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    res["check_rows"] = n
    res["check_max_1_minus_cos"] = float(1 - cos.min())
    ok = bool(1 - cos.min() <= 1e-3 and np.isfinite(hip_out).all())
    res["check_ok"] = ok
    print(json.dumps(res))
    dec.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
