"""all-mpnet-base-v2 on the HIP encoder with MPNet's relative-position bias (archi_amd.encoder.HipEncoder, rel_bias), seeded weights:
per (chunks, tokens) shape the ms per forward and chunks/s timed with HIP events after warm-up, achieved TFLOP/s and share of
the 2.5 PF bf16 peak (the bge-base flop count: the bias adds no matrix work), and two same-run baselines -- the bge-base forward
at the same (B, S) (identical GEMMs: the difference is the bias) and transformers MPNetModel in bf16 on the same GPU and ids --,
then an embedding check against float32 MPNetModel on the CPU (exit status 1 on a mismatch). Prints ONE JSON line.

    python scripts/bench_mpnet_embed.py [--shapes 256x384,128x512] [--iters 5] [--no-baseline]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPE = "sentence-transformers/all-mpnet-base-v2"
BGE = "BAAI/bge-base-en-v1.5"
PEAK_TFLOPS = 2500.0
EPS = 1e-5


def flops(n_chunks, S, H=768, I=3072, L=12):
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
    ap.add_argument("--shapes", default="256x384,128x512")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--check-rows", type=int, default=2)
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    import torch
    from archi_amd.encoder import (MODEL_SHAPES, MPNET_SHAPES, HipEncoder, mpnet_rel_bias_table, random_init_weights,
                                   random_mpnet_weights)
    vocab, H, L, heads, I, max_pos_emb = MPNET_SHAPES[SHAPE][:6]
    n_rel = max_pos_emb - 2
    w, rel, _ = random_mpnet_weights(SHAPE, seed=args.seed)
    enc = HipEncoder(vocab, H, L, heads, I, n_rel, w, ln_eps=EPS, device=0, rel_bias=mpnet_rel_bias_table(rel, n_rel))
    dev = enc._dev
    bv, bH, bL, bheads, bI, bpos = MODEL_SHAPES[BGE][:6]
    bge = HipEncoder(bv, bH, bL, bheads, bI, bpos, random_init_weights(bv, bH, bL, bI, bpos, seed=args.seed), device=0)
    model = None
    if not args.no_baseline:
        from tests.mpnet_ref import hf_model
        model = hf_model(SHAPE, args.seed)[0].to(device=dev, dtype=torch.bfloat16)
    res = {"bench": "mpnet_embed", "shape": SHAPE, "precision": "bf16", "runs": []}
    ok = True
    first = None
    for spec in args.shapes.split(","):
        B, S = (int(x) for x in spec.split("x"))
        rng = np.random.default_rng(args.seed + S)
        ids = rng.integers(5, vocab, (B, S)).astype(np.int32)
        stage = torch.from_numpy(np.concatenate([ids, np.full((B, 1), S, np.int32)], 1)).to(dev).contiguous()
        out = torch.empty((B, H), dtype=torch.float32, device=dev)
        hip_ms, hip_all = timed(lambda: enc.forward_lens(stage, B, S, out), args.iters, args.warmup)
        out_b = torch.empty_like(out)
        bge_ms, _ = timed(lambda: bge.forward_lens(stage, B, S, out_b), args.iters, args.warmup)
        enc.forward_lens(stage, B, S, out)
        fl = flops(B, S)
        run = {"chunks": B, "tokens": S, "hip_ms": round(hip_ms, 3), "hip_ms_all": [round(x, 3) for x in hip_all],
               "chunks_per_s": round(B / hip_ms * 1e3, 1), "tflops": round(fl / hip_ms / 1e9, 1),
               "peak_share": round(fl / hip_ms / 1e9 / PEAK_TFLOPS, 3), "bge_base_ms": round(bge_ms, 3),
               "ratio_vs_bge_base": round(hip_ms / bge_ms, 3)}
        if model is not None:
            t_ids = torch.from_numpy(ids).long().to(dev)
            mask = torch.ones_like(t_ids)

            def base():
                with torch.no_grad():
                    h = model(input_ids=t_ids, attention_mask=mask).last_hidden_state
                    return torch.nn.functional.normalize(h.float().mean(1), dim=-1)
            base_ms, _ = timed(base, args.iters, args.warmup)
            run["torch_bf16_ms"] = round(base_ms, 3)
            run["speedup_vs_torch"] = round(base_ms / hip_ms, 2)
        ok = ok and bool(np.isfinite(out.cpu().numpy()).all())
        if first is None:
            first = (ids, out.cpu().numpy())
        res["runs"].append(run)
    del model
    torch.cuda.empty_cache()
    from tests.mpnet_ref import hf_embed, hf_model
    ids, got = first
    n = args.check_rows
    want = hf_embed(hf_model(SHAPE, args.seed)[0], ids[:n], np.ones_like(ids[:n]))
    cos = (got[:n] * want).sum(1) / (np.linalg.norm(got[:n], axis=1) * np.linalg.norm(want, axis=1))
    res["check_rows"] = n
    res["check_max_1_minus_cos"] = float(1 - cos.min())
    res["check_max_abs"] = float(np.abs(got[:n] - want).max())
    ok = ok and bool(1 - cos.min() <= 1e-3)
    res["check_ok"] = ok
    print(json.dumps(res))
    enc.close()
    bge.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
