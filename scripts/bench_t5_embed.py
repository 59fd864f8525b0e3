"""T5 embedders on the HIP T5 encoder (archi_amd.t5.HipT5), seeded weights: the gtr-t5-base shape (12 layers, hidden 768, ReLU
feed-forward, Dense 768 -> 768) at 128 x 512 and at 8 x 8192. Every GPU step is a child process of this script under its own time
limit; the first step that fails ends the run (nothing more is started on the GPU) and the exit status is 1.

    forward steps   per workload, TWICE in the same process: ms per forward and chunks/s (HIP events after warm-up), algorithmic
                    TFLOP/s and share of the 2.5 PF bf16 peak; in the same process transformers T5EncoderModel in bf16 on the same GPU
                    and ids, and (128 x 512) the bge-base forward: the same GEMM flops per token as t5-base with ReLU (4 H^2 + 2 H I per
                    layer and token, times 2), so the ratio isolates what the bias and the RMSNorm joins cost against bge-base's fused
                    LayerNorm path
    launches step   on libarchi_hip_dbg.so: ONE biased attention launch (ak_kts_t5_attn, k_attn_long_relbias) against ONE
                    un-biased launch (ak_kt_attn_window at window -1, k_attn_long<false>) on the same q / k / V^T, 12 heads, at both
                    workloads: `rounds` rounds of the median of 10 back-to-back launches each, so the un-biased launch's own spread
                    between rounds is there to judge the difference by
    check           the timed 512-token outputs against float32 T5EncoderModel on the CPU on sampled rows

Prints ONE JSON line and writes it to --out.

    python scripts/bench_t5_embed.py [--iters 5] [--rounds 5] [--no-baseline] [--out profiles/t5_bench.json]
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

BASE = "sentence-transformers/gtr-t5-base"
BGE = "BAAI/bge-base-en-v1.5"
PEAK_TFLOPS = 2500.0
WORKLOADS = {"base512": (128, 512), "base8192": (8, 8192)}
STEP_LIMIT_S = {"base512": 420, "base8192": 420, "launches": 300}


def flops(shape, n_chunks, S):
    """(total, attention share) of one forward over n_chunks full rows of S tokens: GEMMs 2 (4 H^2 + 2 H d_ff), attention 4 H S."""
    H, L, dff = shape[1], shape[2], shape[5]
    gemm = 2 * (4 * H * H + 2 * H * dff)
    att = 4 * H * S
    tot = n_chunks * S * L * (gemm + att)
    return tot, att / (gemm + att)


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


def step_forward(key, args):
    import torch
    from archi_amd.t5 import T5_SHAPES, HipT5, random_t5_weights
    shape = T5_SHAPES[BASE]
    B, S = WORKLOADS[key]
    w = random_t5_weights(shape, seed=args.seed, std=0.02)       # at 0.05 a 12-layer hidden-768 stack has score std 15: HF's own bf16 run is off by 1e-2
    enc = HipT5(shape, w, device=0)
    dev = enc._dev
    ids = np.random.default_rng(args.seed + S).integers(3, shape[0], (B, S)).astype(np.int32)
    st = torch.from_numpy(np.concatenate([ids, np.full((B, 1), S, np.int32)], 1)).to(dev).contiguous()
    out = torch.empty((B, enc.out_dim), dtype=torch.float32, device=dev)
    fwd = lambda: enc.forward_lens(st, B, S, out, pooling="mean")
    run1, all1 = timed(fwd, args.iters, args.warmup)
    run2, all2 = timed(fwd, args.iters, 0)
    hip_ms = min(run1, run2)
    fl, att_share = flops(shape, B, S)
    run = {"workload": key, "shape": BASE, "chunks": B, "tokens": S, "hip_ms_run1": round(run1, 3), "hip_ms_run2": round(run2, 3),
           "hip_ms_all": [round(x, 3) for x in all1 + all2], "attention_flop_share": round(att_share, 3),
           "chunks_per_s": round(B / hip_ms * 1e3, 1), "tflops": round(fl / hip_ms / 1e9, 1), "peak_share": round(fl / hip_ms / 1e9 / PEAK_TFLOPS, 4)}
    if key == "base512" and not args.no_baseline:
        from archi_amd.encoder import MODEL_SHAPES, HipEncoder, random_init_weights
        bv, bH, bL, bheads, bI, bpos = MODEL_SHAPES[BGE][:6]
        bge = HipEncoder(bv, bH, bL, bheads, bI, bpos, random_init_weights(bv, bH, bL, bI, bpos, seed=args.seed), device=0)
        stage = torch.from_numpy(np.concatenate([np.minimum(ids, bv - 1), np.full((B, 1), S, np.int32)], 1)).to(dev).contiguous()
        out_b = torch.empty((B, bH), dtype=torch.float32, device=dev)
        bge_ms, _ = timed(lambda: bge.forward_lens(stage, B, S, out_b), args.iters, args.warmup)
        run["bge_base_ms"] = round(bge_ms, 3)
        run["ratio_vs_bge_base"] = round(hip_ms / bge_ms, 3)
        bge.close()
        del bge
    if not args.no_baseline:
        from tests.t5_ref import hf_model
        model = hf_model(shape, w).to(device=dev, dtype=torch.bfloat16)
        t_ids = torch.from_numpy(ids).long().to(dev)
        mask = torch.ones_like(t_ids)
        dense = torch.from_numpy(w["dense0"]).to(dev)

        def base():
            with torch.no_grad():
                h = model(input_ids=t_ids, attention_mask=mask).last_hidden_state
                return torch.nn.functional.normalize(h.float().mean(1) @ dense.t(), dim=-1)
        base_ms, _ = timed(base, max(2, args.iters // 2), 1)
        run["torch_bf16_ms"] = round(base_ms, 3)
        run["speedup_vs_torch"] = round(base_ms / hip_ms, 2)
        del model
        torch.cuda.empty_cache()
    fwd()
    got = out.cpu().numpy()
    ok = bool(np.isfinite(got).all())
    enc.close()
    if S == 512 and not args.no_check:
        from tests.t5_ref import cos_gap, dense_tail, hf_model, reference
        n = args.check_rows
        want = reference(hf_model(shape, w), ids[:n], [S] * n, "mean", dense_tail(w))
        gap = float(cos_gap(got[:n], want).max())
        run["check"] = {"rows": n, "max_1_minus_cos": gap, "max_abs": float(np.abs(got[:n] - want).max())}
        ok = ok and gap <= 1e-3
    run["ok"] = ok
    return run


def step_launches(args):
    """One attention launch with the bias against one without, same inputs, heads = 12, D = 128."""
    import ctypes
    import torch
    from archi_amd import _lib
    lib = _lib.init(0)
    assert _lib.is_dbg_library()
    heads, H, D, rep = 12, 768, 128, 10
    g = torch.Generator().manual_seed(args.seed)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    out = []
    for key, (B, S) in WORKLOADS.items():
        T = B * S
        q = (torch.randn(T, H, generator=g) * 0.3).to(torch.bfloat16).cuda()
        k, vt = torch.randn(T, H, generator=g).to(torch.bfloat16).cuda(), torch.randn(B, H, S, generator=g).to(torch.bfloat16).cuda()
        mask = torch.ones(T, dtype=torch.int32, device="cuda")
        lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
        tab = (torch.randn(heads, 2 * D + 1, generator=g) * 2.0).cuda()
        ctx = torch.empty((T, H), dtype=torch.bfloat16, device="cuda")

        def biased():
            for _ in range(rep):
                _lib.check(lib.ak_kts_t5_attn(P(q), P(k), P(vt), P(mask), P(lens), P(ctx), B, S, H, heads, 0, 0, P(tab), D, None), "ak_kts_t5_attn")

        def plain():
            for _ in range(rep):
                _lib.check(lib.ak_kt_attn_window(P(q), P(k), P(vt), P(mask), P(lens), P(ctx), B, S, H, heads, 0, 0, -1, None), "ak_kt_attn_window")

        rounds = {"biased": [], "unbiased": []}
        for r in range(args.rounds):                          # interleaved, so a drift of the clock meets both alike
            for name, fn in (("unbiased", plain), ("biased", biased)):
                ms, _ = timed(fn, args.iters, 1 if r else 2)
                rounds[name].append(ms * 1e3 / rep)
        ub, bi = rounds["unbiased"], rounds["biased"]
        out.append({"workload": key, "chunks": B, "tokens": S, "heads": heads, "D": D, "unbiased_us_rounds": [round(x, 2) for x in ub],
                    "biased_us_rounds": [round(x, 2) for x in bi], "unbiased_us": round(float(np.median(ub)), 2),
                    "biased_us": round(float(np.median(bi)), 2), "unbiased_spread_us": round(max(ub) - min(ub), 2),
                    "biased_minus_unbiased_us": round(float(np.median(bi) - np.median(ub)), 2),
                    "biased_over_unbiased": round(float(np.median(bi) / np.median(ub)), 4)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--check-rows", type=int, default=2)
    ap.add_argument("--no-baseline", action="store_true", help="skip transformers bf16 and the bge-base forward")
    ap.add_argument("--no-check", action="store_true", help="skip the float32 CPU check")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "t5_bench.json"))
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step_launches(args) if args.step == "launches" else step_forward(args.step, args)))
        return
    res = {"bench": "t5_embed", "precision": "bf16", "runs": [], "launches": None, "failed_step": None}
    passed = [a for a in sys.argv[1:]]
    for step in ("base512", "base8192", "launches"):
        env = dict(os.environ, ARCHI_HIP_DBG="1") if step == "launches" else dict(os.environ)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step] + passed, env=env, stdout=subprocess.PIPE,
                               timeout=STEP_LIMIT_S[step])
            rc = p.returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            res["failed_step"] = {"step": step, "exit": rc}      # nothing more is started on the GPU
            break
        got = json.loads(p.stdout.decode().strip().splitlines()[-1])
        if step == "launches":
            res["launches"] = got
        else:
            res["runs"].append(got)
    res["check_ok"] = res["failed_step"] is None and all(r.get("ok") for r in res["runs"])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if res["check_ok"] else 1)


if __name__ == "__main__":
    main()
