"""NomicBERT embedders on the HIP NomicBERT encoder (archi_amd.nomic.HipNomicBert), seeded weights: the nomic-embed-text-v1.5 shape at
128 x 512 and at 8 x 8192; per workload, TWICE in the same call, ms per forward and chunks/s (HIP events after warm-up), algorithmic
TFLOP/s and share of the 2.5 PF bf16 peak; beside them in the same run the bge-base forward at 128 x 512 (the project's flagship
encoder on the same token count) and transformers NomicBertModel bf16 + SDPA on the same GPU and ids; per-launch times of the three new
launches (k_nb_embed, k_nb_add_ln, k_nb_pool_part + k_nb_pool_fin) at both workloads' token counts with their GB/s and share of the
8 TB/s HBM peak, measured in a child process on libarchi_hip_dbg.so through the ak_kts_nb_* wrappers; then a check of the timed outputs
against float32 NomicBertModel on the CPU on sampled rows of the 512-token workload (exit status 1 on a mismatch; 8192-token rows are
checked by tests/test_nomic_gpu.py on a small shape). Prints ONE JSON line and writes it to --out.

Algorithmic flops per token and layer: 2 (4 H^2 + 3 H I) for the GEMMs (q / k / v 3 H^2, o H^2, gate / up 2 H I, down H I; base:
18.9 MFLOP) plus 4 H S for attention.
Bytes per token of the row launches (H = 768): embed 2 H (bf16 word row) + 4 H + 2 H (x32, h16) = 8 H; add + LayerNorm 4 H + 4 H in,
4 H + 2 H out = 14 H; pooling 4 H in.

    python scripts/bench_nomic_embed.py [--iters 5] [--no-baseline] [--no-check] [--no-launches] [--only base512,base8192] [--out profiles/nomic_bench.json]
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

BASE = "nomic-ai/nomic-embed-text-v1.5"
BGE = "BAAI/bge-base-en-v1.5"
PEAK_TFLOPS, PEAK_GBS = 2500.0, 8000.0
WORKLOADS = {"base512": (BASE, 128, 512), "base8192": (BASE, 8, 8192)}


def flops(shape, n_chunks, S):
    """(total, attention share, gemm flops per token and layer) of one forward over n_chunks full rows of S tokens."""
    H, L, I = shape[1], shape[2], shape[4]
    gemm = 2 * (4 * H * H + 3 * H * I)
    att = L * 4 * H * S
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


def launches(iters, warmup, seed):
    """The child's work (ARCHI_HIP_DBG=1): each new launch alone at H = 768, B x S = 128 x 512 and 8 x 8192, median of `iters`
    HIP-event times of 10 back-to-back launches each."""
    import ctypes
    import torch
    from archi_amd import _lib
    lib = _lib.init(0)
    assert _lib.is_dbg_library()
    H, vocab, rep = 768, 30528, 10
    g = torch.Generator().manual_seed(seed)
    word = (torch.randn(vocab, H, generator=g) * 0.02).to(torch.bfloat16).cuda()
    typ, gam, bet = torch.randn(2, H, generator=g).cuda(), (1 + 0.1 * torch.randn(H, generator=g)).cuda(), (0.1 * torch.randn(H, generator=g)).cuda()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    out = []
    for B, S in ((128, 512), (8, 8192)):
        T = B * S
        stage = torch.randint(3, vocab, (B, S + 1), generator=g, dtype=torch.int32)
        stage[:, S] = S
        stage = stage.cuda()
        x32, y32 = torch.empty((T, H), device="cuda"), torch.randn((T, H), device="cuda")
        h16 = torch.empty((T, H), dtype=torch.bfloat16, device="cuda")
        mask, lens = torch.empty(T, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        nch = (S + 63) // 64
        part, pooled = torch.empty((B * nch, H), device="cuda"), torch.empty((B, H), device="cuda")
        eps = ctypes.c_float(1e-12)

        def embed():
            for _ in range(rep):
                _lib.check(lib.ak_kts_nb_embed(P(stage), S + 1, ctypes.c_void_p(stage.data_ptr() + 4 * S), S + 1, B, S, H, vocab, P(word), P(typ), P(gam),
                                            P(bet), eps, P(x32), P(h16), P(mask), P(lens), None), "ak_kts_nb_embed")

        def add_ln():
            for _ in range(rep):
                _lib.check(lib.ak_kts_nb_add_ln(P(x32), P(y32), T, H, P(gam), P(bet), eps, P(h16), None), "ak_kts_nb_add_ln")

        def pool():
            for _ in range(rep):
                _lib.check(lib.ak_kts_nb_pool(P(x32), P(lens), B, S, H, 0, 1, P(part), P(pooled), None), "ak_kts_nb_pool")

        for name, fn, bytes_tok in (("k_nb_embed", embed, 8 * H), ("k_nb_add_ln", add_ln, 14 * H), ("k_nb_pool_part+fin", pool, 4 * H)):
            ms, _ = timed(fn, iters, warmup)
            us = ms * 1e3 / rep
            gbs = T * bytes_tok / (us * 1e-6) / 1e9
            out.append({"launch": name, "chunks": B, "tokens": S, "us": round(us, 2), "gb_per_s": round(gbs, 1), "hbm_peak_share": round(gbs / PEAK_GBS, 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--check-rows", type=int, default=2)
    ap.add_argument("--no-baseline", action="store_true", help="skip transformers bf16 + SDPA and the bge-base forward")
    ap.add_argument("--no-check", action="store_true", help="skip the float32 CPU check (kernel-trace runs)")
    ap.add_argument("--no-launches", action="store_true", help="skip the per-launch times (they need libarchi_hip_dbg.so)")
    ap.add_argument("--launches-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nomic_bench.json"))
    args = ap.parse_args()
    if args.launches_child:
        print(json.dumps(launches(args.iters, args.warmup, args.seed)))
        return
    import torch
    from archi_amd.encoder import MODEL_SHAPES, HipEncoder, random_init_weights
    from archi_amd.nomic import NOMIC_SHAPES, HipNomicBert, random_nomic_weights
    from tests.nomic_ref import cos_gap, hf_model, reference
    res = {"bench": "nomic_embed", "precision": "bf16", "runs": []}
    ok = True
    checks = []
    shape = NOMIC_SHAPES[BASE]
    w = random_nomic_weights(shape, seed=args.seed)
    for key in args.only.split(","):
        name, B, S = WORKLOADS[key]
        enc = HipNomicBert(shape, w, device=0)
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
            model = hf_model(shape, w, attn="sdpa").to(device=dev, dtype=torch.bfloat16)
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
            checks.append((key, ids, got))
        res["runs"].append(run)
    if not args.no_launches:
        # a process of its own: the single-launch wrappers live in libarchi_hip_dbg.so, and a process binds one library
        env = dict(os.environ, ARCHI_HIP_DBG="1")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--launches-child", "--iters", str(args.iters), "--warmup", str(args.warmup),
                            "--seed", str(args.seed)], env=env, stdout=subprocess.PIPE, timeout=600)
        ok = ok and p.returncode == 0
        res["launches"] = json.loads(p.stdout.decode().strip().splitlines()[-1]) if p.returncode == 0 else None
    # float32 CPU check of sampled rows of the timed outputs (a row's embedding does not depend on its neighbours)
    n = args.check_rows
    res["check"] = []
    for key, ids, got in checks:
        want = reference(hf_model(shape, w), ids[:n], [ids.shape[1]] * n, "mean")
        gap = float(cos_gap(got[:n], want).max())
        res["check"].append({"workload": key, "rows": n, "max_1_minus_cos": gap, "max_abs": float(np.abs(got[:n] - want).max())})
        ok = ok and gap <= 1e-3
    res["check_ok"] = ok
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
