"""Mistral-7B embedders on the HIP Mistral / Llama decoder (archi_amd.llama.HipLlama), seeded weights of the
intfloat/e5-mistral-7b-instruct shape (drawn on the GPU, bf16: 7.1 G parameters do not pass through host memory) at 64 x 512 and at
8 x 8192 (the latter walks the sliding window of 4096); per workload ms per forward and chunks/s (HIP events after warm-up), algorithmic
TFLOP/s and share of the 2.5 PF bf16 peak; beside them in the same run transformers MistralModel bf16 + SDPA on the same GPU, weights and
ids with the cosine between the two outputs, and the Qwen3-Embedding-8B shape's forward (archi_amd.decoder.HipDecoder) on the same token
counts; the per-launch time of ONE banded (w = 4096) against ONE un-banded launch_attn_causal at 8 x 8192 (a child process on the dbg
library, whose ak_kts_ll_attn wrapper calls the launcher the forward pass calls). These are records, not pass criteria: the exit status
is 1 only for a non-finite output. Prints ONE JSON line.

Algorithmic flops per token and layer: 2 H (NQ + 2 NKV) + 2 NQ H + 6 H I for the GEMMs (NQ = 32 x 128, NKV = 8 x 128: 436 MFLOP) plus
4 NQ keys for attention, keys = the mean number of keys a query of a full row sees (key <= query, query - key <= w - 1).

    python scripts/bench_llama_embed.py [--iters 3] [--no-baseline] [--no-qwen3] [--no-attn] [--only m512,m8192] [--out profiles/llama_bench.json]
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

NAME = "intfloat/e5-mistral-7b-instruct"
QWEN3 = "Qwen/Qwen3-Embedding-8B"
PEAK_TFLOPS = 2500.0
WORKLOADS = {"m512": (64, 512), "m8192": (8, 8192)}
HD = 128


def visible_keys(S, w):
    """Mean number of keys a query of a full S-token row sees under the causal mask with window w (0: none)."""
    q = np.arange(S)
    return float((np.minimum(q + 1, w) if w else q + 1).mean())


def flops(H, L, nq, nkv, I, w, n_chunks, S):
    """(total, attention share, gemm flops per token and layer) of one forward over n_chunks full rows of S tokens."""
    gemm = 2 * H * (nq + 2 * nkv) * HD + 2 * nq * HD * H + 6 * H * I
    att = 4 * nq * HD * visible_keys(S, w)
    return n_chunks * S * L * (gemm + att), att / (gemm + att), gemm


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


def gpu_weights(names, dims, seed, std=0.02):
    """Seeded weights drawn on the GPU: bf16 matrices of std `std`, float32 norm vectors around 1. dims(name) -> the tensor's shape."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = {}
    for n in names:
        d = dims(n)
        if len(d) == 2:
            w[n] = (torch.randn(d, device="cuda", generator=g, dtype=torch.float32) * std).to(torch.bfloat16)
        else:
            w[n] = 1.0 + 0.1 * torch.randn(d, device="cuda", generator=g, dtype=torch.float32)
    return w


def decoder_dims(vocab, H, nq, nkv, I):
    def dims(name):
        k = name.split(".")[-1]
        return {"embed_tokens": (vocab, H), "norm": (H,), "wq": (nq * HD, H), "wk": (nkv * HD, H), "wv": (nkv * HD, H), "wo": (H, nq * HD),
                "ln_in": (H,), "ln_post": (H,), "w_gate": (I, H), "w_up": (I, H), "w_down": (H, I), "q_norm": (HD,), "k_norm": (HD,)}[k]
    return dims


def attn_child(iters):
    """One launch_attn_causal at a time on random operands, B = 8, S = 8192, 32 query heads on 8 kv heads: the un-banded launch
    (window 0) and the banded one (window 4096). Runs in a process that loaded the dbg library."""
    import ctypes
    import torch
    from archi_amd import _lib
    lib = _lib.init(0)
    assert _lib.is_dbg_library()
    B, S, nq, nkv, w = 8, 8192, 32, 8, 4096
    g = torch.Generator(device="cuda").manual_seed(0)
    q = (torch.randn((B, nq, S, HD), device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    k = torch.randn((B, nkv, S, HD), device="cuda", generator=g).to(torch.bfloat16)
    v = torch.randn((B, nkv, S, HD), device="cuda", generator=g).to(torch.bfloat16)
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
    ctx = torch.empty((B, S, nq * HD), dtype=torch.bfloat16, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    out = {"B": B, "S": S, "q_heads": nq, "kv_heads": nkv, "window": w}
    for name, win in (("causal", 0), ("banded", w)):
        def launch():
            _lib.check(lib.ak_kts_ll_attn(P(q), P(k), P(v), P(lens), P(ctx), B, S, nq, nkv, win, 0, None), "ak_kts_ll_attn")
        ms, _ = timed(launch, iters, 2)
        fl = 4.0 * nq * HD * visible_keys(S, win) * B * S
        out[name + "_ms"] = round(ms, 4)
        out[name + "_peak_share"] = round(fl / ms / 1e9 / PEAK_TFLOPS, 4)
    out["banded_over_causal"] = round(out["banded_ms"] / out["causal_ms"], 3)
    # key blocks a workgroup of 32 query rows walks, summed over the row: causal qb + 1, banded min(qb + 1, w / 32 + 1)
    qb = np.arange(S // 32)
    out["key_blocks_walked_ratio_derived"] = round(float(np.minimum(qb + 1, w // 32 + 1).sum() / (qb + 1).sum()), 3)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-baseline", action="store_true", help="skip transformers MistralModel bf16 + SDPA")
    ap.add_argument("--no-qwen3", action="store_true", help="skip the Qwen3-Embedding-8B shape's forward")
    ap.add_argument("--no-attn", action="store_true", help="skip the per-launch attention child")
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--attn-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.attn_child:
        return attn_child(args.iters)
    import torch
    from archi_amd import decoder, llama
    shape = llama.LLAMA_SHAPES[NAME]
    res = {"bench": "llama_embed", "precision": "bf16", "shape": NAME, "runs": []}
    ok = True
    w = gpu_weights(llama.weight_order(shape.layers), decoder_dims(shape.vocab, shape.hidden, shape.q_heads, shape.kv_heads, shape.intermediate),
                    args.seed)
    enc = llama.HipLlama(shape, w, device=0)
    dev = enc._dev
    model = None
    if not args.no_baseline:
        from transformers import MistralModel
        from tests.llama_ref import hf_config
        cfg = hf_config(shape)
        cfg._attn_implementation = "sdpa"
        with torch.device("meta"):
            model = MistralModel(cfg)
        model.load_state_dict({k: v.to(torch.bfloat16) for k, v in llama.hf_state_dict(w, shape.layers).items()}, assign=True, strict=True)
        model.rotary_emb = type(model.rotary_emb)(config=cfg).to(dev)
        model = model.eval()
    runs = {}
    for key in args.only.split(","):
        B, S = WORKLOADS[key]
        ids = np.random.default_rng(args.seed + S).integers(3, shape.vocab, (B, S)).astype(np.int32)
        st = torch.from_numpy(np.concatenate([ids, np.full((B, 1), S, np.int32)], 1)).to(dev).contiguous()
        out = torch.empty((B, enc.out_dim), dtype=torch.float32, device=dev)
        fwd = lambda: enc.forward_lens(st, B, S, out)
        hip_ms, all_ms = timed(fwd, args.iters, args.warmup)
        fl, att_share, gemm_tok = flops(shape.hidden, shape.layers, shape.q_heads, shape.kv_heads, shape.intermediate, shape.window, B, S)
        run = {"workload": key, "chunks": B, "tokens": S, "window": shape.window, "hip_ms": round(hip_ms, 3),
               "hip_ms_all": [round(x, 3) for x in all_ms], "gemm_mflop_per_token_layer": round(gemm_tok / 1e6, 2),
               "attention_flop_share": round(att_share, 3), "chunks_per_s": round(B / hip_ms * 1e3, 2),
               "tflops": round(fl / hip_ms / 1e9, 1), "peak_share": round(fl / hip_ms / 1e9 / PEAK_TFLOPS, 4)}
        got = out.clone()
        ok = ok and bool(torch.isfinite(got).all())
        if model is not None:
            t_ids = torch.from_numpy(ids).long().to(dev)

            def base():
                with torch.no_grad():
                    return torch.nn.functional.normalize(model(input_ids=t_ids).last_hidden_state[:, -1].float(), dim=-1)
            base_ms, _ = timed(base, args.iters, args.warmup)
            run["torch_bf16_sdpa_ms"] = round(base_ms, 3)
            run["speedup_vs_torch"] = round(base_ms / hip_ms, 2)
            run["min_cos_vs_torch_bf16"] = round(float((got * base()).sum(1).min()), 5)
        runs[key] = run
        res["runs"].append(run)
    enc.close()
    del enc, model, w
    torch.cuda.empty_cache()
    if not args.no_qwen3:
        qs = decoder.QWEN3_SHAPES[QWEN3]
        vocab, H, L, nq, nkv, I = qs[:6]
        qw = gpu_weights(decoder.weight_order(L), decoder_dims(vocab, H, nq, nkv, I), args.seed)
        dec = decoder.HipDecoder(qs, qw, device=0)
        for key in args.only.split(","):
            B, S = WORKLOADS[key]
            ids = np.random.default_rng(args.seed + S).integers(3, vocab, (B, S)).astype(np.int32)
            st = torch.from_numpy(np.concatenate([ids, np.full((B, 1), S, np.int32)], 1)).to(dec._dev).contiguous()
            out = torch.empty((B, H), dtype=torch.float32, device=dec._dev)
            q_ms, _ = timed(lambda: dec.forward_lens(st, B, S, out), args.iters, args.warmup)
            fl = flops(H, L, nq, nkv, I, 0, B, S)[0]
            runs[key]["qwen3_8b_ms"] = round(q_ms, 3)
            runs[key]["qwen3_8b_peak_share"] = round(fl / q_ms / 1e9 / PEAK_TFLOPS, 4)
        dec.close()
        del dec, qw
        torch.cuda.empty_cache()
    if not args.no_attn:
        # a fresh child on the dbg library (the single-launch wrapper lives there); this process has released its buffers
        env = dict(os.environ, ARCHI_HIP_DBG="1")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--attn-child", "--iters", str(max(args.iters, 10))], env=env,
                           stdout=subprocess.PIPE, timeout=300)
        ok = ok and p.returncode == 0
        if p.returncode == 0:
            res["attention_launch"] = json.loads(p.stdout.decode().strip().splitlines()[-1])
    res["ok"] = ok
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
