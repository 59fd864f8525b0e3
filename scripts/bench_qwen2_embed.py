"""Qwen2 embedders on the HIP Qwen2 decoder (archi_amd.qwen2.HipQwen2), seeded weights drawn on the GPU (bf16 matrices, float32 biases
N(0, 2) and norm vectors): the Alibaba-NLP/gte-Qwen2-1.5B-instruct shape at 128 x 512 and the gte-Qwen2-7B-instruct shape at 64 x 512
and at 8 x 8192; per workload ms per forward and chunks/s (HIP events after warm-up), algorithmic TFLOP/s and share of the 2.5 PF bf16
peak; beside them in the same run transformers Qwen2Model bf16 + SDPA on the same GPU, weights and ids with the cosine between the two
outputs, and the Mistral-7B shape's forward (archi_amd.llama.HipLlama) on the 7B token counts; and the per-launch time of the split
attention mapping (a child process on the dbg library, whose ak_kts_q2_attn / ak_kts_ll_attn wrappers call the launchers the forward
passes call): ONE G = 7 launch at 28 / 4 heads against ONE G = 4 launch of the unsplit kernel at 32 / 8 heads, S = 8192, in alternating
runs. Per query head the G = 7 launch should cost at most 8 / 7 of the G = 4 one -- the per-wave work is the same, two workgroups of
4 + 3 waves serve 7 heads and a 3-wave workgroup costs at most a 4-wave one -- plus the spread measured between the repeated runs of the
G = 4 launch. These are records, not pass criteria: the exit status is 1 only for a non-finite output. Prints ONE JSON line.

Algorithmic flops per token and layer: 2 H (NQ + 2 NKV) + 2 NQ H + 6 H I for the GEMMs (NQ = q_heads x 128, NKV = kv_heads x 128) plus
4 NQ keys for attention, keys = the mean number of keys a query of a full causal row sees.

    python scripts/bench_qwen2_embed.py [--iters 3] [--no-baseline] [--no-mistral] [--no-attn] [--only q15_512,q7_512,q7_8192] [--out profiles/qwen2_bench.json]
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

from scripts.bench_llama_embed import HD, PEAK_TFLOPS, decoder_dims, flops, gpu_weights, timed, visible_keys  # noqa: E402

Q15, Q7, MISTRAL = "Alibaba-NLP/gte-Qwen2-1.5B-instruct", "Alibaba-NLP/gte-Qwen2-7B-instruct", "intfloat/e5-mistral-7b-instruct"
WORKLOADS = {"q15_512": (Q15, 128, 512), "q7_512": (Q7, 64, 512), "q7_8192": (Q7, 8, 8192)}


def qwen2_weights(shape, seed, bias_std=2.0):
    """gpu_weights of the Qwen2 names; the q / k / v biases float32 N(0, bias_std) rounded to bf16."""
    import torch
    from archi_amd import qwen2
    names = qwen2.weight_order(shape.layers)
    dims = decoder_dims(shape.vocab, shape.hidden, shape.q_heads, shape.kv_heads, shape.intermediate)
    w = gpu_weights([n for n in names if n.split(".")[-1] not in ("bq", "bk", "bv")], dims, seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    for n in names:
        k = n.split(".")[-1]
        if k in ("bq", "bk", "bv"):
            rows = (shape.q_heads if k == "bq" else shape.kv_heads) * HD
            w[n] = (torch.randn(rows, device="cuda", generator=g, dtype=torch.float32) * bias_std).to(torch.bfloat16).float()
    return w


def attn_child(iters):
    """One attention launch at a time on random operands, B = 8, S = 8192: launch_attn_causal_split at 28 query heads on 4 kv heads
    (G = 7: workgroups of 4 + 3 waves) and launch_attn_causal at 32 on 8 (G = 4), alternating, `iters` timed launches each per round
    and 5 rounds; causal and bidirectional. Runs in a process that loaded the dbg library."""
    import ctypes
    import torch
    from archi_amd import _lib
    lib = _lib.init(0)
    assert _lib.is_dbg_library()
    B, S = 8, 8192
    g = torch.Generator(device="cuda").manual_seed(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    ops = {}
    for tag, (nq, nkv) in (("g7", (28, 4)), ("g4", (32, 8))):
        ops[tag] = dict(nq=nq, nkv=nkv, q=(torch.randn((B, nq, S, HD), device="cuda", generator=g) * 0.05).to(torch.bfloat16),
                        k=torch.randn((B, nkv, S, HD), device="cuda", generator=g).to(torch.bfloat16),
                        v=torch.randn((B, nkv, S, HD), device="cuda", generator=g).to(torch.bfloat16),
                        ctx=torch.empty((B, S, nq * HD), dtype=torch.bfloat16, device="cuda"))
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda")

    def launch(tag, bidir):
        o = ops[tag]
        if tag == "g7":
            rc = lib.ak_kts_q2_attn(P(o["q"]), P(o["k"]), P(o["v"]), P(lens), P(o["ctx"]), B, S, o["nq"], o["nkv"], bidir, None)
        else:
            rc = lib.ak_kts_ll_attn(P(o["q"]), P(o["k"]), P(o["v"]), P(lens), P(o["ctx"]), B, S, o["nq"], o["nkv"], 0, bidir, None)
        _lib.check(rc, "attention launch " + tag)

    out = {"B": B, "S": S, "g7_heads": [28, 4], "g4_heads": [32, 8], "bound_derived": round(8 / 7, 4)}
    for mode, bidir in (("causal", 0), ("bidirectional", 1)):
        rounds = {"g7": [], "g4": []}
        for _ in range(5):
            for tag in ("g4", "g7"):
                rounds[tag].append(timed(lambda: launch(tag, bidir), iters, 1)[0])
        g7, g4 = float(np.median(rounds["g7"])), float(np.median(rounds["g4"]))
        keys = S if bidir else visible_keys(S, 0)
        spread = (max(rounds["g4"]) - min(rounds["g4"])) / g4
        ratio = (g7 / 28) / (g4 / 32)
        out[mode] = {"g7_ms": round(g7, 4), "g4_ms": round(g4, 4), "g7_ms_rounds": [round(x, 4) for x in rounds["g7"]],
                     "g4_ms_rounds": [round(x, 4) for x in rounds["g4"]], "g4_spread": round(spread, 4),
                     "per_query_head_ratio_g7_over_g4": round(ratio, 4), "within_bound_plus_spread": bool(ratio <= 8 / 7 * (1 + spread)),
                     "g7_peak_share": round(4.0 * 28 * HD * keys * B * S / g7 / 1e9 / PEAK_TFLOPS, 4),
                     "g4_peak_share": round(4.0 * 32 * HD * keys * B * S / g4 / 1e9 / PEAK_TFLOPS, 4)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-baseline", action="store_true", help="skip transformers Qwen2Model bf16 + SDPA")
    ap.add_argument("--no-mistral", action="store_true", help="skip the Mistral-7B shape's forward")
    ap.add_argument("--no-attn", action="store_true", help="skip the per-launch attention child")
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--attn-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.attn_child:
        return attn_child(args.iters)
    import torch
    from archi_amd import llama, qwen2
    res = {"bench": "qwen2_embed", "precision": "bf16", "runs": []}
    ok = True
    only = args.only.split(",")
    runs = {}
    for name in (Q15, Q7):
        keys = [k for k in only if WORKLOADS[k][0] == name]
        if not keys:
            continue
        shape = qwen2.QWEN2_SHAPES[name]
        w = qwen2_weights(shape, args.seed)
        enc = qwen2.HipQwen2(shape, w, device=0)
        dev = enc._dev
        model = None
        if not args.no_baseline:
            from transformers import Qwen2Model
            from tests.qwen2_ref import hf_config
            cfg = hf_config(shape)
            cfg._attn_implementation = "sdpa"
            with torch.device("meta"):
                model = Qwen2Model(cfg)
            model.load_state_dict({k: v.to(torch.bfloat16) for k, v in qwen2.hf_state_dict(w, shape.layers).items()}, assign=True, strict=True)
            model.rotary_emb = type(model.rotary_emb)(config=cfg).to(dev)
            model = model.eval()
        for key in keys:
            _, B, S = WORKLOADS[key]
            ids = np.random.default_rng(args.seed + S).integers(3, shape.vocab, (B, S)).astype(np.int32)
            st = torch.from_numpy(np.concatenate([ids, np.full((B, 1), S, np.int32)], 1)).to(dev).contiguous()
            out = torch.empty((B, enc.out_dim), dtype=torch.float32, device=dev)
            hip_ms, all_ms = timed(lambda: enc.forward_lens(st, B, S, out), args.iters, args.warmup)
            fl, att_share, gemm_tok = flops(shape.hidden, shape.layers, shape.q_heads, shape.kv_heads, shape.intermediate, 0, B, S)
            run = {"workload": key, "shape": name, "chunks": B, "tokens": S, "query_heads_per_kv_head": shape.q_heads // shape.kv_heads,
                   "hip_ms": round(hip_ms, 3), "hip_ms_all": [round(x, 3) for x in all_ms], "gemm_mflop_per_token_layer": round(gemm_tok / 1e6, 2),
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
    if not args.no_mistral and any(WORKLOADS[k][0] == Q7 for k in only):
        ms = llama.LLAMA_SHAPES[MISTRAL]
        mw = gpu_weights(llama.weight_order(ms.layers), decoder_dims(ms.vocab, ms.hidden, ms.q_heads, ms.kv_heads, ms.intermediate), args.seed)
        dec = llama.HipLlama(ms, mw, device=0)
        for key in (k for k in only if WORKLOADS[k][0] == Q7):
            _, B, S = WORKLOADS[key]
            ids = np.random.default_rng(args.seed + S).integers(3, ms.vocab, (B, S)).astype(np.int32)
            st = torch.from_numpy(np.concatenate([ids, np.full((B, 1), S, np.int32)], 1)).to(dec._dev).contiguous()
            out = torch.empty((B, ms.hidden), dtype=torch.float32, device=dec._dev)
            m_ms, _ = timed(lambda: dec.forward_lens(st, B, S, out), args.iters, args.warmup)
            fl = flops(ms.hidden, ms.layers, ms.q_heads, ms.kv_heads, ms.intermediate, ms.window, B, S)[0]
            runs[key]["mistral_7b_ms"] = round(m_ms, 3)
            runs[key]["mistral_7b_peak_share"] = round(fl / m_ms / 1e9 / PEAK_TFLOPS, 4)
        dec.close()
        del dec, mw
        torch.cuda.empty_cache()
    if not args.no_attn:
        # a fresh child on the dbg library (the single-launch wrappers live there); this process has released its buffers
        env = dict(os.environ, ARCHI_HIP_DBG="1")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--attn-child", "--iters", str(max(args.iters, 5))], env=env,
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
