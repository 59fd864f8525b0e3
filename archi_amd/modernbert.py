"""HipModernBert -- Python handle of the HIP ModernBERT encoder (ak_mbert_*): nomic-ai/modernbert-embed-base,
Alibaba-NLP/gte-modernbert-base, lightonai/modernbert-embed-large and the answerdotai/ModernBERT base models they are tuned from.

PyTorch-ROCm only HOLDS the weights in HBM (bf16 matrices, fp32 vectors) and hands raw device pointers to the C ABI; every
arithmetic step of the forward pass runs in hand-written HIP kernels (archi_amd/csrc/mbert.hip, attn_long.hip, gemm.hip).
Also here: the config.json reader that refuses what the kernels do not implement, the checkpoint loader and seeded random
weights of the named shapes.
"""
from __future__ import annotations

import ctypes
import json
import os
from typing import Dict, List, Optional

import numpy as np

from ._lib import MBERT_MAX_LAYERS, AkModernBertConfig
from ._stack import HipStack, read_safetensors_dir, seeded_mat_vec

MAX_SEQ = 8192          # longest row the kernels take (attn_long.hip)
HEAD_DIM = 64


def _every(n_layers: int, every: int):
    """layer_types of the released models: a global layer every `every` layers, starting with layer 0 (1 = global, 0 = sliding)."""
    return tuple(1 if l % every == 0 else 0 for l in range(n_layers))


# name -> (vocab, hidden, layers, heads, intermediate, max_position, norm_eps, global theta, local theta, local_attention,
#          layer types (1 global / 0 sliding), default pooling)
MODERNBERT_SHAPES = {
    "answerdotai/ModernBERT-base": (50368, 768, 22, 12, 1152, 8192, 1e-5, 160000.0, 10000.0, 128, _every(22, 3), "mean"),
    "answerdotai/ModernBERT-large": (50368, 1024, 28, 16, 2624, 8192, 1e-5, 160000.0, 10000.0, 128, _every(28, 3), "mean"),
    "nomic-ai/modernbert-embed-base": (50368, 768, 22, 12, 1152, 8192, 1e-5, 160000.0, 10000.0, 128, _every(22, 3), "mean"),
    "Alibaba-NLP/gte-modernbert-base": (50368, 768, 22, 12, 1152, 8192, 1e-5, 160000.0, 10000.0, 128, _every(22, 3), "cls"),
    "lightonai/modernbert-embed-large": (50368, 1024, 28, 16, 2624, 8192, 1e-5, 160000.0, 10000.0, 128, _every(28, 3), "mean"),
    # small shapes of the test fixtures (tests/golden/make_modernbert_fixtures.py)
    "modernbert-tiny-mix": (1000, 128, 4, 2, 192, 8192, 1e-5, 160000.0, 10000.0, 128, (1, 0, 0, 1), "mean"),
    "modernbert-tiny-cls": (1000, 128, 4, 2, 192, 8192, 1e-5, 160000.0, 10000.0, 128, (1, 0, 0, 1), "cls"),
    "modernbert-tiny-global": (1000, 128, 2, 2, 192, 8192, 1e-5, 160000.0, 10000.0, 128, (1, 1), "mean"),
    "modernbert-tiny-local": (1000, 128, 3, 2, 192, 8192, 1e-5, 160000.0, 10000.0, 128, (0, 0, 0), "mean"),
    "modernbert-tiny-256": (1000, 256, 3, 4, 320, 8192, 1e-5, 160000.0, 10000.0, 128, (1, 0, 0), "mean"),
    # the large shape's width through a two-layer cut
    "modernbert-large-cut2": (2000, 1024, 2, 16, 2624, 8192, 1e-5, 160000.0, 10000.0, 128, (1, 0), "mean"),
}

LAYER_KEYS = ("attn_norm", "wqkv", "wo", "mlp_norm", "wi", "mlp_wo")
MATRIX_KEYS = {"wqkv", "wo", "wi", "mlp_wo"}
# our name -> HF ModernBertModel state-dict name (layer keys under "layers.{l}."); layer 0 has no attn_norm (nn.Identity)
HF_LAYER_NAMES = {"attn_norm": "attn_norm.weight", "wqkv": "attn.Wqkv.weight", "wo": "attn.Wo.weight", "mlp_norm": "mlp_norm.weight",
                  "wi": "mlp.Wi.weight", "mlp_wo": "mlp.Wo.weight"}


def weight_names(layers: int) -> List[str]:
    """Every weight of a ModernBERT model in the header's order, without layer 0's attn_norm (the identity: the model has none)."""
    names = ["tok_embeddings", "emb_norm", "final_norm"]
    for l in range(layers):
        names += [f"l{l}.{k}" for k in LAYER_KEYS if not (l == 0 and k == "attn_norm")]
    return names


def hf_state_dict(weights: Dict[str, "np.ndarray"]) -> Dict[str, "np.ndarray"]:
    """Our weight names -> HF ModernBertModel's (no "model." prefix)."""
    sd = {"embeddings.tok_embeddings.weight": weights["tok_embeddings"], "embeddings.norm.weight": weights["emb_norm"],
          "final_norm.weight": weights["final_norm"]}
    for name, arr in weights.items():
        if name[0] == "l" and "." in name:
            l, k = name[1:].split(".", 1)
            sd[f"layers.{l}.{HF_LAYER_NAMES[k]}"] = arr
    return sd


def random_modernbert_weights(shape, seed: int = 0, std: float = 0.02) -> Dict[str, "np.ndarray"]:
    """Seeded random weights of a ModernBERT shape (a MODERNBERT_SHAPES tuple or name). Matrices are drawn with `std` and ROUNDED
    TO bf16 (kept as float32 values), as random_qwen3_weights does: a float32 reference on the same values measures the kernels'
    activation rounding alone. Norm weights are drawn around 1, not set to it."""
    if isinstance(shape, str):
        shape = MODERNBERT_SHAPES[shape]
    vocab, H, L, heads, I = shape[:5]
    mat, vec = seeded_mat_vec(seed, std)
    w = {"tok_embeddings": mat(vocab, H), "emb_norm": vec(H), "final_norm": vec(H)}
    for l in range(L):
        p = f"l{l}."
        if l:
            w[p + "attn_norm"] = vec(H)
        w[p + "wqkv"], w[p + "wo"] = mat(3 * H, H), mat(H, H)
        w[p + "mlp_norm"] = vec(H)
        w[p + "wi"], w[p + "mlp_wo"] = mat(2 * I, H), mat(H, I)
    return w


def modernbert_config_shape(cfg: dict, where: str = "config.json", pooling: str = "mean"):
    """config.json of a ModernBERT checkpoint (transformers 5 `layer_types` / `rope_parameters`, or transformers 4
    `global_attn_every_n_layers` / `global_rope_theta` / `local_rope_theta`) -> MODERNBERT_SHAPES-style tuple; everything the
    kernels do not implement is refused with a ValueError that names the field."""
    if cfg.get("model_type") != "modernbert":
        raise ValueError(f"{where}: model_type {cfg.get('model_type')!r} is not modernbert")
    for flag in ("attention_bias", "mlp_bias", "norm_bias"):
        if cfg.get(flag, False):
            raise ValueError(f"{where}: {flag} is not supported (the HIP ModernBERT kernels carry no bias)")
    if cfg.get("hidden_activation", "gelu") != "gelu":
        raise ValueError(f"{where}: hidden_activation {cfg.get('hidden_activation')!r} (the HIP ModernBERT kernels implement exact GELU / GeGLU)")
    H, heads, L = int(cfg["hidden_size"]), int(cfg["num_attention_heads"]), int(cfg["num_hidden_layers"])
    if heads <= 0 or H % heads or H // heads != HEAD_DIM:
        raise ValueError(f"{where}: head size hidden_size / num_attention_heads = {H / max(heads, 1):g} (the HIP ModernBERT kernels implement {HEAD_DIM})")
    rp = cfg.get("rope_parameters") or {}
    thetas = {}
    for kind, old in (("full_attention", "global_rope_theta"), ("sliding_attention", "local_rope_theta")):
        sub = rp.get(kind) if isinstance(rp.get(kind), dict) else None
        if sub is None and "rope_theta" in rp:
            sub = rp                                   # one flat rope_parameters block for both layer types
        if sub is not None:
            rt = sub.get("rope_type", sub.get("type", "default"))
            if rt not in ("default", None):
                raise ValueError(f"{where}: rope_parameters.{kind}.rope_type {rt!r} is not supported (default RoPE only)")
            theta = sub.get("rope_theta")
        else:
            theta = cfg.get(old)
        if theta is None:
            raise ValueError(f"{where}: no rope theta for {kind} layers (rope_parameters.{kind}.rope_theta / {old})")
        thetas[kind] = float(theta)
    if cfg.get("rope_scaling"):
        raise ValueError(f"{where}: rope_scaling is not supported (default RoPE only)")
    lt = cfg.get("layer_types")
    if lt is None:
        every = cfg.get("global_attn_every_n_layers")
        if not every:
            raise ValueError(f"{where}: neither layer_types nor global_attn_every_n_layers")
        lt = ["full_attention" if l % int(every) == 0 else "sliding_attention" for l in range(L)]
    if len(lt) != L or any(t not in ("full_attention", "sliding_attention") for t in lt):
        raise ValueError(f"{where}: layer_types must name full_attention / sliding_attention for each of the {L} layers")
    if L > MBERT_MAX_LAYERS:
        raise ValueError(f"{where}: num_hidden_layers {L} (at most {MBERT_MAX_LAYERS})")
    local = int(cfg.get("local_attention", 128))
    if local < 2 or local % 2:
        raise ValueError(f"{where}: local_attention {local} must be even and >= 2 (the window is local_attention / 2 keys to each side)")
    I = int(cfg["intermediate_size"])
    if H % 128 or H > 1024 or I % 64:
        raise ValueError(f"{where}: hidden_size {H} / intermediate_size {I} (the HIP GEMM takes hidden_size % 128 == 0, <= 1024, and "
                         "intermediate_size % 64 == 0)")
    return (int(cfg["vocab_size"]), H, L, heads, I, int(cfg.get("max_position_embeddings", 8192)), float(cfg.get("norm_eps", 1e-5)),
            thetas["full_attention"], thetas["sliding_attention"], local, tuple(1 if t == "full_attention" else 0 for t in lt), pooling)


def shape_hf_config(shape, **extra):
    """A MODERNBERT_SHAPES tuple -> transformers.ModernBertConfig (the tests' float32 reference; pad / special ids inside the vocabulary)."""
    from transformers import ModernBertConfig
    if isinstance(shape, str):
        shape = MODERNBERT_SHAPES[shape]
    vocab, H, L, heads, I, max_pos, eps, tg, tl, local, types, _ = shape
    kw = dict(vocab_size=vocab, hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, intermediate_size=I,
              max_position_embeddings=max_pos, norm_eps=eps, local_attention=local,
              layer_types=["full_attention" if t else "sliding_attention" for t in types],
              rope_parameters={"full_attention": {"rope_type": "default", "rope_theta": tg},
                               "sliding_attention": {"rope_type": "default", "rope_theta": tl}},
              pad_token_id=0, bos_token_id=1, eos_token_id=2, cls_token_id=1, sep_token_id=2)
    kw.update(extra)
    lt = kw.pop("layer_types")
    # (transformers 5.15 cannot validate rope_parameters at construction when layer_types names one type only: set it afterwards)
    cfg = ModernBertConfig(**kw)
    cfg.layer_types = lt
    return cfg


def load_modernbert_weights(model_dir: str):
    """Local ModernBERT checkpoint directory (config.json + model.safetensors or sharded model-*.safetensors) -> (shape, weights in
    our names). A "model." prefix on the tensor names is stripped; heads of a masked-LM checkpoint are ignored. No network."""
    cfg = json.load(open(os.path.join(model_dir, "config.json")))
    shape = modernbert_config_shape(cfg, os.path.join(model_dir, "config.json"))
    sd = read_safetensors_dir(model_dir)
    L = shape[2]
    w = {"tok_embeddings": sd["embeddings.tok_embeddings.weight"], "emb_norm": sd["embeddings.norm.weight"],
         "final_norm": sd["final_norm.weight"]}
    for l in range(L):
        for k, hf in HF_LAYER_NAMES.items():
            if l == 0 and k == "attn_norm":
                continue
            w[f"l{l}.{k}"] = sd[f"layers.{l}.{hf}"]
    return shape, w


def interleave_wi(wi: "np.ndarray") -> "np.ndarray":
    """Wi [2 I][H] -> the row order ak_mbert_create builds for the GeGLU epilogue (gemm.hip MODE 8): row 2 j = Wi row j (the GELU
    input), row 2 j + 1 = Wi row I + j (the gate)."""
    I = wi.shape[0] // 2
    out = np.empty_like(wi)
    out[0::2], out[1::2] = wi[:I], wi[I:]
    return out


def geglu_interleaved(y: "np.ndarray") -> "np.ndarray":
    """The MODE 8 epilogue restated in numpy on product rows [.., 2 I] in the interleaved order: gelu_erf(y[2 j]) * y[2 j + 1]."""
    from math import sqrt
    import torch
    a, g = y[..., 0::2], y[..., 1::2]
    erf = torch.erf(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) / sqrt(2.0)).numpy()
    return (0.5 * a * (1.0 + erf) * g).astype(np.float32)


class HipModernBert(HipStack):
    family, prefix, embed_key, matrix_keys, pooling_noun = "ModernBERT", "mbert", "tok_embeddings", MATRIX_KEYS, "ModernBERT models"

    def __init__(self, shape, weights: Dict[str, "np.ndarray"], device: Optional[int] = None):
        """shape: a MODERNBERT_SHAPES tuple or name; weights: our names (weight_names), numpy arrays or torch tensors."""
        if isinstance(shape, str):
            shape = MODERNBERT_SHAPES[shape]
        vocab, H, L, heads, I, max_pos, eps, theta_g, theta_l, local, types, pooling = shape
        if L > MBERT_MAX_LAYERS or len(types) != L:
            raise ValueError(f"ModernBERT shape: {L} layers with {len(types)} layer types (at most {MBERT_MAX_LAYERS} layers)")
        self.shape = tuple(shape)
        self.hidden, self.layers, self.vocab, self.pooling, self.out_dim = H, L, vocab, pooling, H
        self.max_seq = min(int(max_pos), MAX_SEQ)
        self._upload(weights, weight_names(L), device)
        ptr_names = ["tok_embeddings", "emb_norm", "final_norm"]
        for l in range(L):              # layer 0's attn_norm is the identity: the library does not read the pointer
            ptr_names += ["emb_norm" if (l == 0 and k == "attn_norm") else f"l{l}.{k}" for k in LAYER_KEYS]
        self._create(AkModernBertConfig(vocab, H, L, heads, I, max_pos, eps, theta_g, theta_l, local // 2, (ctypes.c_int * MBERT_MAX_LAYERS)(*types)),
                     ptr_names)
