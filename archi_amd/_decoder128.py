"""What the Python sides of the head-128 decoder families share (decoder.py: Qwen3, llama.py: Mistral / Llama, qwen2.py: Qwen2;
csrc/decoder128.hip is the library's side): one weight naming, one HF name mapping in both directions, one seeded generator and one
reader of a checkpoint's sentence-transformers files. A family states its LAYER_KEYS (the header's per-layer pointer order) and
HF_LAYER_NAMES and keeps thin functions of its own names over these.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Sequence

from ._stack import seeded_mat_vec

MAX_SEQ = 8192          # longest row the kernels take (attn_causal.hip)
HEAD_DIM = 128

MATRIX_KEYS = {"wq", "wk", "wv", "wo", "w_gate", "w_up", "w_down"}
# our name -> HF state-dict name (layer keys under "layers.{l}."), every key a family may have; HF's decoder classes agree on them
HF_NAMES = {"wq": "self_attn.q_proj.weight", "wk": "self_attn.k_proj.weight", "wv": "self_attn.v_proj.weight",
            "bq": "self_attn.q_proj.bias", "bk": "self_attn.k_proj.bias", "bv": "self_attn.v_proj.bias",
            "q_norm": "self_attn.q_norm.weight", "k_norm": "self_attn.k_norm.weight", "wo": "self_attn.o_proj.weight",
            "ln_in": "input_layernorm.weight", "ln_post": "post_attention_layernorm.weight",
            "w_gate": "mlp.gate_proj.weight", "w_up": "mlp.up_proj.weight", "w_down": "mlp.down_proj.weight"}


def layer_keys(qkv_bias: bool = False, qk_norm: bool = False) -> tuple:
    """The header's per-layer pointer order: the optional keys sit directly after wv."""
    return (("wq", "wk", "wv") + (("bq", "bk", "bv") if qkv_bias else ()) + (("q_norm", "k_norm") if qk_norm else ())
            + ("wo", "ln_in", "ln_post", "w_gate", "w_up", "w_down"))


def weight_order(keys: Sequence[str], layers: int) -> List[str]:
    """embed_tokens, final norm, then per layer `keys`."""
    names = ["embed_tokens", "norm"]
    for l in range(layers):
        names += [f"l{l}.{k}" for k in keys]
    return names


def hf_layer_names(keys: Sequence[str]) -> Dict[str, str]:
    """A family's HF_LAYER_NAMES: HF_NAMES of its LAYER_KEYS, in their order."""
    return {k: HF_NAMES[k] for k in keys}


def hf_state_dict(hf_names: Dict[str, str], weights: Dict[str, object], layers: int) -> Dict[str, object]:
    """Our weight names -> the HF model's (no "model." prefix)."""
    sd = {"embed_tokens.weight": weights["embed_tokens"], "norm.weight": weights["norm"]}
    for l in range(layers):
        for k, hf in hf_names.items():
            sd[f"layers.{l}.{hf}"] = weights[f"l{l}.{k}"]
    return sd


def from_hf_state_dict(hf_names: Dict[str, str], sd: Dict[str, object], layers: int) -> Dict[str, object]:
    """The HF model's names (no "model." prefix; what is not named, lm_head for one, is ignored) -> ours."""
    w = {"embed_tokens": sd["embed_tokens.weight"], "norm": sd["norm.weight"]}
    for l in range(layers):
        for k, hf in hf_names.items():
            w[f"l{l}.{k}"] = sd[f"layers.{l}.{hf}"]
    return w


def random_weights(keys: Sequence[str], shape, seed: int, std: float = 0.02, bias_std: float = 2.0) -> Dict[str, object]:
    """Seeded random weights of a shape (vocab, hidden, layers, q_heads, kv_heads, intermediate, ...) from ONE torch generator, drawn
    in weight_order(keys): the committed fixtures hold results of these draws. Matrices are drawn with std `std` and ROUNDED TO bf16
    (kept as float32 values): the released checkpoints are bf16, and a float32 reference on the same values measures the kernels'
    activation rounding alone. Norm weights are drawn around 1, not set to it; biases as one-row matrices of std `bias_std`."""
    vocab, H, L, nq, nkv, I = shape[:6]
    mat, vec = seeded_mat_vec(seed, std=std)
    q, kv = nq * HEAD_DIM, nkv * HEAD_DIM
    draw = {"wq": lambda: mat(q, H), "wk": lambda: mat(kv, H), "wv": lambda: mat(kv, H),
            "bq": lambda: mat(1, q, bias_std)[0], "bk": lambda: mat(1, kv, bias_std)[0], "bv": lambda: mat(1, kv, bias_std)[0],
            "q_norm": lambda: vec(HEAD_DIM), "k_norm": lambda: vec(HEAD_DIM), "wo": lambda: mat(H, q),
            "ln_in": lambda: vec(H), "ln_post": lambda: vec(H),
            "w_gate": lambda: mat(I, H), "w_up": lambda: mat(I, H), "w_down": lambda: mat(H, I)}
    w = {"embed_tokens": mat(vocab, H), "norm": vec(H)}
    for l in range(L):
        for k in keys:
            w[f"l{l}.{k}"] = draw[k]()
    return w


def read_st_config(model_dir: str, poolings: Dict[str, str], known_modules_only: bool, needs: str, implements: str):
    """sentence-transformers files of a decoder checkpoint: `modules.json` (Normalize module?), the Pooling module's config and
    `sentence_bert_config.json` (max_seq_length). Returns (pooling, max_seq_length | None, always_normalise). poolings: the one
    pooling mode the family takes -> its name here; known_modules_only: a module other than Transformer / Pooling / Normalize is
    refused (else ignored); needs / implements: how the two refusals end."""
    max_len, norm, pool_dir = None, False, "1_Pooling"
    mj = os.path.join(model_dir, "modules.json")
    if os.path.exists(mj):
        for m in json.load(open(mj)):
            kind = m.get("type", "")
            if kind.endswith("Normalize"):
                norm = True
            elif kind.endswith("Pooling"):
                pool_dir = m.get("path", pool_dir)
            elif known_modules_only and not kind.endswith("Transformer"):
                raise ValueError(f"{model_dir}: modules.json module {kind!r} is not supported (Transformer, Pooling, Normalize)")
    pj = os.path.join(model_dir, pool_dir, "config.json")
    if not os.path.exists(pj):
        raise ValueError(f"{model_dir}: no {pool_dir}/config.json ({needs})")
    pc = json.load(open(pj))
    modes = [k for k in ("cls_token", "mean_tokens", "max_tokens", "mean_sqrt_len_tokens", "weightedmean_tokens", "lasttoken")
             if pc.get("pooling_mode_" + k)]
    if len(modes) != 1 or modes[0] not in poolings:
        raise ValueError(f"{model_dir}: pooling modes {modes} ({implements})")
    sj = os.path.join(model_dir, "sentence_bert_config.json")
    if os.path.exists(sj):
        max_len = json.load(open(sj)).get("max_seq_length")
    return poolings[modes[0]], max_len, norm
