"""HipNomicBert -- Python handle of the HIP NomicBERT encoder (ak_nomic_*): nomic-ai/nomic-embed-text-v1, -v1.5, -v1-unsupervised and
the models tuned from them (Snowflake/snowflake-arctic-embed-m-long).

PyTorch-ROCm only HOLDS the weights in HBM (bf16 matrices, fp32 vectors) and hands raw device pointers to the C ABI; every
arithmetic step of the forward pass runs in hand-written HIP kernels (archi_amd/csrc/nomic.hip, attn_long.hip, gemm.hip).
Also here: the config.json reader of both config dialects (transformers' NomicBertConfig and the Hub checkpoints' original one)
that refuses what the kernels do not implement, the checkpoint loader of both tensor-name dialects and seeded random weights of
the named shapes.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional

import numpy as np

from ._lib import MBERT_MAX_LAYERS, AkNomicBertConfig
from ._stack import HipStack, read_safetensors_dir, seeded_mat_vec

MAX_SEQ = 8192          # longest row the kernels take (attn_long.hip)
HEAD_DIM = 64

# name -> (vocab, hidden, layers, heads, intermediate, type_vocab, max_position, ln_eps, rope theta, default pooling)
_BASE = (30528, 768, 12, 12, 3072, 2, 8192, 1e-12, 1000.0)
NOMIC_SHAPES = {
    "nomic-ai/nomic-embed-text-v1": _BASE + ("mean",),
    "nomic-ai/nomic-embed-text-v1.5": _BASE + ("mean",),
    "nomic-ai/nomic-embed-text-v1-unsupervised": _BASE + ("mean",),
    "Snowflake/snowflake-arctic-embed-m-long": _BASE + ("cls",),
    # small shapes of the test fixtures (tests/golden/make_nomic_fixtures.py); intermediate 192: 2 I = 384 is no multiple of 256,
    # so the gate / up matrix is padded at create
    "nomic-tiny-mean": (1000, 128, 3, 2, 192, 2, 8192, 1e-12, 1000.0, "mean"),
    "nomic-tiny-cls": (1000, 128, 3, 2, 192, 2, 8192, 1e-12, 1000.0, "cls"),
    "nomic-tiny-256": (1000, 256, 2, 4, 512, 2, 8192, 1e-12, 1000.0, "mean"),
    "nomic-tiny-long": (1000, 128, 2, 2, 192, 2, 8192, 1e-12, 1000.0, "mean"),
    # the base shape's width through a two-layer cut
    "nomic-base-cut2": (2000, 768, 2, 12, 3072, 2, 8192, 1e-12, 1000.0, "mean"),
}

GLOBAL_KEYS = ("word_emb", "type_emb", "emb_ln_g", "emb_ln_b")
LAYER_KEYS = ("wq", "wk", "wv", "wo", "ln1_g", "ln1_b", "w_gate", "w_up", "w_down", "ln2_g", "ln2_b")
MATRIX_KEYS = {"wq", "wk", "wv", "wo", "w_gate", "w_up", "w_down"}
# our name -> HF NomicBertModel state-dict name (layer keys under "layers.{l}.")
HF_GLOBAL_NAMES = {"word_emb": "embeddings.word_embeddings.weight", "type_emb": "embeddings.token_type_embeddings.weight",
                   "emb_ln_g": "embeddings.LayerNorm.weight", "emb_ln_b": "embeddings.LayerNorm.bias"}
HF_LAYER_NAMES = {"wq": "self_attn.q_proj.weight", "wk": "self_attn.k_proj.weight", "wv": "self_attn.v_proj.weight",
                  "wo": "self_attn.o_proj.weight", "ln1_g": "post_attention_layernorm.weight", "ln1_b": "post_attention_layernorm.bias",
                  "w_gate": "mlp.gate_proj.weight", "w_up": "mlp.up_proj.weight", "w_down": "mlp.down_proj.weight",
                  "ln2_g": "post_mlp_layernorm.weight", "ln2_b": "post_mlp_layernorm.bias"}
# the Hub checkpoints' original names (the renaming table transformers/conversion_mapping.py holds for nomic_bert, backwards):
# fc11 is UP, fc12 is GATE; attn.Wqkv is q | k | v along dim 0
ORIGINAL_GLOBAL_NAMES = dict(HF_GLOBAL_NAMES, emb_ln_g="emb_ln.weight", emb_ln_b="emb_ln.bias")
ORIGINAL_LAYER_NAMES = {"wo": "attn.out_proj.weight", "ln1_g": "norm1.weight", "ln1_b": "norm1.bias", "w_gate": "mlp.fc12.weight",
                        "w_up": "mlp.fc11.weight", "w_down": "mlp.fc2.weight", "ln2_g": "norm2.weight", "ln2_b": "norm2.bias"}
PREFIXES = ("model.", "nomic_bert.", "bert.")


def weight_names(layers: int) -> List[str]:
    """Every weight of a NomicBERT model in the header's order."""
    return list(GLOBAL_KEYS) + [f"l{l}.{k}" for l in range(layers) for k in LAYER_KEYS]


def hf_state_dict(weights: Dict[str, "np.ndarray"]) -> Dict[str, "np.ndarray"]:
    """Our weight names -> HF NomicBertModel's (no prefix)."""
    sd = {HF_GLOBAL_NAMES[k]: weights[k] for k in GLOBAL_KEYS}
    for name, arr in weights.items():
        if name[0] == "l" and "." in name:
            l, k = name[1:].split(".", 1)
            sd[f"layers.{l}.{HF_LAYER_NAMES[k]}"] = arr
    return sd


def original_state_dict(weights: Dict[str, "np.ndarray"]) -> Dict[str, "np.ndarray"]:
    """Our weight names -> the Hub checkpoints' original ones (fused attn.Wqkv, fc11 = up, fc12 = gate), no prefix."""
    sd = {ORIGINAL_GLOBAL_NAMES[k]: weights[k] for k in GLOBAL_KEYS}
    layers = 1 + max(int(n[1:].split(".", 1)[0]) for n in weights if n[0] == "l" and "." in n)
    for l in range(layers):
        p = f"encoder.layers.{l}."
        sd[p + "attn.Wqkv.weight"] = np.concatenate([np.asarray(weights[f"l{l}.{k}"]) for k in ("wq", "wk", "wv")], axis=0)
        for k, name in ORIGINAL_LAYER_NAMES.items():
            sd[p + name] = weights[f"l{l}.{k}"]
    return sd


def random_nomic_weights(shape, seed: int = 0, std: float = 0.02) -> Dict[str, "np.ndarray"]:
    """Seeded random weights of a NomicBERT shape (a NOMIC_SHAPES tuple or name). Matrices (and the token-type rows) are drawn with
    `std` and ROUNDED TO bf16 (kept as float32 values), as random_modernbert_weights does. LayerNorm weights are drawn around 1 and
    the biases around 0, neither set to it; the two token-type rows differ."""
    if isinstance(shape, str):
        shape = NOMIC_SHAPES[shape]
    vocab, H, L, heads, I, types = shape[:6]
    mat, vec = seeded_mat_vec(seed, std)
    _, bias = seeded_mat_vec(seed + 7919, std, vec_mean=0.0)
    w = {"word_emb": mat(vocab, H), "type_emb": mat(types, H), "emb_ln_g": vec(H), "emb_ln_b": bias(H)}
    for l in range(L):
        p = f"l{l}."
        w[p + "wq"], w[p + "wk"], w[p + "wv"], w[p + "wo"] = mat(H, H), mat(H, H), mat(H, H), mat(H, H)
        w[p + "ln1_g"], w[p + "ln1_b"] = vec(H), bias(H)
        w[p + "w_gate"], w[p + "w_up"], w[p + "w_down"] = mat(I, H), mat(I, H), mat(H, I)
        w[p + "ln2_g"], w[p + "ln2_b"] = vec(H), bias(H)
    return w


def _refuse(where: str, field: str, value, why: str):
    raise ValueError(f"{where}: {field} {value!r} is not supported ({why})")


def nomic_config_info(cfg: dict, where: str = "config.json", pooling: str = "mean"):
    """config.json of a NomicBERT checkpoint in either dialect -- transformers' NomicBertConfig (hidden_size, rope_parameters, ...)
    or the Hub checkpoints' original one (n_embd, rotary_emb_base, ...) -> (NOMIC_SHAPES-style tuple, dynamic). Everything the
    kernels do not implement is refused with a ValueError that names the field. dynamic: the checkpoint asks for dynamic-NTK RoPE,
    which equals the default RoPE on rows up to the trained length; the tuple's max_position is then that length (the row cap)."""
    if cfg.get("model_type") != "nomic_bert":
        raise ValueError(f"{where}: model_type {cfg.get('model_type')!r} is not nomic_bert")
    original = "n_embd" in cfg
    if cfg.get("moe_every_n_layers", 0) and int(cfg["moe_every_n_layers"]) > 0:
        _refuse(where, "moe_every_n_layers", cfg["moe_every_n_layers"], "mixture-of-experts layers: nomic-embed-text-v2-moe is out of scope")
    if cfg.get("num_experts", 0) and int(cfg["num_experts"]) > 1:
        _refuse(where, "num_experts", cfg["num_experts"], "mixture-of-experts layers: nomic-embed-text-v2-moe is out of scope")
    if cfg.get("prenorm", False):
        _refuse(where, "prenorm", cfg["prenorm"], "the HIP NomicBERT layer is post-norm")
    for flag in ("qkv_proj_bias", "mlp_fc1_bias", "mlp_fc2_bias"):
        if cfg.get(flag, False):
            _refuse(where, flag, cfg[flag], "the HIP NomicBERT kernels carry no bias in a Linear")
    if cfg.get("use_rms_norm", False):
        _refuse(where, "use_rms_norm", cfg["use_rms_norm"], "the HIP NomicBERT kernels implement LayerNorm")
    if float(cfg.get("rotary_emb_fraction", 1.0)) != 1.0:
        _refuse(where, "rotary_emb_fraction", cfg["rotary_emb_fraction"], "the whole head is rotated")
    if cfg.get("rotary_emb_interleaved", False):
        _refuse(where, "rotary_emb_interleaved", cfg["rotary_emb_interleaved"], "rotate_half RoPE only")
    if cfg.get("rotary_emb_scale_base") is not None:
        _refuse(where, "rotary_emb_scale_base", cfg["rotary_emb_scale_base"], "no xPos scaling")
    if original:
        H, heads, L = int(cfg["n_embd"]), int(cfg["n_head"]), int(cfg["n_layer"])
        I = int(cfg["n_inner"]) if cfg.get("n_inner") is not None else 4 * H
        eps = float(cfg.get("layer_norm_epsilon", 1e-12))
        act = cfg.get("activation_function", "swiglu")
        if act != "swiglu":
            _refuse(where, "activation_function", act, "the HIP NomicBERT kernels implement SwiGLU")
        theta = float(cfg.get("rotary_emb_base", 1000.0))
        factor = cfg.get("rotary_scaling_factor")
        dynamic = factor is not None and float(factor) != 1.0
        max_pos = int(cfg.get("n_positions", 2048))
        if dynamic:
            max_pos = int(cfg.get("max_trained_positions", max_pos))
    else:
        H, heads, L = int(cfg["hidden_size"]), int(cfg["num_attention_heads"]), int(cfg["num_hidden_layers"])
        I = int(cfg["intermediate_size"])
        eps = float(cfg.get("layer_norm_eps", 1e-12))
        act = cfg.get("hidden_act", "silu")
        if act != "silu":
            _refuse(where, "hidden_act", act, "the HIP NomicBERT kernels implement SwiGLU: silu")
        rp = cfg.get("rope_parameters") or {}
        rt = rp.get("rope_type", rp.get("type", "default")) or "default"
        if rt not in ("default", "dynamic"):
            _refuse(where, "rope_parameters.rope_type", rt, "default RoPE, or dynamic-NTK up to the trained length")
        if float(rp.get("partial_rotary_factor", 1.0)) != 1.0:
            _refuse(where, "rope_parameters.partial_rotary_factor", rp["partial_rotary_factor"], "the whole head is rotated")
        theta = float(rp.get("rope_theta", cfg.get("rope_theta", 1000.0)))
        dynamic = rt == "dynamic"
        max_pos = int(cfg.get("max_position_embeddings", 2048))
        hd = cfg.get("head_dim")
        if hd is not None and heads > 0 and int(hd) * heads != H:
            _refuse(where, "head_dim", hd, f"an explicit head_dim must equal hidden_size / num_attention_heads = {H / heads:g}")
    if heads <= 0 or H % heads or H // heads != HEAD_DIM:
        field = "n_embd / n_head" if original else "hidden_size / num_attention_heads"
        raise ValueError(f"{where}: head size {field} = {H / max(heads, 1):g} (the HIP NomicBERT kernels implement {HEAD_DIM})")
    if L > MBERT_MAX_LAYERS:
        raise ValueError(f"{where}: {'n_layer' if original else 'num_hidden_layers'} {L} (at most {MBERT_MAX_LAYERS})")
    if H % 128 or H > 1024 or I % 64:
        names = ("n_embd", "n_inner") if original else ("hidden_size", "intermediate_size")
        raise ValueError(f"{where}: {names[0]} {H} / {names[1]} {I} (the HIP GEMM takes {names[0]} % 128 == 0, <= 1024, and "
                         f"{names[1]} % 64 == 0)")
    if not theta > 0 or not eps > 0 or max_pos <= 0:
        raise ValueError(f"{where}: rope theta {theta}, layer norm eps {eps} and the position count {max_pos} must be positive")
    return (int(cfg["vocab_size"]), H, L, heads, I, int(cfg.get("type_vocab_size", 2)), max_pos, eps, theta, pooling), dynamic


def nomic_config_shape(cfg: dict, where: str = "config.json", pooling: str = "mean"):
    """nomic_config_info's shape tuple alone."""
    return nomic_config_info(cfg, where, pooling)[0]


def shape_hf_config(shape, **extra):
    """A NOMIC_SHAPES tuple -> transformers.NomicBertConfig (the tests' float32 reference)."""
    from transformers import NomicBertConfig
    if isinstance(shape, str):
        shape = NOMIC_SHAPES[shape]
    vocab, H, L, heads, I, types, max_pos, eps, theta, _ = shape
    kw = dict(vocab_size=vocab, hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, intermediate_size=I, hidden_act="silu",
              max_position_embeddings=max_pos, type_vocab_size=types, layer_norm_eps=eps, pad_token_id=0,
              rope_parameters={"rope_type": "default", "rope_theta": theta})
    kw.update(extra)
    return NomicBertConfig(**kw)


def shape_original_config(shape, **extra) -> dict:
    """A NOMIC_SHAPES tuple -> config.json in the Hub checkpoints' original dialect."""
    if isinstance(shape, str):
        shape = NOMIC_SHAPES[shape]
    vocab, H, L, heads, I, types, max_pos, eps, theta, _ = shape
    cfg = dict(model_type="nomic_bert", architectures=["NomicBertModel"], vocab_size=vocab, n_embd=H, n_layer=L, n_head=heads, n_inner=I,
               type_vocab_size=types, n_positions=max_pos, max_trained_positions=max_pos, layer_norm_epsilon=eps, rotary_emb_base=theta,
               rotary_emb_fraction=1.0, rotary_emb_interleaved=False, rotary_emb_scale_base=None, rotary_scaling_factor=None,
               activation_function="swiglu", prenorm=False, qkv_proj_bias=False, mlp_fc1_bias=False, mlp_fc2_bias=False, use_rms_norm=False)
    cfg.update(extra)
    return cfg


def load_nomic_weights(model_dir: str):
    """Local NomicBERT checkpoint directory (config.json + model.safetensors or sharded model-*.safetensors) in either tensor-name
    dialect -> (shape, weights in our names). A "model." / "nomic_bert." / "bert." prefix on the tensor names is stripped; heads of a
    masked-LM checkpoint are ignored. No network."""
    cfg = json.load(open(os.path.join(model_dir, "config.json")))
    shape = nomic_config_shape(cfg, os.path.join(model_dir, "config.json"))
    sd = {}
    for k, v in read_safetensors_dir(model_dir).items():
        for p in PREFIXES:
            if k.startswith(p):
                k = k[len(p):]
                break
        sd[k] = v
    L = shape[2]
    original = "emb_ln.weight" in sd
    w = {k: sd[(ORIGINAL_GLOBAL_NAMES if original else HF_GLOBAL_NAMES)[k]] for k in GLOBAL_KEYS}
    for l in range(L):
        if original:
            p = f"encoder.layers.{l}."
            w[f"l{l}.wq"], w[f"l{l}.wk"], w[f"l{l}.wv"] = (t.contiguous() for t in sd[p + "attn.Wqkv.weight"].chunk(3, dim=0))
            for k, name in ORIGINAL_LAYER_NAMES.items():
                w[f"l{l}.{k}"] = sd[p + name]
        else:
            for k, name in HF_LAYER_NAMES.items():
                w[f"l{l}.{k}"] = sd[f"layers.{l}.{name}"]
    return shape, w


class HipNomicBert(HipStack):
    family, prefix, embed_key, matrix_keys, pooling_noun = "nomic", "nomic", "word_emb", MATRIX_KEYS, "NomicBERT models"

    def __init__(self, shape, weights: Dict[str, "np.ndarray"], device: Optional[int] = None):
        """shape: a NOMIC_SHAPES tuple or name; weights: our names (weight_names), numpy arrays or torch tensors."""
        if isinstance(shape, str):
            shape = NOMIC_SHAPES[shape]
        vocab, H, L, heads, I, types, max_pos, eps, theta, pooling = shape
        if L > MBERT_MAX_LAYERS:
            raise ValueError(f"NomicBERT shape: {L} layers (at most {MBERT_MAX_LAYERS})")
        self.shape = tuple(shape)
        self.hidden, self.layers, self.vocab, self.pooling, self.out_dim = H, L, vocab, pooling, H
        self.max_seq = min(int(max_pos), MAX_SEQ)
        names = weight_names(L)
        self._upload(weights, names, device)
        self._create(AkNomicBertConfig(vocab, H, L, heads, I, types, max_pos, eps, theta), names)
