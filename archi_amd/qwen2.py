"""HipQwen2 -- Python handle of the HIP Qwen2 decoder (ak_qwen2_*): the instruction-aware embedders built on Qwen2 / Qwen2.5 decoders
(Alibaba-NLP/gte-Qwen2-1.5B-instruct and -7B-instruct, gte-Qwen1.5-7B-instruct, infly/inf-retriever-v1 and -1.5b), the kind the
reference's retrievers single out (src/data_manager/vectorstore/retrievers/utils.py:7-19) and loads by name through HuggingFaceEmbeddings.

PyTorch-ROCm only HOLDS the weights in HBM (bf16 matrices, fp32 vectors and biases) and hands raw device pointers to the C ABI; every
arithmetic step of the forward pass runs in hand-written HIP kernels (archi_amd/csrc/decoder128.hip, the head-128 decoder stack behind
qwen2.hip's ABI; attn_causal.hip, gemm.hip). Against the Mistral / Llama path (llama.py): a bias on the q, k and v projections, up to
8 query heads per kv head (attn_causal.hip's split mapping from 5 on), no sliding window. Also here: the config check
(qwen2_config_shape), the checkpoint loader and seeded random weights of the named shapes. The handle's body, the sentence-transformers
files, the attention / pooling modes and the rotary frequencies are llama.py's.

Attention is causal unless the checkpoint's config.json says `is_causal: false` or the caller states
model_kwargs={"attention": "bidirectional"} (which always wins); pooling is last-token or mean, resolved as llama.resolve_mode does.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, NamedTuple, Optional

import numpy as np

from . import _decoder128 as _d128
from ._decoder128 import HEAD_DIM, MATRIX_KEYS, MAX_SEQ, hf_layer_names, layer_keys  # noqa: F401 (re-exported)
from ._lib import AkQwen2Config
from ._stack import read_safetensors_dir
from .llama import HipLlama, Llama3Scaling, _rope, read_llama_st_config, resolve_mode, rope_inv_freq  # noqa: F401 (re-exported)

MAX_GROUP = 8           # most query heads per kv head (attn_causal.hip: one workgroup up to 4, two workgroups for 5 .. 8)


class Qwen2Shape(NamedTuple):
    """config.json numbers of a Qwen2 checkpoint as the handle takes them (LlamaShape without the window)."""
    vocab: int
    hidden: int
    layers: int
    q_heads: int
    kv_heads: int
    intermediate: int
    max_position: int
    rope_theta: float
    rms_eps: float
    pooling: str = "last"
    scaling: Optional[Llama3Scaling] = None
    attention: str = "causal"      # "bidirectional": every key below the row's length


QWEN2_SHAPES = {
    "Alibaba-NLP/gte-Qwen2-1.5B-instruct": Qwen2Shape(151646, 1536, 28, 12, 2, 8960, 131072, 1e6, 1e-6),
    "Alibaba-NLP/gte-Qwen2-7B-instruct": Qwen2Shape(151646, 3584, 28, 28, 4, 18944, 131072, 1e6, 1e-6),
    # small shapes of the test fixtures (tests/golden/make_qwen2_fixtures.py): 5 to 8 query heads per kv head (the split attention
    # mapping: 3 + 2, 3 + 3, 4 + 3, 4 + 4) and 2 (the unsplit kernel, with biases), two kv heads each
    "q2-tiny-g5": Qwen2Shape(1000, 256, 2, 10, 2, 512, 8192, 1e6, 1e-6),
    "q2-tiny-g6": Qwen2Shape(1000, 256, 2, 12, 2, 512, 8192, 1e6, 1e-6),
    "q2-tiny-g7": Qwen2Shape(1000, 256, 2, 14, 2, 512, 8192, 1e6, 1e-6),
    "q2-tiny-g8": Qwen2Shape(1000, 256, 3, 16, 2, 512, 8192, 1e6, 1e-6),
    "q2-tiny-g2": Qwen2Shape(1000, 256, 2, 4, 2, 512, 8192, 1e6, 1e-6),
    # the 7B and 1.5B layer shapes cut to 2 layers and 2000 vocabulary rows: the GEMM widths and group sizes of the released models
    "gte-qwen2-7b-2l": Qwen2Shape(2000, 3584, 2, 28, 4, 18944, 131072, 1e6, 1e-6),
    "gte-qwen2-1.5b-2l": Qwen2Shape(2000, 1536, 2, 12, 2, 8960, 131072, 1e6, 1e-6),
}

LAYER_KEYS = layer_keys(qkv_bias=True)     # wq wk wv bq bk bv wo ln_in ln_post w_gate w_up w_down
HF_LAYER_NAMES = hf_layer_names(LAYER_KEYS)      # our name -> HF Qwen2Model state-dict name (layer keys under "layers.{l}.")


def weight_order(layers: int) -> List[str]:
    """The header's weight order: embed_tokens, final norm, then per layer LAYER_KEYS (2 + 12 * layers names)."""
    return _d128.weight_order(LAYER_KEYS, layers)


def hf_state_dict(weights: Dict[str, "np.ndarray"], layers: int) -> Dict[str, "np.ndarray"]:
    """Our weight names -> HF Qwen2Model's (no "model." prefix)."""
    return _d128.hf_state_dict(HF_LAYER_NAMES, weights, layers)


def random_qwen2_weights(shape, seed: int = 0, std: float = 0.02, bias_std: float = 2.0) -> Dict[str, "np.ndarray"]:
    """Seeded random weights of a shape (a Qwen2Shape or a QWEN2_SHAPES name), as _decoder128.random_weights draws them; the q / k / v
    biases are drawn at their own `bias_std` (released Qwen2 biases are large, the k biases above all) and ROUNDED TO bf16 like the
    matrices (kept as float32 values): the released checkpoints are bf16."""
    return _d128.random_weights(LAYER_KEYS, QWEN2_SHAPES[shape] if isinstance(shape, str) else shape, seed, std, bias_std)


def qwen2_config_shape(cfg: dict, where: str = "config.json") -> Qwen2Shape:
    """config.json of a Qwen2 checkpoint -> Qwen2Shape; everything the kernels do not implement is refused with a ValueError that names
    the field, before any GPU work. `sliding_window` is ignored unless `use_sliding_window` is true. A top-level `is_causal: false` (the
    gte-Qwen2 checkpoints run a model class without the causal mask) makes the shape's attention "bidirectional"."""
    mt = cfg.get("model_type")
    if mt != "qwen2":
        raise ValueError(f"{where}: model_type {mt!r} is not qwen2")
    if cfg.get("use_sliding_window", False):
        raise ValueError(f"{where}: use_sliding_window is not supported (HF slides only the layers from max_window_layers on: a mixed stack)")
    kinds = set(cfg.get("layer_types") or [])
    if kinds - {"full_attention"}:
        raise ValueError(f"{where}: layer_types {sorted(kinds)} (full_attention in every layer only)")
    if cfg.get("hidden_act", "silu") != "silu":
        raise ValueError(f"{where}: hidden_act {cfg.get('hidden_act')!r} (the HIP decoder implements SiLU / SwiGLU)")
    H, nq, I = cfg["hidden_size"], cfg["num_attention_heads"], cfg["intermediate_size"]
    nkv = cfg.get("num_key_value_heads") or nq
    hd = cfg.get("head_dim") or H // nq
    if hd != HEAD_DIM:
        raise ValueError(f"{where}: head_dim {hd} (the HIP decoder implements 128)")
    if nq % nkv or nq // nkv > MAX_GROUP:
        raise ValueError(f"{where}: num_attention_heads {nq} / num_key_value_heads {nkv} (a whole ratio of at most {MAX_GROUP} query heads per kv head)")
    if H % 128:
        raise ValueError(f"{where}: hidden_size {H} is not a multiple of 128")
    if I % 64:
        raise ValueError(f"{where}: intermediate_size {I} is not a multiple of 64")
    try:
        theta, scaling = _rope(cfg)
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    causal = cfg.get("is_causal", True)
    if causal not in (True, False):
        raise ValueError(f"{where}: is_causal {causal!r} (true or false)")
    return Qwen2Shape(cfg["vocab_size"], H, cfg["num_hidden_layers"], nq, nkv, I, cfg.get("max_position_embeddings", 32768), theta,
                      float(cfg.get("rms_norm_eps", 1e-6)), "last", scaling, "causal" if causal else "bidirectional")


def load_qwen2_weights(model_dir: str):
    """Local Qwen2 checkpoint directory (config.json + model.safetensors or sharded model-*.safetensors) -> (shape, weights in the
    header's names). A "model." prefix on the tensor names is stripped; lm_head is ignored. No network."""
    cj = os.path.join(model_dir, "config.json")
    shape = qwen2_config_shape(json.load(open(cj)), cj)
    return shape, _d128.from_hf_state_dict(HF_LAYER_NAMES, read_safetensors_dir(model_dir), shape.layers)


def apply_mode(shape: Qwen2Shape, model_kwargs: dict) -> Qwen2Shape:
    """The shape with model_kwargs["attention"] taken in (llama.resolve_mode has checked it); without the keyword the shape's own."""
    return Qwen2Shape(*shape)._replace(attention=model_kwargs.get("attention", Qwen2Shape(*shape).attention))


class HipQwen2(HipLlama):
    """HipLlama (its __init__: shape: a Qwen2Shape or a plain tuple in its order) behind ak_qwen2_*, on Qwen2's shape and weight names."""
    family, prefix, pooling_noun = "qwen2", "qwen2", "Qwen2 embedders"
    shape_type, layer_keys = Qwen2Shape, LAYER_KEYS

    def _config(self, shape):
        return AkQwen2Config(shape.vocab, shape.hidden, shape.layers, shape.q_heads, shape.kv_heads, HEAD_DIM, shape.intermediate,
                             shape.max_position, shape.rms_eps, shape.rope_theta, int(self.bidirectional))
