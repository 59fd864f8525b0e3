"""HipQwen2 -- Python handle of the HIP Qwen2 decoder (ak_qwen2_*): the instruction-aware embedders built on Qwen2 / Qwen2.5 decoders
(Alibaba-NLP/gte-Qwen2-1.5B-instruct and -7B-instruct, gte-Qwen1.5-7B-instruct, infly/inf-retriever-v1 and -1.5b), the kind the
reference's retrievers single out (src/data_manager/vectorstore/retrievers/utils.py:7-19) and loads by name through HuggingFaceEmbeddings.

PyTorch-ROCm only HOLDS the weights in HBM (bf16 matrices, fp32 vectors and biases) and hands raw device pointers to the C ABI; every
arithmetic step of the forward pass runs in hand-written HIP kernels (archi_amd/csrc/qwen2.hip on llama.hip's layer loop, attn_causal.hip,
decoder.hip, gemm.hip). Against the Mistral / Llama path (llama.py): a bias on the q, k and v projections, up to 8 query heads per kv
head (attn_causal.hip's split mapping from 5 on), no sliding window. Also here: the config check (qwen2_config_shape), the checkpoint
loader and seeded random weights of the named shapes. The sentence-transformers files, the attention / pooling modes and the rotary
frequencies are llama.py's.

Attention is causal unless the checkpoint's config.json says `is_causal: false` or the caller states
model_kwargs={"attention": "bidirectional"} (which always wins); pooling is last-token or mean, resolved as llama.resolve_mode does.
"""
from __future__ import annotations

import ctypes
import json
import os
from typing import Dict, List, NamedTuple, Optional

import numpy as np

from ._lib import AkQwen2Config, check
from ._stack import HipStack, read_safetensors_dir, seeded_mat_vec
from .llama import HEAD_DIM, MAX_SEQ, Llama3Scaling, _rope, read_llama_st_config, resolve_mode, rope_inv_freq  # noqa: F401 (re-exported)

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

LAYER_KEYS = ("wq", "wk", "wv", "bq", "bk", "bv", "wo", "ln_in", "ln_post", "w_gate", "w_up", "w_down")
MATRIX_KEYS = {"wq", "wk", "wv", "wo", "w_gate", "w_up", "w_down"}
# our name -> HF Qwen2Model state-dict name (layer keys under "layers.{l}.")
HF_LAYER_NAMES = {"wq": "self_attn.q_proj.weight", "wk": "self_attn.k_proj.weight", "wv": "self_attn.v_proj.weight",
                  "bq": "self_attn.q_proj.bias", "bk": "self_attn.k_proj.bias", "bv": "self_attn.v_proj.bias",
                  "wo": "self_attn.o_proj.weight", "ln_in": "input_layernorm.weight", "ln_post": "post_attention_layernorm.weight",
                  "w_gate": "mlp.gate_proj.weight", "w_up": "mlp.up_proj.weight", "w_down": "mlp.down_proj.weight"}


def weight_order(layers: int) -> List[str]:
    """The header's weight order: embed_tokens, final norm, then per layer wq wk wv bq bk bv wo ln_in ln_post w_gate w_up w_down
    (2 + 12 * layers names)."""
    names = ["embed_tokens", "norm"]
    for l in range(layers):
        names += [f"l{l}.{k}" for k in LAYER_KEYS]
    return names


def hf_state_dict(weights: Dict[str, "np.ndarray"], layers: int) -> Dict[str, "np.ndarray"]:
    """Our weight names -> HF Qwen2Model's (no "model." prefix)."""
    sd = {"embed_tokens.weight": weights["embed_tokens"], "norm.weight": weights["norm"]}
    for l in range(layers):
        for k, hf in HF_LAYER_NAMES.items():
            sd[f"layers.{l}.{hf}"] = weights[f"l{l}.{k}"]
    return sd


def random_qwen2_weights(shape, seed: int = 0, std: float = 0.02, bias_std: float = 2.0) -> Dict[str, "np.ndarray"]:
    """Seeded random weights of a shape (a Qwen2Shape or a QWEN2_SHAPES name), as llama.random_llama_weights draws them; the q / k / v
    biases are drawn at their own `bias_std` (released Qwen2 biases are large, the k biases above all) and ROUNDED TO bf16 like the
    matrices (kept as float32 values): the released checkpoints are bf16."""
    if isinstance(shape, str):
        shape = QWEN2_SHAPES[shape]
    vocab, H, L, nq, nkv, I = shape[:6]
    mat, vec = seeded_mat_vec(seed, std=std)
    w = {"embed_tokens": mat(vocab, H), "norm": vec(H)}
    for l in range(L):
        p = f"l{l}."
        w[p + "wq"], w[p + "wk"], w[p + "wv"] = mat(nq * HEAD_DIM, H), mat(nkv * HEAD_DIM, H), mat(nkv * HEAD_DIM, H)
        w[p + "bq"], w[p + "bk"], w[p + "bv"] = (mat(1, n * HEAD_DIM, bias_std)[0] for n in (nq, nkv, nkv))
        w[p + "wo"] = mat(H, nq * HEAD_DIM)
        w[p + "ln_in"], w[p + "ln_post"] = vec(H), vec(H)
        w[p + "w_gate"], w[p + "w_up"], w[p + "w_down"] = mat(I, H), mat(I, H), mat(H, I)
    return w


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
    sd = read_safetensors_dir(model_dir)
    w = {"embed_tokens": sd["embed_tokens.weight"], "norm": sd["norm.weight"]}
    for l in range(shape.layers):
        for k, hf in HF_LAYER_NAMES.items():
            w[f"l{l}.{k}"] = sd[f"layers.{l}.{hf}"]
    return shape, w


def apply_mode(shape: Qwen2Shape, model_kwargs: dict) -> Qwen2Shape:
    """The shape with model_kwargs["attention"] taken in (llama.resolve_mode has checked it); without the keyword the shape's own."""
    return Qwen2Shape(*shape)._replace(attention=model_kwargs.get("attention", Qwen2Shape(*shape).attention))


class HipQwen2(HipStack):
    family, prefix, embed_key, matrix_keys = "qwen2", "qwen2", "embed_tokens", MATRIX_KEYS
    poolings, pooling_noun = ("last", "mean"), "Qwen2 embedders"

    def __init__(self, shape, weights: Dict[str, "np.ndarray"], device: Optional[int] = None):
        """shape: a Qwen2Shape (or a plain tuple in its order); weights: the header's names (weight_order), numpy arrays or torch
        tensors. Under llama3 scaling the rotary table is rebuilt from llama.rope_inv_freq(shape), HF's own float32 frequencies."""
        shape = Qwen2Shape(*shape)
        self.shape = shape
        self.hidden, self.layers, self.vocab, self.out_dim = shape.hidden, shape.layers, shape.vocab, shape.hidden
        self.max_seq = min(int(shape.max_position), MAX_SEQ)
        if shape.attention not in ("causal", "bidirectional"):
            raise ValueError(f"attention {shape.attention!r} (\"causal\" or \"bidirectional\")")
        self.bidirectional = shape.attention == "bidirectional"
        self.pooling = shape.pooling            # what forward() pools with when it is not told
        self._upload(weights, weight_order(shape.layers), device)
        self._create(AkQwen2Config(shape.vocab, shape.hidden, shape.layers, shape.q_heads, shape.kv_heads, HEAD_DIM, shape.intermediate,
                                   shape.max_position, shape.rms_eps, shape.rope_theta, int(self.bidirectional)),
                     weight_order(shape.layers))
        if shape.scaling is not None:           # default RoPE: the table ak_qwen2_create built from theta
            inv = np.ascontiguousarray(rope_inv_freq(shape), np.float32)
            check(self._lib.ak_qwen2_set_rope_inv_freq(self._h, ctypes.c_void_p(inv.ctypes.data)), "ak_qwen2_set_rope_inv_freq")

    def forward(self, ids, lens, pooling: Optional[str] = None, normalise: bool = True, S: Optional[int] = None):
        """ids [B, W] (row i holds lens[i] ids), lens [B] -> [B, hidden] float32 CUDA tensor (one tile, S = W rounded up to 32)."""
        return super().forward(ids, lens, pooling=pooling, normalise=normalise, S=S)
