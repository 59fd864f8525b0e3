"""HipLlama -- Python handle of the HIP Mistral / Llama decoder (ak_llama_*): the instruction-aware embedders built on plain
Mistral-7B / Llama-3.1-8B decoders (intfloat/e5-mistral-7b-instruct, Salesforce/SFR-Embedding-Mistral, Linq-AI-Research/Linq-Embed-Mistral),
the other group the reference's retrievers single out beside Qwen3-Embedding (src/data_manager/vectorstore/retrievers/utils.py:7-19).

PyTorch-ROCm only HOLDS the weights in HBM (bf16 matrices, fp32 vectors) and hands raw device pointers to the C ABI; every arithmetic
step of the forward pass runs in hand-written HIP kernels (archi_amd/csrc/decoder128.hip, the head-128 decoder stack behind llama.hip's
ABI; attn_causal.hip, gemm.hip). Against the Qwen3 decoder (decoder.py): no per-head q / k norm, Mistral's sliding window inside the
causal mask, Llama-3's frequency-dependent RoPE scaling. Also here: the config check (llama_config_shape), the checkpoint loader, seeded
random weights of the named shapes and the sentence-transformers configuration of such a checkpoint (the last three on _decoder128.py,
which the three families share). HipQwen2 (qwen2.py) is this handle with its own shape, keys and config struct.

Attention is causal with the config's window unless the caller states model_kwargs={"attention": "bidirectional"} (an embedder trained
without the causal mask: every key below the row's length, mean pooling by default); pooling is last-token or mean (the mean of the
final norm per token).
"""
from __future__ import annotations

import ctypes
import json
import math
import os
from typing import Dict, List, NamedTuple, Optional

import numpy as np

from . import _decoder128 as _d128
from ._decoder128 import HEAD_DIM, MATRIX_KEYS, MAX_SEQ, hf_layer_names, layer_keys  # noqa: F401 (re-exported)
from ._lib import AkLlamaConfig, check
from ._stack import HipStack, read_safetensors_dir


class Llama3Scaling(NamedTuple):
    """rope_type llama3: factor, low_freq_factor, high_freq_factor, original_max_position_embeddings."""
    factor: float
    low: float
    high: float
    original: int


class LlamaShape(NamedTuple):
    """config.json numbers of a Mistral / Llama checkpoint as the handle takes them. window 0: no sliding window."""
    vocab: int
    hidden: int
    layers: int
    q_heads: int
    kv_heads: int
    intermediate: int
    max_position: int
    rope_theta: float
    rms_eps: float
    window: int = 0
    pooling: str = "last"
    scaling: Optional[Llama3Scaling] = None
    attention: str = "causal"      # "bidirectional": every key below the row's length; the window is then ignored


_MISTRAL_7B = LlamaShape(32000, 4096, 32, 32, 8, 14336, 32768, 1e4, 1e-5, 4096, "last")
LLAMA_SHAPES = {
    # Mistral-7B-v0.1 numbers: every embedder below is a fine-tune of it
    "intfloat/e5-mistral-7b-instruct": _MISTRAL_7B,
    "Salesforce/SFR-Embedding-Mistral": _MISTRAL_7B,
    "Linq-AI-Research/Linq-Embed-Mistral": _MISTRAL_7B,
    "llama-3.1-8b": LlamaShape(128256, 4096, 32, 32, 8, 14336, 131072, 5e5, 1e-5, 0, "last", Llama3Scaling(8.0, 1.0, 4.0, 8192)),
    # small shapes of the test fixtures (tests/golden/make_llama_fixtures.py): GQA ratios 1 - 4 at head dim 128, a window, llama3 scaling
    "ll-tiny-g1": LlamaShape(1000, 256, 2, 2, 2, 512, 8192, 1e4, 1e-5),
    "ll-tiny-g2": LlamaShape(1000, 256, 3, 4, 2, 768, 8192, 1e4, 1e-5),
    "ll-tiny-g3": LlamaShape(1000, 256, 2, 3, 1, 512, 8192, 1e6, 1e-5),
    "ll-tiny-g4": LlamaShape(1000, 256, 4, 8, 2, 512, 8192, 1e4, 1e-5),
    "ll-win": LlamaShape(1000, 256, 2, 4, 2, 512, 8192, 1e4, 1e-5, 48),
    "ll-long": LlamaShape(1000, 256, 2, 4, 2, 512, 8192, 1e4, 1e-5, 4096),
    "ll-l3": LlamaShape(1000, 256, 2, 4, 2, 512, 8192, 5e5, 1e-5, 0, "last", Llama3Scaling(8.0, 1.0, 4.0, 64)),
    # the Mistral-7B layer shape cut to 2 layers and 2000 vocabulary rows: every GEMM on the wide tile
    "mistral-7b-2l": LlamaShape(2000, 4096, 2, 32, 8, 14336, 32768, 1e4, 1e-5, 4096),
}

LAYER_KEYS = layer_keys()                  # wq wk wv wo ln_in ln_post w_gate w_up w_down
HF_LAYER_NAMES = hf_layer_names(LAYER_KEYS)      # our name -> HF MistralModel / LlamaModel state-dict name (layer keys under "layers.{l}.")


def weight_order(layers: int) -> List[str]:
    """The header's weight order: embed_tokens, final norm, then per layer LAYER_KEYS (2 + 9 * layers names)."""
    return _d128.weight_order(LAYER_KEYS, layers)


def hf_state_dict(weights: Dict[str, "np.ndarray"], layers: int) -> Dict[str, "np.ndarray"]:
    """Our weight names -> HF MistralModel / LlamaModel's (no "model." prefix)."""
    return _d128.hf_state_dict(HF_LAYER_NAMES, weights, layers)


def random_llama_weights(shape, seed: int = 0, std: float = 0.02) -> Dict[str, "np.ndarray"]:
    """Seeded random weights of a shape (a LlamaShape or a LLAMA_SHAPES name), as _decoder128.random_weights draws them."""
    return _d128.random_weights(LAYER_KEYS, LLAMA_SHAPES[shape] if isinstance(shape, str) else shape, seed, std)


def _rope(cfg: dict):
    """(theta, Llama3Scaling | None) from rope_parameters (transformers 5) or rope_theta + rope_scaling (transformers 4), as
    decoder._rope_theta reads them; rope types other than default / llama3 are refused."""
    rp = cfg.get("rope_parameters") or {}
    rs = cfg.get("rope_scaling") or {}
    scaling = None
    for what, field in ((rs, "rope_scaling"), (rp, "rope_parameters")):
        kind = what.get("rope_type", what.get("type", "default")) or "default"
        if kind == "llama3":
            try:
                scaling = Llama3Scaling(float(what["factor"]), float(what["low_freq_factor"]), float(what["high_freq_factor"]),
                                        int(what["original_max_position_embeddings"]))
            except KeyError as e:
                raise ValueError(f"{field}: rope type 'llama3' needs {e.args[0]}") from None
            if scaling.high <= scaling.low or scaling.factor <= 0 or scaling.low <= 0 or scaling.original <= 0:
                raise ValueError(f"{field}: llama3 scaling needs factor > 0, 0 < low_freq_factor < high_freq_factor, original length > 0")
        elif kind != "default":
            raise ValueError(f"{field}: rope type {kind!r} is not supported (default and llama3 only)")
    theta = cfg.get("rope_theta", rp.get("rope_theta"))
    if theta is None:
        raise ValueError("config.json has no rope_theta")
    return float(theta), scaling


def llama_config_shape(cfg: dict, where: str = "config.json") -> LlamaShape:
    """config.json of a Mistral / Llama checkpoint -> LlamaShape; everything the kernels do not implement is refused with a ValueError
    that names the field, before any GPU work. `sliding_window: null` and Llama both mean no window."""
    mt = cfg.get("model_type")
    if mt not in ("mistral", "llama"):
        raise ValueError(f"{where}: model_type {mt!r} is not mistral or llama")
    if cfg.get("attention_bias", False):
        raise ValueError(f"{where}: attention_bias is not supported")
    if cfg.get("mlp_bias", False):
        raise ValueError(f"{where}: mlp_bias is not supported")
    if cfg.get("hidden_act", "silu") != "silu":
        raise ValueError(f"{where}: hidden_act {cfg.get('hidden_act')!r} (the HIP decoder implements SiLU / SwiGLU)")
    H, nq, I = cfg["hidden_size"], cfg["num_attention_heads"], cfg["intermediate_size"]
    nkv = cfg.get("num_key_value_heads") or nq
    hd = cfg.get("head_dim") or H // nq
    if hd != HEAD_DIM:
        raise ValueError(f"{where}: head_dim {hd} (the HIP decoder implements 128)")
    if nq % nkv or nq // nkv > 4:
        raise ValueError(f"{where}: num_attention_heads {nq} / num_key_value_heads {nkv} (a whole ratio of at most 4 query heads per kv head)")
    if H % 128:
        raise ValueError(f"{where}: hidden_size {H} is not a multiple of 128")
    if I % 64:
        raise ValueError(f"{where}: intermediate_size {I} is not a multiple of 64")
    try:
        theta, scaling = _rope(cfg)
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    window = cfg.get("sliding_window", 4096) if mt == "mistral" else None      # an absent key: MistralConfig's own default
    if window is not None and int(window) < 1:
        raise ValueError(f"{where}: sliding_window {window} must be >= 1 when set")
    kinds = set(cfg.get("layer_types") or [])
    if len(kinds) > 1:
        raise ValueError(f"{where}: layer_types mixes {sorted(kinds)} (one attention kind for every layer only)")
    if kinds == {"full_attention"}:
        window = None
    elif kinds and kinds != {"sliding_attention"}:
        raise ValueError(f"{where}: layer_types {sorted(kinds)} is not supported")
    return LlamaShape(cfg["vocab_size"], H, cfg["num_hidden_layers"], nq, nkv, I, cfg.get("max_position_embeddings", 32768), theta,
                      float(cfg.get("rms_norm_eps", 1e-6)), int(window or 0), "last", scaling)


def rope_inv_freq(shape) -> "np.ndarray":
    """The 64 float32 inverse frequencies of the model's rotary embedding, by the torch expressions HF evaluates: the default
    initialisation, 1 / theta^(2 i / 128), and -- shape.scaling set -- modeling_rope_utils' llama3 rule on top of it (wavelengths above
    original / low are divided by factor, those between original / high and original / low are interpolated). Taken from torch rather
    than from the library's host routine for the reason gemma.rope_inv_freq states: the same expression in the same library gives HF's
    buffer to the bit."""
    import torch
    if isinstance(shape, str):
        shape = LLAMA_SHAPES[shape]
    inv_freq = 1.0 / (float(shape.rope_theta) ** (torch.arange(0, HEAD_DIM, 2, dtype=torch.int64).to(dtype=torch.float) / HEAD_DIM))
    if shape.scaling is not None:
        factor, low_freq_factor, high_freq_factor, old_context_len = shape.scaling
        low_freq_wavelen = old_context_len / low_freq_factor
        high_freq_wavelen = old_context_len / high_freq_factor
        wavelen = 2 * math.pi / inv_freq
        inv_freq_llama = torch.where(wavelen > low_freq_wavelen, inv_freq / factor, inv_freq)
        smooth_factor = (old_context_len / wavelen - low_freq_factor) / (high_freq_factor - low_freq_factor)
        smoothed_inv_freq = (1 - smooth_factor) * inv_freq_llama / factor + smooth_factor * inv_freq_llama
        is_medium_freq = ~(wavelen < high_freq_wavelen) * ~(wavelen > low_freq_wavelen)
        inv_freq = torch.where(is_medium_freq, smoothed_inv_freq, inv_freq_llama)
    return inv_freq.numpy().astype(np.float32)


def load_llama_weights(model_dir: str):
    """Local Mistral / Llama checkpoint directory (config.json + model.safetensors or sharded model-*.safetensors) -> (shape, weights
    in the header's names). A "model." prefix on the tensor names is stripped; lm_head is ignored. No network."""
    cj = os.path.join(model_dir, "config.json")
    shape = llama_config_shape(json.load(open(cj)), cj)
    return shape, _d128.from_hf_state_dict(HF_LAYER_NAMES, read_safetensors_dir(model_dir), shape.layers)


def read_llama_st_config(model_dir: str):
    """sentence-transformers files of a Mistral / Llama checkpoint: `modules.json` (Normalize module?), the Pooling module's config and
    `sentence_bert_config.json` (max_seq_length). Returns (pooling, max_seq_length | None, always_normalise); pooling is "last"
    (lasttoken) or "mean" (mean_tokens) -- what the checkpoint says; what the kernels implement is HipLlama's to decide --, anything
    else is refused, a module other than Transformer / Pooling / Normalize too."""
    return _d128.read_st_config(model_dir, {"lasttoken": "last", "mean_tokens": "mean"}, True, "a decoder embedder states its pooling there",
                                "a Mistral / Llama embedder pools lasttoken or mean_tokens")


def resolve_mode(model_name: str, shape: Optional[LlamaShape], model_kwargs: dict, st_pool: Optional[str]) -> str:
    """The pooling a model runs with, after checking the attention mode. model_kwargs["attention"] is the CALLER'S statement of how the
    checkpoint was trained: "causal" (the default; with the config's window) or "bidirectional" (every key below the row's length for
    every query, the window ignored) -- no released checkpoint's custom code is read, so an embedder trained without the causal mask
    (its model card says so) needs the keyword. Pooling: model_kwargs["pooling"] ("last" | "mean"), else the checkpoint's Pooling
    module, else "mean" under bidirectional attention, else the shape's. Anything else is refused by name, before any GPU work."""
    attention = model_kwargs.get("attention", shape.attention if shape is not None else "causal")
    if attention not in ("causal", "bidirectional"):
        raise ValueError(f"{model_name}: attention {attention!r} (\"causal\" or \"bidirectional\")")
    default = "mean" if attention == "bidirectional" else (shape.pooling if shape is not None else "last")
    pooling = model_kwargs.get("pooling", st_pool or default)
    if pooling not in ("last", "mean"):
        raise ValueError(f"{model_name}: pooling {pooling!r} (Mistral / Llama embedders pool 'last' or 'mean')")
    return pooling


def apply_mode(shape: LlamaShape, model_kwargs: dict) -> LlamaShape:
    """The shape with model_kwargs["attention"] taken in (resolve_mode has checked it)."""
    return LlamaShape(*shape)._replace(attention=model_kwargs.get("attention", LlamaShape(*shape).attention))


class HipLlama(HipStack):
    family, prefix, embed_key, matrix_keys = "llama", "llama", "embed_tokens", MATRIX_KEYS
    poolings, pooling_noun = ("last", "mean"), "Mistral / Llama embedders"
    shape_type, layer_keys = LlamaShape, LAYER_KEYS      # HipQwen2 restates these, the four names above and _config

    def __init__(self, shape, weights: Dict[str, "np.ndarray"], device: Optional[int] = None):
        """shape: a LlamaShape (or a plain tuple in its order); weights: the header's names (weight_order), numpy arrays or torch
        tensors. Under llama3 scaling the rotary table is rebuilt from rope_inv_freq(shape), HF's own float32 frequencies."""
        shape = self.shape_type(*shape)
        self.shape = shape
        self.hidden, self.layers, self.vocab, self.out_dim = shape.hidden, shape.layers, shape.vocab, shape.hidden
        self.max_seq = min(int(shape.max_position), MAX_SEQ)
        if shape.attention not in ("causal", "bidirectional"):
            raise ValueError(f"attention {shape.attention!r} (\"causal\" or \"bidirectional\")")
        self.bidirectional = shape.attention == "bidirectional"
        self.pooling = shape.pooling            # what forward() pools with when it is not told
        names = _d128.weight_order(self.layer_keys, shape.layers)
        self._upload(weights, names, device)
        self._create(self._config(shape), names)
        if shape.scaling is not None:           # default RoPE: the table ak_<prefix>_create built from theta
            inv = np.ascontiguousarray(rope_inv_freq(shape), np.float32)
            fn = f"ak_{self.prefix}_set_rope_inv_freq"
            check(getattr(self._lib, fn)(self._h, ctypes.c_void_p(inv.ctypes.data)), fn)

    def _config(self, shape):
        """The library's config struct of a checked shape."""
        self.window = 0 if self.bidirectional else int(shape.window)
        return AkLlamaConfig(shape.vocab, shape.hidden, shape.layers, shape.q_heads, shape.kv_heads, HEAD_DIM, shape.intermediate,
                             shape.max_position, shape.rms_eps, shape.rope_theta, self.window, int(self.bidirectional))

    def forward(self, ids, lens, pooling: Optional[str] = None, normalise: bool = True, S: Optional[int] = None):
        """ids [B, W] (row i holds lens[i] ids), lens [B] -> [B, hidden] float32 CUDA tensor (one tile, S = W rounded up to 32)."""
        return super().forward(ids, lens, pooling=pooling, normalise=normalise, S=S)
