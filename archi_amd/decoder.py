"""HipDecoder -- Python handle of the HIP Qwen3 decoder (ak_decoder_*): the Qwen3-Embedding models the reference's retrievers
name as instruction-aware embedders (src/data_manager/vectorstore/retrievers/utils.py:7-11).

PyTorch-ROCm only HOLDS the weights in HBM (bf16 matrices, fp32 vectors) and hands raw device pointers to the C ABI; every
arithmetic step of the forward pass runs in hand-written HIP kernels (archi_amd/csrc/decoder128.hip, the head-128 decoder stack
behind decoder.hip's ABI; attn_causal.hip, gemm.hip). Also here: the checkpoint loader (load_qwen3_weights), seeded random weights
of the named shapes, the sentence-transformers configuration of a decoder checkpoint (all three on _decoder128.py, which the
Mistral / Llama and Qwen2 handles share) and the byte-level BPE tokenizer wrapper.
"""
from __future__ import annotations

import ctypes
import json
import os
import threading
from typing import Dict, List, Optional

import numpy as np

from . import _lib
from ._lib import AkDecoderConfig, check
from . import _decoder128 as _d128
from ._decoder128 import HEAD_DIM, MATRIX_KEYS, MAX_SEQ, hf_layer_names, layer_keys  # noqa: F401 (re-exported)
from ._stack import HipStack, read_safetensors_dir

# name -> config.json numbers (vocab, hidden, layers, q_heads, kv_heads, intermediate, max_position, rope_theta, rms_eps)
QWEN3_SHAPES = {
    "Qwen/Qwen3-Embedding-0.6B": (151669, 1024, 28, 16, 8, 3072, 32768, 1e6, 1e-6),
    "Qwen/Qwen3-Embedding-4B": (151669, 2560, 36, 32, 8, 9728, 40960, 1e6, 1e-6),
    "Qwen/Qwen3-Embedding-8B": (151669, 4096, 36, 32, 8, 12288, 40960, 1e6, 1e-6),
    # small shapes of the test fixtures (tests/golden/make_decoder_fixtures.py): GQA ratios 1, 2 and 4 at head dim 128
    "qwen3-tiny-g1": (1000, 256, 2, 2, 2, 512, 8192, 1e6, 1e-6),
    "qwen3-tiny-g2": (1000, 256, 3, 4, 2, 768, 8192, 1e6, 1e-6),
    "qwen3-tiny-g4": (1000, 256, 4, 8, 2, 512, 8192, 1e4, 1e-6),
}

LAYER_KEYS = layer_keys(qk_norm=True)      # wq wk wv q_norm k_norm wo ln_in ln_post w_gate w_up w_down
HF_LAYER_NAMES = hf_layer_names(LAYER_KEYS)      # our name -> HF Qwen3Model state-dict name (layer keys under "layers.{l}.")


def weight_order(layers: int) -> List[str]:
    """The header's weight order: embed_tokens, final norm, then per layer LAYER_KEYS (2 + 11 * layers names)."""
    return _d128.weight_order(LAYER_KEYS, layers)


def hf_state_dict(weights: Dict[str, "np.ndarray"], layers: int) -> Dict[str, "np.ndarray"]:
    """Our weight names -> HF Qwen3Model's (no "model." prefix)."""
    return _d128.hf_state_dict(HF_LAYER_NAMES, weights, layers)


def random_qwen3_weights(shape, seed: int = 0) -> Dict[str, "np.ndarray"]:
    """Seeded random weights of a Qwen3 shape (a QWEN3_SHAPES tuple or name), as _decoder128.random_weights draws them."""
    return _d128.random_weights(LAYER_KEYS, QWEN3_SHAPES[shape] if isinstance(shape, str) else shape, seed)


def _rope_theta(cfg: dict) -> float:
    """rope_theta at the top level (transformers 4) or inside rope_parameters (transformers 5); default RoPE only."""
    rp = cfg.get("rope_parameters") or {}
    rs = cfg.get("rope_scaling")
    for what in (rs, rp):
        if what and what.get("rope_type", what.get("type", "default")) not in ("default", None):
            raise ValueError(f"rope type {what.get('rope_type', what.get('type'))!r} is not supported (default RoPE only)")
    theta = cfg.get("rope_theta", rp.get("rope_theta"))
    if theta is None:
        raise ValueError("config.json has no rope_theta")
    return float(theta)


def qwen3_config_shape(cfg: dict, where: str = "config.json"):
    """config.json of a Qwen3 checkpoint -> QWEN3_SHAPES-style tuple; everything the kernels do not implement is refused."""
    if cfg.get("model_type") != "qwen3":
        raise ValueError(f"{where}: model_type {cfg.get('model_type')!r} is not qwen3")
    if cfg.get("hidden_act", "silu") != "silu":
        raise ValueError(f"{where}: hidden_act {cfg.get('hidden_act')!r} (the HIP decoder implements SiLU / SwiGLU)")
    if cfg.get("attention_bias", False):
        raise ValueError(f"{where}: attention_bias is not supported")
    if cfg.get("use_sliding_window", False) or any(t == "sliding_attention" for t in (cfg.get("layer_types") or [])):
        raise ValueError(f"{where}: sliding-window attention is not supported")
    H, nq = cfg["hidden_size"], cfg["num_attention_heads"]
    hd = cfg.get("head_dim") or H // nq
    if hd != HEAD_DIM:
        raise ValueError(f"{where}: head_dim {hd} (the HIP decoder implements 128)")
    try:
        theta = _rope_theta(cfg)
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    return (cfg["vocab_size"], H, cfg["num_hidden_layers"], nq, cfg.get("num_key_value_heads", nq), cfg["intermediate_size"],
            cfg.get("max_position_embeddings", 32768), theta, float(cfg.get("rms_norm_eps", 1e-6)))


def load_qwen3_weights(model_dir: str):
    """Local Qwen3 checkpoint directory (config.json + model.safetensors or sharded model-*.safetensors) -> (shape, weights in
    the header's names). A "model." prefix on the tensor names is stripped. No network."""
    cfg = json.load(open(os.path.join(model_dir, "config.json")))
    shape = qwen3_config_shape(cfg, os.path.join(model_dir, "config.json"))
    return shape, _d128.from_hf_state_dict(HF_LAYER_NAMES, read_safetensors_dir(model_dir), shape[2])


def read_decoder_st_config(model_dir: str):
    """sentence-transformers files of a decoder checkpoint: `modules.json` (Normalize module?), the Pooling module's config (must be
    lasttoken) and `sentence_bert_config.json` (max_seq_length). Returns (max_seq_length | None, always_normalise)."""
    return _d128.read_st_config(model_dir, {"lasttoken": "last"}, False, "a decoder embedder needs lasttoken pooling",
                                "the HIP decoder implements lasttoken")[1:]


class BpeTokenizer:
    """The checkpoint's own tokenizer.json (byte-level BPE for Qwen3) through the `tokenizers` wheel. Special tokens are whatever
    the file's post-processor adds (Qwen3-Embedding appends <|endoftext|>, the token the last-token pool reads); truncation at
    max_len happens before the post-processor, as PreTrainedTokenizerFast(truncation=True, max_length=max_len) does."""

    def __init__(self, tokenizer_file: str):
        from tokenizers import Tokenizer
        self._tok = Tokenizer.from_file(tokenizer_file)
        self._tok.no_padding()
        self._max = None
        self._lock = threading.Lock()

    def encode_batch(self, texts: List[str], max_len: int) -> List[List[int]]:
        with self._lock:
            if self._max != max_len:
                self._tok.enable_truncation(max_len)
                self._max = max_len
            return [e.ids for e in self._tok.encode_batch(list(texts))]

    def encode(self, text: str, max_len: int) -> List[int]:
        return self.encode_batch([text], max_len)[0]

    def encode_batch_array(self, texts: List[str], max_len: int):
        """-> (ids [n, max_len] int32 zero padded, lens [n] int32)."""
        rows = self.encode_batch(texts, max_len)
        ids = np.zeros((len(rows), max_len), np.int32)
        lens = np.empty(len(rows), np.int32)
        for i, r in enumerate(rows):
            ids[i, : len(r)] = r
            lens[i] = len(r)
        return ids, lens


class HipDecoder(HipStack):
    family, prefix, embed_key, matrix_keys, abi_pooling = "decoder", "decoder", "embed_tokens", MATRIX_KEYS, False

    def __init__(self, shape, weights: Dict[str, "np.ndarray"], device: Optional[int] = None):
        """shape: a QWEN3_SHAPES tuple (vocab, hidden, layers, q_heads, kv_heads, intermediate, max_position, rope_theta, rms_eps);
        weights: the header's names (weight_order), numpy arrays or torch tensors."""
        vocab, H, L, nq, nkv, I, max_pos, theta, eps = shape
        self.shape = tuple(shape)
        self.hidden, self.layers, self.vocab, self.out_dim = H, L, vocab, H
        self.max_seq = min(int(max_pos), MAX_SEQ)
        self._upload(weights, weight_order(L), device)
        self._create(AkDecoderConfig(vocab, H, L, nq, nkv, HEAD_DIM, I, max_pos, eps, theta), weight_order(L))

    def _pooling(self, pooling):
        if pooling != "last":
            raise ValueError(f"pooling {pooling!r}: the decoder implements last-token pooling only")
        return pooling

    def forward_lens(self, stage, n_rows: int, S: int, out, pooling: str = "last", normalise: bool = True) -> None:
        """HipStack.forward_lens with `out` [n_rows, hidden]. Decoder models pool the last token only."""
        super().forward_lens(stage, n_rows, S, out, pooling=pooling, normalise=normalise)

    def forward(self, ids, lens, normalise: bool = True):
        """ids [B, W] (row i holds lens[i] ids), lens [B] -> [B, hidden] float32 CUDA tensor (one tile, S = W rounded up to 32)."""
        return super().forward(ids, lens, pooling="last", normalise=normalise)


def rope_table_inv(inv_freq, n_pos: int):
    """ak_decoder_rope_table_inv (host only): cos, sin [n_pos][len(inv_freq)] float32 from given float32 inverse frequencies."""
    lib = _lib.load()
    inv = np.ascontiguousarray(inv_freq, np.float32)
    c = np.empty((n_pos, inv.size), np.float32)
    s = np.empty((n_pos, inv.size), np.float32)
    check(lib.ak_decoder_rope_table_inv(inv.ctypes.data, inv.size, n_pos, c.ctypes.data, s.ctypes.data), "ak_decoder_rope_table_inv")
    return c, s


def rope_table(theta: float, n_pos: int, head_dim: int = HEAD_DIM):
    """ak_decoder_rope_table (host only): cos, sin [n_pos][head_dim / 2] float32."""
    lib = _lib.load()
    c = np.empty((n_pos, head_dim // 2), np.float32)
    s = np.empty((n_pos, head_dim // 2), np.float32)
    check(lib.ak_decoder_rope_table(ctypes.c_float(theta), head_dim, n_pos, c.ctypes.data, s.ctypes.data), "ak_decoder_rope_table")
    return c, s
