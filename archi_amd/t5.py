"""HipT5 -- Python handle of the HIP T5 encoder (ak_t5_*): sentence-transformers/gtr-t5-base / -large, sentence-t5-base / -large, the
GTR-initialised instructor models loaded as plain sentence-transformers directories, and T5 v1.1 encoders.

PyTorch-ROCm only HOLDS the weights in HBM (bf16 matrices, fp32 vectors, the fp32 bias table and Dense matrices) and hands raw device
pointers to the C ABI; every arithmetic step of the forward pass runs in hand-written HIP kernels (archi_amd/csrc/t5.hip,
attn_long.hip, gemm.hip). Also here: the config.json reader that refuses what the kernels do not implement, the relative-position
bias table (t5_rel_table: HF's own torch expression for the bucket, evaluated once per distance), the checkpoint loader and seeded
random weights of the named shapes.

T5 has no position embedding and no RoPE: position enters only through a learned per-head bias on the attention scores,
bias[h][bucket(key - query)], and the scores are not scaled. The bidirectional bucket saturates: every |key - query| >=
relative_attention_max_distance D maps to the last bucket of its side, so the bias is a function of clamp(key - query, -D, D) alone
and 2 D + 1 floats per head hold it for every row length.
"""
from __future__ import annotations

import ctypes
import json
import math
import os
from typing import Dict, List, Optional

import numpy as np

from ._lib import MBERT_MAX_LAYERS, AkT5Config
from ._stack import HipStack, read_safetensors_dir, seeded_mat_vec
from .gemma import read_dense_modules

MAX_SEQ = 8192          # longest row the kernels take (attn_long.hip); the model has no position limit of its own
HEAD_DIM = 64
MAX_DISTANCE = 4096     # ATTN_RELBIAS_MAX_D: the table lives in LDS
LOG2E = 1.4426950408889634
FFN_KINDS = ("relu", "gated-gelu")

# name -> (vocab, d_model, layers, heads, d_kv, d_ff, feed_forward_proj, relative_attention_num_buckets,
#          relative_attention_max_distance, layer_norm_epsilon, longest row, default pooling, Dense output widths)
_V10_BASE = (32128, 768, 12, 12, 64, 3072, "relu", 32, 128, 1e-6, MAX_SEQ, "mean")
_V10_LARGE = (32128, 1024, 24, 16, 64, 4096, "relu", 32, 128, 1e-6, MAX_SEQ, "mean")
T5_SHAPES = {
    "sentence-transformers/gtr-t5-base": _V10_BASE + ((768,),),
    "sentence-transformers/gtr-t5-large": _V10_LARGE + ((768,),),
    "sentence-transformers/sentence-t5-base": _V10_BASE + ((768,),),
    "sentence-transformers/sentence-t5-large": _V10_LARGE + ((768,),),
    # the encoders alone, in both feed-forward kinds (T5 v1.1: gated-gelu, d_ff 2048 / 2816)
    "t5-base-encoder": _V10_BASE + ((),),
    "t5-large-encoder": _V10_LARGE + ((),),
    "t5-v1_1-base-encoder": (32128, 768, 12, 12, 64, 2048, "gated-gelu", 32, 128, 1e-6, MAX_SEQ, "mean", ()),
    "t5-v1_1-large-encoder": (32128, 1024, 24, 16, 64, 2816, "gated-gelu", 32, 128, 1e-6, MAX_SEQ, "mean", ()),
    # small shapes of the test fixtures (tests/golden/make_t5_fixtures.py). d_ff 192 is no multiple of 128: the un-gated pair is
    # padded at create; D = 16 with 8 buckets reaches every key-block class of the attention kernel at S <= 160
    "t5-tiny-relu": (1000, 128, 2, 2, 64, 192, "relu", 32, 128, 1e-6, MAX_SEQ, "mean", ()),
    "t5-tiny-gated": (1000, 128, 2, 2, 64, 256, "gated-gelu", 32, 128, 1e-6, MAX_SEQ, "mean", ()),
    "t5-tiny-d16": (1000, 128, 2, 2, 64, 256, "gated-gelu", 8, 16, 1e-6, MAX_SEQ, "mean", ()),
    # the base shape's width through a two-layer cut, with gtr's Dense head
    "t5-base-cut2": (2000, 768, 2, 12, 64, 3072, "relu", 32, 128, 1e-6, MAX_SEQ, "mean", (768,)),
}

MATRIX_KEYS = {"wq", "wk", "wv", "wo", "wi", "wi_0", "wi_1", "wo_ff"}
# our name -> HF T5EncoderModel state-dict name under "encoder.block.{l}."
HF_LAYER_NAMES = {"ln0": "layer.0.layer_norm.weight", "wq": "layer.0.SelfAttention.q.weight", "wk": "layer.0.SelfAttention.k.weight",
                  "wv": "layer.0.SelfAttention.v.weight", "wo": "layer.0.SelfAttention.o.weight", "ln1": "layer.1.layer_norm.weight",
                  "wi": "layer.1.DenseReluDense.wi.weight", "wi_0": "layer.1.DenseReluDense.wi_0.weight",
                  "wi_1": "layer.1.DenseReluDense.wi_1.weight", "wo_ff": "layer.1.DenseReluDense.wo.weight"}
HF_REL_BIAS = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"


def layer_keys(kind: str):
    """A layer's weights in the header's order."""
    return ("ln0", "wq", "wk", "wv", "wo", "ln1") + (("wi", "wo_ff") if kind == "relu" else ("wi_0", "wi_1", "wo_ff"))


def weight_names(layers: int, kind: str, n_dense: int = 0) -> List[str]:
    """Every weight of a model in our names: "rel_bias" is HF's [num_buckets][heads] embedding (the handle turns it into the
    header's rel_table)."""
    names = ["shared", "rel_bias", "final_norm"]
    for l in range(layers):
        names += [f"l{l}.{k}" for k in layer_keys(kind)]
    return names + [f"dense{i}" for i in range(n_dense)]


def hf_state_dict(weights: Dict[str, "np.ndarray"]) -> Dict[str, "np.ndarray"]:
    """Our weight names -> HF T5EncoderModel's (the Dense matrices are not part of that model)."""
    sd = {"shared.weight": weights["shared"], "encoder.embed_tokens.weight": weights["shared"], HF_REL_BIAS: weights["rel_bias"],
          "encoder.final_layer_norm.weight": weights["final_norm"]}
    for name, arr in weights.items():
        if name[0] == "l" and "." in name:
            l, k = name[1:].split(".", 1)
            sd[f"encoder.block.{l}.{HF_LAYER_NAMES[k]}"] = arr
    return sd


def t5_relative_position_bucket(relative_position, num_buckets: int, max_distance: int):
    """T5Attention._relative_position_bucket(bidirectional=True) restated with the same torch ops: the float32 log decides the
    boundaries of the large buckets, so the ops are kept as they are. relative_position = key - query (an int64 tensor)."""
    import torch
    relative_buckets = 0
    num_buckets //= 2
    relative_buckets += (relative_position > 0).to(torch.long) * num_buckets
    relative_position = torch.abs(relative_position)
    max_exact = num_buckets // 2
    is_small = relative_position < max_exact
    relative_position_if_large = max_exact + (
        torch.log(relative_position.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)
    ).to(torch.long)
    relative_position_if_large = torch.min(relative_position_if_large, torch.full_like(relative_position_if_large, num_buckets - 1))
    relative_buckets += torch.where(is_small, relative_position, relative_position_if_large)
    return relative_buckets


def t5_rel_table(weight, num_buckets: int, max_distance: int) -> "np.ndarray":
    """relative_attention_bias.weight [num_buckets][heads] -> the clamped table [heads][2 D + 1] float32, D = max_distance: entry
    [h][d + D] is the bias of key - query = d for -D <= d <= D; every larger distance has the bias of +-D (the bucket saturates
    there). In the natural domain, as HF adds it: HipT5 multiplies by log2(e)."""
    import torch
    w = weight if isinstance(weight, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(weight))
    D = int(max_distance)
    bucket = t5_relative_position_bucket(torch.arange(-D, D + 1, dtype=torch.long), int(num_buckets), D)
    return np.ascontiguousarray(w.float()[bucket].t().contiguous().numpy())


def random_t5_weights(shape, seed: int = 0, std: float = 0.05, bias_std: float = 2.0) -> Dict[str, "np.ndarray"]:
    """Seeded random weights of a T5 shape (a T5_SHAPES tuple or name). Matrices are drawn with `std` and ROUNDED TO bf16 (kept as
    float32 values), as the other families' are; the relative-attention bias with `bias_std`, bf16-valued too (a bias of the released
    models' size: without it nothing in the model depends on position); norm weights around 1. Dense matrices with std in ** -0.5."""
    if isinstance(shape, str):
        shape = T5_SHAPES[shape]
    vocab, H, L, heads, dkv, dff, kind, buckets = shape[:8]
    mat, vec = seeded_mat_vec(seed, std)
    w = {"shared": mat(vocab, H), "rel_bias": mat(buckets, heads, bias_std), "final_norm": vec(H)}
    inner = heads * dkv
    for l in range(L):
        p = f"l{l}."
        w[p + "ln0"] = vec(H)
        w[p + "wq"], w[p + "wk"], w[p + "wv"], w[p + "wo"] = mat(inner, H), mat(inner, H), mat(inner, H), mat(H, inner)
        w[p + "ln1"] = vec(H)
        if kind == "relu":
            w[p + "wi"] = mat(dff, H)
        else:
            w[p + "wi_0"], w[p + "wi_1"] = mat(dff, H), mat(dff, H)
        w[p + "wo_ff"] = mat(H, dff)
    din = H
    for i, dout in enumerate(shape[12]):
        w[f"dense{i}"] = mat(dout, din, din ** -0.5)
        din = dout
    return w


def _refuse(where: str, field: str, value, why: str):
    raise ValueError(f"{where}: {field} {value!r} is not supported ({why})")


def t5_config_shape(cfg: dict, where: str = "config.json", pooling: str = "mean", dense=()):
    """config.json of a T5 checkpoint (T5EncoderModel or the full model) -> T5_SHAPES-style tuple; everything the kernels do not
    implement is refused with a ValueError that names the field."""
    if cfg.get("model_type") != "t5":
        raise ValueError(f"{where}: model_type {cfg.get('model_type')!r} is not t5")
    H, heads, dkv, dff = int(cfg["d_model"]), int(cfg["num_heads"]), int(cfg.get("d_kv", 64)), int(cfg["d_ff"])
    L = int(cfg["num_layers"])
    if dkv != HEAD_DIM:
        _refuse(where, "d_kv", dkv, f"the HIP attention kernel implements head size {HEAD_DIM}: t5-3b / t5-11b are out of scope")
    if heads <= 0 or heads * HEAD_DIM != H:
        _refuse(where, "num_heads", heads, f"num_heads * d_kv must equal d_model {H}: t5-small v1.1 and the like are out of scope")
    if H % 128 or H > 1024:
        _refuse(where, "d_model", H, "the HIP kernels take d_model % 128 == 0, <= 1024: xl / xxl are out of scope")
    if dff <= 0 or dff % 64:
        _refuse(where, "d_ff", dff, "the HIP GEMM takes d_ff % 64 == 0")
    if L <= 0 or L > MBERT_MAX_LAYERS:
        _refuse(where, "num_layers", L, f"1 to {MBERT_MAX_LAYERS} layers")
    kind = cfg.get("feed_forward_proj", "relu")
    if kind not in FFN_KINDS:
        _refuse(where, "feed_forward_proj", kind, "relu (T5 v1.0) or gated-gelu (T5 v1.1)")
    act = cfg.get("dense_act_fn")
    if act is not None and act != ("relu" if kind == "relu" else "gelu_new"):
        _refuse(where, "dense_act_fn", act, f"feed_forward_proj {kind!r} runs {'relu' if kind == 'relu' else 'gelu_new'}")
    buckets = int(cfg.get("relative_attention_num_buckets", 32))
    D = int(cfg.get("relative_attention_max_distance", 128))
    if buckets % 2 or buckets < 4:
        _refuse(where, "relative_attention_num_buckets", buckets, "an even count of at least 4: half of them per side")
    if D < 1 or D > MAX_DISTANCE or D <= buckets // 4:
        _refuse(where, "relative_attention_max_distance", D, f"more than num_buckets / 4 = {buckets // 4} and at most {MAX_DISTANCE}")
    eps = float(cfg.get("layer_norm_epsilon", 1e-6))
    if not eps > 0:
        _refuse(where, "layer_norm_epsilon", eps, "must be positive")
    if pooling not in ("mean", "cls"):
        raise ValueError(f"{where}: pooling {pooling!r} (T5 embedders pool 'mean' or 'cls')")
    return (int(cfg["vocab_size"]), H, L, heads, dkv, dff, kind, buckets, D, eps, MAX_SEQ, pooling, tuple(int(d) for d in dense))


def shape_config_dict(shape) -> dict:
    """A T5_SHAPES tuple -> the config.json of such a checkpoint."""
    if isinstance(shape, str):
        shape = T5_SHAPES[shape]
    vocab, H, L, heads, dkv, dff, kind, buckets, D, eps = shape[:10]
    return dict(model_type="t5", architectures=["T5EncoderModel"], vocab_size=vocab, d_model=H, d_kv=dkv, d_ff=dff, num_layers=L, num_heads=heads,
                relative_attention_num_buckets=buckets, relative_attention_max_distance=D, dropout_rate=0.0, layer_norm_epsilon=eps,
                feed_forward_proj=kind, is_encoder_decoder=False, use_cache=False, pad_token_id=0, eos_token_id=1)


def shape_hf_config(shape, **extra):
    """A T5_SHAPES tuple -> transformers.T5Config (the tests' float32 reference)."""
    from transformers import T5Config
    kw = shape_config_dict(shape)
    kw.pop("model_type")
    kw.pop("architectures")
    kw.update(extra)
    return T5Config(**kw)


def load_t5_weights(model_dir: str, pooling: str = "mean"):
    """Local checkpoint directory (config.json + model.safetensors or shards, and the Dense modules when it is a sentence-transformers
    directory) holding a T5EncoderModel or a full T5 model -> (shape, weights in our names). shared.weight (or
    encoder.embed_tokens.weight) and encoder.* are read; decoder.* and lm_head are ignored. No network."""
    cj = os.path.join(model_dir, "config.json")
    dense = read_dense_modules(model_dir)
    shape = t5_config_shape(json.load(open(cj)), cj, pooling=pooling, dense=[d.shape[0] for d in dense])
    sd = read_safetensors_dir(model_dir)
    w = {"shared": sd["shared.weight"] if "shared.weight" in sd else sd["encoder.embed_tokens.weight"], "rel_bias": sd[HF_REL_BIAS],
         "final_norm": sd["encoder.final_layer_norm.weight"]}
    for l in range(shape[2]):
        for k in layer_keys(shape[6]):
            w[f"l{l}.{k}"] = sd[f"encoder.block.{l}.{HF_LAYER_NAMES[k]}"]
    din = shape[1]
    for i, d in enumerate(dense):
        if d.shape[1] != din:
            raise ValueError(f"{model_dir}: Dense module {i} takes {d.shape[1]} features, the model hands it {din}")
        w[f"dense{i}"] = d
        din = d.shape[0]
    return shape, w


class HipT5(HipStack):
    family, prefix, embed_key, matrix_keys, out_name, pooling_noun = "T5", "t5", "shared", MATRIX_KEYS, "out_dim", "T5 embedders"

    def __init__(self, shape, weights: Dict[str, "np.ndarray"], device: Optional[int] = None, dense: bool = True):
        """shape: a T5_SHAPES tuple or name; weights: our names (weight_names), numpy arrays or torch tensors. dense=False leaves
        the Dense head out (the plain encoder, pooled)."""
        if isinstance(shape, str):
            shape = T5_SHAPES[shape]
        vocab, H, L, heads, dkv, dff, kind, buckets, D, eps, max_pos, pooling, dense_out = shape
        if not dense:
            dense_out = ()
        if kind not in FFN_KINDS:
            raise ValueError(f"T5 shape: feed_forward_proj {kind!r} (relu or gated-gelu)")
        if L > MBERT_MAX_LAYERS:
            raise ValueError(f"T5 shape: {L} layers (at most {MBERT_MAX_LAYERS})")
        if len(dense_out) > 2:
            raise ValueError(f"T5 shape: {len(dense_out)} Dense modules (at most 2)")
        self.shape = tuple(shape)
        self.hidden, self.layers, self.vocab, self.pooling = H, L, vocab, pooling
        self.out_dim = dense_out[-1] if dense_out else H
        self.max_seq = min(int(max_pos), MAX_SEQ)
        if "rel_bias" not in weights:
            from ._lib import HipBackendError
            raise HipBackendError("T5 weight 'rel_bias' missing")
        rb = weights["rel_bias"]
        if tuple(rb.shape) != (buckets, heads):
            raise ValueError(f"T5 weight rel_bias: shape {tuple(rb.shape)}, expected {(buckets, heads)}")
        # the header's rel_table: HF's bias per clamped distance, in the base-2 domain of the kernels' softmax
        self.rel_table = t5_rel_table(rb, buckets, D)
        up = dict(weights)
        up["rel_table"] = self.rel_table * np.float32(LOG2E)
        names = ["rel_table" if n == "rel_bias" else n for n in weight_names(L, kind, len(dense_out))]
        self._upload(up, names, device)
        din = H
        for i, dout in enumerate(dense_out):
            if tuple(self._tensors[f"dense{i}"].shape) != (dout, din):
                raise ValueError(f"T5 weight dense{i}: shape {tuple(self._tensors[f'dense{i}'].shape)}, expected {(dout, din)}")
            din = dout
        self._create(AkT5Config(vocab, H, L, heads, dkv, dff, int(kind != "relu"), D, eps, len(dense_out),
                                (ctypes.c_int * 2)(*(list(dense_out) + [0, 0])[:2])), names)
