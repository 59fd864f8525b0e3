"""HipGemma -- Python handle of the HIP EmbeddingGemma encoder (ak_gemma_*): google/embeddinggemma-300m, a Gemma3 text stack run
bidirectionally, and the sentence-transformers tail behind it (mean pooling, Dense modules, Normalize).

PyTorch-ROCm only HOLDS the weights in HBM (bf16 matrices, fp32 vectors and Dense matrices) and hands raw device pointers to the C
ABI; every arithmetic step of the forward pass runs in hand-written HIP kernels (archi_amd/csrc/gemma.hip, attn_gqa.hip, gemm.hip).
Also here: the config.json reader that refuses what the kernels do not implement, the checkpoint loader (safetensors plus the
2_Dense / 3_Dense modules) and seeded random weights of the named shapes.
"""
from __future__ import annotations

import ctypes
import json
import os
from typing import Dict, List, Optional

import numpy as np

from ._lib import GEMMA_MAX_LAYERS, AkGemmaConfig, check
from ._stack import HipStack, read_safetensors_dir, seeded_mat_vec

MAX_SEQ = 2048          # longest row the kernels take (attn_gqa.hip)
HEAD_DIM = 256
MAX_GROUP = 4
ACTIVATION = "gelu_pytorch_tanh"


def _pattern(n_layers: int, every: int):
    """layer_types of the released model: every `every`-th layer full attention (1), the others sliding (0)."""
    return tuple(0 if (l + 1) % every else 1 for l in range(n_layers))


# name -> (vocab, hidden, layers, q heads, kv heads, head_dim, intermediate, max_position, rms_eps, global theta, local theta,
#          sliding_window AS THE CONFIG FILE HOLDS IT (a query sees sliding_window // 2 keys to each side), query_pre_attn_scalar,
#          layer types (1 full / 0 sliding), Dense output widths)
GEMMA_SHAPES = {
    "google/embeddinggemma-300m": (262144, 768, 24, 3, 1, 256, 1152, 2048, 1e-6, 1e6, 1e4, 512, 256, _pattern(24, 6), (3072, 768)),
    # small shapes of the test fixtures (tests/golden/make_gemma_fixtures.py); head size 256 because the kernel takes no other, and
    # query_pre_attn_scalar 128 so that a head_dim ** -0.5 scale would show
    "gm-tiny": (1000, 384, 3, 3, 1, 256, 384, 2048, 1e-6, 1e6, 1e4, 64, 128, (0, 0, 1), (1536, 384)),
    "gm-g2": (1000, 512, 2, 4, 2, 256, 320, 2048, 1e-6, 1e6, 1e4, 64, 128, (0, 1), ()),
    "gm-global": (1000, 384, 2, 3, 1, 256, 384, 2048, 1e-6, 1e6, 1e4, 64, 128, (1, 1), (384,)),
    "gm-local": (1000, 384, 2, 3, 1, 256, 384, 2048, 1e-6, 1e6, 1e4, 64, 128, (0, 0), ()),
    # the base width through cuts of the stack (tests): every GEMM shape of the released model
    "gm-base-cut2": (2000, 768, 2, 3, 1, 256, 1152, 2048, 1e-6, 1e6, 1e4, 512, 256, (0, 1), (3072, 768)),
    "gm-base-24": (2000, 768, 24, 3, 1, 256, 1152, 2048, 1e-6, 1e6, 1e4, 512, 256, _pattern(24, 6), (3072, 768)),
}

LAYER_KEYS = ("input_ln", "wq", "wk", "wv", "q_norm", "k_norm", "wo", "post_attn_ln", "pre_ffn_ln", "w_gate", "w_up", "w_down", "post_ffn_ln")
MATRIX_KEYS = {"wq", "wk", "wv", "wo", "w_gate", "w_up", "w_down"}
# our name -> HF Gemma3TextModel state-dict name (layer keys under "layers.{l}.")
HF_LAYER_NAMES = {"input_ln": "input_layernorm.weight", "wq": "self_attn.q_proj.weight", "wk": "self_attn.k_proj.weight",
                  "wv": "self_attn.v_proj.weight", "q_norm": "self_attn.q_norm.weight", "k_norm": "self_attn.k_norm.weight",
                  "wo": "self_attn.o_proj.weight", "post_attn_ln": "post_attention_layernorm.weight",
                  "pre_ffn_ln": "pre_feedforward_layernorm.weight", "w_gate": "mlp.gate_proj.weight", "w_up": "mlp.up_proj.weight",
                  "w_down": "mlp.down_proj.weight", "post_ffn_ln": "post_feedforward_layernorm.weight"}
DENSE_DIRS = ("2_Dense", "3_Dense")


def weight_names(layers: int, n_dense: int = 0) -> List[str]:
    """Every weight of a model in the header's order."""
    names = ["embed", "final_norm"]
    for l in range(layers):
        names += [f"l{l}.{k}" for k in LAYER_KEYS]
    return names + [f"dense{i}" for i in range(n_dense)]


def hf_state_dict(weights: Dict[str, "np.ndarray"]) -> Dict[str, "np.ndarray"]:
    """Our weight names -> HF Gemma3TextModel's (no "model." prefix; the Dense matrices are not part of that model)."""
    sd = {"embed_tokens.weight": weights["embed"], "norm.weight": weights["final_norm"]}
    for name, arr in weights.items():
        if name[0] == "l" and "." in name:
            l, k = name[1:].split(".", 1)
            sd[f"layers.{l}.{HF_LAYER_NAMES[k]}"] = arr
    return sd


def random_gemma_weights(shape, seed: int = 0, std: float = 0.02) -> Dict[str, "np.ndarray"]:
    """Seeded random weights of a Gemma shape (a GEMMA_SHAPES tuple or name). Matrices are drawn with `std` and ROUNDED TO bf16 (kept
    as float32 values), as random_modernbert_weights does: a float32 reference on the same values measures the kernels' activation
    rounding alone. Norm weights are drawn around 0 (the model multiplies by 1 + w). Dense matrices are drawn with std in ** -0.5."""
    if isinstance(shape, str):
        shape = GEMMA_SHAPES[shape]
    vocab, H, L, nq, nkv, hd, I = shape[:7]
    mat, vec = seeded_mat_vec(seed, std, vec_mean=0.0)
    w = {"embed": mat(vocab, H), "final_norm": vec(H)}
    for l in range(L):
        p = f"l{l}."
        w[p + "input_ln"] = vec(H)
        w[p + "wq"], w[p + "wk"], w[p + "wv"] = mat(nq * hd, H), mat(nkv * hd, H), mat(nkv * hd, H)
        w[p + "q_norm"], w[p + "k_norm"] = vec(hd), vec(hd)
        w[p + "wo"] = mat(H, nq * hd)
        w[p + "post_attn_ln"], w[p + "pre_ffn_ln"] = vec(H), vec(H)
        w[p + "w_gate"], w[p + "w_up"], w[p + "w_down"] = mat(I, H), mat(I, H), mat(H, I)
        w[p + "post_ffn_ln"] = vec(H)
    din = H
    for i, dout in enumerate(shape[14]):
        w[f"dense{i}"] = mat(dout, din, din ** -0.5)
        din = dout
    return w


def rope_inv_freq(theta: float) -> "np.ndarray":
    """The 128 float32 inverse frequencies of a layer type, by the torch expression HF's default rotary initialisation evaluates
    (ROPE_INIT_FUNCTIONS["default"]): 1 / theta^(2 i / 256) with the power in torch's float32 arithmetic. Taken from torch rather than
    from the library's host routine because torch's vectorised float32 pow is 1 ulp off the correctly rounded value at one frequency
    in 128 (i = 74 at theta 1e6, i = 111 at 1e4): the same expression in the same library gives HF's buffer to the bit."""
    import torch
    inv = 1.0 / (float(theta) ** (torch.arange(0, HEAD_DIM, 2, dtype=torch.int64).to(dtype=torch.float) / HEAD_DIM))
    return inv.numpy().astype(np.float32)


def gemma_config_shape(cfg: dict, where: str = "config.json", dense=()):
    """config.json of a Gemma3 text checkpoint (transformers 5 `layer_types` / `rope_parameters`, or the transformers-4 spellings
    `sliding_window_pattern` / `rope_theta` / `rope_local_base_freq`) -> GEMMA_SHAPES-style tuple; everything the kernels do not
    implement is refused with a ValueError that names the field."""
    if cfg.get("model_type") != "gemma3_text":
        raise ValueError(f"{where}: model_type {cfg.get('model_type')!r} is not gemma3_text")
    if not cfg.get("use_bidirectional_attention", False):
        raise ValueError(f"{where}: use_bidirectional_attention must be true (the HIP Gemma kernels run the encoder form of the stack only)")
    if cfg.get("attention_bias", False):
        raise ValueError(f"{where}: attention_bias is not supported (the HIP Gemma kernels carry no bias)")
    for cap in ("attn_logit_softcapping", "final_logit_softcapping"):
        if cfg.get(cap):
            raise ValueError(f"{where}: {cap} {cfg[cap]!r} is not supported (no soft-capping in the HIP Gemma kernels)")
    act = cfg.get("hidden_activation", cfg.get("hidden_act", ACTIVATION))
    if act != ACTIVATION:
        raise ValueError(f"{where}: hidden_activation {act!r} (the HIP Gemma kernels implement {ACTIVATION})")
    H, L = int(cfg["hidden_size"]), int(cfg["num_hidden_layers"])
    nq, nkv = int(cfg["num_attention_heads"]), int(cfg.get("num_key_value_heads", cfg["num_attention_heads"]))
    hd = int(cfg.get("head_dim", 256))
    if hd != HEAD_DIM:
        raise ValueError(f"{where}: head_dim {hd} (the HIP Gemma attention kernel implements {HEAD_DIM})")
    if nq <= 0 or nkv <= 0 or nq % nkv:
        raise ValueError(f"{where}: num_attention_heads {nq} is not a multiple of num_key_value_heads {nkv}")
    if nq // nkv > MAX_GROUP:
        raise ValueError(f"{where}: num_attention_heads / num_key_value_heads = {nq // nkv} (groups of at most {MAX_GROUP} query heads per kv head)")
    rp = cfg.get("rope_parameters") or {}
    thetas = {}
    for kind, old, default in (("full_attention", "rope_theta", 1e6), ("sliding_attention", "rope_local_base_freq", 1e4)):
        sub = rp.get(kind) if isinstance(rp.get(kind), dict) else None
        theta = None
        if sub is not None:
            rt = sub.get("rope_type", sub.get("type", "default"))
            if rt not in ("default", None):
                raise ValueError(f"{where}: rope_parameters.{kind}.rope_type {rt!r} is not supported (default RoPE only)")
            theta = sub.get("rope_theta")
        if theta is None:
            theta = cfg.get(old, default)
        thetas[kind] = float(theta)
    rs = cfg.get("rope_scaling")
    if rs and rs.get("rope_type", rs.get("type", "default")) not in ("default", None):
        raise ValueError(f"{where}: rope_scaling {rs!r} is not supported (default RoPE only)")
    lt = cfg.get("layer_types")
    if lt is None:
        every = int(cfg.get("sliding_window_pattern", 6))
        lt = ["sliding_attention" if (l + 1) % every else "full_attention" for l in range(L)]
    if len(lt) != L or any(t not in ("full_attention", "sliding_attention") for t in lt):
        raise ValueError(f"{where}: layer_types must name full_attention / sliding_attention for each of the {L} layers")
    if L > GEMMA_MAX_LAYERS:
        raise ValueError(f"{where}: num_hidden_layers {L} (at most {GEMMA_MAX_LAYERS})")
    window = int(cfg.get("sliding_window", 4096))
    if window < 2:
        raise ValueError(f"{where}: sliding_window {window} must be >= 2 (a query sees sliding_window // 2 keys to each side)")
    I = int(cfg["intermediate_size"])
    if H % 128 or H > 1024:
        raise ValueError(f"{where}: hidden_size {H} (the HIP GEMM takes hidden_size % 128 == 0, <= 1024)")
    if I % 64:
        raise ValueError(f"{where}: intermediate_size {I} (the HIP GEMM takes intermediate_size % 64 == 0)")
    return (int(cfg["vocab_size"]), H, L, nq, nkv, hd, I, int(cfg.get("max_position_embeddings", 2048)), float(cfg.get("rms_norm_eps", 1e-6)),
            thetas["full_attention"], thetas["sliding_attention"], window, float(cfg.get("query_pre_attn_scalar", 256)),
            tuple(1 if t == "full_attention" else 0 for t in lt), tuple(int(d) for d in dense))


def shape_config_dict(shape) -> dict:
    """A GEMMA_SHAPES tuple -> the config.json of such a checkpoint (sliding_window as a released file holds it)."""
    if isinstance(shape, str):
        shape = GEMMA_SHAPES[shape]
    vocab, H, L, nq, nkv, hd, I, max_pos, eps, tg, tl, window, qpas, types, _ = shape
    return dict(model_type="gemma3_text", vocab_size=vocab, hidden_size=H, num_hidden_layers=L, num_attention_heads=nq, num_key_value_heads=nkv,
                head_dim=hd, intermediate_size=I, max_position_embeddings=max_pos, rms_norm_eps=eps, sliding_window=window,
                query_pre_attn_scalar=int(qpas) if float(qpas).is_integer() else qpas, hidden_activation=ACTIVATION, use_bidirectional_attention=True, attention_bias=False,
                layer_types=["full_attention" if t else "sliding_attention" for t in types],
                rope_parameters={"full_attention": {"rope_type": "default", "rope_theta": tg},
                                 "sliding_attention": {"rope_type": "default", "rope_theta": tl}},
                pad_token_id=0, eos_token_id=1, bos_token_id=2)


def shape_hf_config(shape, **extra):
    """A GEMMA_SHAPES tuple -> transformers.Gemma3TextConfig (the tests' float32 reference). The constructor turns sliding_window W
    into W // 2 + 1 for a bidirectional model: the exclusive bound of |q - k|."""
    from transformers import Gemma3TextConfig
    kw = shape_config_dict(shape)
    kw.pop("model_type")
    kw.update(extra)
    return Gemma3TextConfig(**kw)


def read_dense_modules(model_dir: str):
    """The Dense modules of a sentence-transformers directory, in modules.json order (or 2_Dense, 3_Dense when there is none):
    [(weight [out][in] float32 tensor)]. A module with a bias or an activation other than the identity is refused."""
    from safetensors.torch import load_file
    dirs = []
    mj = os.path.join(model_dir, "modules.json")
    if os.path.exists(mj):
        for m in json.load(open(mj)):
            if str(m.get("type", "")).endswith("Dense"):
                dirs.append(m["path"])
    else:
        dirs = [d for d in DENSE_DIRS if os.path.isdir(os.path.join(model_dir, d))]
    out = []
    for d in dirs:
        p = os.path.join(model_dir, d)
        cj = os.path.join(p, "config.json")
        if os.path.exists(cj):
            c = json.load(open(cj))
            if c.get("bias", False):
                raise ValueError(f"{cj}: bias is not supported (Dense modules are a weight only)")
            act = str(c.get("activation_function", "torch.nn.modules.linear.Identity"))
            if not act.endswith("Identity"):
                raise ValueError(f"{cj}: activation_function {act!r} is not supported (identity only)")
        sd = load_file(os.path.join(p, "model.safetensors"))
        if "linear.bias" in sd:
            raise ValueError(f"{p}: linear.bias is not supported (Dense modules are a weight only)")
        out.append(sd["linear.weight"].float())
    if len(out) > 2:
        raise ValueError(f"{model_dir}: {len(out)} Dense modules (at most 2)")
    return out


def load_gemma_weights(model_dir: str):
    """Local checkpoint directory (config.json + model.safetensors or shards, and the 2_Dense / 3_Dense modules when it is a
    sentence-transformers directory) -> (shape, weights in our names). A "model." prefix on the tensor names is stripped. No network."""
    cfg = json.load(open(os.path.join(model_dir, "config.json")))
    dense = read_dense_modules(model_dir)
    shape = gemma_config_shape(cfg, os.path.join(model_dir, "config.json"), dense=[d.shape[0] for d in dense])
    sd = read_safetensors_dir(model_dir)
    w = {"embed": sd["embed_tokens.weight"], "final_norm": sd["norm.weight"]}
    for l in range(shape[2]):
        for k, hf in HF_LAYER_NAMES.items():
            w[f"l{l}.{k}"] = sd[f"layers.{l}.{hf}"]
    din = shape[1]
    for i, d in enumerate(dense):
        if d.shape[1] != din:
            raise ValueError(f"{model_dir}: Dense module {i} takes {d.shape[1]} features, the model hands it {din}")
        w[f"dense{i}"] = d
        din = d.shape[0]
    return shape, w


def interleave_gate_up(w_gate: "np.ndarray", w_up: "np.ndarray") -> "np.ndarray":
    """gate_proj, up_proj [I][H] -> the row order ak_gemma_create builds for the tanh-GeGLU epilogue (gemm.hip MODE 9): row 2 j = gate
    row j (the GELU input), row 2 j + 1 = up row j."""
    out = np.empty((2 * w_gate.shape[0], w_gate.shape[1]), w_gate.dtype)
    out[0::2], out[1::2] = w_gate, w_up
    return out


def geglu_tanh_interleaved(y: "np.ndarray") -> "np.ndarray":
    """The MODE 9 epilogue restated in numpy on product rows [.., 2 I] in the interleaved order: gelu_tanh(y[2 j]) * y[2 j + 1], in
    the kernel's form a / (1 + exp(-2 u)), u = sqrt(2 / pi) (a + 0.044715 a^3)."""
    a, g = y[..., 0::2].astype(np.float64), y[..., 1::2].astype(np.float64)
    u = 0.7978845608028654 * (a + 0.044715 * a ** 3)
    return (a * g / (1.0 + np.exp(-2.0 * u))).astype(np.float32)


class HipGemma(HipStack):
    family, prefix, embed_key, matrix_keys, out_name = "Gemma", "gemma", "embed", MATRIX_KEYS, "out_dim"
    poolings, pooling_noun = ("mean",), "Gemma embedders"

    def __init__(self, shape, weights: Dict[str, "np.ndarray"], device: Optional[int] = None, dense: bool = True):
        """shape: a GEMMA_SHAPES tuple or name; weights: our names (weight_names), numpy arrays or torch tensors. dense=False leaves
        the Dense head out (the plain Gemma3 text model, mean pooled)."""
        if isinstance(shape, str):
            shape = GEMMA_SHAPES[shape]
        vocab, H, L, nq, nkv, hd, I, max_pos, eps, theta_g, theta_l, window, qpas, types, dense_out = shape
        if not dense:
            dense_out = ()
        if L > GEMMA_MAX_LAYERS or len(types) != L:
            raise ValueError(f"Gemma shape: {L} layers with {len(types)} layer types (at most {GEMMA_MAX_LAYERS} layers)")
        if len(dense_out) > 2:
            raise ValueError(f"Gemma shape: {len(dense_out)} Dense modules (at most 2)")
        self.shape = tuple(shape)
        self.hidden, self.layers, self.vocab, self.pooling = H, L, vocab, "mean"
        self.out_dim = dense_out[-1] if dense_out else H
        self.max_seq = min(int(max_pos), MAX_SEQ)
        names = weight_names(L, len(dense_out))
        self._upload(weights, names, device)
        din = H
        for i, dout in enumerate(dense_out):
            if tuple(self._tensors[f"dense{i}"].shape) != (dout, din):
                raise ValueError(f"Gemma weight dense{i}: shape {tuple(self._tensors[f'dense{i}'].shape)}, expected {(dout, din)}")
            din = dout
        self._create(AkGemmaConfig(vocab, H, L, nq, nkv, hd, I, max_pos, eps, theta_g, theta_l, float(qpas), window // 2, 0.0, 0.0, 0, 0, 0,
                                   len(dense_out), (ctypes.c_int * 2)(*(list(dense_out) + [0, 0])[:2]), (ctypes.c_int * GEMMA_MAX_LAYERS)(*types)),
                     names)
        # the rotary tables from HF's own inverse frequencies (rope_inv_freq) in place of the library's correctly rounded ones
        self._inv_freq = (rope_inv_freq(theta_g), rope_inv_freq(theta_l))
        check(self._lib.ak_gemma_set_rope_inv_freq(self._h, self._inv_freq[0].ctypes.data, self._inv_freq[1].ctypes.data), "ak_gemma_set_rope_inv_freq")
