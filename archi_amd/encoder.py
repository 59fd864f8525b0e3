"""HipEncoder -- Python handle of the HIP BERT encoder (ak_encoder_*).

PyTorch-ROCm only HOLDS the weights in HBM (bf16 matrices, fp32 vectors) and hands raw device
pointers to the C ABI; every arithmetic step of the forward pass runs in hand-written HIP kernels
(archi_amd/csrc/encoder.hip, gemm.hip, attention.hip).
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np

from . import _lib
from ._lib import POOLING, AkBertConfig, HipBackendError, check

# name -> (vocab, hidden, layers, heads, intermediate, max_position, pooling, max_seq_length)
MODEL_SHAPES = {
    "sentence-transformers/all-MiniLM-L6-v2": (30522, 384, 6, 12, 1536, 512, "mean", 256),
    "all-MiniLM-L6-v2": (30522, 384, 6, 12, 1536, 512, "mean", 256),
    "BAAI/bge-base-en": (30522, 768, 12, 12, 3072, 512, "cls", 512),
    "BAAI/bge-base-en-v1.5": (30522, 768, 12, 12, 3072, 512, "cls", 512),
}

# MPNet (sentence-transformers/all-mpnet-base-v2 and its family): name -> (vocab, hidden, layers, heads, intermediate,
# max_position_embeddings, pooling, max_seq_length) as in their config.json / sentence-transformers files. Not in MODEL_SHAPES:
# other code indexes that table as BERT.
MPNET_SHAPES = {
    "sentence-transformers/all-mpnet-base-v2": (30527, 768, 12, 12, 3072, 514, "mean", 384),
    "all-mpnet-base-v2": (30527, 768, 12, 12, 3072, 514, "mean", 384),
    "sentence-transformers/multi-qa-mpnet-base-dot-v1": (30527, 768, 12, 12, 3072, 514, "cls", 512),
    "sentence-transformers/paraphrase-mpnet-base-v2": (30527, 768, 12, 12, 3072, 514, "mean", 512),
    # small shapes of the test fixtures (tests/golden/make_mpnet_fixtures.py): head size 64 (a 2-layer cut of the 768 shape) and 32
    "mpnet-cut2": (30527, 768, 2, 12, 3072, 514, "mean", 512),
    "mpnet-tiny-hd32": (1000, 256, 2, 8, 512, 514, "mean", 512),
}
MPNET_PADDING_IDX = 1           # MPNetEmbeddings.padding_idx: token p of a row sits at position padding_idx + 1 + p
MPNET_NUM_BUCKETS = 32          # MPNetEncoder.compute_position_bias buckets with its default, whatever the config holds
MPNET_MAX_DISTANCE = 128

# XLM-RoBERTa (bge-m3, multilingual-e5, paraphrase-multilingual-mpnet-base-v2): name -> (vocab, hidden, layers, heads, intermediate,
# max_position_embeddings, pooling, max_seq_length) from their published config.json / sentence-transformers files (not checked
# offline; they only shape synthetic benchmarks). Not in MODEL_SHAPES: other code indexes that table as BERT.
XLMR_SHAPES = {
    "BAAI/bge-m3": (250002, 1024, 24, 16, 4096, 8194, "cls", 8192),
    "intfloat/multilingual-e5-large": (250002, 1024, 24, 16, 4096, 514, "mean", 512),
    "intfloat/multilingual-e5-base": (250002, 768, 12, 12, 3072, 514, "mean", 512),
    "sentence-transformers/paraphrase-multilingual-mpnet-base-v2": (250002, 768, 12, 12, 3072, 514, "mean", 128),
    # small shapes of the test fixtures (tests/golden/make_xlmr_fixtures.py): head size 64 and 32, a two-layer cut of the hidden-1024
    # shape, and a head-size-64 shape with bge-m3's 8194-row position table
    "xlmr-tiny-hd64": (1000, 256, 2, 4, 512, 514, "mean", 512),
    "xlmr-tiny-hd32": (1000, 256, 2, 8, 512, 514, "mean", 512),
    "xlmr-1024-cut2": (1000, 1024, 2, 16, 4096, 514, "cls", 512),
    "xlmr-long-hd64": (1000, 256, 2, 4, 512, 8194, "cls", 8192),
}
XLMR_PADDING_IDX = 1            # XLM-R's pad id = the position embedding's padding_idx

LAYER_KEYS = ("wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo", "ln1_g", "ln1_b", "w1", "b1", "w2", "b2", "ln2_g", "ln2_b")
MATRIX_KEYS = {"wq", "wk", "wv", "wo", "w1", "w2"}


def weight_order(layers: int):
    names = ["word_emb", "pos_emb", "type_emb", "emb_ln_g", "emb_ln_b"]
    for l in range(layers):
        names += [f"l{l}.{k}" for k in LAYER_KEYS]
    return names


PRECISIONS = {"bf16": 0, "f32": 1, "bf16x3": 2}        # AkBertConfig.precision
LONG_MAX_SEQ = 8192                                     # longest row of an encoder with positions from ids (csrc/attn_long.hip)


def long_rows_supported(hidden: int, heads: int, precision: str) -> bool:
    """Rows longer than 512 tokens (positions from ids): bf16, head size 64, hidden != 384 (ak_encoder_set_positions_from_ids)."""
    return precision == "bf16" and hidden == 64 * heads and hidden != 384


class HipEncoder:
    def __init__(self, vocab: int, hidden: int, layers: int, heads: int, intermediate: int, max_position: int,
                 weights: Dict[str, np.ndarray], ln_eps: float = 1e-12, device: Optional[int] = None,
                 residual: str = "bf16", precision: str = "bf16", rel_bias=None, positions_from_ids: Optional[int] = None):
        """residual: "bf16" keeps the residual stream between layers in bf16 only (hidden size 384: 60% less epilogue
        traffic; adds ~1e-6 of cosine deviation from the fp32 reference to the ~2e-6 the bf16 GEMM inputs already
        cost); "f32" keeps it in fp32 like the reference's CPU path. ARCHI_ENCODER_RESIDUAL overrides.
        precision: "bf16" = the measured MFMA path; "f32" = parity mode: float32 weights and arithmetic throughout, on
        v_mfma_f32_32x32x2_f32 (~1e-6 from the reference's torch-fp32 CPU embedder, ~1/9 of the bf16 rate); "bf16x3" = split-bf16
        parity mode: float32 weights, every GEMM operand split x = hi + lo into two bf16 values and every product run as
        hi.hi + lo.hi + hi.lo on the bf16 matrix cores with one float32 accumulator, everything between the GEMMs in float32
        (~1e-6 per component from float64, scores within 1e-5 of the CPU path, ~3x the "f32" mode's rate).
        rel_bias: an additive relative-position bias [heads][2 n_rel - 1] (distance key - query at column d + n_rel - 1, natural-log
        domain; MPNet: mpnet_rel_bias_table) added to every attention score (ak_encoder_set_rel_bias); sequences are then limited
        to n_rel tokens. None: no bias.
        positions_from_ids: RoBERTa / XLM-R positions (ak_encoder_set_positions_from_ids) with this padding_idx: weights["pos_emb"]
        is then the full position table and sequences are limited to max_position - padding_idx - 1 tokens, at most 8192
        (long_rows_supported) and 512 otherwise. None: a token's position is its index in the row."""
        import os
        import torch
        residual = os.environ.get("ARCHI_ENCODER_RESIDUAL", residual)
        if residual not in ("bf16", "f32"):
            raise ValueError("residual must be 'bf16' or 'f32'")
        self.residual = residual
        if precision not in PRECISIONS:
            raise ValueError("precision must be 'bf16', 'f32' or 'bf16x3'")
        self.precision = precision
        self._lib = _lib.init(device)
        self.hidden, self.layers, self.max_position, self.vocab = hidden, layers, max_position, vocab
        dev = torch.device("cuda", _lib.bound_device())      # the library's device, not torch's per-thread default
        self._tensors = []   # keeps the device memory alive
        ptrs = []
        for name in weight_order(layers):
            if name not in weights:
                raise HipBackendError(f"encoder weight {name!r} missing")
            arr = weights[name]
            t = arr if isinstance(arr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(arr))
            is_matrix = name in ("word_emb", "pos_emb", "type_emb") or name.split(".")[-1] in MATRIX_KEYS
            t = t.to(device=dev, dtype=torch.bfloat16 if (is_matrix and precision == "bf16") else torch.float32).contiguous()
            self._tensors.append(t)
            ptrs.append(t.data_ptr())
        type_vocab = int(weights["type_emb"].shape[0]) if weights["type_emb"].ndim == 2 else 2     # MPNet: one zero row
        cfg = AkBertConfig(vocab, hidden, layers, heads, intermediate, max_position, type_vocab, ln_eps, int(residual == "bf16"),
                           PRECISIONS[precision])
        arr_t = ctypes.c_void_p * len(ptrs)
        h = ctypes.c_void_p()
        torch.cuda.synchronize(dev)
        check(self._lib.ak_encoder_create(ctypes.byref(cfg), arr_t(*ptrs), len(ptrs), ctypes.byref(h)),
              "ak_encoder_create")
        self._h = h
        self._dev = dev
        if rel_bias is not None:
            # [heads][2 n_rel - 1] float32 per-distance table (mpnet_rel_bias_table): the library copies it
            rb = rel_bias if isinstance(rel_bias, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rel_bias))
            rb = rb.to(device=dev, dtype=torch.float32).contiguous()
            if rb.dim() != 2 or rb.shape[0] != heads or rb.shape[1] % 2 == 0:
                self.close()
                raise ValueError("rel_bias must be [heads][2 n_rel - 1]")
            torch.cuda.synchronize(dev)
            check(self._lib.ak_encoder_set_rel_bias(self._h, ctypes.c_void_p(rb.data_ptr()), heads, (rb.shape[1] + 1) // 2),
                  "ak_encoder_set_rel_bias")
        self.rel_bias = rel_bias is not None
        self.positions_from_ids = positions_from_ids
        self.max_seq = 512
        if positions_from_ids is not None:
            cap = LONG_MAX_SEQ if long_rows_supported(hidden, heads, precision) else 512
            max_seq = self.max_seq = min(max_position - int(positions_from_ids) - 1, cap)
            check(self._lib.ak_encoder_set_positions_from_ids(self._h, int(positions_from_ids), max_seq),
                  "ak_encoder_set_positions_from_ids")

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.ak_encoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward(self, ids, mask, pooling: str = "mean", normalise: bool = True):
        """ids, mask: [B,S] integer arrays/tensors. Returns a [B,hidden] float32 CUDA tensor."""
        import torch
        ids_t = torch.as_tensor(ids, dtype=torch.int32, device=self._dev)
        mask_t = torch.as_tensor(mask, dtype=torch.int32, device=self._dev)
        B, S = ids_t.shape
        if S > self.max_position or S > self.max_seq:
            raise ValueError(f"sequence length {S} exceeds the encoder limit")
        Sp = (S + 31) // 32 * 32
        if Sp != S:   # pad with masked tokens (attention ignores them, pooling skips them)
            ids_t = torch.nn.functional.pad(ids_t, (0, Sp - S))
            mask_t = torch.nn.functional.pad(mask_t, (0, Sp - S))
        ids_t, mask_t = ids_t.contiguous(), mask_t.contiguous()
        out = torch.empty((B, self.hidden), dtype=torch.float32, device=self._dev)
        check(self._lib.ak_encoder_forward(self._h, ctypes.c_void_p(ids_t.data_ptr()),
                                           ctypes.c_void_p(mask_t.data_ptr()), B, Sp, POOLING[pooling],
                                           int(normalise), ctypes.c_void_p(out.data_ptr()),
                                           ctypes.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream)),
              "ak_encoder_forward")
        return out


    def forward_lens(self, stage, n_rows: int, S: int, out, pooling: str = "mean", normalise: bool = True) -> None:
        """Right-padded rows given by their lengths (ak_encoder_forward_lens): `stage` is an int32 CUDA tensor [n_rows, S + 1] --
        S token ids per row, the row's length in column S (the provider's tile layout) --, `out` a float32 CUDA tensor view
        [n_rows, hidden] inside the caller's result buffer. No torch kernel runs: the library lays the mask out itself."""
        import torch
        if stage.dtype != torch.int32 or not stage.is_cuda or not stage.is_contiguous() or tuple(stage.shape) != (n_rows, S + 1):
            raise ValueError("forward_lens: stage must be a contiguous int32 CUDA tensor [n_rows, S + 1]")
        if out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (n_rows, self.hidden):
            raise ValueError("forward_lens: out must be a contiguous float32 CUDA tensor [n_rows, hidden]")
        if S % 32 or S > self.max_position or S > self.max_seq:
            raise ValueError(f"sequence length {S} must be a multiple of 32 within the encoder limit")
        base = stage.data_ptr()
        check(self._lib.ak_encoder_forward_lens(self._h, ctypes.c_void_p(base), S + 1, ctypes.c_void_p(base + 4 * S), S + 1, n_rows, S,
                                                POOLING[pooling], int(normalise), ctypes.c_void_p(out.data_ptr()),
                                                ctypes.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream)),
              "ak_encoder_forward_lens")


def random_init_weights(vocab, hidden, layers, intermediate, max_position, seed: int = 0) -> Dict[str, "np.ndarray"]:
    """Seeded random-init weights of a given architecture (benchmarks: no checkpoints exist offline). LayerNorm weights are drawn
    around (1, 0), not set to it: a trained checkpoint's are not trivial either, and paths that fold the LayerNorm into their
    neighbours (csrc/gemm.hip, lazy LayerNorm) would be measured and checked on a degenerate case otherwise."""
    import torch
    g = torch.Generator().manual_seed(seed)
    w = {}

    def mat(r, c, std=0.02):
        return (torch.randn(r, c, generator=g) * std).numpy()

    w["word_emb"], w["pos_emb"], w["type_emb"] = mat(vocab, hidden), mat(max_position, hidden), mat(2, hidden)
    def ln():
        return ((1.0 + 0.1 * torch.randn(hidden, generator=g)).numpy().astype(np.float32),
                (0.1 * torch.randn(hidden, generator=g)).numpy().astype(np.float32))

    w["emb_ln_g"], w["emb_ln_b"] = ln()
    for l in range(layers):
        p = f"l{l}."
        for k, (r, c) in (("wq", (hidden, hidden)), ("wk", (hidden, hidden)), ("wv", (hidden, hidden)),
                          ("wo", (hidden, hidden)), ("w1", (intermediate, hidden)), ("w2", (hidden, intermediate))):
            w[p + k] = mat(r, c)
        for k, d in (("bq", hidden), ("bk", hidden), ("bv", hidden), ("bo", hidden), ("b1", intermediate), ("b2", hidden)):
            w[p + k] = (torch.randn(d, generator=g) * 0.02).numpy()
        for k in ("ln1", "ln2"):
            w[p + k + "_g"], w[p + k + "_b"] = ln()
    return w


def load_hf_weights(model_dir: str):
    """Load a local HF BERT checkpoint directory (config.json + model.safetensors | pytorch_model.bin). No network.
    Anything the HIP encoder does not implement (non-BERT, non-GELU, relative positions) is refused here."""
    import json
    import os
    cfg = json.load(open(os.path.join(model_dir, "config.json")))
    if cfg.get("model_type", "bert") != "bert":
        raise ValueError(f"{model_dir}: model_type {cfg.get('model_type')!r} is not BERT")
    if cfg.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"{model_dir}: hidden_act {cfg.get('hidden_act')!r} (the HIP encoder implements erf GELU)")
    if cfg.get("position_embedding_type", "absolute") != "absolute":
        raise ValueError(f"{model_dir}: position_embedding_type {cfg.get('position_embedding_type')!r} is not supported")
    st, pt = os.path.join(model_dir, "model.safetensors"), os.path.join(model_dir, "pytorch_model.bin")
    if os.path.exists(st):
        from safetensors.torch import load_file     # torch loader: checkpoints stored in f16/bf16 load too
        sd = load_file(st)
    elif os.path.exists(pt):
        import torch
        sd = torch.load(pt, map_location="cpu", weights_only=True)
    else:
        raise FileNotFoundError(f"{model_dir}: neither model.safetensors nor pytorch_model.bin")
    sd = {(k[5:] if k.startswith("bert.") else k): v.float() for k, v in sd.items()}
    L = cfg["num_hidden_layers"]
    w = {"word_emb": sd["embeddings.word_embeddings.weight"], "pos_emb": sd["embeddings.position_embeddings.weight"],
         "type_emb": sd["embeddings.token_type_embeddings.weight"], "emb_ln_g": sd["embeddings.LayerNorm.weight"],
         "emb_ln_b": sd["embeddings.LayerNorm.bias"]}
    for l in range(L):
        p, q = f"encoder.layer.{l}.", f"l{l}."
        for hf, m in (("attention.self.query", "q"), ("attention.self.key", "k"), ("attention.self.value", "v")):
            w[q + "w" + m], w[q + "b" + m] = sd[p + hf + ".weight"], sd[p + hf + ".bias"]
        w[q + "wo"], w[q + "bo"] = sd[p + "attention.output.dense.weight"], sd[p + "attention.output.dense.bias"]
        w[q + "ln1_g"], w[q + "ln1_b"] = sd[p + "attention.output.LayerNorm.weight"], sd[p + "attention.output.LayerNorm.bias"]
        w[q + "w1"], w[q + "b1"] = sd[p + "intermediate.dense.weight"], sd[p + "intermediate.dense.bias"]
        w[q + "w2"], w[q + "b2"] = sd[p + "output.dense.weight"], sd[p + "output.dense.bias"]
        w[q + "ln2_g"], w[q + "ln2_b"] = sd[p + "output.LayerNorm.weight"], sd[p + "output.LayerNorm.bias"]
    shape = (cfg["vocab_size"], cfg["hidden_size"], L, cfg["num_attention_heads"], cfg["intermediate_size"],
             cfg["max_position_embeddings"])
    return shape, w, float(cfg.get("layer_norm_eps", 1e-12))


def read_sentence_transformers_config(model_dir: str):
    """What SentenceTransformer(model_dir) -- the engine under the reference's HuggingFaceEmbeddings [upstream] --
    reads beside the BERT weights: `modules.json` (is there a Normalize module), `1_Pooling/config.json`
    (cls | mean) and `sentence_bert_config.json` (max_seq_length). A plain HF directory without them gets
    sentence-transformers' defaults: mean pooling, no Normalize module, max_seq_length None (= the model limit).
    Returns (pooling, max_seq_length | None, always_normalise)."""
    import json
    import os
    pooling, max_len, norm = "mean", None, False
    mj = os.path.join(model_dir, "modules.json")
    pool_dir = "1_Pooling"
    if os.path.exists(mj):
        for m in json.load(open(mj)):
            kind = m.get("type", "")
            if kind.endswith("Normalize"):
                norm = True
            elif kind.endswith("Pooling"):
                pool_dir = m.get("path", pool_dir)
    pj = os.path.join(model_dir, pool_dir, "config.json")
    if os.path.exists(pj):
        pc = json.load(open(pj))
        modes = [k for k in ("cls_token", "mean_tokens", "max_tokens", "mean_sqrt_len_tokens", "weightedmean_tokens",
                             "lasttoken") if pc.get("pooling_mode_" + k)]
        if modes == ["cls_token"]:
            pooling = "cls"
        elif modes != ["mean_tokens"]:
            raise ValueError(f"{model_dir}: pooling modes {modes} (the HIP encoder implements cls and mean)")
    sj = os.path.join(model_dir, "sentence_bert_config.json")
    if os.path.exists(sj):
        max_len = json.load(open(sj)).get("max_seq_length")
    return pooling, max_len, norm


def mpnet_relative_position_bucket(relative_position, num_buckets: int = MPNET_NUM_BUCKETS, max_distance: int = MPNET_MAX_DISTANCE):
    """MPNetEncoder.relative_position_bucket restated with the same torch ops (T5-style, bidirectional; the float32 log decides
    the large buckets, so the ops are kept as they are)."""
    import math
    import torch
    ret = 0
    n = -relative_position
    num_buckets //= 2
    ret += (n < 0).to(torch.long) * num_buckets
    n = torch.abs(n)
    max_exact = num_buckets // 2
    is_small = n < max_exact
    val_if_large = max_exact + (
        torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)).to(torch.long)
    val_if_large = torch.min(val_if_large, torch.full_like(val_if_large, num_buckets - 1))
    ret += torch.where(is_small, n, val_if_large)
    return ret


def mpnet_rel_bias_table(weight, n_rel: int) -> "np.ndarray":
    """encoder.relative_attention_bias.weight [buckets][heads] -> the per-distance table [heads][2 n_rel - 1] float32 that
    ak_encoder_set_rel_bias takes: column d + n_rel - 1 holds the bias HF adds for key - query = d."""
    import torch
    w = weight if isinstance(weight, torch.Tensor) else torch.from_numpy(np.asarray(weight))
    d = torch.arange(-(n_rel - 1), n_rel, dtype=torch.long)
    bucket = mpnet_relative_position_bucket(d)
    return w.float()[bucket].t().contiguous().numpy()


def random_mpnet_weights(shape, seed: int = 0):
    """Seeded random weights of an MPNet shape (an MPNET_SHAPES name or tuple) -> (encoder weight dict in the header's order with
    MPNet's positions already offset, relative_attention_bias [32][heads], the raw position table [max_position_embeddings][H]).
    Matrices are ROUNDED TO bf16 (kept as float32): a float32 reference on the same values then measures the kernels' activation
    rounding alone. The relative-bias weights are drawn with std 1, not HF's 0.02, and the attention projections with std 0.06
    (three times the rest): the bias must visibly move the output, or a kernel that dropped it would pass -- with every matrix at
    0.02 the attention sub-layer is a small share of the residual stream and the bias moves the embeddings by ~1.5x the bf16 bar."""
    import torch
    if isinstance(shape, str):
        shape = MPNET_SHAPES[shape]
    vocab, H, L, heads, I, max_pos = shape[:6]
    w = random_init_weights(vocab, H, L, I, max_pos, seed=seed)
    g = torch.Generator().manual_seed(seed + 7919)
    for k, v in list(w.items()):
        if k.split(".")[-1] in ("wq", "wk", "wv", "wo"):
            v = v * 3.0
        if k in ("word_emb", "pos_emb") or k.split(".")[-1] in MATRIX_KEYS:
            w[k] = torch.from_numpy(v).to(torch.bfloat16).float().numpy()
    pos_full = w["pos_emb"]
    rel = torch.randn(MPNET_NUM_BUCKETS, heads, generator=g).numpy().astype(np.float32)
    return mpnet_encoder_weights(w, pos_full), rel, pos_full


def mpnet_encoder_weights(w, pos_full):
    """MPNet's embeddings as the BERT encoder takes them: positions offset by padding_idx + 1 rows, one zero token-type row."""
    w = dict(w)
    w["pos_emb"] = pos_full[MPNET_PADDING_IDX + 1:]
    w["type_emb"] = np.zeros((1, pos_full.shape[1]), np.float32)
    return w


def mpnet_hf_state_dict(w, rel, pos_full, layers: int):
    """Our weight names (mpnet_encoder_weights form) -> HF MPNetModel's state dict (no "mpnet." prefix)."""
    import torch
    t = lambda x: torch.as_tensor(np.asarray(x, np.float32))
    sd = {"embeddings.word_embeddings.weight": t(w["word_emb"]), "embeddings.position_embeddings.weight": t(pos_full),
          "embeddings.LayerNorm.weight": t(w["emb_ln_g"]), "embeddings.LayerNorm.bias": t(w["emb_ln_b"]),
          "encoder.relative_attention_bias.weight": t(rel)}
    for l in range(layers):
        p, q = f"encoder.layer.{l}.", f"l{l}."
        for hf, m in MPNET_LAYER_NAMES:
            sd[p + hf] = t(w[q + m])
    return sd


# HF MPNetLayer names (under encoder.layer.{l}.) -> ours
MPNET_LAYER_NAMES = (("attention.attn.q.weight", "wq"), ("attention.attn.q.bias", "bq"), ("attention.attn.k.weight", "wk"),
                     ("attention.attn.k.bias", "bk"), ("attention.attn.v.weight", "wv"), ("attention.attn.v.bias", "bv"),
                     ("attention.attn.o.weight", "wo"), ("attention.attn.o.bias", "bo"),
                     ("attention.LayerNorm.weight", "ln1_g"), ("attention.LayerNorm.bias", "ln1_b"),
                     ("intermediate.dense.weight", "w1"), ("intermediate.dense.bias", "b1"),
                     ("output.dense.weight", "w2"), ("output.dense.bias", "b2"),
                     ("output.LayerNorm.weight", "ln2_g"), ("output.LayerNorm.bias", "ln2_b"))


def load_mpnet_weights(model_dir: str):
    """Load a local HF MPNet checkpoint directory (config.json model_type "mpnet" + model.safetensors | pytorch_model.bin; an
    "mpnet." prefix on the names is stripped). No network. Returns (shape, weights, rel_weight, eps): shape as load_hf_weights'
    with max_position the positions a row may use (max_position_embeddings - padding_idx - 1), weights in the encoder's order with
    the positions offset and one zero token-type row, rel_weight encoder.relative_attention_bias.weight [buckets][heads]. What the
    HIP encoder does not implement is refused with ValueError."""
    import json
    import os
    cfg = json.load(open(os.path.join(model_dir, "config.json")))
    if cfg.get("model_type") != "mpnet":
        raise ValueError(f"{model_dir}: model_type {cfg.get('model_type')!r} is not MPNet")
    if cfg.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"{model_dir}: hidden_act {cfg.get('hidden_act')!r} (the HIP encoder implements erf GELU)")
    H, heads = cfg["hidden_size"], cfg["num_attention_heads"]
    if H % heads or H // heads not in (32, 64):
        raise ValueError(f"{model_dir}: head size {H / heads:g} (the HIP encoder implements 32 and 64)")
    if int(cfg.get("relative_attention_num_buckets", 32)) < MPNET_NUM_BUCKETS:
        raise ValueError(f"{model_dir}: relative_attention_num_buckets {cfg.get('relative_attention_num_buckets')} < 32 "
                         "(MPNet's position bias indexes 32 buckets)")
    max_pos = int(cfg["max_position_embeddings"]) - MPNET_PADDING_IDX - 1
    if max_pos < 32:
        raise ValueError(f"{model_dir}: max_position_embeddings {cfg['max_position_embeddings']} leaves fewer than 32 positions")
    st, pt = os.path.join(model_dir, "model.safetensors"), os.path.join(model_dir, "pytorch_model.bin")
    if os.path.exists(st):
        from safetensors.torch import load_file
        sd = load_file(st)
    elif os.path.exists(pt):
        import torch
        sd = torch.load(pt, map_location="cpu", weights_only=True)
    else:
        raise FileNotFoundError(f"{model_dir}: neither model.safetensors nor pytorch_model.bin")
    sd = {(k[6:] if k.startswith("mpnet.") else k): v.float() for k, v in sd.items()}
    L = cfg["num_hidden_layers"]
    pos_full = sd["embeddings.position_embeddings.weight"].numpy()
    w = {"word_emb": sd["embeddings.word_embeddings.weight"], "pos_emb": pos_full,
         "emb_ln_g": sd["embeddings.LayerNorm.weight"], "emb_ln_b": sd["embeddings.LayerNorm.bias"]}
    for l in range(L):
        p, q = f"encoder.layer.{l}.", f"l{l}."
        for hf, m in MPNET_LAYER_NAMES:
            w[q + m] = sd[p + hf]
    w = mpnet_encoder_weights(w, pos_full)
    shape = (cfg["vocab_size"], H, L, heads, cfg["intermediate_size"], min(max_pos, 512))
    return shape, w, sd["encoder.relative_attention_bias.weight"], float(cfg.get("layer_norm_eps", 1e-12))


# HF XLMRobertaLayer / BertLayer names (under encoder.layer.{l}.) -> ours
XLMR_LAYER_NAMES = (("attention.self.query.weight", "wq"), ("attention.self.query.bias", "bq"),
                    ("attention.self.key.weight", "wk"), ("attention.self.key.bias", "bk"),
                    ("attention.self.value.weight", "wv"), ("attention.self.value.bias", "bv"),
                    ("attention.output.dense.weight", "wo"), ("attention.output.dense.bias", "bo"),
                    ("attention.output.LayerNorm.weight", "ln1_g"), ("attention.output.LayerNorm.bias", "ln1_b"),
                    ("intermediate.dense.weight", "w1"), ("intermediate.dense.bias", "b1"),
                    ("output.dense.weight", "w2"), ("output.dense.bias", "b2"),
                    ("output.LayerNorm.weight", "ln2_g"), ("output.LayerNorm.bias", "ln2_b"))


def load_xlmr_weights(model_dir: str):
    """Load a local HF XLM-RoBERTa / RoBERTa checkpoint directory (config.json model_type "xlm-roberta" | "roberta" +
    model.safetensors | pytorch_model.bin; a "roberta." or "model." prefix on the names is stripped). No network. Returns
    (shape, weights, eps, padding_idx): shape as load_hf_weights' with max_position = max_position_embeddings (the FULL position table,
    padding_idx row included: the encoder takes its positions from the ids, ak_encoder_set_positions_from_ids), weights in the
    encoder's order with the model's own token-type row. What the HIP encoder does not implement is refused with ValueError."""
    import json
    import os
    cfg = json.load(open(os.path.join(model_dir, "config.json")))
    if cfg.get("model_type") not in ("xlm-roberta", "roberta"):
        raise ValueError(f"{model_dir}: model_type {cfg.get('model_type')!r} is not XLM-RoBERTa / RoBERTa")
    if cfg.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"{model_dir}: hidden_act {cfg.get('hidden_act')!r} (the HIP encoder implements erf GELU)")
    if cfg.get("position_embedding_type", "absolute") != "absolute":
        raise ValueError(f"{model_dir}: position_embedding_type {cfg.get('position_embedding_type')!r} is not supported")
    H, heads = cfg["hidden_size"], cfg["num_attention_heads"]
    if H > 1024:
        raise ValueError(f"{model_dir}: hidden_size {H} (the HIP encoder implements hidden <= 1024)")
    if H % heads or H // heads not in (32, 64):
        raise ValueError(f"{model_dir}: head size {H / heads:g} (the HIP encoder implements 32 and 64)")
    pad = int(cfg.get("pad_token_id", XLMR_PADDING_IDX))
    max_pos = int(cfg["max_position_embeddings"])
    if max_pos - pad - 1 < 32:
        raise ValueError(f"{model_dir}: max_position_embeddings {max_pos} leaves fewer than 32 positions")
    st, pt = os.path.join(model_dir, "model.safetensors"), os.path.join(model_dir, "pytorch_model.bin")
    if os.path.exists(st):
        from safetensors.torch import load_file
        sd = load_file(st)
    elif os.path.exists(pt):
        import torch
        sd = torch.load(pt, map_location="cpu", weights_only=True)
    else:
        raise FileNotFoundError(f"{model_dir}: neither model.safetensors nor pytorch_model.bin")
    strip = lambda k: k[8:] if k.startswith("roberta.") else (k[6:] if k.startswith("model.") else k)
    sd = {strip(k): v.float() for k, v in sd.items()}
    L = cfg["num_hidden_layers"]
    w = {"word_emb": sd["embeddings.word_embeddings.weight"], "pos_emb": sd["embeddings.position_embeddings.weight"],
         "type_emb": sd["embeddings.token_type_embeddings.weight"][:1], "emb_ln_g": sd["embeddings.LayerNorm.weight"],
         "emb_ln_b": sd["embeddings.LayerNorm.bias"]}
    for l in range(L):
        p, q = f"encoder.layer.{l}.", f"l{l}."
        for hf, m in XLMR_LAYER_NAMES:
            w[q + m] = sd[p + hf]
    shape = (cfg["vocab_size"], H, L, heads, cfg["intermediate_size"], max_pos)
    return shape, w, float(cfg.get("layer_norm_eps", 1e-5)), pad


def random_xlmr_weights(shape, seed: int = 0):
    """Seeded random weights of an XLM-R shape (an XLMR_SHAPES name or tuple) in the encoder's order: the full position table
    [max_position_embeddings][H] and ONE non-zero token-type row (XLM-R's type_vocab_size is 1 and its row is trained). Matrices are
    ROUNDED TO bf16 (kept as float32), so a float32 reference on the same values measures the kernels' activation rounding alone.
    The position table is drawn with std 0.1 and the attention projections with std 0.06 (five and three times the rest): which
    position a token gets must visibly move the output, or a kernel that ignored the positions pass would pass."""
    import torch
    if isinstance(shape, str):
        shape = XLMR_SHAPES[shape]
    vocab, H, L, heads, I, max_pos = shape[:6]
    w = random_init_weights(vocab, H, L, I, max_pos, seed=seed)
    w["type_emb"] = w["type_emb"][:1]
    w["pos_emb"] = w["pos_emb"] * 5.0
    for k, v in list(w.items()):
        if k.split(".")[-1] in ("wq", "wk", "wv", "wo"):
            w[k] = v = v * 3.0
        if k in ("word_emb", "pos_emb", "type_emb") or k.split(".")[-1] in MATRIX_KEYS:
            w[k] = torch.from_numpy(v).to(torch.bfloat16).float().numpy()
    return w


def xlmr_hf_state_dict(w, layers: int):
    """Our weight names (random_xlmr_weights form) -> HF XLMRobertaModel's state dict (no "roberta." prefix)."""
    import torch
    t = lambda x: torch.as_tensor(np.asarray(x, np.float32))
    sd = {"embeddings.word_embeddings.weight": t(w["word_emb"]), "embeddings.position_embeddings.weight": t(w["pos_emb"]),
          "embeddings.token_type_embeddings.weight": t(w["type_emb"]), "embeddings.LayerNorm.weight": t(w["emb_ln_g"]),
          "embeddings.LayerNorm.bias": t(w["emb_ln_b"])}
    for l in range(layers):
        p, q = f"encoder.layer.{l}.", f"l{l}."
        for hf, m in XLMR_LAYER_NAMES:
            sd[p + hf] = t(w[q + m])
    return sd
