"""CPU reference and fixtures of the Qwen2 path (archi_amd.qwen2): transformers.Qwen2Model in float32 with eager attention, the defects
the fixtures must discriminate and a sentence-transformers style checkpoint directory. Used by the qwen2 tests and by
tests/golden/make_qwen2_fixtures.py. The per-row reference loop, the tokenizer and the RoPE-dropping module are tests/llama_ref.py's.

The fixtures' numbers. Matrices at std 0.05, the value tests/llama_ref.py settled on. Biases N(0, bias_std) rounded to bf16; measured
on 2 layers at hidden 256 (HF bf16 against its float32 self | the defect "k bias dropped" on rows of 33 to 320 tokens, 1 - cos):

    bias_std 0.5    <= 2.3e-5 / 2.0e-3    1.3e-4 to 1.7e-3: at best about 5 bars of 3e-4 -- too weak
    bias_std 2.0    <= 1.4e-4 / 2.9e-3    >= 4.0e-3: 13 bars

A k bias enters the logits as q . bk, which without RoPE is the same for every key of a query (softmax-invariant): what is left is the
rotation's effect, which needs rows of 32 tokens or more, and a large bias. 2.0 is the value of every causal fixture; the q / v / swap
defects are larger still there. Under a bias of 2.0 the logits are dominated by the bias terms, which are the same with and without the
causal mask, and the causal-vs-bidirectional gap shrinks to 1e-4 .. 2e-3: the bidirectional fixtures take BIDIR_BIAS_STD = 0.5, at which
that gap is >= 10 bars on every row of 5 tokens or more (tests/test_qwen2_cpu.py holds each of these statements)."""
from __future__ import annotations

import json
import os

import numpy as np

from archi_amd.llama import HEAD_DIM
from archi_amd.qwen2 import QWEN2_SHAPES, Qwen2Shape, hf_state_dict, random_qwen2_weights
from tests.llama_ref import ABS_BAR, COS_BAR, _no_rope, make_tokenizer_json, reference  # noqa: F401 (the tests import them from here)

STD, BIAS_STD, BIDIR_BIAS_STD = 0.05, 2.0, 0.5
# name -> (shape name, seed, row lengths, std of the matrices, std of the biases): the fixtures of tests/golden/qwen2_*.npz
FIXTURES = {
    "q2-tiny-g5": ("q2-tiny-g5", 61, (320, 257, 129, 64, 33, 5, 1), STD, BIAS_STD),
    "q2-tiny-g6": ("q2-tiny-g6", 62, (320, 256, 100, 65, 32, 7, 1), STD, BIAS_STD),
    "q2-tiny-g7": ("q2-tiny-g7", 63, (320, 257, 129, 64, 33, 5, 1), STD, BIAS_STD),
    "q2-tiny-g8": ("q2-tiny-g8", 64, (320, 193, 96, 63, 34, 2, 1), STD, BIAS_STD),
    "q2-tiny-g2": ("q2-tiny-g2", 65, (320, 255, 129, 64, 33, 1), STD, BIAS_STD),
    "q2-bidir-mean": ("q2-tiny-g6", 66, (513, 512, 100, 33, 5, 1), STD, BIDIR_BIAS_STD),
    "q2-bidir-last": ("q2-tiny-g7", 67, (320, 257, 129, 64, 33, 5, 1), STD, BIDIR_BIAS_STD),
    "q2-long": ("q2-tiny-g7", 68, (8192, 300, 65), 0.04, BIAS_STD),
}
# name -> (attention, pooling) where it is not (causal, last)
MODES = {"q2-bidir-mean": ("bidirectional", "mean"), "q2-bidir-last": ("bidirectional", "last")}


def _shape(shape) -> Qwen2Shape:
    return QWEN2_SHAPES[shape] if isinstance(shape, str) else Qwen2Shape(*shape)


def hf_config(shape, dialect: str = "v5"):
    """Qwen2Config of a shape; dialect "v4" spells theta as the top-level rope_theta of transformers 4 config files."""
    from transformers import Qwen2Config
    s = _shape(shape)
    rp = {"rope_type": "default", "rope_theta": s.rope_theta}
    if s.scaling is not None:
        rp = {"rope_type": "llama3", "rope_theta": s.rope_theta, "factor": s.scaling.factor, "low_freq_factor": s.scaling.low,
              "high_freq_factor": s.scaling.high, "original_max_position_embeddings": s.scaling.original}
    return Qwen2Config(vocab_size=s.vocab, hidden_size=s.hidden, num_hidden_layers=s.layers, num_attention_heads=s.q_heads,
                       num_key_value_heads=s.kv_heads, head_dim=HEAD_DIM, intermediate_size=s.intermediate, max_position_embeddings=s.max_position,
                       rms_norm_eps=s.rms_eps, hidden_act="silu", tie_word_embeddings=False, use_sliding_window=False, rope_parameters=rp)


def hf_model(shape, weights, dtype=None):
    """float32 (or `dtype`) Qwen2Model on the CPU with eager attention holding `weights` (archi_amd.qwen2 names)."""
    import torch
    from transformers import Qwen2Model
    cfg = hf_config(shape)
    cfg._attn_implementation = "eager"
    with torch.device("meta"):
        m = Qwen2Model(cfg)
    sd = {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float32) for k, v in hf_state_dict(weights, cfg.num_hidden_layers).items()}
    m.load_state_dict(sd, assign=True, strict=True)
    m.rotary_emb = type(m.rotary_emb)(config=cfg)            # non-persistent buffer: built on the CPU, not loaded
    m = m.eval().float()
    return m.to(dtype) if dtype is not None else m


def fixture_weights(name):
    """The seeded weights of a fixture; the mean-pooled one scales each embedding row by a seeded power of two, as
    llama_ref.fixture_weights does and for its reason."""
    shape, seed, _, std, bias_std = FIXTURES[name]
    w = random_qwen2_weights(shape, seed=seed, std=std, bias_std=bias_std)
    if MODES.get(name, ("causal", "last"))[1] == "mean":
        f = 2.0 ** np.random.default_rng(seed + 1000).integers(0, 7, w["embed_tokens"].shape[0])
        w["embed_tokens"] = (w["embed_tokens"] * f[:, None]).astype(np.float32)
    return w


def fixture_inputs(name):
    """(shape name, seed, ids [B][W] int32 zero padded, lens [B], std, bias_std) of a fixture: seeded ids."""
    shape, seed, lens, std, bias_std = FIXTURES[name]
    rng = np.random.default_rng(seed)
    lens = np.array(lens, np.int32)
    ids = np.zeros((len(lens), int(lens.max())), np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.integers(0, QWEN2_SHAPES[shape].vocab, n)
    return shape, seed, ids, lens, std, bias_std


def defect_model(shape, weights, defect: str):
    """The float32 HF model of `shape` with one defect: noqbias | nokbias | novbias (the bias dropped) | swapkv (the k and v biases
    exchanged) | norope."""
    w = dict(weights)
    for l in range(_shape(shape).layers):
        p = f"l{l}."
        if defect in ("noqbias", "nokbias", "novbias"):
            w[p + "b" + defect[2]] = np.zeros_like(w[p + "b" + defect[2]])
        elif defect == "swapkv":
            w[p + "bk"], w[p + "bv"] = w[p + "bv"], w[p + "bk"]
    m = hf_model(shape, w)
    if defect == "norope":
        m.rotary_emb = _no_rope(m.rotary_emb)
    return m


def write_checkpoint(model_dir: str, shape, weights, max_seq_length: int = 512, pooling: str = "lasttoken", normalize: bool = True,
                     is_causal=None) -> str:
    """A gte-Qwen2 style directory: save_pretrained (config.json in transformers' dialect + model.safetensors with the bias tensors),
    tokenizer.json, modules.json, 1_Pooling, 2_Normalize, sentence_bert_config.json. is_causal: written into config.json when given."""
    os.makedirs(model_dir, exist_ok=True)
    hf_model(shape, weights).save_pretrained(model_dir)
    if is_causal is not None:
        cj = os.path.join(model_dir, "config.json")
        cfg = json.load(open(cj))
        cfg["is_causal"] = bool(is_causal)
        json.dump(cfg, open(cj, "w"))
    make_tokenizer_json(os.path.join(model_dir, "tokenizer.json"))
    mods = [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
            {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"}]
    if normalize:
        mods.append({"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"})
        os.makedirs(os.path.join(model_dir, "2_Normalize"), exist_ok=True)
    json.dump(mods, open(os.path.join(model_dir, "modules.json"), "w"))
    os.makedirs(os.path.join(model_dir, "1_Pooling"), exist_ok=True)
    pc = {"word_embedding_dimension": int(weights["norm"].shape[0]), "include_prompt": True}
    for k in ("cls_token", "mean_tokens", "max_tokens", "mean_sqrt_len_tokens", "weightedmean_tokens", "lasttoken"):
        pc["pooling_mode_" + k] = k == pooling
    json.dump(pc, open(os.path.join(model_dir, "1_Pooling", "config.json"), "w"))
    json.dump({"max_seq_length": max_seq_length, "do_lower_case": False}, open(os.path.join(model_dir, "sentence_bert_config.json"), "w"))
    return model_dir
