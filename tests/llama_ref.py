"""CPU reference and fixtures of the Mistral / Llama path (archi_amd.llama): transformers.MistralModel / LlamaModel in float32 with eager
attention, the defects the fixtures must discriminate, a small BPE tokenizer.json and a sentence-transformers style checkpoint directory.
Used by the llama tests and by tests/golden/make_llama_fixtures.py."""
from __future__ import annotations

import json
import os

import numpy as np

from archi_amd.llama import HEAD_DIM, LLAMA_SHAPES, LlamaShape, hf_state_dict
from tests.decoder_ref import CORPUS

# name -> (shape name, seed, row lengths, std of the matrices): the fixtures of tests/golden/llama_*.npz.
# The std: 0.02 (the project's usual) leaves attention near uniform -- window + 1 moves ll-win's rows by 4 to 12 times the bar, the
# theta swap by 2 to 4 times --, 0.1 makes HF's own bf16 run miss its float32 self by 1e-2 and more (0.6 on the 8192-token row), which
# would be the bar. 0.05 keeps HF's bf16 error at the 3e-4 bar and every defect of test_llama_cpu.py at >= 10 bars; the 8192-token row
# at 0.04 (HF's bf16 error there: 2.5e-3 at 0.04, 1.1e-2 at 0.05). ll-win's seed is the one of five tried at which the weakest window
# defect on the 49-token row is 15 bars rather than 10.
STD = 0.05
FIXTURES = {
    "ll-tiny-g1": ("ll-tiny-g1", 41, (320, 255, 129, 64, 33, 1), STD),
    "ll-tiny-g2": ("ll-tiny-g2", 42, (320, 256, 100, 32, 7, 1), STD),
    "ll-tiny-g3": ("ll-tiny-g3", 43, (320, 193, 96, 31, 2, 1), STD),
    "ll-tiny-g4": ("ll-tiny-g4", 44, (320, 257, 128, 65, 5, 1), STD),
    "ll-win": ("ll-win", 345, (300, 65, 49, 48, 5), STD),
    "ll-long": ("ll-long", 46, (8192, 300, 65), 0.04),
    "ll-l3": ("ll-l3", 47, (320, 200, 65, 64, 9), STD),
    "ll-bidir-mean": ("ll-tiny-g2", 48, (513, 512, 100, 1), STD),
    "ll-causal-mean": ("ll-win", 49, (300, 65, 49, 5, 1), STD),
}
# name -> (attention, pooling) where it is not (causal, last)
MODES = {"ll-bidir-mean": ("bidirectional", "mean"), "ll-causal-mean": ("causal", "mean")}
COS_BAR, ABS_BAR = 3e-4, 3e-3      # the bf16 encoder bar of the project's fixtures (1 - cos, max |d|)


def _shape(shape) -> LlamaShape:
    return LLAMA_SHAPES[shape] if isinstance(shape, str) else LlamaShape(*shape)


def hf_config(shape, dialect: str = "mistral"):
    """MistralConfig (a shape with a window, or dialect "mistral") or LlamaConfig (a shape with llama3 scaling, or dialect "llama")."""
    from transformers import LlamaConfig, MistralConfig
    s = _shape(shape)
    common = dict(vocab_size=s.vocab, hidden_size=s.hidden, num_hidden_layers=s.layers, num_attention_heads=s.q_heads,
                  num_key_value_heads=s.kv_heads, head_dim=HEAD_DIM, intermediate_size=s.intermediate, max_position_embeddings=s.max_position,
                  rms_norm_eps=s.rms_eps, hidden_act="silu", tie_word_embeddings=False)
    if s.scaling is not None or (dialect == "llama" and not s.window):
        rp = {"rope_type": "default", "rope_theta": s.rope_theta}
        if s.scaling is not None:
            rp = {"rope_type": "llama3", "rope_theta": s.rope_theta, "factor": s.scaling.factor, "low_freq_factor": s.scaling.low,
                  "high_freq_factor": s.scaling.high, "original_max_position_embeddings": s.scaling.original}
        return LlamaConfig(rope_parameters=rp, attention_bias=False, mlp_bias=False, **common)
    return MistralConfig(rope_parameters={"rope_type": "default", "rope_theta": s.rope_theta}, sliding_window=s.window or None, **common)


def hf_model(shape, weights, dialect: str = "mistral", dtype=None):
    """float32 (or `dtype`) MistralModel / LlamaModel on the CPU with eager attention holding `weights` (archi_amd.llama names)."""
    import torch
    from transformers import LlamaModel, MistralModel
    cfg = hf_config(shape, dialect)
    cfg._attn_implementation = "eager"
    cls = LlamaModel if cfg.model_type == "llama" else MistralModel
    with torch.device("meta"):
        m = cls(cfg)
    sd = {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float32) for k, v in hf_state_dict(weights, cfg.num_hidden_layers).items()}
    m.load_state_dict(sd, assign=True, strict=True)
    m.rotary_emb = type(m.rotary_emb)(config=cfg)            # non-persistent buffer: built on the CPU, not loaded
    m = m.eval().float()
    return m.to(dtype) if dtype is not None else m


def reference(model, ids, lens, normalise=True, rows=None, attention="causal", pooling="last", defect=None):
    """Each row alone (no padding) through the model: the final-normed hidden state of its last token (sentence-transformers' lasttoken
    Pooling) or the mean of the final-normed states (mean Pooling), L2-normalised in float32 (Normalize). attention "bidirectional": HF
    gets an explicit 4D mask with every key visible, which its mask construction returns as it is. defect (mean pooling): pad8 (eight pad
    tokens, id 0, run with the row and ATTENDED; the mean still over the row's own tokens) | prenorm (the mean taken before the final norm)."""
    import torch
    out = []
    with torch.no_grad():
        for i, (row, n) in enumerate(zip(np.asarray(ids), np.asarray(lens))):
            if rows is not None and i not in rows:
                continue
            n = int(n)
            t = torch.as_tensor(row[:n], dtype=torch.long)[None]
            if defect == "pad8":
                t = torch.cat([t, torch.zeros((1, 8), dtype=torch.long)], 1)
            kw = {}
            if attention == "bidirectional":
                kw["attention_mask"] = torch.zeros((1, 1, t.shape[1], t.shape[1]), dtype=next(model.parameters()).dtype)
            norm = model.norm
            if defect == "prenorm":
                model.norm = torch.nn.Identity()
            try:
                hs = model(input_ids=t, **kw).last_hidden_state[0, :n].float()
            finally:
                model.norm = norm
            if defect == "prenorm":
                h = norm.float()(hs.mean(0)) if pooling == "mean" else norm.float()(hs[n - 1])
            else:
                h = hs.mean(0) if pooling == "mean" else hs[n - 1]
            if normalise:
                h = torch.nn.functional.normalize(h, dim=0)
            out.append(h.numpy())
    return np.stack(out).astype(np.float32)


def fixture_weights(name):
    """The seeded weights of a fixture. The mean-pooled fixtures scale each embedding row by a seeded power of two in [1, 64] (exact in
    bf16): with rows of one common norm the token states have nearly equal RMS, and the mean taken BEFORE the final norm moves the
    embedding by 1 - cos 4e-6 -- no test would see that defect. Released checkpoints' embedding rows differ in norm as well."""
    from archi_amd.llama import random_llama_weights
    shape, seed, _, std = FIXTURES[name]
    w = random_llama_weights(shape, seed=seed, std=std)
    if MODES.get(name, ("causal", "last"))[1] == "mean":
        f = 2.0 ** np.random.default_rng(seed + 1000).integers(0, 7, w["embed_tokens"].shape[0])
        w["embed_tokens"] = (w["embed_tokens"] * f[:, None]).astype(np.float32)
    return w


def fixture_inputs(name):
    """(shape name, seed, ids [B][W] int32 zero padded, lens [B], std) of a fixture: seeded ids."""
    shape, seed, lens, std = FIXTURES[name]
    rng = np.random.default_rng(seed)
    lens = np.array(lens, np.int32)
    ids = np.zeros((len(lens), int(lens.max())), np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.integers(0, LLAMA_SHAPES[shape].vocab, n)
    return shape, seed, ids, lens, std


def _no_rope(inner):
    """RoPE dropped: a rotary module that returns cos = 1, sin = 0 at every position."""
    import torch

    class NoRope(torch.nn.Module):
        def forward(self, x, position_ids, **kw):
            c, s = inner(x, position_ids, **kw)
            return torch.ones_like(c), torch.zeros_like(s)

    return NoRope()


def defect_model(shape, weights, defect: str):
    """The float32 HF model of `shape` with one defect: window+1 | window-1 | nowindow | norope | theta (1e4 <-> 1e6) | noscaling (llama3
    scaling dropped)."""
    s = _shape(shape)
    if defect == "window+1":
        s = s._replace(window=s.window + 1)
    elif defect == "window-1":
        s = s._replace(window=s.window - 1)
    elif defect == "nowindow":
        s = s._replace(window=0)
    elif defect == "theta":
        s = s._replace(rope_theta=1e6 if s.rope_theta == 1e4 else 1e4)
    elif defect == "noscaling":
        s = s._replace(scaling=None)
    m = hf_model(s, weights, dialect="llama" if _shape(shape).scaling is not None else "mistral")
    if defect == "norope":
        m.rotary_emb = _no_rope(m.rotary_emb)
    return m


def make_tokenizer_json(path: str, vocab_size: int = 600) -> str:
    """A small byte-level BPE trained from CORPUS with a Mistral-style post-processor (<s> $A </s>: e5-mistral's tokenizer adds both)."""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors, trainers
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=["<unk>", "<s>", "</s>"],
                                  initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False)
    tok.train_from_iterator(CORPUS * 4, trainer=trainer)
    bos, eos = tok.token_to_id("<s>"), tok.token_to_id("</s>")
    tok.post_processor = processors.TemplateProcessing(single="<s> $A </s>", special_tokens=[("<s>", bos), ("</s>", eos)])
    tok.save(path)
    return path


def write_checkpoint(model_dir: str, shape, weights, dialect: str = "mistral", max_seq_length: int = 512, pooling: str = "lasttoken",
                     normalize: bool = True) -> str:
    """An e5-mistral style directory: save_pretrained (config.json + model.safetensors), tokenizer.json, modules.json, 1_Pooling,
    2_Normalize, sentence_bert_config.json."""
    os.makedirs(model_dir, exist_ok=True)
    hf_model(shape, weights, dialect).save_pretrained(model_dir)
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
