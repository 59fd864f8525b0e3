"""The float32 reference of the NomicBERT tests: transformers.NomicBertModel on the CPU (eager attention), fed the project's seeded
weights, pooled and normalised the way sentence-transformers does. Also the ablated references the fixtures must be able to tell
from the true one (another theta, no RoPE, gate and up swapped, no token-type row, no LayerNorm biases, another attention scale),
the all-bf16 run that sets the bf16 bar, and a checkpoint directory in either dialect with a small WordPiece vocabulary."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from archi_amd.nomic import (NOMIC_SHAPES, hf_state_dict, original_state_dict, random_nomic_weights, shape_hf_config,
                             shape_original_config)

# the project's stated bf16 encoder bar (tests/test_xlmr_gpu.py): 1 - cos and max |d| on L2-normalised embeddings
PROJECT_BAR_COS, PROJECT_BAR_ABS = 3e-4, 3e-3
ABLATIONS = ("theta", "no_rope", "swap_gate_up", "no_type", "no_ln_bias", "scale")


def ablated_weights(weights, ablation):
    """The weights an ablated model holds: gate and up swapped, the token-type rows zero, every LayerNorm bias zero."""
    w = dict(weights)
    if ablation == "swap_gate_up":
        for k in [k for k in w if k.endswith(".w_gate")]:
            up = k[:-len("w_gate")] + "w_up"
            w[k], w[up] = w[up], w[k]
    elif ablation == "no_type":
        w["type_emb"] = np.zeros_like(w["type_emb"])
    elif ablation == "no_ln_bias":
        for k in [k for k in w if k.endswith("_b")]:
            w[k] = np.zeros_like(w[k])
    return w


def hf_model(shape, weights, dtype=torch.float32, ablation=None, attn="eager", **config):
    """NomicBertModel (eager attention, eval) of a NOMIC_SHAPES tuple / name holding `weights` (our names). ablation: one of
    ABLATIONS -- theta 10000 instead of the shape's, RoPE removed (cos 1, sin 0), gate_proj and up_proj swapped, the token-type row
    dropped, the LayerNorm biases dropped, the attention scale times sqrt(2). config: NomicBertConfig fields to override."""
    if isinstance(shape, str):
        shape = NOMIC_SHAPES[shape]
    if ablation == "theta":
        config = dict(config, rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
    cfg = shape_hf_config(shape, **config)
    cfg._attn_implementation = attn
    from transformers import NomicBertModel
    model = NomicBertModel(cfg)
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in hf_state_dict(ablated_weights(weights, ablation)).items()}
    model.load_state_dict(sd, strict=True)
    if ablation == "no_rope":
        model.rotary_emb.inv_freq.zero_()
        model.rotary_emb.original_inv_freq.zero_()
    elif ablation == "scale":
        for layer in model.layers:
            layer.self_attn.scaling *= 2.0 ** 0.5
    return model.to(dtype).eval()


def reference(model, ids, lens, pooling: str, normalise: bool = True) -> np.ndarray:
    """Each row alone, unpadded: last hidden states -> cls / mean pooling -> L2 normalisation, pooled in float32 (sentence-transformers'
    Pooling + Normalize; the model has no final norm)."""
    out = []
    with torch.no_grad():
        for row, n in zip(np.asarray(ids), np.asarray(lens)):
            n = int(n)
            x = torch.from_numpy(np.asarray(row[:n], np.int64))[None]
            h = model(input_ids=x, attention_mask=torch.ones_like(x)).last_hidden_state[0].float()
            e = h[0] if pooling == "cls" else h.mean(0)
            out.append(torch.nn.functional.normalize(e, dim=0) if normalise else e)
    return torch.stack(out).numpy()


def cos_gap(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """1 - cos per row, in float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def make_ids(shape, seed, lens):
    lens = np.asarray(lens, np.int32)
    rng = np.random.RandomState(seed + 1000)
    ids = np.zeros((len(lens), int(lens.max())), np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.randint(3, shape[0], size=int(n))
    return ids, lens


def make_case(shape_name: str, seed: int, std: float, lens, pooling: str, with_bf16: bool = True):
    """One fixture's content, computed from NomicBertModel alone: ids, expected (float32 reference), the error of the all-bf16 run per
    figure, and the bar (the larger of the project's bf16 bar and that error, per figure)."""
    shape = NOMIC_SHAPES[shape_name]
    w = random_nomic_weights(shape, seed=seed, std=std)
    ids, lens = make_ids(shape, seed, lens)
    exp = reference(hf_model(shape, w), ids, lens, pooling)
    case = dict(shape_name=shape_name, seed=seed, std=std, ids=ids, lens=lens, pooling=pooling, expected=exp)
    if with_bf16:
        got = reference(hf_model(shape, w, dtype=torch.bfloat16), ids, lens, pooling)
        case["bf16_cos"] = float(cos_gap(got, exp).max())
        case["bf16_abs"] = float(np.abs(got - exp).max())
    else:
        case["bf16_cos"] = case["bf16_abs"] = 0.0
    case["bar_cos"] = max(PROJECT_BAR_COS, case["bf16_cos"])
    case["bar_abs"] = max(PROJECT_BAR_ABS, case["bf16_abs"])
    return case


def sensitivities(shape_name, seed, std, ids, lens, pooling, expected, max_len=None):
    """{ablation: 1 - cos per row between the ablated float32 NomicBertModel and `expected`}; rows longer than max_len are left out
    (NaN) to keep a CPU test short."""
    shape = NOMIC_SHAPES[shape_name]
    w = random_nomic_weights(shape, seed=seed, std=std)
    keep = np.flatnonzero(np.asarray(lens) <= (max_len or np.max(lens)))
    out = {}
    for ab in ABLATIONS:
        gap = np.full(len(lens), np.nan)
        gap[keep] = cos_gap(reference(hf_model(shape, w, ablation=ab), np.asarray(ids)[keep], np.asarray(lens)[keep], pooling),
                            np.asarray(expected)[keep])
        out[ab] = gap
    return out


# ---- text end to end: a checkpoint directory as sentence-transformers lays it out -------------------------------------------
def make_wordpiece(path: str, corpus, vocab_size: int = 1000, lowercase: bool = True):
    """A small BERT WordPiece vocabulary built from `corpus`: <path>/vocab.txt and the matching <path>/tokenizer.json
    ([PAD] [UNK] [CLS] [SEP] [MASK] first; [CLS] $A [SEP]) and tokenizer_config.json. Returns the number of tokens.
    The vocabulary is a FUNCTION of the corpus: the words the BERT normaliser and pre-tokeniser cut it into, counted; every character
    and its ## form, then whole words, word beginnings and ## word endings of 2 to 4 characters in turn, each list by (count descending,
    text). (It used to be trained with tokenizers' WordPiece trainer, whose ties fall by the iteration order of a hash map seeded per
    process: every run gave another vocabulary, hence other token ids and other embeddings of the same texts, and what a test saw of
    its own assertions -- how many ranks of a top-k are separated, say -- changed from run to run.)"""
    from collections import Counter
    from tokenizers import BertWordPieceTokenizer
    tok = BertWordPieceTokenizer(lowercase=lowercase)
    words = Counter()
    for text in corpus:
        for wd, _ in tok._tokenizer.pre_tokenizer.pre_tokenize_str(tok._tokenizer.normalizer.normalize_str(text)):
            words[wd] += 1
    heads, tails = Counter(), Counter()
    for wd, n in words.items():
        for m in (2, 3, 4):
            if len(wd) > m:
                heads[wd[:m]] += n
                tails["##" + wd[-m:]] += n
    by_count = lambda c: [t for t, _ in sorted(c.items(), key=lambda kv: (-kv[1], kv[0]))]
    chars = sorted({ch for wd in words for ch in wd})
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + chars + ["##" + ch for ch in chars]
    seen = set(vocab)
    lists = [by_count(words), by_count(heads), by_count(tails)]
    i = 0
    while len(vocab) < vocab_size and any(lists):
        if lists[i % 3]:
            t = lists[i % 3].pop(0)
            if t not in seen:
                seen.add(t)
                vocab.append(t)
        i += 1
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "vocab.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(vocab[:vocab_size]) + "\n")
    full = BertWordPieceTokenizer(os.path.join(path, "vocab.txt"), lowercase=lowercase)
    full.save(os.path.join(path, "tokenizer.json"))
    json.dump({"do_lower_case": lowercase, "tokenizer_class": "BertTokenizer"}, open(os.path.join(path, "tokenizer_config.json"), "w"))
    return full.get_vocab_size()


def hf_tokenizer(path: str):
    """transformers' fast tokenizer over the directory's tokenizer.json (the engine under SentenceTransformer / AutoTokenizer)."""
    from transformers import PreTrainedTokenizerFast
    return PreTrainedTokenizerFast(tokenizer_file=os.path.join(path, "tokenizer.json"), cls_token="[CLS]", sep_token="[SEP]",
                                   unk_token="[UNK]", pad_token="[PAD]", mask_token="[MASK]")


def write_checkpoint(path, shape, weights, dialect="hf", pooling="mean", max_seq_length=128, normalize=True, corpus=None, vocab_txt=True,
                     prefix="", config=None):
    """sentence-transformers-style NomicBERT checkpoint directory holding `weights`: config.json + model.safetensors in transformers'
    dialect ("hf") or the Hub checkpoints' original one ("original": n_embd ..., fused attn.Wqkv, fc11 / fc12), a small WordPiece
    vocab.txt + tokenizer.json trained from `corpus` (none when corpus is None; vocab_txt=False: tokenizer.json alone), modules.json,
    1_Pooling, 2_Normalize, sentence_bert_config.json. prefix: put in front of every tensor name; config: fields to override."""
    from safetensors.torch import save_file
    if isinstance(shape, str):
        shape = NOMIC_SHAPES[shape]
    os.makedirs(path, exist_ok=True)
    if dialect == "hf":
        cfg = shape_hf_config(shape).to_dict()
        cfg["model_type"] = "nomic_bert"
        cfg["architectures"] = ["NomicBertModel"]
        sd = hf_state_dict(weights)
    else:
        cfg, sd = shape_original_config(shape), original_state_dict(weights)
    cfg.update(config or {})
    cfg = {k: v for k, v in cfg.items() if k not in ("dtype", "torch_dtype")}
    json.dump(cfg, open(os.path.join(path, "config.json"), "w"), default=str)
    save_file({prefix + k: torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float32))) for k, v in sd.items()},
              os.path.join(path, "model.safetensors"))
    if corpus is not None:
        n = make_wordpiece(path, corpus, vocab_size=shape[0])
        assert n <= shape[0], (n, shape[0])
        if not vocab_txt:
            os.remove(os.path.join(path, "vocab.txt"))
    modules = [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"}]
    if normalize:
        modules.append({"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"})
        os.makedirs(os.path.join(path, "2_Normalize"), exist_ok=True)
    json.dump(modules, open(os.path.join(path, "modules.json"), "w"))
    os.makedirs(os.path.join(path, "1_Pooling"), exist_ok=True)
    json.dump({"word_embedding_dimension": shape[1], "pooling_mode_cls_token": pooling == "cls",
               "pooling_mode_mean_tokens": pooling == "mean", "pooling_mode_max_tokens": False,
               "pooling_mode_mean_sqrt_len_tokens": False}, open(os.path.join(path, "1_Pooling", "config.json"), "w"))
    json.dump({"max_seq_length": max_seq_length, "do_lower_case": False}, open(os.path.join(path, "sentence_bert_config.json"), "w"))
    return path
