"""The float32 reference of the T5 tests: transformers.T5EncoderModel on the CPU (eager attention), fed the project's seeded weights,
pooled, sent through the Dense matrices and normalised the way sentence-transformers does. Also the mutated references the fixtures
must be able to tell from the true one (MUTANTS), the all-bf16 run that sets the bf16 bar, and a sentence-transformers checkpoint
directory with a small Unigram tokenizer.json."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from archi_amd.t5 import T5_SHAPES, hf_state_dict, random_t5_weights, shape_config_dict, shape_hf_config

# the project's stated bf16 encoder bar (tests/test_xlmr_gpu.py): 1 - cos and max |d| on L2-normalised embeddings
PROJECT_BAR_COS, PROJECT_BAR_ABS = 3e-4, 3e-3
# the bias zeroed; key - query mirrored; the delta shifted by one; q scaled by 1 / 8 (a model that scaled its scores like BERT); the
# gate and linear halves of the gated feed-forward swapped; the bias clamped at D / 2 (moves rows longer than D + 64 only)
MUTANTS = ("no_bias", "mirror", "shift", "qscale", "swap_gate", "clamp_half")


def mutated_weights(weights, mutant):
    w = dict(weights)
    if mutant == "no_bias":
        w["rel_bias"] = np.zeros_like(w["rel_bias"])
    elif mutant == "qscale":
        for k in [k for k in w if k.endswith(".wq")]:
            w[k] = w[k] * np.float32(0.125)
    elif mutant == "swap_gate":
        for k in [k for k in w if k.endswith(".wi_0")]:
            other = k[:-1] + "1"
            w[k], w[other] = w[other], w[k]
    return w


def hf_model(shape, weights, dtype=torch.float32, mutant=None):
    """T5EncoderModel (eager attention, eval) of a T5_SHAPES tuple / name holding `weights` (our names). mutant: one of MUTANTS; the
    three that change the distance replace block 0's compute_bias by HF's own expression on a changed key - query."""
    if isinstance(shape, str):
        shape = T5_SHAPES[shape]
    cfg = shape_hf_config(shape)
    cfg._attn_implementation = "eager"
    from transformers import T5EncoderModel
    model = T5EncoderModel(cfg)
    sd = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float32))) for k, v in hf_state_dict(mutated_weights(weights, mutant)).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("embed_tokens" in m or m == "shared.weight" for m in missing), (missing, unexpected)
    model = model.to(dtype).eval()
    if mutant in ("mirror", "shift", "clamp_half"):
        attn = model.encoder.block[0].layer[0].SelfAttention
        D = shape[8]

        def compute_bias(query_length, key_length, device=None, past_seen_tokens=0):
            rel = torch.arange(key_length, dtype=torch.long)[None, :] - torch.arange(query_length, dtype=torch.long)[:, None]
            rel = -rel if mutant == "mirror" else rel + 1 if mutant == "shift" else rel.clamp(-(D // 2), D // 2)
            b = attn._relative_position_bucket(rel, bidirectional=True, num_buckets=attn.relative_attention_num_buckets,
                                               max_distance=attn.relative_attention_max_distance)
            return attn.relative_attention_bias(b).permute([2, 0, 1]).unsqueeze(0)

        attn.compute_bias = compute_bias
    return model


def dense_tail(weights):
    """The Dense matrices of `weights` in order, float32 tensors."""
    out, i = [], 0
    while f"dense{i}" in weights:
        out.append(torch.from_numpy(np.ascontiguousarray(np.asarray(weights[f"dense{i}"], np.float32))))
        i += 1
    return out


def reference(model, ids, lens, pooling: str, dense=(), normalise: bool = True) -> np.ndarray:
    """Each row alone, unpadded: last hidden states (behind final_layer_norm) -> cls / mean pooling -> the Dense matrices -> L2
    normalisation, all behind the model in float32 (sentence-transformers' Pooling + Dense + Normalize)."""
    out = []
    with torch.no_grad():
        for row, n in zip(np.asarray(ids), np.asarray(lens)):
            n = int(n)
            x = torch.from_numpy(np.asarray(row[:n], np.int64))[None]
            h = model(input_ids=x, attention_mask=torch.ones_like(x)).last_hidden_state[0].float()
            e = h[0] if pooling == "cls" else h.mean(0)
            for d in dense:
                e = d @ e
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


def make_case(shape_name: str, seed: int, std: float, bias_std: float, lens, pooling: str):
    """One fixture's content, computed from T5EncoderModel alone: ids, expected (float32 reference), the error of the all-bf16 run
    per figure, and the bar (the larger of the project's bf16 bar and that error, per figure; no margin)."""
    shape = T5_SHAPES[shape_name]
    w = random_t5_weights(shape, seed=seed, std=std, bias_std=bias_std)
    ids, lens = make_ids(shape, seed, lens)
    dense = dense_tail(w)
    exp = reference(hf_model(shape, w), ids, lens, pooling, dense)
    got = reference(hf_model(shape, w, dtype=torch.bfloat16), ids, lens, pooling, dense)
    case = dict(shape_name=shape_name, seed=seed, std=std, bias_std=bias_std, ids=ids, lens=lens, pooling=pooling, expected=exp,
                bf16_cos=float(cos_gap(got, exp).max()), bf16_abs=float(np.abs(got - exp).max()))
    case["bar_cos"] = max(PROJECT_BAR_COS, case["bf16_cos"])
    case["bar_abs"] = max(PROJECT_BAR_ABS, case["bf16_abs"])
    return case


def clamp_half_is_identity(shape, weights) -> bool:
    """True where the bias of clamp(key - query, -D / 2, D / 2) equals the bias of key - query at every distance: the last bucket of
    a side starts at or below D / 2 (8 buckets, D = 16: at distance 6)."""
    from archi_amd.t5 import t5_rel_table
    D = shape[8]
    tab = t5_rel_table(weights["rel_bias"], shape[7], D)
    return bool(np.array_equal(tab[:, np.clip(np.arange(-D, D + 1), -(D // 2), D // 2) + D], tab))


def sensitivities(case, max_len=None):
    """{mutant: 1 - cos per row between the mutated float32 T5EncoderModel and the case's expected rows}; rows longer than max_len
    are left out (NaN) to keep a CPU test short. swap_gate only for the gated feed-forward; clamp_half only where it changes the bias
    table at all (clamp_half_is_identity)."""
    shape = T5_SHAPES[case["shape_name"]]
    w = random_t5_weights(shape, seed=case["seed"], std=case["std"], bias_std=case["bias_std"])
    lens = np.asarray(case["lens"])
    keep = np.flatnonzero(lens <= (max_len or lens.max()))
    out = {}
    for mu in MUTANTS:
        if (mu == "swap_gate" and shape[6] != "gated-gelu") or (mu == "clamp_half" and clamp_half_is_identity(shape, w)):
            continue
        gap = np.full(len(lens), np.nan)
        gap[keep] = cos_gap(reference(hf_model(shape, w, mutant=mu), np.asarray(case["ids"])[keep], lens[keep], case["pooling"], dense_tail(w)),
                            np.asarray(case["expected"])[keep])
        out[mu] = gap
    return out


# ---- text end to end: a checkpoint directory as sentence-transformers lays it out -------------------------------------------
def make_unigram(path: str, corpus, vocab_size: int = 400):
    """A small Unigram tokenizer trained offline from `corpus`, shaped like T5's: <pad> = 0, </s> = 1, <unk> = 2, Metaspace
    pre-tokenizer and decoder, a post-processor that appends </s>. Writes <path>/tokenizer.json; returns the vocabulary size."""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors, trainers
    tok = Tokenizer(models.Unigram())
    tok.pre_tokenizer = pre_tokenizers.Metaspace()
    tok.decoder = decoders.Metaspace()
    trainer = trainers.UnigramTrainer(vocab_size=vocab_size, special_tokens=["<pad>", "</s>", "<unk>"], unk_token="<unk>", show_progress=False)
    tok.train_from_iterator(list(corpus) * 4, trainer=trainer)
    tok.post_processor = processors.TemplateProcessing(single="$A </s>", special_tokens=[("</s>", tok.token_to_id("</s>"))])
    os.makedirs(path, exist_ok=True)
    tok.save(os.path.join(path, "tokenizer.json"))
    return tok.get_vocab_size()


def hf_tokenizer(path: str):
    from transformers import PreTrainedTokenizerFast
    return PreTrainedTokenizerFast(tokenizer_file=os.path.join(path, "tokenizer.json"), eos_token="</s>", unk_token="<unk>", pad_token="<pad>")


def write_checkpoint(path, shape, weights, pooling="mean", max_seq_length=128, normalize=True, corpus=None, full_model=False,
                     pooling_extra=None):
    """sentence-transformers-style T5 checkpoint directory holding `weights`: config.json + model.safetensors (T5EncoderModel's
    tensors; full_model: a whole T5 checkpoint's, with decoder.* and lm_head tensors the loader must ignore), a Unigram tokenizer.json
    trained from `corpus` (none when corpus is None), modules.json, 1_Pooling, the Dense modules of `weights`, Normalize,
    sentence_bert_config.json. pooling_extra: further fields of 1_Pooling/config.json."""
    from safetensors.torch import save_file
    if isinstance(shape, str):
        shape = T5_SHAPES[shape]
    os.makedirs(path, exist_ok=True)
    cfg = shape_config_dict(shape)
    sd = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.float32))) for k, v in hf_state_dict(weights).items()}
    if full_model:
        cfg.update(architectures=["T5ForConditionalGeneration"], is_encoder_decoder=True, num_decoder_layers=1)
        del sd["encoder.embed_tokens.weight"]
        g = torch.Generator().manual_seed(5)
        sd["decoder.block.0.layer.0.SelfAttention.q.weight"] = torch.randn(shape[1], shape[1], generator=g)
        sd["decoder.final_layer_norm.weight"] = torch.ones(shape[1])
        sd["lm_head.weight"] = torch.randn(8, shape[1], generator=g)
    else:
        del sd["shared.weight"]
        sd = {k: v.clone() for k, v in sd.items()}
    json.dump(cfg, open(os.path.join(path, "config.json"), "w"))
    save_file(sd, os.path.join(path, "model.safetensors"))
    if corpus is not None:
        n = make_unigram(path, corpus)
        assert n <= shape[0], (n, shape[0])
    modules = [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"}]
    for i, d in enumerate(dense_tail(weights)):
        name = f"{len(modules)}_Dense"
        modules.append({"idx": len(modules), "name": str(len(modules)), "path": name, "type": "sentence_transformers.models.Dense"})
        os.makedirs(os.path.join(path, name), exist_ok=True)
        json.dump({"in_features": d.shape[1], "out_features": d.shape[0], "bias": False,
                   "activation_function": "torch.nn.modules.linear.Identity"}, open(os.path.join(path, name, "config.json"), "w"))
        save_file({"linear.weight": d.contiguous()}, os.path.join(path, name, "model.safetensors"))
    if normalize:
        name = f"{len(modules)}_Normalize"
        modules.append({"idx": len(modules), "name": str(len(modules)), "path": name, "type": "sentence_transformers.models.Normalize"})
        os.makedirs(os.path.join(path, name), exist_ok=True)
    json.dump(modules, open(os.path.join(path, "modules.json"), "w"))
    os.makedirs(os.path.join(path, "1_Pooling"), exist_ok=True)
    pc = {"word_embedding_dimension": shape[1], "pooling_mode_cls_token": pooling == "cls", "pooling_mode_mean_tokens": pooling == "mean",
          "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False}
    pc.update(pooling_extra or {})
    json.dump(pc, open(os.path.join(path, "1_Pooling", "config.json"), "w"))
    json.dump({"max_seq_length": max_seq_length, "do_lower_case": False}, open(os.path.join(path, "sentence_bert_config.json"), "w"))
    return path
