"""The float32 reference of the EmbeddingGemma tests: transformers.Gemma3TextModel on the CPU (eager attention, eval) with
use_bidirectional_attention, fed the project's seeded weights, run row by row, mean pooled, put through the Dense head and normalised
the way sentence-transformers does. Also the ablated references the fixtures must be able to tell from the true one (causal, window
removed, both rope thetas equal, head_dim ** -0.5 as the score scale) and the all-bf16 run that sets the bf16 bar."""
from __future__ import annotations

import numpy as np
import torch

from archi_amd.gemma import GEMMA_SHAPES, hf_state_dict, random_gemma_weights, shape_config_dict, shape_hf_config

# the project's stated bf16 encoder bar (tests/test_xlmr_gpu.py): 1 - cos and max |d| on L2-normalised embeddings
PROJECT_BAR_COS, PROJECT_BAR_ABS = 3e-4, 3e-3
NO_WINDOW = 2 * 2048 + 2          # sliding_window whose half covers every pair of a 2048-token row
ABLATIONS = ("causal", "no_window", "same_theta", "wrong_scale")


def hf_model(shape, weights, dtype=torch.float32, ablate: str | None = None):
    """Gemma3TextModel (eager attention, eval) of a GEMMA_SHAPES tuple / name holding `weights` (our names). ablate: "causal" (a
    causal stack whose sliding layers keep the same reach to the left), "no_window" (every key visible in the sliding layers too; their
    theta stays), "same_theta" (the sliding layers rotate with the global theta), "wrong_scale" (scores scaled by head_dim ** -0.5)."""
    if isinstance(shape, str):
        shape = GEMMA_SHAPES[shape]
    extra = {}
    if ablate == "causal":
        extra.update(use_bidirectional_attention=False, sliding_window=shape[11] // 2 + 1)      # (not rewritten for a causal model)
    elif ablate == "no_window":
        extra["sliding_window"] = NO_WINDOW
    elif ablate == "same_theta":
        extra["rope_parameters"] = {k: {"rope_type": "default", "rope_theta": shape[9]} for k in ("full_attention", "sliding_attention")}
    elif ablate == "wrong_scale":
        extra["query_pre_attn_scalar"] = shape[5]
    elif ablate is not None:
        raise ValueError(ablate)
    cfg = shape_hf_config(shape, **extra)
    cfg._attn_implementation = "eager"
    from transformers import Gemma3TextModel
    model = Gemma3TextModel(cfg)
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in hf_state_dict(weights).items()}
    model.load_state_dict(sd, strict=True)
    return model.to(dtype).eval()


def dense_matrices(shape, weights, use_dense: bool = True):
    if isinstance(shape, str):
        shape = GEMMA_SHAPES[shape]
    n = len(shape[14]) if use_dense else 0
    return [torch.from_numpy(np.ascontiguousarray(weights[f"dense{i}"], dtype=np.float32)) for i in range(n)]


def reference_embed(model, ids, lens, dense=(), normalise: bool = True) -> np.ndarray:
    """Row by row (no padding inside a forward): final hidden states -> mean pooling in float32 -> the Dense matrices in float32 ->
    L2 normalisation."""
    out = []
    with torch.no_grad():
        for row, n in zip(np.asarray(ids), np.asarray(lens)):
            n = int(n)
            x = torch.from_numpy(np.asarray(row[:n], np.int64))[None]
            h = model(input_ids=x, attention_mask=torch.ones_like(x)).last_hidden_state[0].float()
            e = h.mean(0)
            for w in dense:
                e = w @ e
            out.append(torch.nn.functional.normalize(e, dim=0) if normalise else e)
    return torch.stack(out).numpy()


def cos_gap(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """1 - cos per row, in float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def make_ids(shape, seed: int, lens) -> np.ndarray:
    lens = np.asarray(lens, np.int32)
    rng = np.random.RandomState(seed + 1000)
    ids = np.zeros((len(lens), int(lens.max())), np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.randint(3, shape[0], size=int(n))
    return ids


def make_case(shape_name: str, seed: int, std: float, lens, with_bf16: bool = True, ablations=ABLATIONS):
    """One fixture's content, computed from Gemma3TextModel alone: ids, expected (float32 reference), the sensitivity of every row
    to each ablation the shape's layer types can show (1 - cos against the ablated reference), the error of the all-bf16 run per
    figure, and the bar (the larger of the project's bf16 bar and that error, per figure)."""
    shape = GEMMA_SHAPES[shape_name]
    w = random_gemma_weights(shape, seed=seed, std=std)
    lens = np.asarray(lens, np.int32)
    ids = make_ids(shape, seed, lens)
    dense = dense_matrices(shape, w)
    exp = reference_embed(hf_model(shape, w), ids, lens, dense)
    case = dict(shape_name=shape_name, seed=seed, std=std, ids=ids, lens=lens, expected=exp)
    types = shape[13]
    shows = {"causal": True, "no_window": 0 in types, "same_theta": 0 in types and 1 in types, "wrong_scale": shape[12] != shape[5]}
    for ab in ABLATIONS:
        on = ab in ablations and shows[ab]
        case["sens_" + ab] = cos_gap(reference_embed(hf_model(shape, w, ablate=ab), ids, lens, dense), exp) if on else np.zeros(0)
    if with_bf16:
        got = reference_embed(hf_model(shape, w, dtype=torch.bfloat16), ids, lens, dense)
        case["bf16_cos"] = float(cos_gap(got, exp).max())
        case["bf16_abs"] = float(np.abs(got - exp).max())
    else:
        case["bf16_cos"] = case["bf16_abs"] = 0.0
    case["bar_cos"] = max(PROJECT_BAR_COS, case["bf16_cos"])
    case["bar_abs"] = max(PROJECT_BAR_ABS, case["bf16_abs"])
    return case


# ---- text end to end: a checkpoint directory as sentence-transformers lays it out -------------------------------------------
CORPUS = ["The muon detector calibration run finished.", "Die Kalibrierung des Myon-Detektors ist abgeschlossen.",
          "grid site job failed: tier-2 storage is full", "jet energy scale of a beam trigger", "naïve café résumé — 3 µm ± 0.2 σ",
          "task: search result | query: which trigger failed?", "title: none | text: the level-1 trigger of the muon chambers timed out",
          "Datensätze im Tier-2-Zentrum, Jobs fehlgeschlagen", "σ = 0.5 µs, Δt < 3 ns", "conditions database tag for the 2024 reprocessing"]
TEXTS = CORPUS + ["run " * 40, "", "Ω" * 100, "tier-2 tier-2 storage"]


def make_tokenizer_json(path: str, vocab_size: int = 1000) -> str:
    """A small byte-level BPE tokenizer.json laid out like Gemma's specials: <pad> <eos> <bos> <unk> at ids 0-3 and the
    <bos> $A <eos> post-processor of the EmbeddingGemma checkpoint."""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors, trainers
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=["<pad>", "<eos>", "<bos>", "<unk>"],
                                  initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False)
    tok.train_from_iterator(CORPUS * 20, trainer=trainer)
    tok.post_processor = processors.TemplateProcessing(single="<bos> $A <eos>", pair="<bos> $A <eos> <bos> $B <eos>",
                                                       special_tokens=[("<bos>", 2), ("<eos>", 1)])
    tok.save(path)
    return path


def hf_tokenizer(path: str):
    """transformers' fast tokenizer over the same tokenizer.json (the engine under SentenceTransformer / AutoTokenizer)."""
    from transformers import PreTrainedTokenizerFast
    return PreTrainedTokenizerFast(tokenizer_file=path, bos_token="<bos>", eos_token="<eos>", unk_token="<unk>", pad_token="<pad>")


def write_checkpoint(path, shape_name="gm-tiny", seed=0, std=0.1, max_seq_length=128, normalize=True, tokenizer_json=True, n_dense=None):
    """sentence-transformers-style EmbeddingGemma checkpoint directory: config.json as a released file holds it (sliding_window before
    the constructor's rewrite), model.safetensors of Gemma3TextModel's tensors, a byte-level BPE tokenizer.json, modules.json /
    1_Pooling / 2_Dense / 3_Dense / sentence_bert_config.json. n_dense: how many of the shape's Dense modules to write (None: all).
    Returns (float32 model, Dense matrices written)."""
    import json
    import os
    from safetensors.torch import save_file
    shape = GEMMA_SHAPES[shape_name]
    w = random_gemma_weights(shape, seed=seed, std=std)
    model = hf_model(shape, w)
    os.makedirs(path, exist_ok=True)
    json.dump(shape_config_dict(shape), open(os.path.join(path, "config.json"), "w"))
    save_file({k: v.contiguous() for k, v in model.state_dict().items()}, os.path.join(path, "model.safetensors"))
    if tokenizer_json:
        make_tokenizer_json(os.path.join(path, "tokenizer.json"), vocab_size=shape[0])
    modules = [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"}]
    dense = dense_matrices(shape, w)
    dense = dense if n_dense is None else dense[:n_dense]
    for i, d in enumerate(dense):
        sub = f"{i + 2}_Dense"
        os.makedirs(os.path.join(path, sub), exist_ok=True)
        json.dump({"in_features": d.shape[1], "out_features": d.shape[0], "bias": False, "activation_function": "torch.nn.modules.linear.Identity"},
                  open(os.path.join(path, sub, "config.json"), "w"))
        save_file({"linear.weight": d.contiguous()}, os.path.join(path, sub, "model.safetensors"))
        modules.append({"idx": len(modules), "name": str(len(modules)), "path": sub, "type": "sentence_transformers.models.Dense"})
    if normalize:
        modules.append({"idx": len(modules), "name": str(len(modules)), "path": f"{len(modules)}_Normalize", "type": "sentence_transformers.models.Normalize"})
    json.dump(modules, open(os.path.join(path, "modules.json"), "w"))
    os.makedirs(os.path.join(path, "1_Pooling"), exist_ok=True)
    json.dump({"word_embedding_dimension": shape[1], "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True,
               "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False}, open(os.path.join(path, "1_Pooling", "config.json"), "w"))
    json.dump({"max_seq_length": max_seq_length, "do_lower_case": False}, open(os.path.join(path, "sentence_bert_config.json"), "w"))
    return model, dense
