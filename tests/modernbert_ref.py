"""The float32 reference of the ModernBERT tests: transformers.ModernBertModel on the CPU (eager attention), fed the project's
seeded weights, pooled and normalised the way sentence-transformers does. Also the two ablated references the fixtures must be
able to tell from the true one (window removed, both rope thetas equal) and the all-bf16 run that sets the bf16 bar."""
from __future__ import annotations

import numpy as np
import torch

from archi_amd.modernbert import MODERNBERT_SHAPES, hf_state_dict, random_modernbert_weights, shape_hf_config

# the project's stated bf16 encoder bar (tests/test_xlmr_gpu.py): 1 - cos and max |d| on L2-normalised embeddings
PROJECT_BAR_COS, PROJECT_BAR_ABS = 3e-4, 3e-3
NO_WINDOW = 2 * 8192 + 2          # local_attention whose half-window covers every pair of an 8192-token row


def hf_model(shape, weights, dtype=torch.float32, no_window: bool = False, same_theta: bool = False):
    """ModernBertModel (eager attention, eval) of a MODERNBERT_SHAPES tuple / name holding `weights` (our names).
    no_window: every key visible in the sliding layers too (their rope theta stays); same_theta: the sliding layers rotate with
    the global theta (the window stays)."""
    if isinstance(shape, str):
        shape = MODERNBERT_SHAPES[shape]
    extra = {}
    if no_window:
        extra["local_attention"] = NO_WINDOW
    if same_theta:
        extra["rope_parameters"] = {k: {"rope_type": "default", "rope_theta": shape[7]} for k in ("full_attention", "sliding_attention")}
    cfg = shape_hf_config(shape, **extra)
    cfg._attn_implementation = "eager"
    from transformers import ModernBertModel
    model = ModernBertModel(cfg)
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in hf_state_dict(weights).items()}
    model.load_state_dict(sd, strict=True)
    return model.to(dtype).eval()


def reference_embed(model, ids, lens, pooling: str, normalise: bool = True) -> np.ndarray:
    """Row by row (no padding inside a forward): final hidden states -> cls / mean pooling -> L2 normalisation, pooled in float32."""
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


def make_case(shape_name: str, seed: int, std: float, lens, pooling: str, with_bf16: bool = True):
    """One fixture's content, computed from ModernBertModel alone: ids, expected (float32 reference), the sensitivities to the
    window and to the thetas per row, the error of the all-bf16 run per figure, and the bar (the larger of the project's bf16 bar and
    that error, per figure)."""
    shape = MODERNBERT_SHAPES[shape_name]
    w = random_modernbert_weights(shape, seed=seed, std=std)
    lens = np.asarray(lens, np.int32)
    rng = np.random.RandomState(seed + 1000)
    ids = np.zeros((len(lens), int(lens.max())), np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.randint(3, shape[0], size=int(n))
    exp = reference_embed(hf_model(shape, w), ids, lens, pooling)
    case = dict(shape_name=shape_name, seed=seed, std=std, ids=ids, lens=lens, pooling=pooling, expected=exp)
    types = shape[10]
    has_local, has_both = 0 in types, 0 in types and 1 in types
    case["sens_window"] = cos_gap(reference_embed(hf_model(shape, w, no_window=True), ids, lens, pooling), exp) if has_local else np.zeros(0)
    case["sens_theta"] = cos_gap(reference_embed(hf_model(shape, w, same_theta=True), ids, lens, pooling), exp) if has_both else np.zeros(0)
    if with_bf16:
        wb = {k: v for k, v in w.items()}
        got = reference_embed(hf_model(shape, wb, dtype=torch.bfloat16), ids, lens, pooling)
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
          "search_query: which trigger failed?", "search_document: the level-1 trigger of the muon chambers timed out",
          "Datensätze im Tier-2-Zentrum, Jobs fehlgeschlagen", "σ = 0.5 µs, Δt < 3 ns", "conditions database tag for the 2024 reprocessing"]
TEXTS = CORPUS + ["run " * 40, "", "Ω" * 100, "a [SEP] b", "tier-2 tier-2 storage"]


def make_tokenizer_json(path: str, vocab_size: int = 1000) -> str:
    """A small byte-level BPE tokenizer.json laid out like ModernBERT's: [PAD] [CLS] [SEP] [UNK] [MASK] at ids 0-4 and the
    [CLS] $A [SEP] post-processor."""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors, trainers
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=["[PAD]", "[CLS]", "[SEP]", "[UNK]", "[MASK]"],
                                  initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False)
    tok.train_from_iterator(CORPUS * 20, trainer=trainer)
    tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B [SEP]",
                                                       special_tokens=[("[CLS]", 1), ("[SEP]", 2)])
    tok.save(path)
    return path


def hf_tokenizer(path: str):
    """transformers' fast tokenizer over the same tokenizer.json (the engine under SentenceTransformer / AutoTokenizer)."""
    from transformers import PreTrainedTokenizerFast
    return PreTrainedTokenizerFast(tokenizer_file=path, cls_token="[CLS]", sep_token="[SEP]", unk_token="[UNK]", pad_token="[PAD]",
                                   mask_token="[MASK]")


def write_checkpoint(path, shape_name="modernbert-tiny-256", seed=0, std=0.1, pooling="mean", max_seq_length=128, normalize=True,
                     tokenizer_json=True):
    """sentence-transformers-style ModernBERT checkpoint directory (save_pretrained of ModernBertModel holding the seeded weights,
    a byte-level BPE tokenizer.json, modules.json / 1_Pooling / sentence_bert_config.json). Returns the float32 model."""
    import json
    import os
    shape = MODERNBERT_SHAPES[shape_name]
    model = hf_model(shape, random_modernbert_weights(shape, seed=seed, std=std))
    os.makedirs(path, exist_ok=True)
    model.save_pretrained(path, safe_serialization=True)
    if tokenizer_json:
        make_tokenizer_json(os.path.join(path, "tokenizer.json"), vocab_size=shape[0])
    modules = [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"}]
    if normalize:
        modules.append({"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"})
    json.dump(modules, open(os.path.join(path, "modules.json"), "w"))
    os.makedirs(os.path.join(path, "1_Pooling"), exist_ok=True)
    json.dump({"word_embedding_dimension": shape[1], "pooling_mode_cls_token": pooling == "cls",
               "pooling_mode_mean_tokens": pooling == "mean", "pooling_mode_max_tokens": False,
               "pooling_mode_mean_sqrt_len_tokens": False}, open(os.path.join(path, "1_Pooling", "config.json"), "w"))
    json.dump({"max_seq_length": max_seq_length, "do_lower_case": False}, open(os.path.join(path, "sentence_bert_config.json"), "w"))
    return model
