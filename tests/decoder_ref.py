"""CPU reference and fixtures of the Qwen3 decoder path (archi_amd.decoder): transformers.Qwen3Model in float32, a small byte-level
BPE tokenizer.json trained offline, and a sentence-transformers style checkpoint directory. Used by the decoder tests and by
tests/golden/make_decoder_fixtures.py."""
from __future__ import annotations

import json
import os

import numpy as np

from archi_amd.decoder import HEAD_DIM, QWEN3_SHAPES, hf_state_dict

CORPUS = [
    "The detector readout chain digitises every channel at 40 MHz before the trigger decision.",
    "Muon chambers measure the momentum of tracks that leave the calorimeter.",
    "Instruct: Given a physics question, retrieve relevant passages\nQuery: what is the σ of the beam spot?",
    "Résumé of the µ-metal shielding test: the field dropped by a factor of 40 — “good enough”.",
    "Für die Kalibrierung wird eine Quelle mit bekannter Aktivität verwendet.",
    "The quick brown fox jumps over the lazy dog; 0123456789 + - * / = ( ) [ ] { }",
    "Η ενέργεια του δέσμου ήταν 6.8 TeV ανά πρωτόνιο.",
    "日本語のテキストもトークン化されます。",
]


def hf_config(shape):
    from transformers import Qwen3Config
    if isinstance(shape, str):
        shape = QWEN3_SHAPES[shape]
    vocab, H, L, nq, nkv, I, max_pos, theta, eps = shape
    return Qwen3Config(vocab_size=vocab, hidden_size=H, num_hidden_layers=L, num_attention_heads=nq, num_key_value_heads=nkv,
                       head_dim=HEAD_DIM, intermediate_size=I, max_position_embeddings=max_pos, rms_norm_eps=eps, rope_theta=theta,
                       hidden_act="silu", attention_bias=False, use_sliding_window=False, tie_word_embeddings=False)


def hf_model(shape, weights, attn: str = "eager"):
    """float32 Qwen3Model on the CPU holding `weights` (archi_amd.decoder names)."""
    import torch
    from transformers import Qwen3Model
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RotaryEmbedding
    cfg = hf_config(shape)
    cfg._attn_implementation = attn
    with torch.device("meta"):
        m = Qwen3Model(cfg)
    sd = {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float32) for k, v in hf_state_dict(weights, cfg.num_hidden_layers).items()}
    m.load_state_dict(sd, assign=True, strict=True)
    m.rotary_emb = Qwen3RotaryEmbedding(config=cfg)          # non-persistent buffer: built on the CPU, not loaded
    return m.eval().float()


def reference(model, ids, lens, normalise=True):
    """Each row alone (no padding) through the float32 model: final-normed hidden state of its last token, L2-normalised
    (sentence-transformers' lasttoken Pooling + Normalize)."""
    import torch
    out = []
    with torch.no_grad():
        for row, n in zip(np.asarray(ids), np.asarray(lens)):
            n = int(n)
            h = model(input_ids=torch.as_tensor(row[:n], dtype=torch.long)[None]).last_hidden_state[0, n - 1]
            if normalise:
                h = torch.nn.functional.normalize(h, dim=0)
            out.append(h.numpy())
    return np.stack(out).astype(np.float32)


def make_tokenizer_json(path: str, vocab_size: int = 600) -> str:
    """A small byte-level BPE trained from CORPUS with the Qwen3-Embedding post-processor ($A <|endoftext|>)."""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors, trainers
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=["<|endoftext|>"],
                                  initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False)
    tok.train_from_iterator(CORPUS * 4, trainer=trainer)
    eot = tok.token_to_id("<|endoftext|>")
    tok.post_processor = processors.TemplateProcessing(single="$A <|endoftext|>", special_tokens=[("<|endoftext|>", eot)])
    tok.save(path)
    return path


def write_checkpoint(model_dir: str, shape, weights, max_seq_length: int = 512, tokenizer: bool = True) -> str:
    """A Qwen3-Embedding style directory: Qwen3Model.save_pretrained (config.json + model.safetensors), tokenizer.json,
    modules.json, 1_Pooling (lasttoken), 2_Normalize, sentence_bert_config.json."""
    os.makedirs(model_dir, exist_ok=True)
    hf_model(shape, weights).save_pretrained(model_dir)
    if tokenizer:
        make_tokenizer_json(os.path.join(model_dir, "tokenizer.json"))
    json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
               {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}],
              open(os.path.join(model_dir, "modules.json"), "w"))
    os.makedirs(os.path.join(model_dir, "1_Pooling"), exist_ok=True)
    os.makedirs(os.path.join(model_dir, "2_Normalize"), exist_ok=True)
    json.dump({"word_embedding_dimension": int(weights["norm"].shape[0]), "pooling_mode_cls_token": False,
               "pooling_mode_mean_tokens": False, "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False,
               "pooling_mode_weightedmean_tokens": False, "pooling_mode_lasttoken": True, "include_prompt": True},
              open(os.path.join(model_dir, "1_Pooling", "config.json"), "w"))
    json.dump({"max_seq_length": max_seq_length, "do_lower_case": False},
              open(os.path.join(model_dir, "sentence_bert_config.json"), "w"))
    return model_dir
