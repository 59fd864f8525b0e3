"""Test helper: the float32 CPU reference of the XLM-RoBERTa path -- transformers.XLMRobertaModel on the weights of
archi_amd.encoder.random_xlmr_weights, cls / mean pooling and L2 as sentence-transformers applies them --, the small Unigram
tokenizer.json of tests/golden (specials <s> <pad> </s> <unk> at ids 0-3, <mask> last, template <s> $A </s>) and a
sentence-transformers-style XLM-R checkpoint directory written at test time."""
import json
import os
import shutil

import numpy as np

from archi_amd.encoder import XLMR_PADDING_IDX, XLMR_SHAPES, random_xlmr_weights, xlmr_hf_state_dict

PAD_ID = XLMR_PADDING_IDX
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOKENIZER_JSON = os.path.join(GOLDEN, "xlmr_tokenizer.json")
EPS = 1e-5

# the tokenizer's training text (make_tokenizer_json) and the texts of the tokenizer / end-to-end tests: German, Greek, Japanese,
# accents and µ / σ as archi's documents hold them, and literal special tokens
CORPUS = ["The muon detector calibration run finished.", "Die Kalibrierung des Myon-Detektors ist abgeschlossen.",
          "Η βαθμονόμηση του ανιχνευτή μιονίων ολοκληρώθηκε.", "ミューオン検出器の較正が完了しました。",
          "naïve café résumé — 3 µm ± 0.2 σ", "grid site job failed: tier-2 storage is full", "jet energy scale of a beam trigger",
          "Datensätze im Tier-2-Zentrum, Jobs fehlgeschlagen", "σ = 0.5 µs, Δt < 3 ns", "検出器 データ 解析 ジョブ"]
TEXTS = CORPUS + ["a <pad> b", "<mask> trigger", "<s> run </s>", "ÄÖÜ äöü ß", "run " * 40, "", "Ω" * 300]


def make_tokenizer_json(path: str, vocab_size: int = 1000) -> str:
    """A small Unigram tokenizer.json with XLM-R's layout: <s> <pad> </s> <unk> at ids 0-3, <mask> as the last id, Metaspace
    pre-tokenisation and the <s> $A </s> post-processor (tests/golden/make_xlmr_fixtures.py writes the committed one)."""
    from tokenizers import Tokenizer, decoders, models, normalizers, pre_tokenizers, processors, trainers
    tok = Tokenizer(models.Unigram())
    tok.normalizer = normalizers.NFKC()
    tok.pre_tokenizer = pre_tokenizers.Metaspace()
    tok.decoder = decoders.Metaspace()
    trainer = trainers.UnigramTrainer(vocab_size=vocab_size - 1, special_tokens=["<s>", "<pad>", "</s>", "<unk>"], unk_token="<unk>",
                                      show_progress=False)
    tok.train_from_iterator(CORPUS * 20, trainer=trainer)
    tok.add_special_tokens(["<mask>"])
    tok.post_processor = processors.TemplateProcessing(single="<s> $A </s>", pair="<s> $A </s> </s> $B </s>",
                                                       special_tokens=[("<s>", 0), ("</s>", 2)])
    tok.save(path)
    return path


def hf_tokenizer(path: str = TOKENIZER_JSON):
    """transformers' fast tokenizer over the same tokenizer.json (the engine under SentenceTransformer)."""
    from transformers import PreTrainedTokenizerFast
    return PreTrainedTokenizerFast(tokenizer_file=path, bos_token="<s>", eos_token="</s>", unk_token="<unk>", pad_token="<pad>",
                                   mask_token="<mask>")


def hf_config(shape, eps=EPS):
    from transformers import XLMRobertaConfig
    vocab, H, L, heads, I, max_pos = shape[:6]
    return XLMRobertaConfig(vocab_size=vocab, hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, intermediate_size=I,
                            max_position_embeddings=max_pos, type_vocab_size=1, hidden_act="gelu", layer_norm_eps=eps,
                            hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, pad_token_id=PAD_ID, bos_token_id=0,
                            eos_token_id=2)


def hf_model(shape_name, seed):
    """XLMRobertaModel (float32, eval, eager attention) holding random_xlmr_weights(shape, seed); also returns those weights."""
    from transformers import XLMRobertaModel
    shape = XLMR_SHAPES[shape_name]
    w = random_xlmr_weights(shape, seed)
    cfg = hf_config(shape)
    cfg._attn_implementation = "eager"
    model = XLMRobertaModel(cfg, add_pooling_layer=False).eval()
    missing, unexpected = model.load_state_dict(xlmr_hf_state_dict(w, shape[2]), strict=False)
    assert not unexpected and all("position_ids" in m or "token_type_ids" in m for m in missing), (missing, unexpected)
    return model.float(), w


def pad_rows(toks, S):
    """Token lists -> ids [B][S] padded with XLM-R's pad id, 0 / 1 mask."""
    ids = np.full((len(toks), S), PAD_ID, np.int32)
    mask = np.zeros((len(toks), S), np.int32)
    for i, t in enumerate(toks):
        ids[i, :len(t)] = t
        mask[i, :len(t)] = 1
    return ids, mask


def hf_embed(model, ids, mask, pooling="cls", normalize=True, position_ids=None):
    import torch
    kw = {}
    if position_ids is not None:
        kw["position_ids"] = torch.as_tensor(position_ids).long()
    with torch.no_grad():
        h = model(input_ids=torch.as_tensor(np.asarray(ids)).long(), attention_mask=torch.as_tensor(np.asarray(mask)).long(),
                  **kw).last_hidden_state
    mk = torch.as_tensor(np.asarray(mask)).float()
    out = h[:, 0] if pooling == "cls" else (h * mk[:, :, None]).sum(1) / mk.sum(1, keepdim=True).clamp(min=1e-9)
    if normalize:
        out = torch.nn.functional.normalize(out, p=2, dim=1)
    return out.numpy()


def offset_positions(ids):
    """The offset scheme's positions (padding_idx + 1 + token index), which ignore pad ids inside a row."""
    return np.broadcast_to(np.arange(ids.shape[1]) + PAD_ID + 1, ids.shape).copy()


def write_checkpoint(path, shape_name="xlmr-tiny-hd64", seed=0, pooling="cls", max_seq_length=128, normalize=True,
                     tokenizer_json=True, vocab_txt=False):
    """sentence-transformers-style XLM-R checkpoint directory (random_xlmr_weights of the shape, the golden tokenizer.json)."""
    model, _ = hf_model(shape_name, seed)
    os.makedirs(path, exist_ok=True)
    model.save_pretrained(path, safe_serialization=True)
    if tokenizer_json:
        shutil.copy(TOKENIZER_JSON, os.path.join(path, "tokenizer.json"))
    if vocab_txt:
        with open(os.path.join(path, "vocab.txt"), "w") as f:
            f.write("\n".join(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"tok{i}" for i in range(995)]) + "\n")
    modules = [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"}]
    if normalize:
        modules.append({"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"})
    json.dump(modules, open(os.path.join(path, "modules.json"), "w"))
    os.makedirs(os.path.join(path, "1_Pooling"), exist_ok=True)
    json.dump({"word_embedding_dimension": XLMR_SHAPES[shape_name][1], "pooling_mode_cls_token": pooling == "cls",
               "pooling_mode_mean_tokens": pooling == "mean", "pooling_mode_max_tokens": False,
               "pooling_mode_mean_sqrt_len_tokens": False}, open(os.path.join(path, "1_Pooling", "config.json"), "w"))
    json.dump({"max_seq_length": max_seq_length, "do_lower_case": False},
              open(os.path.join(path, "sentence_bert_config.json"), "w"))
    return model
