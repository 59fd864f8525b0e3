"""Test helper: the float32 CPU reference of the MPNet path -- transformers.MPNetModel on the weights of
archi_amd.encoder.random_mpnet_weights, mean / cls pooling and L2 as sentence-transformers applies them -- and a small
sentence-transformers-style MPNet checkpoint directory written at test time (the layout of tests/hf_checkpoint.py with
config.json model_type "mpnet" and MPNet's tokenizer files)."""
import json
import os

import numpy as np

from archi_amd.encoder import MPNET_PADDING_IDX, MPNET_SHAPES, mpnet_hf_state_dict, random_mpnet_weights

PAD_ID = MPNET_PADDING_IDX


def hf_config(shape, eps=1e-5):
    from transformers import MPNetConfig
    vocab, H, L, heads, I, max_pos = shape[:6]
    return MPNetConfig(vocab_size=vocab, hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, intermediate_size=I,
                       max_position_embeddings=max_pos, hidden_act="gelu", layer_norm_eps=eps, hidden_dropout_prob=0.0,
                       attention_probs_dropout_prob=0.0, relative_attention_num_buckets=32, pad_token_id=PAD_ID)


def hf_model(shape_name, seed, zero_bias=False, eps=1e-5):
    """MPNetModel (float32, eval) holding random_mpnet_weights(shape, seed); also returns those weights."""
    import torch
    from transformers import MPNetModel
    shape = MPNET_SHAPES[shape_name]
    w, rel, pos_full = random_mpnet_weights(shape, seed)
    if zero_bias:
        rel = np.zeros_like(rel)
    model = MPNetModel(hf_config(shape, eps), add_pooling_layer=False).eval()
    sd = mpnet_hf_state_dict(w, rel, pos_full, shape[2])
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in m for m in missing), (missing, unexpected)
    return model.float(), (w, rel, pos_full)


def pad_rows(toks, S):
    """Token lists -> ids [B][S] padded with MPNet's pad id, 0 / 1 mask."""
    ids = np.full((len(toks), S), PAD_ID, np.int32)
    mask = np.zeros((len(toks), S), np.int32)
    for i, t in enumerate(toks):
        ids[i, :len(t)] = t
        mask[i, :len(t)] = 1
    return ids, mask


def hf_embed(model, ids, mask, pooling="mean", normalize=True, position_ids=None):
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


WORDS = ["the", "muon", "detector", "cal", "##ib", "##ration", "run", "grid", ".", ",", "beam", "trigger", "##s",
         "jet", "energy", "of", "a", "is", "in", "and", "data", "##set", "tier", "site", "job", "fail", "##ed", "e", "##e",
         "<", ">", "/", "s", "mask", "pad", "[", "]", "unk", "cafe", "##s", "!"]


def write_vocab(path, size=1000):
    """An MPNet-style vocab.txt: <s> <pad> </s> <unk> first (ids 0-3, pad = 1 = padding_idx), then BERT-style entries."""
    vocab = ["<s>", "<pad>", "</s>", "<unk>", "[PAD]"] + [f"[unused{i}]" for i in range(95)] + ["[UNK]", "[CLS]", "[SEP]",
                                                                                                  "[MASK]"] + WORDS
    seen, out = set(), []
    for v in vocab:
        if v not in seen:
            seen.add(v)
            out.append(v)
    out += [f"tok{i}" for i in range(size - 1 - len(out))] + ["<mask>"]
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    return out


def write_checkpoint(path, shape_name="mpnet-tiny-hd32", seed=0, pooling="mean", max_seq_length=128, normalize=True):
    """sentence-transformers-style MPNet checkpoint directory (random_mpnet_weights of the shape, vocab of 1000 entries)."""
    import torch
    from transformers import MPNetModel
    shape = MPNET_SHAPES[shape_name]
    assert shape[0] == 1000
    model, _ = hf_model(shape_name, seed)
    os.makedirs(path, exist_ok=True)
    model.save_pretrained(path, safe_serialization=True)
    write_vocab(os.path.join(path, "vocab.txt"), shape[0])
    json.dump({"do_lower_case": True, "model_max_length": 512}, open(os.path.join(path, "tokenizer_config.json"), "w"))
    modules = [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"}]
    if normalize:
        modules.append({"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"})
    json.dump(modules, open(os.path.join(path, "modules.json"), "w"))
    os.makedirs(os.path.join(path, "1_Pooling"), exist_ok=True)
    json.dump({"word_embedding_dimension": shape[1], "pooling_mode_cls_token": pooling == "cls",
               "pooling_mode_mean_tokens": pooling == "mean", "pooling_mode_max_tokens": False,
               "pooling_mode_mean_sqrt_len_tokens": False}, open(os.path.join(path, "1_Pooling", "config.json"), "w"))
    json.dump({"max_seq_length": max_seq_length, "do_lower_case": False},
              open(os.path.join(path, "sentence_bert_config.json"), "w"))
    return model


def hf_tokenizer(vocab_file):
    """transformers' MPNet tokenizer from a vocab.txt (the fast one where the installed transformers has it)."""
    import inspect
    import transformers
    cls = getattr(transformers, "MPNetTokenizerFast", None) or transformers.MPNetTokenizer
    if "vocab" in inspect.signature(cls.__init__).parameters:       # transformers 5: the vocabulary as a dict
        vocab = {}
        for i, line in enumerate(open(vocab_file, encoding="utf-8")):
            vocab.setdefault(line.rstrip("\n"), i)
        return cls(vocab=vocab, do_lower_case=True)
    return cls(vocab_file=vocab_file, do_lower_case=True)


TEXTS = ["The muon detector calibration run.", "grid, grid grid", "jet energy of a beam trigger",
         "datasets in the tier site and jobs failed", "run " * 40, "unknownword the data", "café data <s> run </s>",
         "a <mask> trigger [UNK] job", "[CLS] run [SEP] <unk>", "CAFÉ Ünïcode naïve"]
# ... and for the tokenizer alone: a literal <pad> is id 1 = padding_idx, which HF's positions then skip (a known gap)
TOKENIZER_TEXTS = TEXTS + ["<pad>less beam", "x" * 150, "<s>", "</s></s>", "<mask>", "", "   ", "a\tb\nc", "run " * 300]
