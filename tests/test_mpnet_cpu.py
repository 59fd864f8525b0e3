"""CPU tests of the MPNet path (all-mpnet-base-v2 and its family): the checkpoint loader and what it refuses, the per-distance
relative-position bias table against transformers' MPNetEncoder, the tokenizer (native and fallback) against transformers'
MPNet tokenizer, a control that the fixture weights make the bias and the position offset matter, and the new C ABI entries."""
import ctypes
import json
import os

import numpy as np
import pytest

from archi_amd.encoder import (MPNET_SHAPES, load_hf_weights, load_mpnet_weights, mpnet_rel_bias_table, random_mpnet_weights,
                               weight_order)
from tests.mpnet_ref import TOKENIZER_TEXTS, hf_config, hf_embed, hf_model, hf_tokenizer, pad_rows, write_checkpoint, write_vocab

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16_ABS_TOL, BF16_COS_TOL = 3e-3, 3e-4     # the hidden-768 bf16 bar of the GPU tests


def test_loader_reads_an_mpnet_checkpoint(tmp_path):
    d = str(tmp_path / "m")
    model = write_checkpoint(d, "mpnet-tiny-hd32", seed=1)
    shape, w, rel, eps = load_mpnet_weights(d)
    vocab, H, L, heads, I, max_pos = MPNET_SHAPES["mpnet-tiny-hd32"][:6]
    assert shape == (vocab, H, L, heads, I, max_pos - 2) and eps == 1e-5
    assert set(weight_order(L)) <= set(w)
    sd = model.state_dict()
    assert np.array_equal(np.asarray(w["pos_emb"]), sd["embeddings.position_embeddings.weight"].numpy()[2:])
    assert np.array_equal(np.asarray(w["type_emb"]), np.zeros((1, H), np.float32))
    assert np.array_equal(np.asarray(w["l1.wo"]), sd["encoder.layer.1.attention.attn.o.weight"].numpy())
    assert np.array_equal(rel.numpy(), sd["encoder.relative_attention_bias.weight"].numpy())
    # the BERT loader keeps refusing it
    with pytest.raises(ValueError, match="not BERT"):
        load_hf_weights(d)


@pytest.mark.parametrize("change, match", [({"model_type": "bert"}, "not MPNet"), ({"hidden_act": "relu"}, "hidden_act"),
                                           ({"num_attention_heads": 16}, "head size"),
                                           ({"relative_attention_num_buckets": 16}, "buckets")])
def test_loader_refuses_what_it_does_not_implement(tmp_path, change, match):
    d = str(tmp_path / "m")
    write_checkpoint(d, "mpnet-tiny-hd32", seed=1)
    cj = os.path.join(d, "config.json")
    cfg = json.load(open(cj))
    cfg.update(change)
    json.dump(cfg, open(cj, "w"))
    with pytest.raises(ValueError, match=match):
        load_mpnet_weights(d)


def test_rel_bias_table_equals_hf_compute_position_bias_for_every_length():
    import torch
    from transformers.models.mpnet.modeling_mpnet import MPNetEncoder
    cfg = hf_config(MPNET_SHAPES["mpnet-tiny-hd32"])
    cfg.num_hidden_layers, cfg.num_attention_heads = 1, 2
    enc = MPNetEncoder(cfg)
    with torch.no_grad():
        enc.relative_attention_bias.weight.copy_(torch.randn(32, 2, generator=torch.Generator().manual_seed(0)))
    tab = mpnet_rel_bias_table(enc.relative_attention_bias.weight.detach(), 512)
    assert tab.shape == (2, 1023) and tab.dtype == np.float32
    with torch.no_grad():
        for S in range(1, 513):
            want = enc.compute_position_bias(torch.zeros(1, S, 1))[0].numpy()           # [heads][query][key]
            i = np.arange(S)
            assert np.array_equal(tab[:, i[None, :] - i[:, None] + 511], want), S


def _tokenizers(tmp_path):
    from archi_amd.embeddings import MPNET_SPECIALS, NativeWordPiece, VocabWordPiece
    vf = str(tmp_path / "vocab.txt")
    write_vocab(vf)
    return vf, NativeWordPiece(vf, specials=MPNET_SPECIALS), VocabWordPiece(vf, specials=MPNET_SPECIALS)


@pytest.mark.parametrize("max_len", [8, 128, 512])
def test_tokenizer_matches_transformers_mpnet_tokenizer(tmp_path, max_len):
    vf, native, fallback = _tokenizers(tmp_path)
    tok = hf_tokenizer(vf)
    texts = TOKENIZER_TEXTS
    ids, lens = native.encode_batch_array(texts, max_len)
    for i, t in enumerate(texts):
        ref = tok(t)["input_ids"]
        if len(ref) > max_len:
            ref = ref[:max_len - 1] + [ref[-1]]
        assert ref[0] == tok.convert_tokens_to_ids("<s>") and ref[-1] == tok.convert_tokens_to_ids("</s>")
        assert ids[i, :lens[i]].tolist() == ref, t
        assert fallback.encode(t, max_len) == ref, t


def test_native_tokenizer_flags_this_models_specials_only(tmp_path):
    """The native tokenizer hands texts with MPNet's literal specials (or non-ASCII) to the fallback, and tokenises BERT's
    specials itself: for MPNet they are plain text."""
    from archi_amd import _lib
    vf, native, _ = _tokenizers(tmp_path)
    texts = ["plain run", "a <s> b", "x </s>", "<pad>", "the <mask>", "[UNK] job", "[CLS] run [SEP]", "[MASK]", "café"]
    enc = [t.encode() for t in texts]
    offs = np.zeros(len(texts) + 1, np.int64)
    np.cumsum([len(e) for e in enc], out=offs[1:])
    ids = np.empty((len(texts), 32), np.int32)
    lens = np.empty(len(texts), np.int32)
    assert native._lib.ak_wordpiece_encode(native._h, b"".join(enc), offs.ctypes.data, len(texts), 32, 1, ids.ctypes.data,
                                           lens.ctypes.data) == 0
    assert [bool(l < 0) for l in lens] == [False, True, True, True, True, True, False, False, True]
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.ak_wordpiece_create_ex(vf.encode(), 1, b"<s>", b"</s>", b"[NOPE]", None, 0, ctypes.byref(h)) != 0
    assert "[NOPE]" in _lib.last_error()


def test_bias_and_position_offset_move_the_reference():
    """Control on the fixture weights: dropping the relative-position bias, or the positions' padding_idx + 1 offset, moves the
    float32 reference by far more than the bf16 bar -- a kernel that ignored either could not pass the GPU fixtures."""
    shape, seed, S = "mpnet-tiny-hd32", 23, 64
    rng = np.random.default_rng(0)
    lens = [64, 17, 40]
    ids, mask = pad_rows([rng.integers(5, 1000, n).tolist() for n in lens], S)
    model, _ = hf_model(shape, seed)
    base = hf_embed(model, ids, mask)

    def moved(other):
        return np.abs(other - base).max() > 10 * BF16_ABS_TOL and 1 - (other * base).sum(1).min() > 10 * BF16_COS_TOL

    no_bias, _ = hf_model(shape, seed, zero_bias=True)
    assert moved(hf_embed(no_bias, ids, mask))
    shifted = np.broadcast_to(np.arange(S), ids.shape).copy()         # positions 0 .. S - 1 instead of 2 .. S + 1
    assert moved(hf_embed(model, ids, mask, position_ids=shifted))
    assert np.allclose(hf_embed(model, ids, mask, position_ids=shifted + 2), base, atol=1e-6)


def test_seeded_weights_are_bf16_exact_with_a_large_bias():
    w, rel, pos_full = random_mpnet_weights("mpnet-tiny-hd32", seed=3)
    import torch
    m = w["l0.wq"]
    assert np.array_equal(torch.from_numpy(m).to(torch.bfloat16).float().numpy(), m)
    assert rel.shape == (32, 8) and 0.5 < rel.std() < 2.0
    assert w["pos_emb"].shape[0] == pos_full.shape[0] - 2


def test_new_abi_entries_are_declared_and_exported():
    from archi_amd import _lib
    names = {n for n, *_ in _lib.SYMBOLS}
    hdr = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    for sym in ("ak_encoder_set_rel_bias", "ak_wordpiece_create_ex"):
        assert sym + "(" in hdr
        assert sym in names
        assert hasattr(_lib.load(), sym)
    assert _lib.ABI_VERSION == 5


def test_embedding_dimensions_and_routing():
    from archi_amd.config_plugin import EMBEDDING_DIMENSIONS
    from archi_amd.embeddings import _is_mpnet
    for name in ("sentence-transformers/all-mpnet-base-v2", "sentence-transformers/multi-qa-mpnet-base-dot-v1",
                 "sentence-transformers/paraphrase-mpnet-base-v2"):
        assert EMBEDDING_DIMENSIONS[name] == 768 and _is_mpnet(name)
    assert not _is_mpnet("BAAI/bge-base-en-v1.5")
