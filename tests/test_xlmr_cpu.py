"""CPU tests of the XLM-RoBERTa path (bge-m3, multilingual-e5, paraphrase-multilingual-mpnet-base-v2): the checkpoint loader and
what it refuses, the tokenizer.json route against transformers' fast tokenizer (literal <pad> / <mask> included), tokenizer routing
of BERT directories, the refusal of rows over 512 tokens before any GPU work, the new C ABI entry, dimensions and routing, a control
that the fixtures' positions matter, and a compile check that the kernels the feature adds or touches do not spill."""
import json
import os
import re

import numpy as np
import pytest

from archi_amd.encoder import XLMR_SHAPES, load_hf_weights, load_xlmr_weights, random_xlmr_weights, weight_order
from tests.xlmr_ref import (PAD_ID, TEXTS, TOKENIZER_JSON, hf_embed, hf_model, hf_tokenizer, offset_positions, pad_rows,
                            write_checkpoint)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16_ABS_TOL, BF16_COS_TOL = 3e-3, 3e-4     # the bf16 bar of the GPU tests


def test_loader_reads_an_xlmr_checkpoint(tmp_path):
    d = str(tmp_path / "m")
    model = write_checkpoint(d, "xlmr-tiny-hd64", seed=1)
    shape, w, eps, pad = load_xlmr_weights(d)
    assert shape == XLMR_SHAPES["xlmr-tiny-hd64"][:6] and eps == 1e-5 and pad == PAD_ID
    assert set(weight_order(shape[2])) <= set(w)
    sd = model.state_dict()
    # the FULL position table (padding_idx row included) and the model's own, non-zero token-type row
    assert np.array_equal(np.asarray(w["pos_emb"]), sd["embeddings.position_embeddings.weight"].numpy())
    tt = sd["embeddings.token_type_embeddings.weight"].numpy()
    assert tt.shape[0] == 1 and np.abs(tt).max() > 0 and np.array_equal(np.asarray(w["type_emb"]), tt)
    assert np.array_equal(np.asarray(w["l1.wo"]), sd["encoder.layer.1.attention.output.dense.weight"].numpy())
    assert np.array_equal(np.asarray(w["l0.ln2_g"]), sd["encoder.layer.0.output.LayerNorm.weight"].numpy())
    # the BERT loader keeps refusing it
    with pytest.raises(ValueError, match="not BERT"):
        load_hf_weights(d)


def test_loader_strips_prefixes_and_reads_roberta(tmp_path):
    from safetensors.torch import load_file, save_file
    d = str(tmp_path / "m")
    write_checkpoint(d, "xlmr-tiny-hd32", seed=2)
    st = os.path.join(d, "model.safetensors")
    ref = load_xlmr_weights(d)[1]
    sd0 = load_file(st)
    assert not any(k.startswith(("roberta.", "model.")) for k in sd0)
    for prefix, mtype in (("roberta.", "roberta"), ("model.", "xlm-roberta")):
        save_file({prefix + k: v.contiguous() for k, v in sd0.items()}, st)
        cfg = json.load(open(os.path.join(d, "config.json")))
        cfg["model_type"] = mtype
        json.dump(cfg, open(os.path.join(d, "config.json"), "w"))
        w = load_xlmr_weights(d)[1]
        assert all(np.array_equal(np.asarray(w[k]), np.asarray(ref[k])) for k in ref), prefix


@pytest.mark.parametrize("change, match", [({"model_type": "bert"}, "not XLM-RoBERTa"), ({"hidden_act": "relu"}, "hidden_act"),
                                           ({"position_embedding_type": "relative_key"}, "position_embedding_type"),
                                           ({"num_attention_heads": 2}, "head size"),
                                           ({"hidden_size": 1280, "num_attention_heads": 20}, "hidden_size")])
def test_loader_refuses_what_it_does_not_implement(tmp_path, change, match):
    d = str(tmp_path / "m")
    write_checkpoint(d, "xlmr-tiny-hd64", seed=1)
    cj = os.path.join(d, "config.json")
    cfg = json.load(open(cj))
    cfg.update(change)
    json.dump(cfg, open(cj, "w"))
    with pytest.raises(ValueError, match=match):
        load_xlmr_weights(d)


@pytest.mark.parametrize("max_len", [8, 64, 512])
def test_tokenizer_matches_transformers_fast(max_len):
    from archi_amd.decoder import BpeTokenizer
    ref = hf_tokenizer()
    ours = BpeTokenizer(TOKENIZER_JSON)
    want = ref(TEXTS, truncation=True, max_length=max_len)["input_ids"]
    got = ours.encode_batch(TEXTS, max_len)
    assert got == want
    assert all(r[0] == 0 and r[-1] == 2 for r in got)                 # <s> ... </s>
    assert any(PAD_ID in r[1:-1] for r in got)                        # a literal <pad> is the pad id
    mask_id = ref.convert_tokens_to_ids("<mask>")
    assert any(mask_id in r for r in got)
    ids, lens = ours.encode_batch_array(TEXTS, max_len)
    assert [ids[i, :n].tolist() for i, n in enumerate(lens)] == want


def _bert_dir(tmp_path, vocab, tokjson):
    from tests.hf_checkpoint import write_checkpoint as write_bert
    d = str(tmp_path / f"bert_{int(vocab)}{int(tokjson)}")
    write_bert(d)
    if not vocab:
        os.remove(os.path.join(d, "vocab.txt"))
    if tokjson:
        import shutil
        shutil.copy(TOKENIZER_JSON, os.path.join(d, "tokenizer.json"))
    return d


@pytest.mark.parametrize("vocab, tokjson, want", [(False, True, "BpeTokenizer"), (True, False, "NativeWordPiece"),
                                                   (True, True, "NativeWordPiece"), (False, False, None)])
def test_bert_directory_tokenizer_routing(tmp_path, monkeypatch, vocab, tokjson, want):
    """A BERT checkpoint takes vocab.txt (native WordPiece, unchanged) when it has one, else its tokenizer.json, else is refused
    with a message naming vocab.txt; the encoder itself is not built here."""
    import archi_amd.embeddings as em
    d = _bert_dir(tmp_path, vocab, tokjson)
    monkeypatch.setattr(em, "HipEncoder", lambda *a, **k: None)
    if want is None:
        with pytest.raises(FileNotFoundError, match="vocab.txt"):
            em.ArchiHipEmbeddings(d)
        return
    emb = em.ArchiHipEmbeddings(d)
    assert type(emb.tokenizer).__name__ == want


def test_xlmr_directory_routing_and_tokenizer(tmp_path, monkeypatch):
    import archi_amd.embeddings as em
    d = str(tmp_path / "x")
    write_checkpoint(d, "xlmr-tiny-hd64", seed=1, pooling="cls", max_seq_length=128)
    seen = {}
    monkeypatch.setattr(em, "HipEncoder", lambda *a, **k: seen.update(k))
    emb = em.ArchiHipEmbeddings(d)
    assert type(emb.tokenizer).__name__ == "BpeTokenizer" and emb.pooling == "cls" and emb.normalize
    assert emb.max_seq_length == 128 and seen["positions_from_ids"] == PAD_ID and seen["ln_eps"] == 1e-5
    os.remove(os.path.join(d, "tokenizer.json"))
    with pytest.raises(FileNotFoundError, match="tokenizer.json"):
        em.ArchiHipEmbeddings(d)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
def test_long_rows_in_parity_modes_are_refused_before_gpu_work(tmp_path, monkeypatch, precision):
    """bge-m3 asks for 8192-token rows, which run in bf16 only: in f32 / bf16x3 they are refused (no silent truncation) with the
    model_kwargs that truncate at 512, before any weights are made or any GPU work; with that setting the model routes as usual."""
    import archi_amd.embeddings as em
    monkeypatch.setattr(em, "random_xlmr_weights", lambda *a, **k: pytest.fail("weights built before the refusal"))
    with pytest.raises(ValueError, match=r"'max_seq_length': 512"):
        em.ArchiHipEmbeddings("BAAI/bge-m3", model_kwargs={"synthetic_seed": 0, "precision": precision})
    d = str(tmp_path / "x")
    write_checkpoint(d, "xlmr-long-hd64", seed=1, max_seq_length=8192)
    with pytest.raises(ValueError, match=r"'max_seq_length': 512"):
        em.ArchiHipEmbeddings(d, model_kwargs={"precision": precision})
    seen = {}
    monkeypatch.setattr(em, "HipEncoder", lambda *a, **k: seen.update(k))
    emb = em.ArchiHipEmbeddings(d, model_kwargs={"precision": precision, "max_seq_length": 512})
    assert emb.max_seq_length == 512 and seen["positions_from_ids"] == PAD_ID and seen["precision"] == precision


def test_long_rows_route_in_bf16_at_head_size_64(tmp_path, monkeypatch):
    import archi_amd.embeddings as em
    from archi_amd.encoder import long_rows_supported
    d = str(tmp_path / "x")
    write_checkpoint(d, "xlmr-long-hd64", seed=1, max_seq_length=8192)
    seen = {}
    monkeypatch.setattr(em, "HipEncoder", lambda *a, **k: seen.update(k))
    emb = em.ArchiHipEmbeddings(d)
    assert emb.max_seq_length == 8192 and seen["positions_from_ids"] == PAD_ID and seen["precision"] == "bf16"
    assert long_rows_supported(1024, 16, "bf16") and not long_rows_supported(256, 8, "bf16")
    assert not long_rows_supported(384, 6, "bf16") and not long_rows_supported(1024, 16, "f32")
    d = str(tmp_path / "hd32")                                         # head size 32: 512 at most
    write_checkpoint(d, "xlmr-tiny-hd32", seed=1, max_seq_length=512)
    cj = os.path.join(d, "config.json")
    cfg = json.load(open(cj))
    cfg["max_position_embeddings"] = 8194
    json.dump(cfg, open(cj, "w"))
    with pytest.raises(ValueError, match="head size 32"):
        em.ArchiHipEmbeddings(d, model_kwargs={"max_seq_length": 4096})


def test_positions_decide_the_reference():
    """Control on the fixture weights: the offset scheme's positions (ignoring pad ids inside a row) move the float32 reference far
    past the bf16 bar on rows holding a literal <pad>, and equal HF's own positions on rows without one."""
    shape, seed, S = "xlmr-tiny-hd64", 61, 64
    rng = np.random.default_rng(0)
    toks = [rng.integers(4, 1000, n).tolist() for n in (64, 30, 41)]
    toks[0][5] = toks[1][9] = PAD_ID
    ids, mask = pad_rows(toks, S)
    model, _ = hf_model(shape, seed)
    base = hf_embed(model, ids, mask, pooling="mean")
    off = hf_embed(model, ids, mask, pooling="mean", position_ids=offset_positions(ids))
    assert np.abs(off[:2] - base[:2]).max() > 10 * BF16_ABS_TOL and 1 - (off[:2] * base[:2]).sum(1).max() > 10 * BF16_COS_TOL
    assert np.allclose(off[2], base[2], atol=1e-6)


def test_seeded_weights_are_bf16_exact_with_one_token_type_row():
    import torch
    w = random_xlmr_weights("xlmr-tiny-hd32", seed=3)
    for k in ("l0.wq", "word_emb", "pos_emb", "type_emb"):
        m = w[k]
        assert np.array_equal(torch.from_numpy(m).to(torch.bfloat16).float().numpy(), m)
    assert w["type_emb"].shape == (1, 256) and w["pos_emb"].shape == (514, 256)


def test_new_abi_entry_is_declared_and_exported():
    from archi_amd import _lib
    names = {n for n, *_ in _lib.SYMBOLS}
    hdr = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    assert "ak_encoder_set_positions_from_ids(" in hdr
    assert "ak_encoder_set_positions_from_ids" in names
    assert hasattr(_lib.load(), "ak_encoder_set_positions_from_ids")
    assert _lib.ABI_VERSION == 5


def test_embedding_dimensions_and_routing():
    from archi_amd.config_plugin import EMBEDDING_DIMENSIONS
    from archi_amd.embeddings import _is_mpnet, _is_xlmr
    want = {"BAAI/bge-m3": 1024, "intfloat/multilingual-e5-large": 1024, "intfloat/multilingual-e5-base": 768,
            "sentence-transformers/paraphrase-multilingual-mpnet-base-v2": 768}
    for name, dim in want.items():
        assert EMBEDDING_DIMENSIONS[name] == dim and XLMR_SHAPES[name][1] == dim and _is_xlmr(name) and not _is_mpnet(name)
    assert not _is_xlmr("BAAI/bge-base-en-v1.5") and not _is_xlmr("sentence-transformers/all-mpnet-base-v2")


def test_touched_kernels_do_not_spill():
    """-Rpass-analysis=kernel-resource-usage on encoder.hip and encoder_f32.hip: k_positions and every embedding kernel that reads
    the position rows report `VGPRs Spill: 0` (and no scratch)."""
    from scripts.kernel_resources import HIPCC, kernel_resources
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    seen = {}
    for src in ("encoder.hip", "encoder_f32.hip", "attn_long.hip"):
        for name, use in kernel_resources(src).items():
            if re.search(r"k_positions|k_embed|k32_embed|k3_embed|k_attn_long|k_pool", name):
                seen[name] = use["VGPRs Spill"]
    assert all(any(k in n for n in seen) for k in ("k_positions", "k3_embed", "k_attn_long", "k_pool")) and len(seen) >= 10, seen
    assert all(v == 0 for v in seen.values()), seen
