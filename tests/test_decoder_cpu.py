"""CPU tests of the Qwen3 decoder path (no GPU): the checkpoint loader and its refusals, the byte-level BPE tokenizer wrapper
against transformers' fast tokenizer, the host RoPE table against HF's rotary embedding, the C struct's size, and the provider's
refusals for decoder checkpoints."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from archi_amd import decoder as dm
from archi_amd.decoder import QWEN3_SHAPES, random_qwen3_weights
from tests.decoder_ref import CORPUS, hf_config, make_tokenizer_json, write_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = "qwen3-tiny-g2"


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("qwen3") / "ckpt")
    w = random_qwen3_weights(TINY, seed=3)
    write_checkpoint(d, QWEN3_SHAPES[TINY], w, max_seq_length=64)
    return d, w


def test_loader_maps_save_pretrained_into_header_order(ckpt):
    d, w = ckpt
    shape, got = dm.load_qwen3_weights(d)
    assert shape == QWEN3_SHAPES[TINY]
    names = dm.weight_order(shape[2])
    assert names[:2] == ["embed_tokens", "norm"]
    assert names[2:13] == [f"l0.{k}" for k in ("wq", "wk", "wv", "q_norm", "k_norm", "wo", "ln_in", "ln_post", "w_gate", "w_up", "w_down")]
    assert len(names) == 2 + 11 * shape[2] and set(got) == set(names)
    for k in names:
        assert np.array_equal(np.asarray(got[k], np.float32), w[k]), k


def test_loader_strips_model_prefix(ckpt, tmp_path):
    from safetensors.torch import load_file, save_file
    d, w = ckpt
    sd = load_file(os.path.join(d, "model.safetensors"))
    e = tmp_path / "prefixed"
    e.mkdir()
    save_file({"model." + k: v.contiguous() for k, v in sd.items()}, str(e / "model.safetensors"))
    (e / "config.json").write_text(open(os.path.join(d, "config.json")).read())
    _, got = dm.load_qwen3_weights(str(e))
    assert np.array_equal(np.asarray(got["l1.wo"], np.float32), w["l1.wo"])


def _cfg(**kw):
    c = json.loads(hf_config(TINY).to_json_string())
    c.update(kw)
    return c


def test_config_reads_rope_theta_both_places():
    c = _cfg()
    c.pop("rope_theta", None)
    c["rope_parameters"] = {"rope_type": "default", "rope_theta": 12345.0}
    assert dm.qwen3_config_shape(c)[7] == 12345.0
    c = _cfg()
    c.pop("rope_parameters", None)
    c["rope_theta"] = 777.0
    assert dm.qwen3_config_shape(c)[7] == 777.0


@pytest.mark.parametrize("change, msg", [
    ({"hidden_act": "gelu"}, "hidden_act"),
    ({"attention_bias": True}, "attention_bias"),
    ({"use_sliding_window": True}, "sliding"),
    ({"rope_scaling": {"rope_type": "yarn", "factor": 4.0}}, "rope type"),
    ({"rope_parameters": {"rope_type": "linear", "factor": 2.0, "rope_theta": 1e6}}, "rope type"),
    ({"head_dim": 64}, "head_dim"),
    ({"model_type": "llama"}, "qwen3"),
])
def test_config_refusals(change, msg):
    with pytest.raises(ValueError, match=msg):
        dm.qwen3_config_shape(_cfg(**change))


def test_load_hf_weights_stays_bert_only(ckpt):
    from archi_amd.encoder import load_hf_weights
    with pytest.raises(ValueError, match="not BERT"):
        load_hf_weights(ckpt[0])


def test_decoder_st_config(ckpt, tmp_path):
    assert dm.read_decoder_st_config(ckpt[0]) == (64, True)
    e = tmp_path / "meanpool"
    (e / "1_Pooling").mkdir(parents=True)
    (e / "1_Pooling" / "config.json").write_text(json.dumps({"pooling_mode_mean_tokens": True}))
    with pytest.raises(ValueError, match="lasttoken"):
        dm.read_decoder_st_config(str(e))


TEXTS = CORPUS + ["", "a", "µσé “quoted” ‘single’ – dash", "naïve café — 3 µm ± 0.2 σ", "x " * 700, "Ω" * 300,
                  "Instruct: Given a physics question, retrieve relevant passages Query:what is σ?"]


@pytest.mark.parametrize("max_len", [8, 64, 512])
def test_tokenizer_matches_transformers_fast(tmp_path, max_len):
    from transformers import PreTrainedTokenizerFast
    tf = make_tokenizer_json(str(tmp_path / "tokenizer.json"))
    ours = dm.BpeTokenizer(tf)
    ref = PreTrainedTokenizerFast(tokenizer_file=tf)
    want = ref(TEXTS, truncation=True, max_length=max_len)["input_ids"]
    got = ours.encode_batch(TEXTS, max_len)
    assert got == want
    eot = ref.convert_tokens_to_ids("<|endoftext|>")
    assert all(r[-1] == eot for r in got)                    # the post-processor's token is what the last-token pool reads
    assert max(len(r) for r in got) == max_len               # some texts are over the limit
    ids, lens = ours.encode_batch_array(TEXTS, max_len)
    assert ids.shape == (len(TEXTS), max_len) and [ids[i, :n].tolist() for i, n in enumerate(lens)] == want


def _ulp_diff(a, b):
    ai, bi = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -(ai & 0x7fffffff), ai)
    bi = np.where(bi < 0, -(bi & 0x7fffffff), bi)
    return np.abs(ai - bi)


def _hf_cos_sin(theta, n_pos):
    import torch
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RotaryEmbedding
    cfg = hf_config((1000, 256, 1, 2, 1, 256, n_pos, theta, 1e-6))
    rot = Qwen3RotaryEmbedding(config=cfg)
    cos, sin = rot(torch.zeros(1, dtype=torch.float32), torch.arange(n_pos)[None])
    return cos[0].numpy(), sin[0].numpy(), rot.inv_freq.numpy()


@pytest.mark.parametrize("theta", [1e4, 5e5, 1e6])
def test_rope_table_matches_hf(theta):
    n = 8192
    c, s = dm.rope_table(theta, n)
    hc, hs, inv = _hf_cos_sin(theta, n)
    assert np.array_equal(hc[:, :64], hc[:, 64:]) and c.shape == (n, 64)
    # the table's inverse frequencies are 1 / theta^(2i/128) rounded once from double; HF's come from torch's vectorised float32
    # pow, which at theta = 1e6 is one ulp off the correctly rounded value at i = 37 -- and an angle of thousands of radians
    # magnifies that ulp. The 1-ulp bar is held wherever the frequencies agree.
    e = np.arange(0, 128, 2, dtype=np.float32) / np.float32(128)
    mine = (np.float32(1) / np.power(np.float64(theta), e.astype(np.float64)).astype(np.float32)).astype(np.float32)
    same = mine == inv
    assert same.sum() >= 63
    assert _ulp_diff(c[:, same], hc[:, :64][:, same]).max() <= 1
    assert _ulp_diff(s[:, same], hs[:, :64][:, same]).max() <= 1
    assert np.abs(c - hc[:, :64]).max() <= 2 ** -21 and np.abs(s - hs[:, :64]).max() <= 2 ** -21


def test_rope_table_refuses_bad_arguments():
    from archi_amd import _lib
    lib = _lib.load()
    buf = np.empty(64, np.float32)
    assert lib.ak_decoder_rope_table(ctypes.c_float(1e6), 127, 1, buf.ctypes.data, buf.ctypes.data) != 0
    assert lib.ak_decoder_rope_table(ctypes.c_float(0.0), 128, 1, buf.ctypes.data, buf.ctypes.data) != 0


def test_decoder_config_struct_matches_header():
    from archi_amd._lib import AkDecoderConfig
    src = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    body = re.search(r"typedef struct AkDecoderConfig \{(.*?)\} AkDecoderConfig;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int|float)\s+(\w+)\s*;", body)
    assert [n for _, n in fields] == [n for n, _ in AkDecoderConfig._fields_]
    assert ctypes.sizeof(AkDecoderConfig) == 4 * len(fields) == 40
    kinds = {"int": ctypes.c_int, "float": ctypes.c_float}
    assert all(kinds[k] is t for (k, _), (_, t) in zip(fields, AkDecoderConfig._fields_))


def test_abi_version_bumped_together():
    from archi_amd import _lib
    src = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    assert int(re.search(r"#define AK_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 5
    assert _lib.load().ak_abi_version() == 5


def test_embedding_dimensions_for_qwen3():
    from archi_amd.config_plugin import EMBEDDING_DIMENSIONS
    assert EMBEDDING_DIMENSIONS["Qwen/Qwen3-Embedding-0.6B"] == 1024
    assert EMBEDDING_DIMENSIONS["Qwen/Qwen3-Embedding-4B"] == 2560
    assert EMBEDDING_DIMENSIONS["Qwen/Qwen3-Embedding-8B"] == 4096
    for name in ("Qwen/Qwen3-Embedding-0.6B", "Qwen/Qwen3-Embedding-4B", "Qwen/Qwen3-Embedding-8B"):
        assert QWEN3_SHAPES[name][1] == EMBEDDING_DIMENSIONS[name]


def test_provider_refuses_parity_modes_for_decoders(ckpt):
    from archi_amd.embeddings import ArchiHipEmbeddings
    for p in ("f32", "bf16x3"):
        with pytest.raises(ValueError, match="bf16 only"):
            ArchiHipEmbeddings(ckpt[0], model_kwargs={"precision": p})
    with pytest.raises(FileNotFoundError):
        ArchiHipEmbeddings("Qwen/Qwen3-Embedding-0.6B")      # no checkpoint, no synthetic_seed


def test_bert_lasttoken_still_refused(tmp_path):
    from archi_amd.encoder import read_sentence_transformers_config
    (tmp_path / "1_Pooling").mkdir()
    (tmp_path / "1_Pooling" / "config.json").write_text(json.dumps({"pooling_mode_lasttoken": True}))
    with pytest.raises(ValueError, match="cls and mean"):
        read_sentence_transformers_config(str(tmp_path))
