"""CPU tests of the NomicBERT path: config.json -> shape in both config dialects (and what is refused), the checkpoint loader in both
tensor-name dialects, the host rotary table at theta 1000 against HF's, dynamic-NTK RoPE against the default up to the trained length,
the committed fixtures (reproduced from float32 NomicBertModel and sensitive enough to RoPE, its theta, the gate / up order, the
token-type row, the LayerNorm biases and the attention scale that a forward pass without one of them could not pass), the WordPiece
tokeniser against tokenizer.json, the provider's routing and refusals, the new symbols in header / binding / library, and the float64
references of the three new kernels held to float32 emulations and to their mutants (tests/nomic_kernel_refs.py)."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import archi_amd.nomic as nm
from archi_amd.nomic import NOMIC_SHAPES
from tests import kernel_refs as kr
from tests import nomic_kernel_refs as nk
from tests import nomic_ref as nr
from tests import stack_kernel_refs as sr
from tests.golden import make_nomic_fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = "nomic-tiny-256"
BASE = NOMIC_SHAPES["nomic-ai/nomic-embed-text-v1.5"]


# ---- config reader -----------------------------------------------------------------------------------------------------------------
def _hf(**change):
    d = nm.shape_hf_config(BASE).to_dict()
    d["model_type"] = "nomic_bert"
    d.update(change)
    return d


def _orig(**change):
    return nm.shape_original_config(BASE, **change)


def test_released_shapes_and_both_dialects_give_the_same_tuple():
    for name in ("nomic-ai/nomic-embed-text-v1", "nomic-ai/nomic-embed-text-v1.5", "nomic-ai/nomic-embed-text-v1-unsupervised"):
        assert NOMIC_SHAPES[name] == (30528, 768, 12, 12, 3072, 2, 8192, 1e-12, 1000.0, "mean")
    assert NOMIC_SHAPES["Snowflake/snowflake-arctic-embed-m-long"] == (30528, 768, 12, 12, 3072, 2, 8192, 1e-12, 1000.0, "cls")
    assert nm.nomic_config_shape(_hf()) == nm.nomic_config_shape(_orig()) == BASE
    assert nm.nomic_config_shape(_orig(), pooling="cls") == NOMIC_SHAPES["Snowflake/snowflake-arctic-embed-m-long"]
    for name in ("nomic-tiny-mean", "nomic-tiny-256", "nomic-base-cut2"):
        s = NOMIC_SHAPES[name]
        hf = nm.shape_hf_config(s).to_dict()
        hf["model_type"] = "nomic_bert"
        assert nm.nomic_config_shape(hf) == nm.nomic_config_shape(nm.shape_original_config(s)) == s[:9] + ("mean",)
    # an explicit head_dim equal to hidden_size / num_attention_heads is what NomicBertConfig itself writes
    assert _hf()["head_dim"] == 64


@pytest.mark.parametrize("cfg,msg", [
    (_orig(prenorm=True), "prenorm"), (_orig(qkv_proj_bias=True), "qkv_proj_bias"), (_orig(mlp_fc1_bias=True), "mlp_fc1_bias"),
    (_orig(mlp_fc2_bias=True), "mlp_fc2_bias"), (_orig(use_rms_norm=True), "use_rms_norm"), (_orig(rotary_emb_fraction=0.5), "rotary_emb_fraction"),
    (_orig(rotary_emb_interleaved=True), "rotary_emb_interleaved"), (_orig(rotary_emb_scale_base=512), "rotary_emb_scale_base"),
    (_orig(activation_function="gelu"), "activation_function"), (_orig(moe_every_n_layers=2), "moe_every_n_layers"),
    (_orig(num_experts=8), "num_experts"), (_orig(n_head=24), "n_embd / n_head"), (_orig(n_inner=3000), "n_inner"),
    (_orig(n_layer=65), "n_layer"), (_orig(model_type="bert"), "model_type"),
    (_hf(hidden_act="gelu"), "hidden_act"), (_hf(head_dim=32), "head_dim"), (_hf(num_attention_heads=24, head_dim=None), "hidden_size / num_attention_heads"),
    (_hf(rope_parameters={"rope_type": "yarn", "rope_theta": 1000.0, "factor": 2.0}), "rope_type"),
    (_hf(rope_parameters={"rope_type": "linear", "rope_theta": 1000.0, "factor": 2.0}), "rope_type"),
    (_hf(intermediate_size=3000), "intermediate_size"), (_hf(hidden_size=1152, num_attention_heads=18, head_dim=None), "hidden_size"),
    (_hf(num_hidden_layers=65), "num_hidden_layers"), (_hf(moe_every_n_layers=2), "moe_every_n_layers"),
])
def test_config_refusals_name_the_field(cfg, msg):
    with pytest.raises(ValueError, match=msg):
        nm.nomic_config_shape(cfg)


def test_dynamic_rope_checkpoint_is_accepted_with_the_row_cap():
    """transformers' dialect: rope_type dynamic + factor, rows capped at max_position_embeddings; the original dialect:
    rotary_scaling_factor, rows capped at max_trained_positions (nomic-embed-text-v1: n_positions 8192, trained on 2048)."""
    shape, dyn = nm.nomic_config_info(_hf(max_position_embeddings=2048, rope_parameters={"rope_type": "dynamic", "rope_theta": 1000.0, "factor": 2.0}))
    assert dyn and shape == BASE[:6] + (2048,) + BASE[7:]
    shape, dyn = nm.nomic_config_info(_orig(n_positions=8192, max_trained_positions=2048, rotary_scaling_factor=2.0))
    assert dyn and shape[6] == 2048
    shape, dyn = nm.nomic_config_info(_orig(n_positions=8192, max_trained_positions=2048))
    assert not dyn and shape[6] == 8192
    assert nm.nomic_config_info(_hf())[1] is False


def test_dynamic_rope_equals_default_up_to_the_trained_length():
    """HF NomicBertModel with rope_type dynamic against rope_type default on rows up to max_position_embeddings: bit for bit."""
    shape = NOMIC_SHAPES[TINY]
    w = nm.random_nomic_weights(shape, seed=2, std=0.1)
    ids, lens = nr.make_ids(shape, 2, [256, 64, 5])
    a = nr.reference(nr.hf_model(shape, w, max_position_embeddings=256), ids, lens, "mean")
    b = nr.reference(nr.hf_model(shape, w, max_position_embeddings=256, rope_parameters={"rope_type": "dynamic", "rope_theta": 1000.0, "factor": 2.0}),
                     ids, lens, "mean")
    assert np.array_equal(a, b)


# ---- weights -----------------------------------------------------------------------------------------------------------------------
def test_weight_names_load_strictly_into_nomic_bert_model():
    import torch
    from transformers import NomicBertModel
    shape = NOMIC_SHAPES[TINY]
    w = nm.random_nomic_weights(shape, seed=3)
    assert sorted(w) == sorted(nm.weight_names(shape[2])) and len(w) == 4 + 11 * shape[2]
    assert all(np.array_equal(v, torch.from_numpy(v).to(torch.bfloat16).float().numpy()) for k, v in w.items() if v.ndim == 2)
    assert not np.array_equal(w["type_emb"][0], w["type_emb"][1]) and np.abs(w["emb_ln_b"]).max() > 0.05
    model = NomicBertModel(nm.shape_hf_config(shape))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in nm.hf_state_dict(w).items()}, strict=True)
    assert nm.weight_names(1) == list(nm.GLOBAL_KEYS) + ["l0." + k for k in nm.LAYER_KEYS]
    assert nm.LAYER_KEYS == ("wq", "wk", "wv", "wo", "ln1_g", "ln1_b", "w_gate", "w_up", "w_down", "ln2_g", "ln2_b")


@pytest.mark.parametrize("prefix", ["", "model.", "nomic_bert.", "bert."])
def test_both_tensor_dialects_load_to_identical_arrays(tmp_path, prefix):
    """The same weights saved under transformers' names and under the Hub checkpoints' original ones (attn.Wqkv = q | k | v along
    dim 0, fc11 = up, fc12 = gate, norm1 / norm2, emb_ln), with an optional prefix and a masked-LM head beside them."""
    from safetensors.torch import load_file, save_file
    shape = NOMIC_SHAPES[TINY]
    w = nm.random_nomic_weights(shape, seed=4, std=0.1)
    got = {}
    for dialect in ("hf", "original"):
        d = nr.write_checkpoint(str(tmp_path / dialect), shape, w, dialect=dialect, prefix=prefix)
        f = os.path.join(d, "model.safetensors")
        sd = load_file(f)
        sd["cls.predictions.bias"] = sd[next(iter(sd))].new_zeros(shape[0])
        save_file(sd, f)
        got_shape, got[dialect] = nm.load_nomic_weights(d)
        assert got_shape == shape[:9] + ("mean",)
        assert sorted(got[dialect]) == sorted(w) and all(np.array_equal(np.asarray(got[dialect][k]), w[k]) for k in w), dialect
    names = set(load_file(os.path.join(str(tmp_path / "original"), "model.safetensors")))
    assert prefix + "encoder.layers.0.attn.Wqkv.weight" in names and prefix + "encoder.layers.1.mlp.fc11.weight" in names
    assert prefix + "emb_ln.bias" in names and not any("q_proj" in n or "gate_proj" in n for n in names)
    # the original file's tensors are the renaming table's: Wqkv chunks are q | k | v, fc11 is up, fc12 is gate
    sd = {k[len(prefix):]: v.numpy() for k, v in load_file(os.path.join(str(tmp_path / "original"), "model.safetensors")).items()}
    H = shape[1]
    assert np.array_equal(sd["encoder.layers.1.attn.Wqkv.weight"][H:2 * H], w["l1.wk"])
    assert np.array_equal(sd["encoder.layers.1.mlp.fc11.weight"], w["l1.w_up"]) and np.array_equal(sd["encoder.layers.1.mlp.fc12.weight"], w["l1.w_gate"])


def test_original_dialect_loads_into_transformers_to_the_same_model(tmp_path):
    """transformers' own conversion of the original dialect (conversion_mapping.py) gives the model our hf dialect gives: the
    renaming table restated in archi_amd.nomic is transformers'."""
    from transformers import NomicBertModel
    shape = NOMIC_SHAPES[TINY]
    w = nm.random_nomic_weights(shape, seed=5, std=0.1)
    d = nr.write_checkpoint(str(tmp_path / "orig_hfcfg"), shape, w, dialect="original")
    cfg = nm.shape_hf_config(shape).to_dict()
    cfg["model_type"], cfg["architectures"] = "nomic_bert", ["NomicBertModel"]
    json.dump({k: v for k, v in cfg.items() if k not in ("dtype", "torch_dtype")}, open(os.path.join(d, "config.json"), "w"), default=str)
    model = NomicBertModel.from_pretrained(d, attn_implementation="eager").float().eval()
    ids, lens = nr.make_ids(shape, 5, [40, 7])
    assert np.array_equal(nr.reference(model, ids, lens, "mean"), nr.reference(nr.hf_model(shape, w), ids, lens, "mean"))


# ---- rotary table ------------------------------------------------------------------------------------------------------------------
def _ulp_diff(a, b):
    ai, bi = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -(ai & 0x7fffffff), ai)
    bi = np.where(bi < 0, -(bi & 0x7fffffff), bi)
    return np.abs(ai - bi)


def test_rope_table_at_theta_1000_matches_hf():
    """The table ak_nomic_create uploads (ak_decoder_rope_table at head size 64, theta 1000) against HF's NomicBertRotaryEmbedding,
    positions 0 .. 8191: the 32 float32 inverse frequencies of the host routine, restated in numpy, equal HF's inv_freq bit for bit;
    the cos / sin rows are within 1 ulp where the frequencies are equal and within 2^-23 everywhere."""
    import torch
    from archi_amd.decoder import rope_table
    from transformers.models.nomic_bert.modeling_nomic_bert import NomicBertRotaryEmbedding
    n = 8192
    c, s = rope_table(1000.0, n, head_dim=64)
    rot = NomicBertRotaryEmbedding(config=nm.shape_hf_config(NOMIC_SHAPES[TINY]))
    hc, hs = rot(torch.zeros(1, dtype=torch.float32), torch.arange(n)[None])
    hc, hs = hc[0].numpy(), hs[0].numpy()
    inv = rot.inv_freq.numpy()
    assert c.shape == (n, 32) and hc.shape == (n, 64) and np.array_equal(hc[:, :32], hc[:, 32:]) and inv.shape == (32,)
    e = np.arange(0, 64, 2, dtype=np.float32) / np.float32(64)
    mine = (np.float32(1) / np.power(np.float64(1000.0), e.astype(np.float64)).astype(np.float32)).astype(np.float32)
    assert np.array_equal(mine.view(np.uint32), inv.view(np.uint32)), np.flatnonzero(mine != inv)
    worst_ulp = max(_ulp_diff(c, hc[:, :32]).max(), _ulp_diff(s, hs[:, :32]).max())
    worst_abs = max(np.abs(c - hc[:, :32]).max(), np.abs(s - hs[:, :32]).max())
    print(f"theta 1000: 32 of 32 frequencies equal, worst ulp distance {worst_ulp}, worst |d| {worst_abs:.3g}")
    assert worst_ulp <= 1 and worst_abs <= 2.0 ** -23


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def test_fixture_set_is_what_the_issue_lists():
    names = sorted(fx.CASES)
    assert names == ["base_cut2", "tiny_256", "tiny_cls", "tiny_long", "tiny_mean"] and all(os.path.exists(fx.path(n)) for n in names)
    assert fx.CASES["tiny_mean"][3] == [320, 130, 64, 33, 32, 17, 5, 1] and fx.CASES["tiny_cls"][3] == [513, 512, 100, 1]
    assert fx.CASES["tiny_256"][3] == [160, 129, 2] and fx.CASES["tiny_long"][3] == [8192, 300, 65]
    assert len(fx.CASES["base_cut2"][3]) == 64 and max(fx.CASES["base_cut2"][3]) == 512
    assert [NOMIC_SHAPES[fx.CASES[n][0]][:5] for n in names] == [(2000, 768, 2, 12, 3072), (1000, 256, 2, 4, 512), (1000, 128, 3, 2, 192),
                                                                 (1000, 128, 2, 2, 192), (1000, 128, 3, 2, 192)]
    assert nm.NOMIC_SHAPES["nomic-tiny-mean"][4] * 2 % 256 != 0                                # the padded-intermediate path runs
    assert all(os.path.getsize(fx.path(n)) < 512 * 1024 for n in names)
    assert all(fx.CASES[n][2] >= 0.065 for n in names) and fx.SENS_FACTOR == 10.0 and fx.MIN_SENS_ROW == 5


@pytest.mark.parametrize("name", sorted(fx.CASES))
def test_fixture_is_reproduced_and_can_see_the_features(name):
    """The committed fixture against the generating script run now (rows up to 600 tokens; the 8192-token row is the generating
    script's to pay for twice): expected to 1e-6. The bar is per figure the larger of the project's bf16 bar and the all-bf16
    NomicBertModel's own error stored in the fixture. And, mean-pooled fixtures, from NomicBertModel alone: theta 10000, no RoPE, gate
    and up swapped, the token-type row dropped, the LayerNorm biases dropped and the attention scale times sqrt(2) each move every
    row of 5 tokens or more by at least 10x the fixture's 1 - cos bar."""
    stored = fx.load(name)
    shape, seed, std, lens, pooling = fx.CASES[name]
    assert (stored["shape_name"], stored["seed"], stored["std"], stored["pooling"]) == (shape, seed, std, pooling)
    assert list(stored["lens"]) == list(lens) and stored["expected"].shape == (len(lens), NOMIC_SHAPES[shape][1])
    ids, lens_now = nr.make_ids(NOMIC_SHAPES[shape], seed, lens)
    assert np.array_equal(ids, stored["ids"])
    w = nm.random_nomic_weights(shape, seed=seed, std=std)
    short = np.flatnonzero(np.asarray(lens) <= 600)
    now = nr.reference(nr.hf_model(shape, w), ids[short], lens_now[short], pooling)
    assert np.abs(now - stored["expected"][short]).max() <= 1e-6
    assert stored["bar_cos"] == max(nr.PROJECT_BAR_COS, stored["bf16_cos"]) and stored["bar_abs"] == max(nr.PROJECT_BAR_ABS, stored["bf16_abs"])
    assert 0 < stored["bf16_cos"] and 0 < stored["bf16_abs"]
    if pooling != "mean":
        return
    sens = nr.sensitivities(shape, seed, std, stored["ids"], stored["lens"], pooling, stored["expected"])
    assert sorted(sens) == sorted(("theta", "no_rope", "swap_gate_up", "no_type", "no_ln_bias", "scale"))
    ok, text = fx.sensitivity_ok(stored, sens)
    print(f"{name}: bar {stored['bar_cos']:.3g} / {stored['bar_abs']:.3g}; {text}")
    assert ok, text


# ---- tokeniser ---------------------------------------------------------------------------------------------------------------------
def test_native_wordpiece_ids_equal_the_tokenizer_json_ids(tmp_path):
    """vocab.txt through NativeWordPiece against the same vocabulary's tokenizer.json through BpeTokenizer (the `tokenizers` wheel)
    and through transformers' fast tokenizer, on the decoder suite's multilingual CORPUS."""
    from archi_amd.decoder import BpeTokenizer
    from archi_amd.embeddings import NativeWordPiece
    from tests.decoder_ref import CORPUS
    d = str(tmp_path / "tok")
    n = nr.make_wordpiece(d, CORPUS, vocab_size=1000)
    assert 100 < n <= 1000
    native = NativeWordPiece(os.path.join(d, "vocab.txt"), lowercase=True)
    js, hf = BpeTokenizer(os.path.join(d, "tokenizer.json")), nr.hf_tokenizer(d)
    texts = [t.replace("\n", " ") for t in CORPUS] + ["", "run " * 60, "a [SEP] b"]
    for max_len in (16, 128):
        want = js.encode_batch(texts, max_len)
        assert native.encode_batch(texts, max_len) == want
        assert hf(texts, truncation=True, max_length=max_len)["input_ids"] == want
    cls, sep = want[0][0], want[0][-1]
    assert all(r[0] == cls and r[-1] == sep for r in want) and max(max(r) for r in want) < n
    native.close()


# ---- provider ----------------------------------------------------------------------------------------------------------------------
def test_provider_routes_nomic_checkpoints_and_refuses_before_any_gpu_work(tmp_path):
    from archi_amd._lib import HipBackendError
    from archi_amd.embeddings import ArchiHipEmbeddings, NativeWordPiece, _is_modernbert, _is_nomic
    from tests.decoder_ref import CORPUS
    shape = NOMIC_SHAPES[TINY]
    w = nm.random_nomic_weights(shape, seed=1, std=0.1)
    d = nr.write_checkpoint(str(tmp_path / "ckpt"), shape, w, dialect="original", pooling="cls", max_seq_length=96, corpus=CORPUS)
    assert _is_nomic(d) and not _is_modernbert(d) and _is_nomic("nomic-ai/nomic-embed-text-v1.5") and not _is_nomic("nomic-ai/modernbert-embed-base")
    try:
        emb = ArchiHipEmbeddings(d)
    except HipBackendError:
        pass
    else:       # a GPU is present: the checkpoint's sentence-transformers files were read, vocab.txt is the tokeniser
        assert (emb.pooling, emb.max_seq_length, emb.normalize, emb.dimensions) == ("cls", 96, True, 256)
        assert isinstance(emb.tokenizer, NativeWordPiece)
        emb.encoder.close()
    for p in ("f32", "bf16x3"):
        with pytest.raises(ValueError, match="bf16 only"):
            ArchiHipEmbeddings(d, model_kwargs={"precision": p})
        with pytest.raises(ValueError, match="bf16 only"):
            ArchiHipEmbeddings("nomic-ai/nomic-embed-text-v1.5", model_kwargs={"precision": p, "synthetic_seed": 0})
    with pytest.raises(FileNotFoundError, match="synthetic_seed"):
        ArchiHipEmbeddings("nomic-ai/nomic-embed-text-v1.5")
    with pytest.raises(FileNotFoundError, match="synthetic_seed"):
        ArchiHipEmbeddings("Snowflake/snowflake-arctic-embed-m-long")
    # a dynamic-NTK checkpoint: a max_seq_length past the trained length is refused by name, before the weights are read
    dyn = nr.write_checkpoint(str(tmp_path / "dyn"), shape, w, dialect="original", max_seq_length=64, corpus=CORPUS,
                              config=dict(n_positions=8192, max_trained_positions=128, rotary_scaling_factor=2.0))
    os.remove(os.path.join(dyn, "model.safetensors"))
    with pytest.raises(ValueError, match="max_seq_length 256"):
        ArchiHipEmbeddings(dyn, model_kwargs={"max_seq_length": 256})
    with pytest.raises(FileNotFoundError, match="safetensors"):              # ... and one inside it gets as far as the weights
        ArchiHipEmbeddings(dyn, model_kwargs={"max_seq_length": 128})
    # pooling other than mean / cls, a refused config field, no tokeniser at all
    json.dump({"pooling_mode_max_tokens": True}, open(os.path.join(d, "1_Pooling", "config.json"), "w"))
    with pytest.raises(ValueError, match="pooling"):
        ArchiHipEmbeddings(d)
    cfg = json.load(open(os.path.join(d, "config.json")))
    json.dump(dict(cfg, prenorm=True), open(os.path.join(d, "config.json"), "w"))
    with pytest.raises(ValueError, match="prenorm"):
        ArchiHipEmbeddings(d)
    os.remove(os.path.join(d, "vocab.txt"))
    os.remove(os.path.join(d, "tokenizer.json"))
    with pytest.raises(FileNotFoundError, match="tokenizer.json"):
        ArchiHipEmbeddings(d)


def test_handle_and_dimensions():
    from archi_amd.config_plugin import EMBEDDING_DIMENSIONS
    for name in ("nomic-ai/nomic-embed-text-v1", "nomic-ai/nomic-embed-text-v1.5", "nomic-ai/nomic-embed-text-v1-unsupervised",
                 "Snowflake/snowflake-arctic-embed-m-long"):
        assert EMBEDDING_DIMENSIONS[name] == 768 == NOMIC_SHAPES[name][1]
    assert (nm.HipNomicBert.family, nm.HipNomicBert.prefix, nm.HipNomicBert.embed_key, nm.HipNomicBert.abi_pooling) == ("nomic", "nomic", "word_emb", True)
    assert nm.HipNomicBert.matrix_keys == {"wq", "wk", "wv", "wo", "w_gate", "w_up", "w_down"}
    with pytest.raises(ValueError, match="layers"):
        nm.HipNomicBert(BASE[:2] + (65,) + BASE[3:], {})


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_in_header_binding_and_library():
    from archi_amd import _lib
    src = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    assert int(re.search(r"#define AK_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 5
    lib = _lib.load()
    assert lib.ak_abi_version() == 5
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in ("ak_nomic_create", "ak_nomic_forward_lens", "ak_nomic_destroy"):
        assert re.search(rf"\bint {name}\(", src) and name in bound and hasattr(lib, name)
    assert src.count("manager.py:373") >= 3
    args = {n: a for n, _, a in _lib.SYMBOLS}
    assert args["ak_nomic_forward_lens"] == args["ak_mbert_forward_lens"] == args["ak_encoder_forward_lens"]      # the same tile layout


def test_config_struct_matches_header():
    from archi_amd._lib import AkNomicBertConfig
    src = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    body = re.search(r"typedef struct AkNomicBertConfig \{(.*?)\} AkNomicBertConfig;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int|float)\s+(\w+)\s*;", body)
    assert [n for _, n in fields] == [n for n, _ in AkNomicBertConfig._fields_] == \
        ["vocab_size", "hidden", "layers", "heads", "intermediate", "type_vocab", "max_position", "ln_eps", "rope_theta"]
    kinds = {"int": ctypes.c_int, "float": ctypes.c_float}
    assert all(kinds[k] is t for (k, _), (_, t) in zip(fields, AkNomicBertConfig._fields_)) and ctypes.sizeof(AkNomicBertConfig) == 36


def test_nomic_wrappers_stay_out_of_the_product_library():
    """ak_kts_nb_* (csrc/kernel_test.hip) exist in libarchi_hip_dbg.so only, are exactly the nb entries of _lib.KTS_SYMBOLS, and none
    of them is in the other two sets; no library exports a wrapper under the earlier ak_ktn_* names."""
    from archi_amd import _lib

    def exported(name):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "archi_amd", "lib", name)], stdout=subprocess.PIPE,
                             check=True).stdout.decode()
        return set(re.findall(r"\b(ak_kts_nb_[a-z0-9_]+|ak_ktn_[a-z0-9_]+)\b", out))

    _lib.load()
    assert exported("libarchi_hip.so") == set()
    names = {n for n, _, _ in _lib.KTS_SYMBOLS if n.startswith("ak_kts_nb_")}
    assert exported("libarchi_hip_dbg.so") == names == {"ak_kts_nb_embed", "ak_kts_nb_add_ln", "ak_kts_nb_pool"}
    assert sum(n.startswith("ak_kts_nb_") for n, _, _ in _lib.KTS_SYMBOLS) == 3 and not hasattr(_lib, "KTN_SYMBOLS")
    others = {n for n, _, _ in _lib.KT_SYMBOLS + _lib.KTG_SYMBOLS}
    assert not names & others and not any(n.startswith(("ak_kt_", "ak_ktg_")) for n in names)
    header = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    assert "ak_kts_" not in header and "ak_ktn_" not in header


def test_new_kernels_do_not_spill_and_read_no_environment():
    """-Rpass-analysis=kernel-resource-usage with the Makefile's flags: every kernel of nomic.hip reports no spilled VGPRs and no
    scratch; the file reads no environment variable."""
    from scripts.kernel_resources import kernel_resources
    seen = {}
    for name, use in kernel_resources("nomic.hip").items():
        if "k_nb_" in name:
            seen.update({(name, key): use[key] for key in ("VGPRs Spill", "ScratchSize [bytes/lane]")})
    names = {n for n, _ in seen}
    for k in ("k_nb_embedILi1E", "k_nb_embedILi4E", "k_nb_add_lnILi1E", "k_nb_add_lnILi2E", "k_nb_add_lnILi3E", "k_nb_add_lnILi4E", "k_nb_pool_part",
              "k_nb_pool_fin"):
        assert any(k in n for n in names), (k, names)
    assert all(v == 0 for v in seen.values()), {k: v for k, v in seen.items() if v}
    src = open(os.path.join(ROOT, "archi_amd", "csrc", "nomic.hip")).read()
    assert "getenv" not in src and "switches.h" not in src
    assert "nomic.hip" in open(os.path.join(ROOT, "archi_amd", "csrc", "Makefile")).read()


# ---- kernel references -------------------------------------------------------------------------------------------------------------
def _groups():
    """{group: [(case, expect(mut), emulate())]} over every nb case of tests/test_stack_kernels_gpu.py."""
    out = {"embed": [], "addnorm": [], "pool": []}
    for c in nk.embed_cases():
        out["embed"].append((c, lambda mut=None, c=c: nk.embed_expect(c, nk.embed_inputs(c), mut), lambda c=c: nk.embed_emulate(c, nk.embed_inputs(c))))
    for c in nk.addnorm_cases():
        out["addnorm"].append((c, lambda mut=None, c=c: nk.addnorm_expect(c, nk.addnorm_inputs(c), mut),
                               lambda c=c: nk.addnorm_emulate(c, nk.addnorm_inputs(c))))
    for c in nk.pool_cases():
        for mode in nk.POOL_MODES:
            out["pool"].append((dict(c, name=f"{c['name']}:{mode[0]}", mode=mode),
                                lambda mut=None, c=c, mode=mode: nk.pool_expect(c, nk.pool_inputs(c), mode, mut),
                                lambda c=c, mode=mode: nk.pool_emulate(c, nk.pool_inputs(c), mode)))
    return out


GROUPS = _groups()


def test_kernel_case_lists_say_what_the_issue_asks():
    assert nk.HS == (128, 256, 384, 640, 768, 1024) and {c["H"] for c in nk.embed_cases()} == {c["H"] for c in nk.addnorm_cases()} == set(nk.HS)
    assert {c["S"] for c in nk.embed_cases()} == {32, 96, 192} and {c["S"] for c in nk.pool_cases()} == {32, 96, 192, 2048}
    for S in (32, 96, 192):
        assert {S, S - 1, 65, 1, 0} <= set(nk.raw_lens(S).tolist())
        assert {S, S - 1, 1, 0} <= set(nk.pool_lens(S))
    assert {63, 64, 65} <= set(nk.pool_lens(192)) and {63, 64, 65} <= set(nk.pool_lens(96))
    assert {c["H"] for c in nk.pool_cases() if c["S"] == 192} == set(nk.HS)
    c = nk.pool_cases()[0]
    x = nk.pool_inputs(c)["x"]
    assert all(np.isfinite(x[b]).all(axis=1).sum() == n for b, n in enumerate(c["lens"]))     # rows that must not be read are NaN
    assert {m[1:] for m in nk.POOL_MODES} == {(0, 1), (0, 0), (1, 1), (1, 0)}
    inp = nk.embed_inputs(nk.embed_cases()[0])
    assert inp["type"].shape[0] == 2 and not np.array_equal(inp["type"][0], inp["type"][1]) and np.abs(inp["b"]).max() > 0.1


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_float32_emulation_stays_within_the_bound(group):
    """The kernels' arithmetic restated in numpy float32, in their summation order, against the float64 statement: err / bound <= 1
    on every GPU case, exact outputs bit for bit."""
    worst, bad = kr.Worst(), []
    for c, expect, emulate in GROUPS[group]:
        bad += [f"{c['name']}:{n}" for n in sr.compare(expect(), emulate(), worst, c["name"], need_all=False)]
    print(f"{group} nb: {worst}")
    assert not bad, bad[:8]
    assert worst.n > 0 and worst.ratio <= 1.0, str(worst)


# mutant -> the groups in each of which at least one case must flag it
MUTANTS = {
    "onepass": ("embed", "addnorm"), "no_bias": ("embed", "addnorm"), "y_alone": ("addnorm",), "type_1": ("embed",), "cls_1": ("pool",),
    "div_S": ("pool",), "no_writeback": ("addnorm",), "stray_id": ("embed",), "len_unclamped": ("embed",), "n_plus_1": ("pool",),
    "n_ceil64": ("pool",),
}


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_mutant_is_flagged(mut):
    """The variance as E[x^2] - mean^2; a dropped LayerNorm bias; the LayerNorm of y alone; token-type row 1; cls reading token 1;
    the mean divided by S; the normalised row not written back to x32; a stray id read as it is; the length not clamped; pooling n + 1
    / ceil(n / 64) 64 tokens -- each, applied to the reference, misses the expectation on the GPU tests' own inputs."""
    for group in MUTANTS[mut]:
        hit = []
        for c, expect, _ in GROUPS[group]:
            if group == "pool" and ((mut == "cls_1") != (c["mode"][1] == 1)) and mut in ("cls_1", "div_S"):
                continue                                                   # cls_1 shows under cls pooling, div_S under mean pooling
            if (not hit or group != "pool") and sr.flagged(expect(), expect(mut)):
                hit.append(c["name"])
        print(f"{mut} / {group}: {len(hit)} cases")
        assert hit, (mut, group)
    if mut in ("no_bias", "y_alone", "no_writeback", "type_1"):           # these show in EVERY case of their kernels
        for group in MUTANTS[mut]:
            assert all(sr.flagged(expect(), expect(mut)) for _, expect, _ in GROUPS[group]), (mut, group)
