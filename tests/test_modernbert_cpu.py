"""CPU tests of the ModernBERT path: config.json -> shape (and what is refused), weight naming against transformers.ModernBertModel,
the interleaved Wi layout of the GeGLU epilogue, the host rotary tables at head size 64 for both thetas, the provider's routing and
refusals, the three new symbols in header / binding / library, and the committed fixtures: reproduced from ModernBertModel (float32,
eager attention) and sensitive enough to the window and to the second theta that a forward pass without them could not pass."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import archi_amd.modernbert as mb
from archi_amd.modernbert import MODERNBERT_SHAPES
from tests.golden import make_modernbert_fixtures as fx
from tests.modernbert_ref import PROJECT_BAR_ABS, PROJECT_BAR_COS, hf_model, write_checkpoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = "modernbert-tiny-256"


def _cfg(**change):
    from transformers import ModernBertConfig
    d = ModernBertConfig().to_dict()
    d.update(change)
    for k in [k for k, v in change.items() if v is None]:
        d.pop(k)
    return d


def test_default_config_is_the_base_shape():
    assert mb.modernbert_config_shape(_cfg()) == MODERNBERT_SHAPES["answerdotai/ModernBERT-base"]
    assert mb.modernbert_config_shape(_cfg(), pooling="cls") == MODERNBERT_SHAPES["Alibaba-NLP/gte-modernbert-base"]
    large = _cfg(hidden_size=1024, num_hidden_layers=28, num_attention_heads=16, intermediate_size=2624, layer_types=None,
                 global_attn_every_n_layers=3)
    assert mb.modernbert_config_shape(large) == MODERNBERT_SHAPES["lightonai/modernbert-embed-large"]


def test_config_of_transformers_4_checkpoints():
    """global_attn_every_n_layers / global_rope_theta / local_rope_theta instead of layer_types / rope_parameters."""
    old = _cfg(layer_types=None, rope_parameters=None, global_attn_every_n_layers=3, global_rope_theta=160000.0, local_rope_theta=10000.0)
    assert mb.modernbert_config_shape(old) == MODERNBERT_SHAPES["answerdotai/ModernBERT-base"]


@pytest.mark.parametrize("change,msg", [
    ({"attention_bias": True}, "attention_bias"), ({"mlp_bias": True}, "mlp_bias"), ({"norm_bias": True}, "norm_bias"),
    ({"hidden_activation": "silu"}, "hidden_activation"), ({"num_attention_heads": 24}, "head size"),
    ({"rope_parameters": {"full_attention": {"rope_type": "yarn", "rope_theta": 160000.0},
                          "sliding_attention": {"rope_type": "default", "rope_theta": 10000.0}}}, "rope_type"),
    ({"layer_types": None}, "layer_types"), ({"local_attention": 127}, "local_attention"), ({"model_type": "bert"}, "model_type"),
    ({"intermediate_size": 1100}, "intermediate_size"), ({"rope_parameters": None}, "rope theta"),
])
def test_config_refusals_name_the_field(change, msg):
    with pytest.raises(ValueError, match=msg):
        mb.modernbert_config_shape(_cfg(**change))


def test_weight_names_load_strictly_and_round_trip(tmp_path):
    import torch
    from transformers import ModernBertModel
    shape = MODERNBERT_SHAPES[TINY]
    w = mb.random_modernbert_weights(shape, seed=3)
    assert sorted(w) == sorted(mb.weight_names(shape[2])) and "l0.attn_norm" not in w
    assert all(np.array_equal(v, torch.from_numpy(v).to(torch.bfloat16).float().numpy()) for k, v in w.items() if v.ndim == 2)
    model = ModernBertModel(mb.shape_hf_config(shape))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in mb.hf_state_dict(w).items()}, strict=True)
    d = str(tmp_path / "ckpt")
    model.save_pretrained(d, safe_serialization=True)
    got_shape, got = mb.load_modernbert_weights(d)
    assert got_shape == shape[:11] + ("mean",)
    assert sorted(got) == sorted(w) and all(np.array_equal(np.asarray(got[k]), w[k]) for k in w)
    # a "model." prefix (masked-LM checkpoints) is stripped
    from safetensors.torch import load_file, save_file
    sd = load_file(os.path.join(d, "model.safetensors"))
    save_file({"model." + k: v for k, v in sd.items()}, os.path.join(d, "model.safetensors"))
    _, again = mb.load_modernbert_weights(d)
    assert all(np.array_equal(np.asarray(again[k]), w[k]) for k in w)


def test_interleaved_wi_geglu_equals_hf_mlp():
    """gemm.hip MODE 8 restated in numpy on the interleaved rows (row 2 j = Wi row j, row 2 j + 1 = Wi row I + j) against HF's
    ModernBertMLP on the original rows."""
    import torch
    shape = MODERNBERT_SHAPES[TINY]
    w = mb.random_modernbert_weights(shape, seed=8, std=0.1)
    mlp = hf_model(shape, w).layers[1].mlp
    x = torch.randn(37, shape[1], generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        want = mlp(x).numpy()
    wi = mb.interleave_wi(w["l1.wi"])
    I = shape[4]
    assert np.array_equal(wi[0::2], w["l1.wi"][:I]) and np.array_equal(wi[1::2], w["l1.wi"][I:])
    got = mb.geglu_interleaved(x.numpy() @ wi.T) @ w["l1.mlp_wo"].T
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max())


def _ulp_diff(a, b):
    ai, bi = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -(ai & 0x7fffffff), ai)
    bi = np.where(bi < 0, -(bi & 0x7fffffff), bi)
    return np.abs(ai - bi)


@pytest.mark.parametrize("kind,theta", [("full_attention", 160000.0), ("sliding_attention", 10000.0)])
def test_rope_tables_at_head_size_64_match_hf(kind, theta):
    """The tables ak_mbert_create uploads (ak_decoder_rope_table at head_dim 64) against HF's ModernBertRotaryEmbedding, positions
    0 .. 8191. Measured: for both thetas all 32 float32 inverse frequencies equal HF's bit for bit, the worst ulp distance of cos / sin
    is 1 and the worst absolute distance 6.0e-8 (HF rounds cos / sin in float32 arithmetic, the table once from double)."""
    import torch
    from archi_amd.decoder import rope_table
    from transformers.models.modernbert.modeling_modernbert import ModernBertRotaryEmbedding
    n = 8192
    c, s = rope_table(theta, n, head_dim=64)
    rot = ModernBertRotaryEmbedding(config=mb.shape_hf_config(MODERNBERT_SHAPES[TINY]))
    hc, hs = rot(torch.zeros(1, dtype=torch.float32), torch.arange(n)[None], layer_type=kind)
    hc, hs = hc[0].numpy(), hs[0].numpy()
    inv = getattr(rot, f"{kind}_inv_freq").numpy()
    assert c.shape == (n, 32) and hc.shape == (n, 64) and np.array_equal(hc[:, :32], hc[:, 32:])
    e = np.arange(0, 64, 2, dtype=np.float32) / np.float32(64)
    mine = (np.float32(1) / np.power(np.float64(theta), e.astype(np.float64)).astype(np.float32)).astype(np.float32)
    same = mine == inv
    worst_ulp = max(_ulp_diff(c[:, same], hc[:, :32][:, same]).max(), _ulp_diff(s[:, same], hs[:, :32][:, same]).max())
    worst_abs = max(np.abs(c - hc[:, :32]).max(), np.abs(s - hs[:, :32]).max())
    print(f"{kind} theta {theta:g}: {same.sum()} of 32 frequencies equal, worst ulp distance there {worst_ulp}, worst |d| overall {worst_abs:.3g}")
    assert same.all() and worst_ulp <= 1 and worst_abs <= 2.0 ** -23


def test_provider_routes_modernbert_checkpoints(tmp_path):
    """A model_type modernbert directory reaches the GPU initialisation (HipBackendError on a machine without a GPU) instead of
    "model_type 'modernbert' is not BERT"; without tokenizer.json: FileNotFoundError; the parity precisions: ValueError."""
    from archi_amd._lib import HipBackendError
    from archi_amd.embeddings import ArchiHipEmbeddings, _is_modernbert
    d = str(tmp_path / "ckpt")
    write_checkpoint(d, TINY, seed=1, pooling="cls", max_seq_length=96)
    assert _is_modernbert(d) and _is_modernbert("nomic-ai/modernbert-embed-base") and not _is_modernbert("BAAI/bge-base-en-v1.5")
    try:
        emb = ArchiHipEmbeddings(d)
    except HipBackendError:
        pass
    else:       # a GPU is present: the checkpoint's sentence-transformers files were read
        assert (emb.pooling, emb.max_seq_length, emb.normalize, emb.dimensions) == ("cls", 96, True, 256)
        emb.encoder.close()
    for p in ("f32", "bf16x3"):
        with pytest.raises(ValueError, match="bf16 only"):
            ArchiHipEmbeddings(d, model_kwargs={"precision": p})
        with pytest.raises(ValueError, match="bf16 only"):
            ArchiHipEmbeddings("nomic-ai/modernbert-embed-base", model_kwargs={"precision": p, "synthetic_seed": 0})
    os.remove(os.path.join(d, "tokenizer.json"))
    with pytest.raises(FileNotFoundError, match="tokenizer.json"):
        ArchiHipEmbeddings(d)
    with pytest.raises(FileNotFoundError, match="synthetic_seed"):
        ArchiHipEmbeddings("nomic-ai/modernbert-embed-base")
    cfg = json.load(open(os.path.join(d, "config.json")))
    json.dump(dict(cfg, mlp_bias=True), open(os.path.join(d, "config.json"), "w"))
    open(os.path.join(d, "tokenizer.json"), "w").write("{}")
    with pytest.raises(ValueError, match="mlp_bias"):
        ArchiHipEmbeddings(d)


def test_tokenizer_matches_transformers_fast(tmp_path):
    from archi_amd.decoder import BpeTokenizer
    from tests.modernbert_ref import TEXTS, hf_tokenizer, make_tokenizer_json
    tf = make_tokenizer_json(str(tmp_path / "tokenizer.json"))
    ours, theirs = BpeTokenizer(tf), hf_tokenizer(tf)
    for max_len in (16, 128):
        want = theirs(list(TEXTS), truncation=True, max_length=max_len)["input_ids"]
        assert ours.encode_batch(list(TEXTS), max_len) == want
    assert all(r[0] == 1 and r[-1] == 2 for r in want)


def test_symbols_in_header_binding_and_library():
    from archi_amd import _lib
    src = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    assert int(re.search(r"#define AK_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 5
    lib = _lib.load()
    assert lib.ak_abi_version() == 5
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in ("ak_mbert_create", "ak_mbert_forward_lens", "ak_mbert_destroy"):
        assert re.search(rf"\bint {name}\(", src) and name in bound and hasattr(lib, name)
    assert int(re.search(r"#define AK_MBERT_MAX_LAYERS (\d+)", src).group(1)) == _lib.MBERT_MAX_LAYERS


def test_config_struct_matches_header():
    from archi_amd._lib import MBERT_MAX_LAYERS, AkModernBertConfig
    src = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    body = re.search(r"typedef struct AkModernBertConfig \{(.*?)\} AkModernBertConfig;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int|float)\s+(\w+)\s*(\[\w+\])?;", body)
    assert [n for _, n, _ in fields] == [n for n, _ in AkModernBertConfig._fields_]
    assert fields[-1][2] == "[AK_MBERT_MAX_LAYERS]" and all(not a for _, _, a in fields[:-1])
    assert ctypes.sizeof(AkModernBertConfig) == 4 * (len(fields) - 1) + 4 * MBERT_MAX_LAYERS
    kinds = {"int": ctypes.c_int, "float": ctypes.c_float}
    assert all(kinds[k] is t for (k, _, _), (_, t) in zip(fields[:-1], AkModernBertConfig._fields_))


def test_handle_refuses_without_touching_the_gpu_what_python_can_see():
    from archi_amd.modernbert import HipModernBert
    base = MODERNBERT_SHAPES["modernbert-tiny-global"]
    with pytest.raises(ValueError, match="layer types"):
        HipModernBert(base[:10] + ((1,),) + base[11:], {})


def test_embedding_dimensions_for_modernbert():
    from archi_amd.config_plugin import EMBEDDING_DIMENSIONS
    assert EMBEDDING_DIMENSIONS["nomic-ai/modernbert-embed-base"] == 768
    assert EMBEDDING_DIMENSIONS["Alibaba-NLP/gte-modernbert-base"] == 768
    assert EMBEDDING_DIMENSIONS["lightonai/modernbert-embed-large"] == 1024
    for name, dim in EMBEDDING_DIMENSIONS.items():
        if name in MODERNBERT_SHAPES:
            assert MODERNBERT_SHAPES[name][1] == dim


def test_fixture_set_covers_what_the_gpu_test_needs():
    names = sorted(fx.CASES)
    assert all(os.path.exists(fx.path(n)) for n in names)
    lens = np.concatenate([fx.load(n)["lens"] for n in names])
    assert all(n in lens for n in (1, 64, 65, 129, 130, 512, 513, 8192))
    assert all(os.path.getsize(fx.path(n)) < 64 * 1024 for n in names)


@pytest.mark.parametrize("name", sorted(fx.CASES))
def test_fixture_is_reproduced_and_can_see_the_features(name):
    """The committed fixture against the generating script run now: expected to 1e-6; and, from ModernBertModel alone, the float32
    reference with the window removed and the one with both thetas equal each differ from the true reference by at least 10x the
    fixture's 1 - cos bar on every row of at least 130 tokens. The bar is per figure the larger of the project's bf16 bar and the
    all-bf16 ModernBertModel's own error stored in the fixture."""
    stored = fx.load(name)
    shape, seed, std, lens, pooling = fx.CASES[name]
    assert (stored["shape_name"], stored["seed"], stored["std"], stored["pooling"]) == (shape, seed, std, pooling)
    assert list(stored["lens"]) == list(lens)
    now = fx.build(name, with_bf16=False)
    assert np.array_equal(now["ids"], stored["ids"])
    assert np.abs(now["expected"] - stored["expected"]).max() <= 1e-6
    assert stored["bar_cos"] == max(PROJECT_BAR_COS, stored["bf16_cos"]) and stored["bar_abs"] == max(PROJECT_BAR_ABS, stored["bf16_abs"])
    types = MODERNBERT_SHAPES[shape][10]
    assert (now["sens_window"].size > 0) == (0 in types) and (now["sens_theta"].size > 0) == (0 in types and 1 in types)
    now["bar_cos"] = stored["bar_cos"]
    ok, text = fx.sensitivity_ok(now)
    print(f"{name}: bar {stored['bar_cos']:.3g} / {stored['bar_abs']:.3g}; {text}")
    assert ok, text
    for key in ("sens_window", "sens_theta"):
        assert np.allclose(now[key], stored[key], rtol=1e-2, atol=1e-6)


def test_new_kernels_do_not_spill():
    """-Rpass-analysis=kernel-resource-usage with the Makefile's flags: every kernel of mbert.hip, both instantiations of k_attn_long
    and every k_gemm MODE 8 instantiation report no spilled VGPRs and no scratch."""
    from scripts.kernel_resources import kernel_resources
    seen = {}
    for src, pat in (("mbert.hip", r"k_mb_"), ("attn_long.hip", r"k_attn_long"), ("gemm.hip", r"k_gemmILi8E")):
        for name, use in kernel_resources(src).items():
            if re.search(pat, name):
                seen.update({(name, key): use[key] for key in ("VGPRs Spill", "ScratchSize [bytes/lane]")})
    names = {n for n, _ in seen}
    for k in ("k_mb_embed", "k_mb_add_ln", "k_mb_rope", "k_mb_pool_part", "k_mb_pool_fin", "k_attn_longILb1E", "k_attn_longILb0E",
              "k_gemmILi8ELi256ELb1E", "k_gemmILi8ELi128ELb0E"):
        assert any(k in n for n in names), (k, names)
    assert not any("k_gemmILi8ELi256ELb0E" in n for n in names)      # no wide in-step MODE 8 (it would spill)
    assert all(v == 0 for v in seen.values()), {k: v for k, v in seen.items() if v}
