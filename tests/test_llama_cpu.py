"""CPU tests of the Mistral / Llama family (archi_amd.llama, ak_llama_*): the config check and every refusal by field name, the
inverse frequencies against transformers' own initialisations bit for bit and the host table against HF's cos / sin, the ABI (header,
binding, exports), that the fixtures of tests/golden/llama_*.npz discriminate the defects a wrong kernel would have (from float32 HF
alone), and that the kernel references of tests/llama_kernel_cases.py / llama_kernel_refs.py hold an emulation and flag the mutants."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from archi_amd.llama import (LLAMA_SHAPES, Llama3Scaling, LlamaShape, llama_config_shape, random_llama_weights, read_llama_st_config,
                             resolve_mode, rope_inv_freq, weight_order)
from tests import kernel_refs as kr
from tests import llama_kernel_cases as lc
from tests import llama_kernel_refs as lr
from tests import llama_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISTRAL = {"model_type": "mistral", "vocab_size": 32000, "hidden_size": 4096, "num_hidden_layers": 32, "num_attention_heads": 32,
           "num_key_value_heads": 8, "intermediate_size": 14336, "max_position_embeddings": 32768, "rms_norm_eps": 1e-5, "rope_theta": 10000.0,
           "sliding_window": 4096, "hidden_act": "silu"}
LLAMA31 = {"model_type": "llama", "vocab_size": 128256, "hidden_size": 4096, "num_hidden_layers": 32, "num_attention_heads": 32,
           "num_key_value_heads": 8, "intermediate_size": 14336, "max_position_embeddings": 131072, "rms_norm_eps": 1e-5, "rope_theta": 500000.0,
           "rope_scaling": {"factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 8192,
                            "rope_type": "llama3"}, "attention_bias": False, "mlp_bias": False, "hidden_act": "silu"}


# ---- config ------------------------------------------------------------------------------------------------------------------------
def test_config_acceptance_in_both_dialects():
    assert llama_config_shape(MISTRAL) == LLAMA_SHAPES["intfloat/e5-mistral-7b-instruct"] == LLAMA_SHAPES["Salesforce/SFR-Embedding-Mistral"] \
        == LLAMA_SHAPES["Linq-AI-Research/Linq-Embed-Mistral"]
    assert llama_config_shape(LLAMA31) == LLAMA_SHAPES["llama-3.1-8b"]
    # the transformers-5 spelling: theta and the scaling inside rope_parameters
    m5 = {k: v for k, v in MISTRAL.items() if k != "rope_theta"}
    m5["rope_parameters"] = {"rope_type": "default", "rope_theta": 10000.0}
    assert llama_config_shape(m5) == llama_config_shape(MISTRAL)
    l5 = {k: v for k, v in LLAMA31.items() if k not in ("rope_theta", "rope_scaling")}
    l5["rope_parameters"] = dict(LLAMA31["rope_scaling"], rope_theta=500000.0)
    assert llama_config_shape(l5) == llama_config_shape(LLAMA31)
    assert llama_config_shape(l5).scaling == Llama3Scaling(8.0, 1.0, 4.0, 8192)
    # no window: sliding_window null, Llama (even with the key), full_attention layer types
    assert llama_config_shape(dict(MISTRAL, sliding_window=None)).window == 0
    assert llama_config_shape(dict(LLAMA31, sliding_window=4096)).window == 0
    assert llama_config_shape(dict(MISTRAL, layer_types=["full_attention"] * 32)).window == 0
    assert llama_config_shape(dict(MISTRAL, layer_types=["sliding_attention"] * 32)).window == 4096
    assert llama_config_shape(dict(MISTRAL, head_dim=128, hidden_size=3072, num_attention_heads=32)).hidden == 3072


@pytest.mark.parametrize("change,field", [
    ({"model_type": "qwen2"}, "model_type"), ({"attention_bias": True}, "attention_bias"), ({"mlp_bias": True}, "mlp_bias"),
    ({"hidden_act": "gelu"}, "hidden_act"), ({"num_attention_heads": 64}, "head_dim"), ({"head_dim": 64}, "head_dim"),
    ({"num_key_value_heads": 4}, "num_key_value_heads"), ({"num_key_value_heads": 5}, "num_key_value_heads"),
    ({"rope_scaling": {"rope_type": "linear", "factor": 2.0}}, "linear"), ({"rope_scaling": {"type": "dynamic", "factor": 2.0}}, "dynamic"),
    ({"rope_scaling": {"rope_type": "yarn", "factor": 2.0}}, "yarn"), ({"rope_parameters": {"rope_type": "longrope", "rope_theta": 1e4}}, "longrope"),
    ({"rope_scaling": {"rope_type": "llama3", "factor": 8.0}}, "low_freq_factor"),
    ({"layer_types": ["full_attention", "sliding_attention"] * 16}, "layer_types"), ({"sliding_window": 0}, "sliding_window"),
    ({"sliding_window": -5}, "sliding_window"), ({"hidden_size": 4096 + 64, "head_dim": 128}, "hidden_size"),
    ({"intermediate_size": 14336 + 32}, "intermediate_size")])
def test_config_refusals_name_the_field(change, field):
    with pytest.raises(ValueError, match=field):
        llama_config_shape(dict(MISTRAL, **change), "cfg")


def test_qwen3_still_refuses_llama_and_llama_refuses_qwen3():
    from archi_amd.decoder import qwen3_config_shape
    for cfg in (MISTRAL, LLAMA31):
        with pytest.raises(ValueError, match="is not qwen3"):
            qwen3_config_shape(cfg)
    with pytest.raises(ValueError, match="model_type 'qwen3'"):
        llama_config_shape(dict(MISTRAL, model_type="qwen3"))


def test_attention_mode_and_pooling():
    from archi_amd.llama import apply_mode
    s = LLAMA_SHAPES["ll-win"]
    assert resolve_mode("m", s, {}, None) == resolve_mode("m", s, {"attention": "causal", "pooling": "last"}, "mean") == "last"
    assert resolve_mode("m", None, {}, None) == "last" and resolve_mode("m", None, {}, "mean") == "mean"
    assert resolve_mode("m", s, {"attention": "bidirectional"}, None) == "mean"                 # bidirectional defaults to mean ...
    assert resolve_mode("m", s, {"attention": "bidirectional"}, "last") == "last"               # ... unless the checkpoint says otherwise
    assert resolve_mode("m", s, {"attention": "bidirectional", "pooling": "last"}, "mean") == "last"      # the override wins
    assert apply_mode(s, {"attention": "bidirectional"}).attention == "bidirectional" and apply_mode(s, {}) == s
    with pytest.raises(ValueError, match="pooling 'cls'"):
        resolve_mode("m", s, {"pooling": "cls"}, "last")
    with pytest.raises(ValueError, match="attention 'full'"):
        resolve_mode("m", s, {"attention": "full"}, None)
    from archi_amd import _stack
    for fam in ("decoder", "modernbert", "gemma", "nomic"):      # "last" in _lib.POOLING reaches no other family's library call
        mod = __import__(f"archi_amd.{fam}", fromlist=["x"])
        cls = [v for v in vars(mod).values() if isinstance(v, type) and issubclass(v, _stack.HipStack) and v is not _stack.HipStack][0]
        if fam != "decoder":
            assert "last" not in cls.poolings, fam


def test_st_config(tmp_path):
    def write(modes, modules=("Transformer", "Pooling", "Normalize"), max_len=512):
        d = str(tmp_path / f"m{len(os.listdir(tmp_path))}")
        os.makedirs(os.path.join(d, "1_Pooling"))
        json.dump([{"idx": i, "name": str(i), "path": "1_Pooling" if m == "Pooling" else "", "type": "sentence_transformers.models." + m}
                   for i, m in enumerate(modules)], open(os.path.join(d, "modules.json"), "w"))
        json.dump({"pooling_mode_" + k: True for k in modes}, open(os.path.join(d, "1_Pooling", "config.json"), "w"))
        json.dump({"max_seq_length": max_len}, open(os.path.join(d, "sentence_bert_config.json"), "w"))
        return d
    assert read_llama_st_config(write(["lasttoken"])) == ("last", 512, True)
    assert read_llama_st_config(write(["mean_tokens"], ("Transformer", "Pooling"), 4096)) == ("mean", 4096, False)
    for modes in (["cls_token"], ["mean_tokens", "lasttoken"], ["weightedmean_tokens"], []):
        with pytest.raises(ValueError, match="pooling modes"):
            read_llama_st_config(write(modes))
    with pytest.raises(ValueError, match="Dense"):
        read_llama_st_config(write(["lasttoken"], ("Transformer", "Pooling", "Dense")))


def test_provider_detection_and_dimensions(tmp_path):
    from archi_amd import embeddings as em
    from archi_amd.config_plugin import EMBEDDING_DIMENSIONS
    for name in ("intfloat/e5-mistral-7b-instruct", "Salesforce/SFR-Embedding-Mistral", "Linq-AI-Research/Linq-Embed-Mistral"):
        assert em._is_llama(name) and EMBEDDING_DIMENSIONS[name] == 4096
        assert not any(f(name) for f in (em._is_qwen3, em._is_modernbert, em._is_gemma, em._is_nomic, em._is_mpnet, em._is_xlmr))
    for mt, want in (("mistral", True), ("llama", True), ("qwen3", False), ("bert", False)):
        d = str(tmp_path / mt)
        os.makedirs(d)
        json.dump({"model_type": mt}, open(os.path.join(d, "config.json"), "w"))
        assert em._is_llama(d) == want
    assert not any(n in LLAMA_SHAPES for fam in (em.QWEN3_SHAPES, em.MODERNBERT_SHAPES, em.GEMMA_SHAPES, em.NOMIC_SHAPES) for n in fam)
    with pytest.raises(ValueError, match="Mistral / Llama embedders run in bf16 only"):
        em.ArchiHipEmbeddings("intfloat/e5-mistral-7b-instruct", model_kwargs={"synthetic_seed": 1, "precision": "f32"})
    assert em._LLAMA.max_seq == 8192 and weight_order(2)[2:11] == [f"l0.{k}" for k in ("wq", "wk", "wv", "wo", "ln_in", "ln_post", "w_gate", "w_up", "w_down")]


# ---- rotary frequencies and table ----------------------------------------------------------------------------------------------------
def _hf_rotary(shape):
    cfg = ref.hf_config(shape, "llama")
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding
    return cfg, LlamaRotaryEmbedding(config=cfg)


@pytest.mark.parametrize("theta", (1e4, 5e5, 1e6))
def test_default_inv_freq_is_hf_bit_for_bit(theta):
    shape = LLAMA_SHAPES["ll-tiny-g1"]._replace(rope_theta=theta)
    cfg, rot = _hf_rotary(shape)
    assert cfg.rope_parameters["rope_type"] == "default"
    want = rot.inv_freq.numpy()
    got = rope_inv_freq(shape)
    assert got.dtype == np.float32 and got.shape == (64,) and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("shape", (LLAMA_SHAPES["llama-3.1-8b"], LLAMA_SHAPES["ll-l3"],
                                   LLAMA_SHAPES["ll-l3"]._replace(rope_theta=1e4, scaling=Llama3Scaling(4.0, 1.0, 2.0, 256))))
def test_llama3_inv_freq_is_hf_bit_for_bit(shape):
    from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
    cfg, rot = _hf_rotary(shape._replace(layers=1, vocab=100))
    want, factor = ROPE_INIT_FUNCTIONS["llama3"](cfg, None)
    got = rope_inv_freq(shape)
    assert factor == 1.0 and np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32))
    assert np.array_equal(got.view(np.uint32), rot.inv_freq.numpy().view(np.uint32))
    assert not np.array_equal(got, rope_inv_freq(shape._replace(scaling=None)))


@pytest.mark.parametrize("name", ("llama-3.1-8b", "ll-win"))
def test_host_table_from_the_frequencies_is_within_one_ulp_of_hf(name):
    """ak_decoder_rope_table_inv (the host routine ak_llama_set_rope_inv_freq uploads from) on rope_inv_freq against HF's cos / sin at
    positions < 8192: |d| <= 1 ulp of the float32 value (HF's table is torch's float32 cos / sin of the same float32 angle)."""
    import torch
    from archi_amd.decoder import rope_table_inv
    shape = LLAMA_SHAPES[name]
    cfg, rot = _hf_rotary(shape._replace(layers=1, vocab=100, window=0))
    pos = torch.arange(8192)[None]
    cos, sin = rot(torch.zeros(1, 1, 1, dtype=torch.float32), pos)
    c, s = rope_table_inv(rope_inv_freq(shape), 8192)
    for got, want in ((c, cos[0, :, :64].numpy()), (s, sin[0, :, :64].numpy())):
        ulp = np.spacing(np.abs(want).astype(np.float32))
        assert got.shape == want.shape and (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_config_struct_matches_header():
    from archi_amd._lib import AkLlamaConfig
    src = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    body = re.search(r"typedef struct AkLlamaConfig \{(.*?)\} AkLlamaConfig;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int|float)\s+(\w+)\s*;", body)
    assert [n for _, n in fields] == [n for n, _ in AkLlamaConfig._fields_] == \
        ["vocab_size", "hidden", "layers", "q_heads", "kv_heads", "head_dim", "intermediate", "max_position", "rms_eps", "rope_theta",
         "sliding_window", "bidirectional"]
    kinds = {"int": ctypes.c_int, "float": ctypes.c_float}
    assert all(kinds[k] is t for (k, _), (_, t) in zip(fields, AkLlamaConfig._fields_)) and ctypes.sizeof(AkLlamaConfig) == 48


def _exported(name, pattern):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "archi_amd", "lib", name)], stdout=subprocess.PIPE, check=True).stdout.decode()
    return set(re.findall(pattern, out))


def test_symbols_in_header_binding_and_libraries():
    from archi_amd import _lib
    src = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    assert int(re.search(r"#define AK_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 5
    lib = _lib.load()
    assert lib.ak_abi_version() == 5
    names = {"ak_llama_create", "ak_llama_destroy", "ak_llama_set_rope_inv_freq", "ak_llama_forward_lens"}
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in names:
        assert re.search(rf"\bint {name}\(", src) and name in bound and hasattr(lib, name)
    assert _exported("libarchi_hip.so", r"\b(ak_llama_[a-z0-9_]+)\b") == names == _exported("libarchi_hip_dbg.so", r"\b(ak_llama_[a-z0-9_]+)\b")
    assert "retrievers/utils.py:7-19" in src and int(re.search(r"#define AK_POOL_LAST (\d+)", src).group(1)) == _lib.POOLING["last"]
    args = {n: a for n, _, a in _lib.SYMBOLS}
    assert args["ak_llama_forward_lens"] == args["ak_mbert_forward_lens"]


def test_single_launch_wrappers_stay_out_of_the_product_library():
    """The new wrappers are ak_kts_ll_*, exported by the dbg library only and listed in _lib.KTS_SYMBOLS; the ak_kt_* set stays at 19 and
    ak_kts_nb_* at 3."""
    from archi_amd import _lib
    new = {"ak_kts_ll_attn", "ak_kts_ll_rope", "ak_kts_ll_pool"}
    assert {n for n, _, _ in _lib.KTS_SYMBOLS if n.startswith("ak_kts_ll_")} == new
    assert _exported("libarchi_hip_dbg.so", r"\b(ak_kts_ll_[a-z0-9_]+)\b") == new
    assert not _exported("libarchi_hip.so", r"\b(ak_kt[a-z]*_[a-z0-9_]+)\b")
    assert len(_lib.KT_SYMBOLS) == 19 == len(_exported("libarchi_hip_dbg.so", r"\b(ak_kt_[a-z0-9_]+)\b"))
    assert sum(n.startswith("ak_kts_nb_") for n, _, _ in _lib.KTS_SYMBOLS) == 3
    assert "ak_kts_" not in open(os.path.join(ROOT, "include", "archi_knn.h")).read()


# ---- the fixtures discriminate ---------------------------------------------------------------------------------------------------------
def _cosd(a, b):
    return 1 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


# (fixture, defect, the rows it applies to by their length). Window defects: rows longer than w (w - 1 also moves the row of exactly w
# tokens). RoPE defects: a relative rotation, so a 1-token row cannot move and a row of a few tokens barely does -- rows of >= 32 tokens.
# The llama3 scaling: rows beyond the original length 64.
DEFECTS = [("ll-win", "window+1", lambda n: n > 48), ("ll-win", "window-1", lambda n: n >= 48), ("ll-win", "nowindow", lambda n: n > 48),
           ("ll-win", "norope", lambda n: n >= 32), ("ll-win", "theta", lambda n: n >= 32),
           ("ll-tiny-g4", "norope", lambda n: n >= 32), ("ll-tiny-g4", "theta", lambda n: n >= 32),
           ("ll-l3", "noscaling", lambda n: n > 64), ("ll-l3", "norope", lambda n: n >= 32),
           # bidirectional + mean: run as causal and pad keys attended (rows of >= 5 tokens), the mean taken before the final norm. The mean
           # divided by S instead of len is a scale, which the L2 normalisation of every fixture removes: it is held at kernel level
           # (normalise = 0 cases, tests/llama_kernel_refs.py), not here.
           ("ll-bidir-mean", "causal", lambda n: n >= 5), ("ll-bidir-mean", "pad8", lambda n: n >= 5), ("ll-bidir-mean", "prenorm", lambda n: n >= 5),
           ("ll-causal-mean", "prenorm", lambda n: n >= 5)]
_FIX = {}


def _fixture(name):
    if name not in _FIX:
        z = np.load(os.path.join(ROOT, "tests", "golden", f"llama_{name}.npz"))
        shape, seed, ids, lens, std = ref.fixture_inputs(name)
        assert str(z["shape"]) == shape and int(z["seed"]) == seed and float(z["std"]) == std
        assert np.array_equal(z["ids"], ids) and np.array_equal(z["lens"], lens)
        assert (str(z["attention"]), str(z["pooling"])) == ref.MODES.get(name, ("causal", "last"))
        _FIX[name] = (z, ref.fixture_weights(name))
    return _FIX[name]


@pytest.mark.parametrize("name", ("ll-win", "ll-tiny-g4", "ll-l3", "ll-causal-mean"))
def test_fixture_is_float32_hf(name):
    """The stored expectation is float32 HF on the seeded weights; the stored bar is the larger of the encoder bar and HF's bf16 error."""
    z, w = _fixture(name)
    want = ref.reference(ref.hf_model(str(z["shape"]), w), z["ids"], z["lens"], attention=str(z["attention"]), pooling=str(z["pooling"]))
    assert np.abs(want - z["expected"]).max() <= 1e-5
    assert float(z["cos_bar"]) == max(ref.COS_BAR, float(z["bf16_cos"])) and float(z["abs_bar"]) == max(ref.ABS_BAR, float(z["bf16_abs"]))


@pytest.mark.parametrize("name,defect,applies", DEFECTS, ids=[f"{n}-{d}" for n, d, _ in DEFECTS])
def test_fixture_discriminates(name, defect, applies):
    """Each defect moves every row it applies to by at least 10 times the fixture's 1 - cos bar (float32 HF alone)."""
    z, w = _fixture(name)
    rows = [i for i, n in enumerate(z["lens"]) if applies(int(n))]
    assert len(rows) >= 2
    attention, pooling = str(z["attention"]), str(z["pooling"])
    if defect in ("causal", "pad8", "prenorm"):
        got = ref.reference(ref.hf_model(str(z["shape"]), w), z["ids"], z["lens"], rows=set(rows), pooling=pooling,
                            attention="causal" if defect == "causal" else attention, defect=None if defect == "causal" else defect)
    else:
        got = ref.reference(ref.defect_model(str(z["shape"]), w, defect), z["ids"], z["lens"], rows=set(rows), attention=attention, pooling=pooling)
    moved = _cosd(got, z["expected"][rows])
    print(f"{name} {defect}: moved {np.array2string(moved / float(z['cos_bar']), precision=1)} bars on rows of {z['lens'][rows]} tokens")
    assert (moved >= 10.0 * float(z["cos_bar"])).all(), moved


def test_long_fixture_has_a_row_beyond_its_window():
    z = np.load(os.path.join(ROOT, "tests", "golden", "llama_ll-long.npz"))
    assert LLAMA_SHAPES[str(z["shape"])].window == 4096 and z["lens"].max() == 8192 and os.path.getsize(z.fid.name) < 1 << 20


# ---- kernel references ---------------------------------------------------------------------------------------------------------------------
def _emulated(case, inp, vis_of, other_head=False):
    """attention_emulate (the kernels' rounding scheme) of every (row, head) as ctx bits [B][S][nq * 128]."""
    S, hq, hk = case["S"], case["nq"], case["nkv"]
    G = hq // hk
    ctx = np.zeros((len(inp["lens"]), S, hq * lc.HD), np.float32)
    for b, n in enumerate(int(x) for x in inp["lens"]):
        for h in range(hq if n else 0):
            g = (h // G + 1) % hk if other_head else h // G
            ctx[b, :n, h * lc.HD:(h + 1) * lc.HD] = kr.attention_emulate(kr.bf16_value(inp["q"][b, h])[:n], kr.bf16_value(inp["k"][b, g]),
                                                                         kr.bf16_value(inp["v"][b, g]), vis_of(b, n))
    return kr.bf16_bits(ctx)


ATTN_SMALL = [c for c in lc.attn_cases() if c["name"] in ("llattn_g2_S96_w33", "llattn_g3_S160_w1", "llattn_g4_S160_w64", "llattn_g1_S96_w31")]
BIDIR_SMALL = [c for c in lc.attn_cases() if c["name"] in ("llattn_g2_S96_bidir", "llattn_g3_S160_bidir")]


@pytest.mark.parametrize("case", BIDIR_SMALL, ids=[c["name"] for c in BIDIR_SMALL])
def test_bidirectional_emulation_inside_the_bound_mutants_outside(case):
    inp = lc.attn_inputs(case)

    def ratio(vis_of, **kw):
        w = kr.Worst()
        lc.check_attention(case, inp, _emulated(case, inp, vis_of, **kw), w)
        return w.ratio

    op = lambda b, n: lc.visibility(case, inp["mask"][b])          # noqa: E731
    assert ratio(op) <= 1.0
    mutants = {"causal in place of bidirectional": lambda b, n: kr.Visibility(inp["mask"][b], causal=True),
               "first pad key attended": lambda b, n: lc.visibility(case, inp["mask"][b], pad=1),
               "last real key dropped": lambda b, n: lc.visibility(case, inp["mask"][b], pad=-1) if n > 1 else lc.visibility(case, inp["mask"][b])}
    for name, vis_of in mutants.items():
        assert ratio(vis_of) > 1.0, name
    assert ratio(op, other_head=True) > 1.0, "neighbouring kv head"



@pytest.mark.parametrize("case", ATTN_SMALL, ids=[c["name"] for c in ATTN_SMALL])
def test_attention_emulation_inside_the_bound_mutants_outside(case):
    inp = lc.attn_inputs(case)

    def ratio(vis_of, **kw):
        w = kr.Worst()
        lc.check_attention(case, inp, _emulated(case, inp, vis_of, **kw), w)
        return w.ratio

    op = lambda b, n: lc.visibility(case, inp["mask"][b])          # noqa: E731
    assert ratio(op) <= 1.0
    mutants = {"window+1": lambda b, n: lc.visibility(case, inp["mask"][b], dw=1),
               "last key dropped": lambda b, n: lc.visibility(case, inp["mask"][b], diag=-1) if n > 1 else lc.visibility(case, inp["mask"][b]),
               "window one block coarse": lambda b, n: lc.coarse_visibility(case, n)}
    if case["window"] > 1:             # (at w = 1 the band itself hides the key one past the diagonal: Visibility's band is symmetric)
        mutants["window-1"] = lambda b, n: lc.visibility(case, inp["mask"][b], dw=-1)
        mutants["one past the diagonal"] = lambda b, n: lc.visibility(case, inp["mask"][b], diag=1)
    for name, vis_of in mutants.items():
        assert ratio(vis_of) > 1.0, name
    assert ratio(op, other_head=True) > 1.0, "neighbouring kv head"


def test_attention_case_list():
    cases = lc.attn_cases()
    names = {c["name"] for c in cases}
    assert len(names) == len(cases) == 4 * 2 * 6 + 6 + 1 + 4 * 2 + 1
    for G in (1, 2, 3, 4):
        for S in (96, 160):
            assert {f"llattn_g{G}_S{S}_w{w}" for w in (1, 31, 32, 33, 64, 100)} <= names
    assert {"llattn_g4_S32_w31", "llattn_g4_S64_w100", "llattn_g4_S288_w31", "llattn_g4_S2048_w1000", "llattn_g4_S2048_bidir"} <= names
    assert {f"llattn_g{G}_S{S}_bidir" for G in (1, 2, 3, 4) for S in (96, 160)} <= names
    assert all(c["nq"] // c["nkv"] == c["G"] and c["S"] % 32 == 0 for c in cases)
    assert lc.lengths_for(160) == [160, 159, 77, 1, 0] and len(lc.equal_cases()) == 2


@pytest.mark.parametrize("c", lc.rope_cases()[::5], ids=[c["name"] for c in lc.rope_cases()[::5]])
def test_rope_emulation_inside_the_bound_mutants_outside(c):
    inp = lc.rope_inputs(c)
    exp = lr.rope_expect(c, inp)
    w = kr.Worst()
    assert not lr.compare(exp, lr.rope_emulate(c, inp), w, c["name"]) and 0 < w.ratio <= 1.0
    for mut in ("swap", "sign", "pos", "noscale"):
        assert lr.flagged(exp, lr.rope_expect(c, inp, mut)), mut
    copied = dict(exp, v=("exact", exp["v"][1] ^ np.uint16(1)))
    assert lr.flagged(exp, copied)


POOL_SMALL = [c for c in lc.pool_cases() if c["name"] in ("llpool_H256_S192_n1", "llpool_H1152_S96_n0", "llpool_H4096_S32_n0", "llpool_H4096_S96_n1")]


@pytest.mark.parametrize("c", POOL_SMALL, ids=[c["name"] for c in POOL_SMALL])
def test_mean_pool_emulation_inside_the_bound_mutants_outside(c):
    inp = lc.pool_inputs(c)
    want, bound = lr.pool_expect(c, inp)
    w = kr.Worst()
    w.add(lr.pool_emulate(c, inp), want, bound, c["name"])
    assert 0 < w.ratio <= 1.0, str(w)
    for mut in ("norm_after",) + (("div_S",) if not c["normalise"] else ()):      # (a scale does not survive the L2 normalisation)
        m = kr.Worst()
        m.add(lr.pool_expect(c, inp, mut)[0], want, bound, mut)
        assert m.ratio > 1.0, mut
    assert any(63 in k["lens"] and 64 in k["lens"] and 65 in k["lens"] for k in lc.pool_cases()) and np.isnan(inp["x"][0, c["lens"][0]:]).all()
