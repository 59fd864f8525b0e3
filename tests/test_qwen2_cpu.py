"""CPU tests of the Qwen2 family (archi_amd.qwen2, ak_qwen2_*): the config check and every refusal by field name, the attention default
from is_causal, the ABI (header, binding, exports), that the fixtures of tests/golden/qwen2_*.npz discriminate the defects a wrong
kernel would have (from float32 HF alone), and that the kernel references of tests/qwen2_kernel_cases.py hold an emulation of the split
attention mapping and of the biased QKV GEMM and flag the mutants."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from archi_amd.llama import Llama3Scaling, resolve_mode
from archi_amd.qwen2 import QWEN2_SHAPES, Qwen2Shape, apply_mode, qwen2_config_shape, random_qwen2_weights, weight_order
from tests import kernel_refs as kr
from tests import qwen2_kernel_cases as qc
from tests import qwen2_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QWEN2_7B = {"model_type": "qwen2", "vocab_size": 151646, "hidden_size": 3584, "num_hidden_layers": 28, "num_attention_heads": 28,
            "num_key_value_heads": 4, "intermediate_size": 18944, "max_position_embeddings": 131072, "rms_norm_eps": 1e-6, "rope_theta": 1000000.0,
            "sliding_window": 131072, "use_sliding_window": False, "max_window_layers": 28, "hidden_act": "silu", "attention_dropout": 0.0}
QWEN2_15B = dict(QWEN2_7B, hidden_size=1536, num_attention_heads=12, num_key_value_heads=2, intermediate_size=8960)


# ---- config ------------------------------------------------------------------------------------------------------------------------
def test_config_acceptance_in_both_dialects():
    assert qwen2_config_shape(QWEN2_7B) == QWEN2_SHAPES["Alibaba-NLP/gte-Qwen2-7B-instruct"]
    assert qwen2_config_shape(QWEN2_15B) == QWEN2_SHAPES["Alibaba-NLP/gte-Qwen2-1.5B-instruct"]
    assert qwen2_config_shape(QWEN2_7B)._replace(vocab=2000, layers=2) == QWEN2_SHAPES["gte-qwen2-7b-2l"]
    assert qwen2_config_shape(QWEN2_15B)._replace(vocab=2000, layers=2) == QWEN2_SHAPES["gte-qwen2-1.5b-2l"]
    # the transformers-5 spelling: theta (and a scaling) inside rope_parameters
    c5 = {k: v for k, v in QWEN2_7B.items() if k != "rope_theta"}
    c5["rope_parameters"] = {"rope_type": "default", "rope_theta": 1000000.0}
    assert qwen2_config_shape(c5) == qwen2_config_shape(QWEN2_7B)
    l3 = {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 8192}
    assert qwen2_config_shape(dict(QWEN2_7B, rope_scaling=l3)).scaling == Llama3Scaling(8.0, 1.0, 4.0, 8192) \
        == qwen2_config_shape(dict(c5, rope_parameters=dict(l3, rope_theta=1e6))).scaling
    # sliding_window is ignored while use_sliding_window is false; full_attention layer types; a stated head_dim
    assert qwen2_config_shape(dict(QWEN2_7B, sliding_window=4096)) == qwen2_config_shape(QWEN2_7B)
    assert qwen2_config_shape(dict(QWEN2_7B, layer_types=["full_attention"] * 28)) == qwen2_config_shape(QWEN2_7B)
    assert qwen2_config_shape(dict(QWEN2_7B, head_dim=128, hidden_size=3072)).hidden == 3072
    # 5 and 8 query heads per kv head (Qwen2.5-14B, Qwen2.5-3B)
    assert qwen2_config_shape(dict(QWEN2_7B, hidden_size=5120, num_attention_heads=40, num_key_value_heads=8, intermediate_size=13824)).q_heads == 40
    assert qwen2_config_shape(dict(QWEN2_7B, hidden_size=2048, num_attention_heads=16, num_key_value_heads=2, intermediate_size=11008)).kv_heads == 2
    for name, s in QWEN2_SHAPES.items():
        assert s.rope_theta == 1e6 and s.q_heads % s.kv_heads == 0 and s.q_heads // s.kv_heads <= 8, name
        if name.startswith("q2-tiny"):
            assert s.vocab == 1000 and s.layers in (2, 3) and s.hidden == 256 and s.intermediate == 512 and s.kv_heads == 2
            assert s.q_heads // s.kv_heads == int(name[-1])


@pytest.mark.parametrize("change,field", [
    ({"model_type": "mistral"}, "model_type"), ({"model_type": "qwen3"}, "model_type"), ({"use_sliding_window": True}, "use_sliding_window"),
    ({"layer_types": ["full_attention", "sliding_attention"] * 14}, "layer_types"), ({"layer_types": ["sliding_attention"] * 28}, "layer_types"),
    ({"hidden_act": "gelu"}, "hidden_act"), ({"num_attention_heads": 56}, "head_dim"), ({"head_dim": 64}, "head_dim"),
    ({"hidden_size": 896, "num_attention_heads": 14, "num_key_value_heads": 2}, "head_dim"),                    # Qwen2-0.5B: head 64
    ({"num_key_value_heads": 3}, "num_key_value_heads"), ({"num_key_value_heads": 2}, "num_key_value_heads"),      # not whole; 14 per kv head
    ({"hidden_size": 3584 + 64, "head_dim": 128}, "hidden_size"), ({"intermediate_size": 18944 + 32}, "intermediate_size"),
    ({"rope_scaling": {"rope_type": "linear", "factor": 2.0}}, "linear"), ({"rope_scaling": {"type": "dynamic", "factor": 2.0}}, "dynamic"),
    ({"rope_scaling": {"rope_type": "yarn", "factor": 4.0}}, "yarn"), ({"rope_parameters": {"rope_type": "longrope", "rope_theta": 1e6}}, "longrope"),
    ({"rope_scaling": {"rope_type": "llama3", "factor": 8.0}}, "low_freq_factor")])
def test_config_refusals_name_the_field(change, field):
    with pytest.raises(ValueError, match=field):
        qwen2_config_shape(dict(QWEN2_7B, **change), "cfg")


def test_the_other_decoder_families_still_refuse_qwen2():
    from archi_amd.decoder import qwen3_config_shape
    from archi_amd.llama import llama_config_shape
    with pytest.raises(ValueError, match="model_type 'qwen2'"):
        llama_config_shape(QWEN2_7B)
    with pytest.raises(ValueError, match="is not qwen3"):
        qwen3_config_shape(QWEN2_7B)


def test_attention_default_and_pooling():
    s = qwen2_config_shape(QWEN2_7B)
    assert s.attention == "causal" and s.pooling == "last" and qwen2_config_shape(dict(QWEN2_7B, is_causal=True)) == s
    nc = qwen2_config_shape(dict(QWEN2_7B, is_causal=False))
    assert nc.attention == "bidirectional" and nc._replace(attention="causal") == s
    # the keyword always wins; without it the shape's own
    assert apply_mode(nc, {}).attention == "bidirectional" and apply_mode(nc, {"attention": "causal"}).attention == "causal"
    assert apply_mode(s, {"attention": "bidirectional"}).attention == "bidirectional" and apply_mode(s, {}) == s
    # pooling as llama.resolve_mode: the keyword, else the checkpoint's Pooling module, else the mode's default
    assert resolve_mode("m", s, {}, None) == "last" and resolve_mode("m", s, {}, "mean") == "mean"
    assert resolve_mode("m", nc, {}, None) == "mean" and resolve_mode("m", nc, {}, "last") == "last"
    assert resolve_mode("m", nc, {"attention": "causal"}, None) == "last" and resolve_mode("m", nc, {"pooling": "last"}, "mean") == "last"
    with pytest.raises(ValueError, match="attention 'full'"):
        resolve_mode("m", s, {"attention": "full"}, None)
    with pytest.raises(ValueError, match="pooling 'cls'"):
        resolve_mode("m", s, {"pooling": "cls"}, "last")
    with pytest.raises(ValueError, match="is_causal"):
        qwen2_config_shape(dict(QWEN2_7B, is_causal="no"))


def test_provider_detection_and_dimensions(tmp_path):
    import json
    from archi_amd import embeddings as em
    from archi_amd.config_plugin import EMBEDDING_DIMENSIONS
    for name, dim in (("Alibaba-NLP/gte-Qwen2-1.5B-instruct", 1536), ("Alibaba-NLP/gte-Qwen2-7B-instruct", 3584)):
        assert em._is_qwen2(name) and EMBEDDING_DIMENSIONS[name] == dim == QWEN2_SHAPES[name].hidden
        assert not any(f(name) for f in (em._is_qwen3, em._is_llama, em._is_modernbert, em._is_gemma, em._is_nomic, em._is_mpnet, em._is_xlmr))
    for mt, want in (("qwen2", True), ("qwen3", False), ("mistral", False), ("llama", False)):
        d = str(tmp_path / mt)
        os.makedirs(d)
        json.dump({"model_type": mt}, open(os.path.join(d, "config.json"), "w"))
        assert em._is_qwen2(d) == want and (em._is_llama(d) == (mt in ("mistral", "llama")))
    assert not any(n in QWEN2_SHAPES for fam in (em.QWEN3_SHAPES, em.LLAMA_SHAPES, em.MODERNBERT_SHAPES, em.GEMMA_SHAPES, em.NOMIC_SHAPES) for n in fam)
    with pytest.raises(ValueError, match="Qwen2 embedders run in bf16 only"):
        em.ArchiHipEmbeddings("Alibaba-NLP/gte-Qwen2-7B-instruct", model_kwargs={"synthetic_seed": 1, "precision": "f32"})
    assert em._QWEN2.max_seq == 8192 and Qwen2Shape._fields[em._QWEN2.max_position] == "max_position"
    # a qwen2 directory is refused by its config before any weight is read
    d = str(tmp_path / "sliding")
    os.makedirs(d)
    json.dump(dict(QWEN2_7B, use_sliding_window=True), open(os.path.join(d, "config.json"), "w"))
    open(os.path.join(d, "tokenizer.json"), "w").write("{}")
    os.makedirs(os.path.join(d, "1_Pooling"))
    json.dump({"pooling_mode_lasttoken": True}, open(os.path.join(d, "1_Pooling", "config.json"), "w"))
    with pytest.raises(ValueError, match="use_sliding_window"):
        em.ArchiHipEmbeddings(d)


def test_random_weights_carry_bf16_biases_at_their_own_std():
    w = random_qwen2_weights("q2-tiny-g7", seed=3, std=0.05, bias_std=2.0)
    assert list(w) == weight_order(2) and len(weight_order(28)) == 2 + 12 * 28
    assert weight_order(1)[2:] == [f"l0.{k}" for k in ("wq", "wk", "wv", "bq", "bk", "bv", "wo", "ln_in", "ln_post", "w_gate", "w_up", "w_down")]
    for l in range(2):
        for k, n in (("bq", 14 * 128), ("bk", 256), ("bv", 256)):
            b = w[f"l{l}.{k}"]
            assert b.shape == (n,) and b.dtype == np.float32 and np.array_equal(kr.bf16_round(b), b) and 1.5 < b.std() < 2.5
    assert 0.04 < w["l0.wq"].std() < 0.06
    small = random_qwen2_weights("q2-tiny-g7", seed=3, std=0.05, bias_std=0.5)
    assert np.array_equal(small["l1.wq"], w["l1.wq"]) and 0.35 < small["l1.bk"].std() < 0.65      # the same draws, another scale
    sd = ref.hf_state_dict(w, 2)
    assert sd["layers.1.self_attn.k_proj.bias"] is w["l1.bk"] and len(sd) == 2 + 12 * 2


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_config_struct_matches_header():
    from archi_amd._lib import AkLlamaConfig, AkQwen2Config
    src = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    body = re.search(r"typedef struct AkQwen2Config \{(.*?)\} AkQwen2Config;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int|float)\s+(\w+)\s*;", body)
    assert [n for _, n in fields] == [n for n, _ in AkQwen2Config._fields_] == [n for n, _ in AkLlamaConfig._fields_ if n != "sliding_window"]
    kinds = {"int": ctypes.c_int, "float": ctypes.c_float}
    assert all(kinds[k] is t for (k, _), (_, t) in zip(fields, AkQwen2Config._fields_)) and ctypes.sizeof(AkQwen2Config) == 44
    assert ctypes.sizeof(AkLlamaConfig) == 48


def _exported(name, pattern):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "archi_amd", "lib", name)], stdout=subprocess.PIPE, check=True).stdout.decode()
    return set(re.findall(pattern, out))


def test_symbols_in_header_binding_and_libraries():
    from archi_amd import _lib
    src = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    assert int(re.search(r"#define AK_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 5
    lib = _lib.load()
    names = {"ak_qwen2_create", "ak_qwen2_destroy", "ak_qwen2_set_rope_inv_freq", "ak_qwen2_forward_lens"}
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in names:
        assert re.search(rf"\bint {name}\(", src) and name in bound and hasattr(lib, name)
    assert _exported("libarchi_hip.so", r"\b(ak_qwen2_[a-z0-9_]+)\b") == names == _exported("libarchi_hip_dbg.so", r"\b(ak_qwen2_[a-z0-9_]+)\b")
    args = {n: a for n, _, a in _lib.SYMBOLS}
    for op in ("create", "destroy", "set_rope_inv_freq", "forward_lens"):
        assert [a for a in args[f"ak_qwen2_{op}"][1:]] == [a for a in args[f"ak_llama_{op}"][1:]], op
    assert args["ak_qwen2_create"][0]._type_ is _lib.AkQwen2Config
    assert "2 + 12 * l" in src and "2 + 12 * layers" in src
    # every ak_*( the header declares is bound, and the reverse
    declared = set(re.findall(r"\b(ak_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    assert declared == bound


def test_single_launch_wrapper_stays_out_of_the_product_library():
    from archi_amd import _lib
    new = {"ak_kts_q2_attn"}
    assert {n for n, _, _ in _lib.KTS_SYMBOLS if n.startswith("ak_kts_q2_")} == new
    assert _exported("libarchi_hip_dbg.so", r"\b(ak_kts_q2_[a-z0-9_]+)\b") == new
    assert not _exported("libarchi_hip.so", r"\b(ak_kt[a-z]*_[a-z0-9_]+)\b")
    assert {n for n, _, _ in _lib.KTS_SYMBOLS if n.startswith("ak_kts_ll_")} == {"ak_kts_ll_attn", "ak_kts_ll_rope", "ak_kts_ll_pool"}
    assert "ak_kts_" not in open(os.path.join(ROOT, "include", "archi_knn.h")).read()


# ---- the fixtures discriminate ---------------------------------------------------------------------------------------------------------
def _cosd(a, b):
    return 1 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


# (fixture, defect, the rows it applies to by their length). A 1-token row's softmax has one key: it cannot see a q or k bias, RoPE or
# the mask. A k bias without RoPE is the same logit offset for every key of a query, so what a dropped k bias moves is the rotation's
# share: rows of >= 32 tokens, as the RoPE defects of tests/test_llama_cpu.py. The v bias reaches every row.
_SEES_QK, _SEES_ROPE, _ALL = (lambda n: n >= 5), (lambda n: n >= 32), (lambda n: n >= 1)
DEFECTS = [(f, d, a) for f in ("q2-tiny-g5", "q2-tiny-g7", "q2-tiny-g2")
           for d, a in (("noqbias", _SEES_QK), ("nokbias", _SEES_ROPE), ("novbias", _ALL), ("swapkv", _ALL), ("norope", _SEES_ROPE))]
DEFECTS += [("q2-bidir-mean", "causal", _SEES_QK), ("q2-bidir-last", "causal", _SEES_QK), ("q2-bidir-last", "novbias", _ALL),
            ("q2-bidir-mean", "swapkv", _ALL)]
_FIX = {}


def _fixture(name):
    if name not in _FIX:
        z = np.load(os.path.join(ROOT, "tests", "golden", f"qwen2_{name}.npz"))
        shape, seed, ids, lens, std, bias_std = ref.fixture_inputs(name)
        assert str(z["shape"]) == shape and int(z["seed"]) == seed and float(z["std"]) == std and float(z["bias_std"]) == bias_std
        assert np.array_equal(z["ids"], ids) and np.array_equal(z["lens"], lens)
        assert (str(z["attention"]), str(z["pooling"])) == ref.MODES.get(name, ("causal", "last"))
        _FIX[name] = (z, ref.fixture_weights(name))
    return _FIX[name]


def test_fixture_list():
    names = {f[len("qwen2_"):-len(".npz")] for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f.startswith("qwen2_") and f.endswith(".npz")}
    assert names == set(ref.FIXTURES) and len(names) == 8
    assert {QWEN2_SHAPES[ref.FIXTURES[n][0]].q_heads // 2 for n in names} == {2, 5, 6, 7, 8}
    z = np.load(os.path.join(ROOT, "tests", "golden", "qwen2_q2-long.npz"))
    assert z["lens"].max() == 8192 and str(z["shape"]) == "q2-tiny-g7" and os.path.getsize(z.fid.name) < 1 << 20
    for n in names:
        z = np.load(os.path.join(ROOT, "tests", "golden", f"qwen2_{n}.npz"))
        assert float(z["cos_bar"]) == max(ref.COS_BAR, float(z["bf16_cos"])) and float(z["abs_bar"]) == max(ref.ABS_BAR, float(z["bf16_abs"]))
        assert float(z["bias_std"]) == (ref.BIDIR_BIAS_STD if n in ref.MODES else ref.BIAS_STD)


@pytest.mark.parametrize("name", ("q2-tiny-g7", "q2-bidir-mean"))
def test_fixture_is_float32_hf(name):
    """The stored expectation is float32 HF on the seeded weights."""
    z, w = _fixture(name)
    want = ref.reference(ref.hf_model(str(z["shape"]), w), z["ids"], z["lens"], attention=str(z["attention"]), pooling=str(z["pooling"]))
    assert np.abs(want - z["expected"]).max() <= 1e-5


@pytest.mark.parametrize("name,defect,applies", DEFECTS, ids=[f"{n}-{d}" for n, d, _ in DEFECTS])
def test_fixture_discriminates(name, defect, applies):
    """Each defect moves every row it applies to by at least 10 times the fixture's 1 - cos bar (float32 HF alone)."""
    z, w = _fixture(name)
    rows = [i for i, n in enumerate(z["lens"]) if applies(int(n))]
    assert len(rows) >= 2
    attention, pooling = str(z["attention"]), str(z["pooling"])
    if defect == "causal":
        got = ref.reference(ref.hf_model(str(z["shape"]), w), z["ids"], z["lens"], rows=set(rows), pooling=pooling, attention="causal")
    else:
        got = ref.reference(ref.defect_model(str(z["shape"]), w, defect), z["ids"], z["lens"], rows=set(rows), attention=attention, pooling=pooling)
    moved = _cosd(got, z["expected"][rows])
    print(f"{name} {defect}: moved {np.array2string(moved / float(z['cos_bar']), precision=1)} bars on rows of {z['lens'][rows]} tokens")
    assert (moved >= 10.0 * float(z["cos_bar"])).all(), moved


# ---- kernel references ---------------------------------------------------------------------------------------------------------------------
def _emulated(case, inp, vis_of, head_of=None, kv_of=None, written=None):
    """attention_emulate (the kernels' rounding scheme) of every (row, head) as ctx bits [B][S][nq * 128], on a buffer prefilled with the
    sentinel as the GPU worker's. head_of(h): the head whose q a wave uses; kv_of(h): the kv head it reads; written(h): False for a head
    no wave stores (its columns keep the prefill, the rows at or past the length included)."""
    S, hq, hk = case["S"], case["nq"], case["nkv"]
    G = hq // hk
    ctx = np.full((len(inp["lens"]), S, hq * qc.HD), qc.SENT, np.float32)
    for b, n in enumerate(int(x) for x in inp["lens"]):
        for h in range(hq):
            if written is not None and not written(h):
                continue
            cols = slice(h * qc.HD, (h + 1) * qc.HD)
            ctx[b, n:, cols] = 0.0
            if n:
                hh = head_of(h) if head_of else h
                g = kv_of(h) if kv_of else h // G
                ctx[b, :n, cols] = kr.attention_emulate(kr.bf16_value(inp["q"][b, hh])[:n], kr.bf16_value(inp["k"][b, g]),
                                                        kr.bf16_value(inp["v"][b, g]), vis_of(b, n))
    return kr.bf16_bits(ctx)


def _ratio(case, inp, ctx_bits):
    """The checker's verdict on a ctx buffer: the worst err / bound, inf where it finds a non-zero row at or past a length."""
    w = kr.Worst()
    try:
        qc.check_attention(case, inp, ctx_bits, w)
    except AssertionError:
        return float("inf")
    return w.ratio


SPLIT_SMALL = [c for c in qc.attn_cases() if c["name"] in ("q2attn_g5_S96_causal", "q2attn_g7_S96_bidir", "q2attn_g6_S96_bidir", "q2attn_g8_S160_causal",
                                                           "q2attn_g7_S64_causal", "q2attn_g5_S32_bidir")]


@pytest.mark.parametrize("case", SPLIT_SMALL, ids=[c["name"] for c in SPLIT_SMALL])
def test_split_attention_emulation_inside_the_bound_mutants_outside(case):
    inp = qc.attn_inputs(case)
    G, hk = case["G"], case["nkv"]
    GP = qc.parts(G)[1]
    op = lambda b, n: qc.visibility(case, inp["mask"][b])          # noqa: E731
    assert _ratio(case, inp, _emulated(case, inp, op)) <= 1.0
    # a part's head base forgotten: both workgroups of a group compute heads 0 .. GP - 1, the heads of part 1 are never written
    assert _ratio(case, inp, _emulated(case, inp, op, written=lambda h: h % G < GP)) > 1.0, "part 1 never written"
    # ... or written from the q of part 0's head at the same wave slot
    assert _ratio(case, inp, _emulated(case, inp, op, head_of=lambda h: h - GP if h % G >= GP else h)) > 1.0, "part 1 on part 0's q"
    # the grouped-query map off by one kv head
    assert _ratio(case, inp, _emulated(case, inp, op, kv_of=lambda h: (h // G + 1) % hk)) > 1.0, "neighbouring kv head"
    # a surplus wave (G = 5, 7) storing its zero rows into head 0 of the next kv group / the next token row
    if G % 2:
        stray = kr.bf16_value(_emulated(case, inp, op)).reshape(len(inp["lens"]), case["S"], -1).copy()
        flat = stray.reshape(-1, qc.HD)                           # [(b, s, h)][128]: the head slot behind the last head of a group
        for b, n in enumerate(int(x) for x in inp["lens"]):
            if n < case["S"]:                                      # the workgroups wholly past the length: their surplus wave's zero_row
                for s in range((n + 31) // 32 * 32, case["S"]):
                    for kvh in range(hk):
                        slot = (b * case["S"] + s) * case["nq"] + kvh * G + G
                        if slot < flat.shape[0]:
                            flat[slot] = 0.0
        assert _ratio(case, inp, kr.bf16_bits(stray)) > 1.0, "surplus wave's stray zero rows"
    if case["bidir"]:
        mutants = {"causal in place of bidirectional": lambda b, n: kr.Visibility(inp["mask"][b], causal=True),
                   "first pad key attended": lambda b, n: qc.visibility(case, inp["mask"][b], pad=1),
                   "last real key dropped": lambda b, n: qc.visibility(case, inp["mask"][b], pad=-1) if n > 1 else qc.visibility(case, inp["mask"][b])}
    else:
        mutants = {"one past the diagonal": lambda b, n: qc.visibility(case, inp["mask"][b], diag=1),
                   "diagonal dropped": lambda b, n: qc.visibility(case, inp["mask"][b], diag=-1) if n > 1 else qc.visibility(case, inp["mask"][b]),
                   "bidirectional in place of causal": lambda b, n: kr.Visibility(inp["mask"][b])}
    for name, vis_of in mutants.items():
        assert _ratio(case, inp, _emulated(case, inp, vis_of)) > 1.0, name


def test_attention_case_list():
    cases = qc.attn_cases()
    names = {c["name"] for c in cases}
    assert len(names) == len(cases) == 4 * 2 * 2 + 2 * 3 * 2 + 2
    for G in (5, 6, 7, 8):
        assert {f"q2attn_g{G}_S{S}_{m}" for S in (96, 160) for m in ("causal", "bidir")} <= names
    for G in (5, 7):
        assert {f"q2attn_g{G}_S{S}_{m}" for S in (32, 64, 288) for m in ("causal", "bidir")} <= names
    assert {"q2attn_g7_S2048_causal", "q2attn_g7_S2048_bidir"} <= names and sum(c["S"] >= 2048 for c in cases) == 2
    assert all(c["nq"] // c["nkv"] == c["G"] and c["nkv"] == 2 and c["S"] % 32 == 0 for c in cases)
    assert [qc.parts(G) for G in (5, 6, 7, 8)] == [(2, 3), (2, 3), (2, 4), (2, 4)]
    # a full row directly behind an empty and behind a 1-token row
    assert qc.lengths_for(160) == [160, 0, 159, 1, 77, 160]
    assert sorted(c["nq"] // c["nkv"] for c in qc.equal_cases()) == [2, 3, 4]
    # the probes of a case: a neighbouring kv head, the other part, one past the diagonal, the first pad key
    case = [c for c in cases if c["name"] == "q2attn_g7_S96_causal"][0]
    pairs = qc._probe_pairs(case, 95, 0)
    assert {k for _, _, k in pairs} == {qc.OWN, qc.NEIGHBOUR, qc.OTHER_PART}
    assert (94, 95, qc.OWN) in pairs and (31, 32, qc.OWN) in pairs and (31, 31, qc.OWN) in pairs and (63, 0, qc.OWN) in pairs


def test_qkv_gemm_reference_holds_an_emulation_and_flags_the_bias_mutants():
    """float64 x W^T + bias at kernel_refs' GEMM bound: a float32-accumulated bf16 product inside it; the neighbour's bias (bias[n + 1]
    in place of bias[n]) and the bias dropped outside. On the first 64 rows of each case (the reference costs by the row)."""
    for c in qc.gemm_cases():
        inp = qc.gemm_inputs(c)
        assert inp["bias"].shape == (c["N"],) and (np.abs(inp["bias"]) == 64.0).sum() == 8 and 1.5 < inp["bias"][np.abs(inp["bias"]) < 64].std() < 2.5
        inp = dict(inp, x=inp["x"][:64])
        want, bound = qc.gemm_expect(c, inp)
        emu = kr.bf16_round((kr.bf16_value(inp["x"]).astype(np.float32) @ kr.bf16_value(inp["w"]).astype(np.float32).T + inp["bias"]).astype(np.float32))
        w = kr.Worst()
        w.add(emu, want, bound, c["name"])
        assert 0 < w.ratio <= 1.0, str(w)
        for name, bias in (("neighbour's bias", np.roll(inp["bias"], -1)), ("bias dropped", np.zeros_like(inp["bias"]))):
            m = kr.Worst()
            m.add(kr.bf16_round(qc.gemm_expect(c, inp, bias=bias)[0].astype(np.float32)), want, bound, name)
            assert m.ratio > 1.0, name
