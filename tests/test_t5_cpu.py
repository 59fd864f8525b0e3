"""CPU tests of the T5 path: the clamped relative-bias table against HF's T5Attention.compute_bias, config.json -> shape (and what is
refused, by field name), the checkpoint loader on both checkpoint kinds, the committed fixtures (reproduced from float32
T5EncoderModel, and sensitive enough to the bias, its direction, its alignment, the missing score scale and the gate order that a
forward pass wrong in one of them could not pass), the provider's routing and refusals, the new symbols in header / binding /
library, and the register budget of every k_attn_long instantiation."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import archi_amd.t5 as t5
from archi_amd.t5 import T5_SHAPES
from tests import t5_ref as tr
from tests.golden import make_t5_fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = T5_SHAPES["sentence-transformers/gtr-t5-base"]


# ---- the bias table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("buckets,D,S", [(32, 128, 700), (16, 32, 200), (8, 16, 200)])
def test_clamped_table_is_hf_compute_bias(buckets, D, S):
    """t5_rel_table indexed by clamp(k - q, -D, D) + D is torch.equal to T5Attention.compute_bias's [heads][S][S] bias."""
    from transformers import T5Config
    from transformers.models.t5.modeling_t5 import T5Attention
    heads = 3
    cfg = T5Config(vocab_size=32, d_model=heads * 64, d_kv=64, d_ff=64, num_layers=1, num_heads=heads, relative_attention_num_buckets=buckets,
                   relative_attention_max_distance=D, is_encoder_decoder=False, is_decoder=False)
    attn = T5Attention(cfg, has_relative_attention_bias=True)
    with torch.no_grad():
        attn.relative_attention_bias.weight.copy_(torch.randn(buckets, heads, generator=torch.Generator().manual_seed(buckets)))
        want = attn.compute_bias(S, S)[0]                                                      # [heads][S][S]
    tab = torch.from_numpy(t5.t5_rel_table(attn.relative_attention_bias.weight.detach(), buckets, D))
    assert tab.shape == (heads, 2 * D + 1) and tab.dtype == torch.float32
    idx = (torch.arange(S)[None, :] - torch.arange(S)[:, None]).clamp(-D, D) + D               # key - query
    assert torch.equal(tab[:, idx], want)
    assert not torch.equal(tab, tab.flip(1))                                                   # the two sides differ: direction matters


# ---- config reader -------------------------------------------------------------------------------------------------------------------
def _cfg(**change):
    d = t5.shape_config_dict(BASE)
    d.update(change)
    return d


def test_released_shapes():
    assert t5.t5_config_shape(_cfg(), dense=(768,)) == BASE
    assert t5.t5_config_shape(t5.shape_config_dict("t5-v1_1-large-encoder")) == T5_SHAPES["t5-v1_1-large-encoder"]
    for name, (H, L, heads, dff, kind) in {"sentence-transformers/gtr-t5-base": (768, 12, 12, 3072, "relu"),
                                           "sentence-transformers/gtr-t5-large": (1024, 24, 16, 4096, "relu"),
                                           "sentence-transformers/sentence-t5-base": (768, 12, 12, 3072, "relu"),
                                           "sentence-transformers/sentence-t5-large": (1024, 24, 16, 4096, "relu"),
                                           "t5-v1_1-base-encoder": (768, 12, 12, 2048, "gated-gelu"),
                                           "t5-v1_1-large-encoder": (1024, 24, 16, 2816, "gated-gelu")}.items():
        s = T5_SHAPES[name]
        assert (s[1], s[2], s[3], s[5], s[6]) == (H, L, heads, dff, kind) and s[7:10] == (32, 128, 1e-6)
    # a full T5 checkpoint's config (decoder fields, dense_act_fn as transformers writes it) gives the same tuple
    full = _cfg(is_encoder_decoder=True, num_decoder_layers=12, dense_act_fn="relu", is_gated_act=False, architectures=["T5ForConditionalGeneration"])
    assert t5.t5_config_shape(full, dense=(768,)) == BASE
    hf = t5.shape_hf_config("t5-tiny-gated")
    assert hf.is_gated_act and hf.dense_act_fn == "gelu_new" and hf.d_kv == 64


@pytest.mark.parametrize("cfg,msg", [
    (_cfg(model_type="mt5"), "model_type"),
    (_cfg(d_kv=128, num_heads=6), "d_kv"),                                   # t5-3b / 11b
    (_cfg(num_heads=8), "num_heads"),                                        # inner width != d_model
    (_cfg(d_model=512, num_heads=6), "num_heads"),                           # v1.1-small
    (_cfg(d_model=2048, num_heads=32), "d_model"),                           # xl
    (_cfg(d_model=192, num_heads=3), "d_model"),
    (_cfg(d_ff=1000), "d_ff"),
    (_cfg(relative_attention_max_distance=0), "relative_attention_max_distance"),
    (_cfg(relative_attention_max_distance=5000), "relative_attention_max_distance"),
    (_cfg(layer_norm_epsilon=0.0), "layer_norm_epsilon"),
    (_cfg(feed_forward_proj="gated-silu"), "feed_forward_proj"),
    (_cfg(feed_forward_proj="gelu"), "feed_forward_proj"),
    (_cfg(relative_attention_num_buckets=31), "relative_attention_num_buckets"),
    (_cfg(num_layers=65), "num_layers"),
    (_cfg(dense_act_fn="gelu_new"), "dense_act_fn"),
])
def test_config_refusals_name_the_field(cfg, msg):
    with pytest.raises(ValueError, match=msg):
        t5.t5_config_shape(cfg, "cfg.json")


# ---- weights -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t5-tiny-relu", "t5-tiny-gated"])
def test_weight_names_load_into_t5_encoder_model(name):
    shape = T5_SHAPES[name]
    w = t5.random_t5_weights(shape, seed=3)
    assert sorted(w) == sorted(t5.weight_names(shape[2], shape[6], len(shape[12])))
    model = tr.hf_model(shape, w)                                            # asserts nothing unexpected, nothing but the tied embedding missing
    sd = model.state_dict()
    assert torch.equal(sd["encoder.block.1.layer.0.SelfAttention.k.weight"], torch.from_numpy(w["l1.wk"]))
    assert torch.equal(sd["shared.weight"], torch.from_numpy(w["shared"])) and torch.equal(sd["encoder.embed_tokens.weight"], sd["shared.weight"])
    for k, v in w.items():
        if k.split(".")[-1] in t5.MATRIX_KEYS or k in ("shared", "rel_bias"):
            assert np.array_equal(v, torch.from_numpy(v).to(torch.bfloat16).float().numpy()), k       # bf16-valued
    assert t5.random_t5_weights(shape, seed=3, bias_std=4.0)["rel_bias"].std() > 1.5 * w["rel_bias"].std()


def test_both_checkpoint_kinds_load_to_identical_arrays(tmp_path):
    """A T5EncoderModel checkpoint (encoder.embed_tokens.weight, no shared.weight) and a full T5 checkpoint (shared.weight, decoder.*
    and lm_head beside the encoder) give the same shape and the same arrays; the Dense module comes with them."""
    shape = T5_SHAPES["t5-base-cut2"][:2] + (1,) + T5_SHAPES["t5-base-cut2"][3:]
    w = t5.random_t5_weights(shape, seed=5)
    got = []
    for full in (False, True):
        d = tr.write_checkpoint(str(tmp_path / f"full{int(full)}"), shape, w, full_model=full)
        s, ww = t5.load_t5_weights(d)
        assert s == shape and sorted(ww) == sorted(w)
        got.append(ww)
    for k in w:
        assert torch.equal(torch.as_tensor(got[0][k]), torch.as_tensor(got[1][k])), k
        assert np.array_equal(np.asarray(got[0][k]), w[k]), k
    assert tuple(got[0]["dense0"].shape) == (768, 768)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
def test_fixture_set_is_what_the_issue_lists():
    names = sorted(fx.CASES)
    assert names == ["base_cut2", "tiny_d16", "tiny_gated", "tiny_long", "tiny_relu"] and all(os.path.exists(fx.path(n)) for n in names)
    assert fx.CASES["tiny_relu"][4] == fx.CASES["tiny_gated"][4] == [320, 200, 129, 64, 33, 5, 1]
    assert (T5_SHAPES[fx.CASES["tiny_relu"][0]][6], T5_SHAPES[fx.CASES["tiny_gated"][0]][6]) == ("relu", "gated-gelu")
    assert all(T5_SHAPES[fx.CASES[n][0]][1:4] == (128, 2, 2) for n in names if n != "base_cut2")
    long = fx.CASES["tiny_long"][4]
    assert 1024 < long[0] <= 1152 and long[1:] == [300, 65] and T5_SHAPES[fx.CASES["tiny_long"][0]][8] == 128      # far blocks on both sides, S > 1024
    d16 = T5_SHAPES[fx.CASES["tiny_d16"][0]]
    assert d16[7:9] == (8, 16) and max(fx.CASES["tiny_d16"][4]) <= 160
    cut = T5_SHAPES[fx.CASES["base_cut2"][0]]
    assert cut[1:4] == (768, 2, 12) and cut[12] == (768,)
    assert T5_SHAPES["t5-tiny-relu"][5] % 128 != 0                            # the padded un-gated pair runs
    assert all(os.path.getsize(fx.path(n)) < 512 * 1024 for n in names) and fx.SENS_FACTOR == 10.0 and fx.MIN_SENS_ROW == 5
    assert all(fx.CASES[n][5] == "mean" for n in names)


@pytest.mark.parametrize("name", sorted(fx.CASES))
def test_fixture_is_reproduced_and_can_see_the_feature(name):
    """The committed fixture against the generating code run now: expected to 1e-6; the bar is per figure the larger of the
    project's bf16 bar and the all-bf16 T5EncoderModel's own error stored in the fixture. And from T5EncoderModel alone: the bias
    zeroed, key - query mirrored, the delta shifted by one, q scaled by 1 / 8 and (gated feed-forward) the gate and linear halves
    swapped each move every row of 5 tokens or more by at least 10x the fixture's 1 - cos bar, and the bias clamped at D / 2 moves
    every row longer than D + 64 by as much -- except where that mutant IS the model: with 8 buckets and D = 16 the last bucket of a
    side starts at distance 6, so clamping at 8 changes no entry of the table (asserted below); the D = 16 fixture's alignment
    and direction are covered by the other mutants."""
    stored = fx.load(name)
    shape_name, seed, std, bias_std, lens, pooling = fx.CASES[name]
    shape = T5_SHAPES[shape_name]
    assert (stored["shape_name"], stored["seed"], stored["std"], stored["bias_std"], stored["pooling"]) == (shape_name, seed, std, bias_std, pooling)
    assert list(stored["lens"]) == list(lens) and stored["expected"].shape == (len(lens), shape[12][-1] if shape[12] else shape[1])
    ids, lens_now = tr.make_ids(shape, seed, lens)
    assert np.array_equal(ids, stored["ids"])
    w = t5.random_t5_weights(shape, seed=seed, std=std, bias_std=bias_std)
    now = tr.reference(tr.hf_model(shape, w), ids, lens_now, pooling, tr.dense_tail(w))
    assert np.abs(now - stored["expected"]).max() <= 1e-6
    assert stored["bar_cos"] == max(tr.PROJECT_BAR_COS, stored["bf16_cos"]) and stored["bar_abs"] == max(tr.PROJECT_BAR_ABS, stored["bf16_abs"])
    assert 0 < stored["bf16_cos"] and 0 < stored["bf16_abs"]
    sens = tr.sensitivities(stored)
    same = tr.clamp_half_is_identity(shape, w)
    assert same == (name == "tiny_d16")
    assert sorted(sens) == sorted(m for m in tr.MUTANTS if (m != "swap_gate" or shape[6] == "gated-gelu") and (m != "clamp_half" or not same))
    assert same or (np.asarray(lens) > shape[8] + 64).any()
    ok, text = fx.sensitivity_ok(stored, sens)
    print(f"{name}: bar {stored['bar_cos']:.3g} / {stored['bar_abs']:.3g}; {text}")
    assert ok, text


# ---- provider ------------------------------------------------------------------------------------------------------------------------
def test_provider_routes_t5_checkpoints_and_refuses_before_any_gpu_work(tmp_path):
    from archi_amd._lib import HipBackendError
    from archi_amd.decoder import BpeTokenizer
    from archi_amd.embeddings import ArchiHipEmbeddings, _is_nomic, _is_t5
    from tests.decoder_ref import CORPUS
    shape = T5_SHAPES["t5-tiny-gated"][:12] + ((64,),)
    w = t5.random_t5_weights(shape, seed=1)
    d = tr.write_checkpoint(str(tmp_path / "ckpt"), shape, w, pooling="mean", max_seq_length=96, corpus=CORPUS)
    assert _is_t5(d) and not _is_nomic(d) and _is_t5("sentence-transformers/gtr-t5-base") and not _is_t5("nomic-ai/nomic-embed-text-v1.5")
    tok = BpeTokenizer(os.path.join(d, "tokenizer.json"))
    rows = tok.encode_batch(["tier-2 storage", ""], 96)
    assert all(r[-1] == 1 for r in rows) and rows[1] == [1]                      # the post-processor appends </s>
    try:
        emb = ArchiHipEmbeddings(d)
    except HipBackendError:
        pass
    else:       # a GPU is present: the checkpoint's sentence-transformers files were read
        assert (emb.pooling, emb.max_seq_length, emb.normalize, emb.dimensions) == ("mean", 96, True, 64)
        emb.encoder.close()
    for p in ("f32", "bf16x3"):
        with pytest.raises(ValueError, match="bf16 only"):
            ArchiHipEmbeddings(d, model_kwargs={"precision": p})
    with pytest.raises(FileNotFoundError, match="synthetic_seed"):
        ArchiHipEmbeddings("sentence-transformers/gtr-t5-base")
    pj = os.path.join(d, "1_Pooling", "config.json")
    pc = json.load(open(pj))
    json.dump(dict(pc, include_prompt=False), open(pj, "w"))                     # instructor's pool
    with pytest.raises(ValueError, match="include_prompt"):
        ArchiHipEmbeddings(d)
    json.dump(dict(pc, pooling_mode_mean_tokens=False, pooling_mode_max_tokens=True), open(pj, "w"))
    with pytest.raises(ValueError, match="pooling"):
        ArchiHipEmbeddings(d)
    json.dump(pc, open(pj, "w"))
    cj = os.path.join(d, "config.json")
    cfg = json.load(open(cj))
    json.dump(dict(cfg, feed_forward_proj="gated-silu"), open(cj, "w"))
    with pytest.raises(ValueError, match="feed_forward_proj"):
        ArchiHipEmbeddings(d)
    json.dump(cfg, open(cj, "w"))
    os.remove(os.path.join(d, "tokenizer.json"))
    with pytest.raises(FileNotFoundError, match="tokenizer.json"):
        ArchiHipEmbeddings(d)


def test_handle_and_dimensions():
    from archi_amd.config_plugin import EMBEDDING_DIMENSIONS
    for name in ("sentence-transformers/gtr-t5-base", "sentence-transformers/gtr-t5-large", "sentence-transformers/sentence-t5-base",
                 "sentence-transformers/sentence-t5-large"):
        assert EMBEDDING_DIMENSIONS[name] == 768 == T5_SHAPES[name][12][-1]
    assert (t5.HipT5.family, t5.HipT5.prefix, t5.HipT5.embed_key, t5.HipT5.abi_pooling) == ("T5", "t5", "shared", True)
    with pytest.raises(ValueError, match="layers"):
        t5.HipT5(BASE[:2] + (65,) + BASE[3:], {})


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
def test_symbols_in_header_binding_and_library():
    from archi_amd import _lib
    src = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    assert int(re.search(r"#define AK_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == 5
    lib = _lib.load()
    assert lib.ak_abi_version() == 5
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in ("ak_t5_create", "ak_t5_forward_lens", "ak_t5_destroy"):
        assert re.search(rf"\bint {name}\(", src) and name in bound and hasattr(lib, name)
    declared = set(re.findall(r"\b(ak_[a-z0-9_]+)\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    assert declared == bound                                                     # the header and _lib.SYMBOLS agree
    args = {n: a for n, _, a in _lib.SYMBOLS}
    assert args["ak_t5_forward_lens"] == args["ak_nomic_forward_lens"] and args["ak_t5_create"][1:] == args["ak_nomic_create"][1:]


def test_config_struct_matches_header():
    from archi_amd._lib import AkT5Config
    src = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    body = re.search(r"typedef struct AkT5Config \{(.*?)\} AkT5Config;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int|float)\s+(\w+)(\[2\])?\s*;", body)
    assert [n for _, n, _ in fields] == [n for n, _ in AkT5Config._fields_] == \
        ["vocab_size", "hidden", "layers", "heads", "head_dim", "d_ff", "gated", "max_distance", "ln_eps", "n_dense", "dense_out"]
    assert ctypes.sizeof(AkT5Config) == 48 and AkT5Config._fields_[8][1] is ctypes.c_float


def test_t5_wrappers_stay_out_of_the_product_library():
    """ak_kts_t5_* (csrc/kernel_test.hip) exist in libarchi_hip_dbg.so only and are exactly the t5 entries of _lib.KTS_SYMBOLS; the
    ak_kt_* set and the other ak_kts_* subsets are what they were."""
    from archi_amd import _lib

    def exported(name):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "archi_amd", "lib", name)], stdout=subprocess.PIPE,
                             check=True).stdout.decode()
        return set(re.findall(r"\b(ak_kts_t5_[a-z0-9_]+)\b", out))

    _lib.load()
    assert exported("libarchi_hip.so") == set()
    names = {n for n, _, _ in _lib.KTS_SYMBOLS if n.startswith("ak_kts_t5_")}
    assert exported("libarchi_hip_dbg.so") == names == {"ak_kts_t5_attn", "ak_kts_t5_gemm_relu"}
    assert len(_lib.KT_SYMBOLS) == 19 and not any("t5" in n for n, _, _ in _lib.KT_SYMBOLS + _lib.KTG_SYMBOLS)
    for sub, n in (("ak_kts_nb_", 3), ("ak_kts_ll_", 3), ("ak_kts_q2_", 1)):
        assert sum(k.startswith(sub) for k, _, _ in _lib.KTS_SYMBOLS) == n
    assert "ak_kts_" not in open(os.path.join(ROOT, "include", "archi_knn.h")).read()


def test_no_attn_long_instantiation_spills():
    """-Rpass-analysis=kernel-resource-usage with the Makefile's flags: every k_attn_long kernel -- the two instantiations that existed,
    under the mangled names other tests know them by, and the biased k_attn_long_relbias -- reports no spilled register and no
    scratch, and 16 640 bytes of static LDS (the bias table is dynamic); the biased walk keeps three waves per SIMD."""
    from scripts.kernel_resources import kernel_resources
    res = {n: r for n, r in kernel_resources("attn_long.hip").items() if "k_attn_long" in n}
    assert len(res) == 3 and all(sum(k in n for n in res) == 1 for k in ("k_attn_longILb0EEE", "k_attn_longILb1EEE", "k_attn_long_relbiasE"))
    for n, r in res.items():
        print(n, {k: r[k] for k in ("VGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")})
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (n, r)
        assert r["LDS Size [bytes/block]"] == 16640 and r["Occupancy [waves/SIMD]"] == 3, (n, r)
    t5_res = kernel_resources("t5.hip")
    for k in ("k_t5_embed", "k_t5_pool_part", "k_t5_pool_fin"):
        use = [r for n, r in t5_res.items() if k in n]
        assert use and all(r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0 for r in use), (k, use)
    src = open(os.path.join(ROOT, "archi_amd", "csrc", "t5.hip")).read()
    assert "getenv" not in src and "switches.h" not in src
