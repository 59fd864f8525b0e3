"""GPU tests of the HIP Qwen2 decoder (archi_amd.qwen2.HipQwen2, ak_qwen2_*): the fixtures of tests/golden/make_qwen2_fixtures.py (float32
transformers.Qwen2Model on the CPU, eager attention, each row alone) at the bar each fixture carries -- the larger of the bf16 encoder
bar (3e-4 / 3e-3) and HF's own bf16 error against its float32 self, no margin --, the Qwen2-7B and -1.5B layer shapes cut to two layers
against the same reference, padding / determinism / batching invariances at 7 and 5 query heads per kv head, the refusals, and text end
to end through ArchiHipEmbeddings with the is_causal default, attention="bidirectional" and the pooling override."""
import glob
import json
import os

import numpy as np
import pytest

from archi_amd.qwen2 import QWEN2_SHAPES, random_qwen2_weights
from tests.qwen2_ref import ABS_BAR, COS_BAR

pytestmark = pytest.mark.gpu
FIX = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "qwen2_*.npz")))

_WEIGHTS = {}


def _weights(shape, seed, std=0.05, bias_std=2.0):
    key = (shape, seed, std, bias_std)
    if key not in _WEIGHTS:
        _WEIGHTS[key] = random_qwen2_weights(shape, seed=seed, std=std, bias_std=bias_std)
    return _WEIGHTS[key]


def teardown_module():
    """Nothing of this file stays behind in the suite's process: the cached weights and what torch still holds on either side."""
    import gc
    import torch
    _WEIGHTS.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _qwen2(shape, seed, **kw):
    from archi_amd.qwen2 import HipQwen2
    return HipQwen2(QWEN2_SHAPES[shape], _weights(shape, seed, **kw), device=0)


def _cos(got, want):
    return (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))


def test_fixtures_present():
    assert len(FIX) == 8


@pytest.mark.parametrize("path", FIX, ids=[os.path.basename(p) for p in FIX])
def test_qwen2_matches_hf_fixture(hip, path):
    z = np.load(path)
    from archi_amd.qwen2 import HipQwen2
    from tests.qwen2_ref import fixture_weights
    shape, attention, pooling = str(z["shape"]), str(z["attention"]), str(z["pooling"])
    name = os.path.basename(path)[len("qwen2_"):-len(".npz")]
    m = HipQwen2(QWEN2_SHAPES[shape]._replace(attention=attention, pooling=pooling), fixture_weights(name), device=0)
    got = m.forward(z["ids"], z["lens"]).cpu().numpy()          # pools as the shape says
    m.close()
    want = z["expected"]
    cos = _cos(got, want)
    cos_bar, abs_bar = float(z["cos_bar"]), float(z["abs_bar"])
    err_cos, err_abs = 1 - cos.min(), np.abs(got - want).max()
    print(f"{os.path.basename(path)}: 1 - cos max {err_cos:.2e} (bar {cos_bar:.2e}, err / bar {err_cos / cos_bar:.2f}), "
          f"max |d| {err_abs:.2e} (bar {abs_bar:.2e}, err / bar {err_abs / abs_bar:.2f})")
    assert cos_bar >= COS_BAR and abs_bar >= ABS_BAR
    assert cos_bar == max(COS_BAR, float(z["bf16_cos"])) and abs_bar == max(ABS_BAR, float(z["bf16_abs"]))
    assert err_cos <= cos_bar, f"min cosine {cos.min()}"
    assert err_abs <= abs_bar, f"max abs diff {err_abs}"


@pytest.mark.parametrize("shape,seed,lens,rows", [
    ("gte-qwen2-7b-2l", 71, (512, 300, 129, 65, 33, 17, 9, 5, 3, 2, 1, 64, 31), (3, 5, 11, 12)),
    ("gte-qwen2-1.5b-2l", 72, (512, 129, 65, 33, 9, 1), (2, 3, 4))])
def test_released_layer_shapes_against_hf(hip, shape, seed, lens, rows):
    """The Qwen2-7B layer shape cut to 2 layers (hidden 3584, 28 / 4 heads: 7 query heads per kv head, intermediate 18944: GEMM widths
    3584, 4608 and 18944) on about 1.2 k tokens in rows of 1 to 512, and the 1.5B one (1536, 12 / 2 heads: 6 per kv head, 8960) on
    fewer rows. Against float32 Qwen2Model and at the bar the fixtures use, HF's own bf16 error measured on the spot on a few short rows."""
    import torch
    from archi_amd.qwen2 import HipQwen2
    from tests.qwen2_ref import hf_model, reference
    w = random_qwen2_weights(shape, seed=seed, std=0.02)      # not kept in the cache
    rng = np.random.default_rng(seed)
    lens = np.array(lens, np.int32)
    ids = np.zeros((len(lens), 512), np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.integers(0, QWEN2_SHAPES[shape].vocab, n)
    m = HipQwen2(QWEN2_SHAPES[shape], w, device=0)
    got = m.forward(ids, lens).cpu().numpy()
    m.close()
    del m
    want = reference(hf_model(shape, w), ids, lens)
    low = reference(hf_model(shape, w, dtype=torch.bfloat16), ids, lens, rows=set(rows))
    cos_bar = max(COS_BAR, float((1 - _cos(low, want[list(rows)])).max()))
    abs_bar = max(ABS_BAR, float(np.abs(low - want[list(rows)]).max()))
    cos = _cos(got, want)
    print(f"{shape}: 1 - cos max {1 - cos.min():.2e} (bar {cos_bar:.2e}), max |d| {np.abs(got - want).max():.2e} (bar {abs_bar:.2e})")
    assert 1 - cos.min() <= cos_bar and np.abs(got - want).max() <= abs_bar


@pytest.mark.parametrize("shape", ("q2-tiny-g7", "q2-tiny-g5"))
def test_invariances(hip, shape):
    """Ids past the length do not matter and two forwards are bit-identical (array_equal); a row alone against the same row in a batch of
    64 is within 1 - cos 1e-5."""
    m = _qwen2(shape, 81)
    rng = np.random.default_rng(3)
    S = 160
    lens = np.array([160, 1, 33, 100, 64, 7, 0, 160], np.int32)
    ids = np.zeros((len(lens), S), np.int32)
    noisy = rng.integers(0, 1000, (len(lens), S)).astype(np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = noisy[i, :n]
    a = m.forward(ids, lens).cpu().numpy()
    b = m.forward(noisy, lens).cpu().numpy()
    c = m.forward(noisy, lens).cpu().numpy()
    assert np.isfinite(a).all() and not a[6].any()
    assert np.array_equal(a, b) and np.array_equal(b, c)
    lens = rng.integers(1, 385, 64).astype(np.int32)
    lens[17] = 211
    ids = rng.integers(0, 1000, (64, 384)).astype(np.int32)
    batch = m.forward(ids, lens).cpu().numpy()
    alone = m.forward(ids[17:18, :211], lens[17:18]).cpu().numpy()
    m.close()
    assert 1 - _cos(batch[17:18], alone)[0] <= 1e-5


def test_refusals_before_any_forward(hip):
    from archi_amd._lib import HipBackendError
    from archi_amd.qwen2 import HipQwen2
    shape = QWEN2_SHAPES["q2-tiny-g2"]
    w = _weights("q2-tiny-g2", 82)
    with pytest.raises(HipBackendError, match="8 query heads"):
        HipQwen2(shape._replace(q_heads=18), w, device=0)                    # G = 9
    with pytest.raises(ValueError, match="attention 'full'"):
        HipQwen2(shape._replace(attention="full"), w, device=0)
    m = HipQwen2(shape, w, device=0)
    import ctypes
    from archi_amd._lib import AkQwen2Config
    cfg, h = m._cfg, ctypes.c_void_p()
    ptrs = (ctypes.c_void_p * len(m._ptrs))(*m._ptrs)
    bad = AkQwen2Config(*[getattr(cfg, n) for n, _ in AkQwen2Config._fields_])
    bad.head_dim = 64
    assert m._lib.ak_qwen2_create(ctypes.byref(bad), ptrs, len(m._ptrs), ctypes.byref(h)) != 0 and not h.value
    assert "head_dim" in (m._lib.ak_last_error() or b"").decode()
    assert m._lib.ak_qwen2_create(ctypes.byref(cfg), ptrs, len(m._ptrs) - 3, ctypes.byref(h)) != 0 and not h.value      # the Llama count
    assert "2 + 12 * layers" in (m._lib.ak_last_error() or b"").decode()
    with pytest.raises(ValueError, match="pool 'last' or 'mean'"):
        m.forward(np.zeros((1, 32), np.int32), [3], pooling="cls")
    m.close()


def test_text_end_to_end(hip, tmp_path):
    """Checkpoint directory (config.json in transformers' dialect, safetensors with the bias tensors, tokenizer.json, lasttoken Pooling,
    Normalize) -> ArchiHipEmbeddings, against the float32 CPU model on the same ids; the top-10 of a query wherever the CPU scores are
    separated by more than 1e-3; the bidirectional mode by keyword and by config.json's is_causal, and the pooling override."""
    from archi_amd.embeddings import ArchiHipEmbeddings
    from tests.qwen2_ref import hf_model, reference, write_checkpoint
    shape = "q2-tiny-g7"
    w = _weights(shape, 91, bias_std=0.5)
    d = write_checkpoint(str(tmp_path / shape), shape, w, max_seq_length=64)
    assert json.load(open(os.path.join(d, "config.json")))["model_type"] == "qwen2"
    emb = ArchiHipEmbeddings(d)
    assert emb.dimensions == 256 and emb.pooling == "last" and emb.normalize and emb.max_seq_length == 64
    assert emb.encoder.shape == QWEN2_SHAPES[shape] and not emb.encoder.bidirectional
    docs = ["Muon chambers measure the momentum of tracks.", "Résumé: the µ-metal shield — “good enough” at σ = 3.",
            "Für die Kalibrierung wird eine Quelle verwendet.", "The beam energy was 6.8 TeV per proton.", "日本語のテキスト", "short",
            "Η ενέργεια του δέσμου " * 12, "trigger decision at 40 MHz", "The detector readout chain digitises every channel.",
            "A calorimeter stops the particle and measures its energy.", "Tracks that leave the calorimeter are muons.",
            "The quick brown fox jumps over the lazy dog " * 6]
    got = np.asarray(emb.embed_documents(docs), np.float32)
    ids, lens = emb.tokenizer.encode_batch_array([t.replace("\n", " ") for t in docs], emb.max_seq_length)
    assert lens.max() == 64
    model = hf_model(shape, w)
    want = reference(model, ids, lens)
    assert 1 - _cos(got, want).min() <= COS_BAR
    query = "Instruct: Given a physics question, retrieve relevant passages\nQuery: what is the beam energy?"
    q = np.asarray(emb.embed_query(query), np.float32)
    qi, ql = emb.tokenizer.encode_batch_array([query.replace("\n", " ")], emb.max_seq_length)
    q_want = reference(model, qi, ql)[0]
    assert 1 - float(q @ q_want / (np.linalg.norm(q) * np.linalg.norm(q_want))) <= COS_BAR
    gpu_order = np.argsort(-(got @ q), kind="stable")[:10]
    cpu_scores = want @ q_want
    order = np.argsort(-cpu_scores, kind="stable")
    for rank in range(10):
        sep_prev = rank == 0 or cpu_scores[order[rank - 1]] - cpu_scores[order[rank]] > 1e-3
        sep_next = cpu_scores[order[rank]] - cpu_scores[order[rank + 1]] > 1e-3
        if sep_prev and sep_next:
            assert gpu_order[rank] == order[rank], (gpu_order, order[:10], cpu_scores[order[:11]])
    for kw, what in (({"attention": "full"}, "attention 'full'"), ({"pooling": "cls"}, "pooling 'cls'"), ({"precision": "f32"}, "bf16 only")):
        with pytest.raises(ValueError, match=what):
            ArchiHipEmbeddings(d, model_kwargs=kw)
    emb.encoder.close()
    sub = np.flatnonzero(lens >= 5)
    for kw, attention, pooling in (({"attention": "bidirectional"}, "bidirectional", "last"),      # (the checkpoint's Pooling module: lasttoken)
                                   ({"attention": "bidirectional", "pooling": "mean"}, "bidirectional", "mean"), ({"pooling": "mean"}, "causal", "mean")):
        e2 = ArchiHipEmbeddings(d, model_kwargs=kw)
        assert e2.pooling == pooling and e2.encoder.shape.attention == attention
        got2 = np.asarray(e2.embed_documents(docs), np.float32)
        want2 = reference(model, ids, lens, attention=attention, pooling=pooling)
        assert 1 - _cos(got2, want2).min() <= COS_BAR, kw
        assert (1 - _cos(got2[sub], got[sub])).min() > 10 * COS_BAR, kw      # and it is another embedding than the causal last-token one
        e2.encoder.close()
    # config.json says is_causal: false -> bidirectional without a keyword; the keyword still wins
    d2 = write_checkpoint(str(tmp_path / "noncausal"), shape, w, max_seq_length=64, is_causal=False)
    e3 = ArchiHipEmbeddings(d2)
    assert e3.encoder.bidirectional and e3.pooling == "last"
    got3 = np.asarray(e3.embed_documents(docs), np.float32)
    assert 1 - _cos(got3, reference(model, ids, lens, attention="bidirectional")).min() <= COS_BAR
    e3.encoder.close()
    e4 = ArchiHipEmbeddings(d2, model_kwargs={"attention": "causal"})
    assert not e4.encoder.bidirectional
    assert 1 - _cos(np.asarray(e4.embed_documents(docs), np.float32), want).min() <= COS_BAR
    e4.encoder.close()
