"""GPU tests of the HIP Mistral / Llama decoder (archi_amd.llama.HipLlama, ak_llama_*): the fixtures of
tests/golden/make_llama_fixtures.py (float32 transformers.MistralModel / LlamaModel on the CPU, eager attention, each row alone) at the
bar each fixture carries -- the larger of the bf16 encoder bar (3e-4 / 3e-3) and HF's own bf16 error against its float32 self, no margin
--, the Mistral-7B layer shape cut to two layers against the same reference, padding / determinism / batching invariances, and text end
to end through ArchiHipEmbeddings in both config dialects, with attention="bidirectional" and the pooling override."""
import glob
import os

import numpy as np
import pytest

from archi_amd.llama import LLAMA_SHAPES, random_llama_weights
from tests.llama_ref import ABS_BAR, COS_BAR

pytestmark = pytest.mark.gpu
FIX = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "llama_*.npz")))

_WEIGHTS = {}


def _weights(shape, seed, std):
    if (shape, seed, std) not in _WEIGHTS:
        _WEIGHTS[(shape, seed, std)] = random_llama_weights(shape, seed=seed, std=std)
    return _WEIGHTS[(shape, seed, std)]


def teardown_module():
    """Nothing of this file stays behind in the suite's process: the cached weights and what torch still holds on either side."""
    import gc
    import torch
    _WEIGHTS.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _llama(shape, seed, std=0.05):
    from archi_amd.llama import HipLlama
    return HipLlama(LLAMA_SHAPES[shape], _weights(shape, seed, std), device=0)


def _cos(got, want):
    return (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))


def test_fixtures_present():
    assert len(FIX) == 9


@pytest.mark.parametrize("path", FIX, ids=[os.path.basename(p) for p in FIX])
def test_llama_matches_hf_fixture(hip, path):
    z = np.load(path)
    from archi_amd.llama import HipLlama
    shape, attention, pooling = str(z["shape"]), str(z["attention"]), str(z["pooling"])
    from tests.llama_ref import fixture_weights
    name = os.path.basename(path)[len("llama_"):-len(".npz")]
    m = HipLlama(LLAMA_SHAPES[shape]._replace(attention=attention, pooling=pooling), fixture_weights(name), device=0)
    got = m.forward(z["ids"], z["lens"]).cpu().numpy()          # pools as the shape says
    if pooling == "mean":
        assert np.array_equal(got, m.forward(z["ids"], z["lens"], pooling="mean").cpu().numpy())
    m.close()
    want = z["expected"]
    cos = _cos(got, want)
    cos_bar, abs_bar = float(z["cos_bar"]), float(z["abs_bar"])
    print(f"{os.path.basename(path)}: 1 - cos max {1 - cos.min():.2e} (bar {cos_bar:.2e}), max |d| {np.abs(got - want).max():.2e} (bar {abs_bar:.2e})")
    assert cos_bar >= COS_BAR and abs_bar >= ABS_BAR
    assert 1 - cos.min() <= cos_bar, f"min cosine {cos.min()}"
    assert np.abs(got - want).max() <= abs_bar, f"max abs diff {np.abs(got - want).max()}"


def test_mistral_7b_layer_shape_against_hf(hip):
    """The Mistral-7B layer shape cut to 2 layers (hidden 4096, 32 / 8 heads, intermediate 14336, 2000 vocabulary rows, window 4096),
    16 x 512: every GEMM on the wide tile. Against float32 MistralModel and at the bar the fixtures use, HF's own bf16 error measured
    on the spot."""
    import torch
    from tests.llama_ref import hf_model, reference
    shape, seed, std = "mistral-7b-2l", 51, 0.02
    w = random_llama_weights(shape, seed=seed, std=std)      # 1.7 GB as float32: not kept in the cache
    rng = np.random.default_rng(seed)
    lens = np.array([512, 300, 129, 65, 33, 17, 9, 5, 3, 2, 1, 1, 64, 100, 31, 200], np.int32)      # (the float32 CPU reference costs by the token)
    ids = np.zeros((len(lens), 512), np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.integers(0, LLAMA_SHAPES[shape].vocab, n)
    from archi_amd.llama import HipLlama
    m = HipLlama(LLAMA_SHAPES[shape], w, device=0)
    got = m.forward(ids, lens).cpu().numpy()
    m.close()
    del m
    want = reference(hf_model(shape, w), ids, lens)
    rows = (3, 5, 13, 14)                                      # HF in bf16 on the CPU is slow at this width: its error on four short rows
    low = reference(hf_model(shape, w, dtype=torch.bfloat16), ids, lens, rows=rows)
    cos_bar = max(COS_BAR, float((1 - _cos(low, want[list(rows)])).max()))
    abs_bar = max(ABS_BAR, float(np.abs(low - want[list(rows)]).max()))
    cos = _cos(got, want)
    print(f"mistral-7b-2l: 1 - cos max {1 - cos.min():.2e} (bar {cos_bar:.2e}), max |d| {np.abs(got - want).max():.2e} (bar {abs_bar:.2e})")
    assert 1 - cos.min() <= cos_bar and np.abs(got - want).max() <= abs_bar


def test_ids_past_length_do_not_matter(hip):
    m = _llama("ll-win", 21)
    rng = np.random.default_rng(3)
    S = 160
    lens = np.array([160, 1, 33, 100, 64, 7], np.int32)
    ids = np.zeros((len(lens), S), np.int32)
    noisy = rng.integers(0, 1000, (len(lens), S)).astype(np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = noisy[i, :n]
    a = m.forward(ids, lens).cpu().numpy()
    b = m.forward(noisy, lens).cpu().numpy()
    m.close()
    assert np.isfinite(a).all()
    assert np.array_equal(a, b)


def test_llama_deterministic(hip):
    m = _llama("ll-tiny-g4", 22)
    rng = np.random.default_rng(4)
    lens = rng.integers(1, 257, 24).astype(np.int32)
    ids = rng.integers(0, 1000, (24, 256)).astype(np.int32)
    a = m.forward(ids, lens).cpu().numpy()
    b = m.forward(ids, lens).cpu().numpy()
    m.close()
    assert np.array_equal(a, b)


def test_row_alone_vs_in_batch(hip):
    m = _llama("ll-win", 23)
    rng = np.random.default_rng(6)
    lens = rng.integers(1, 385, 64).astype(np.int32)
    lens[17] = 211
    ids = rng.integers(0, 1000, (64, 384)).astype(np.int32)
    batch = m.forward(ids, lens).cpu().numpy()
    alone = m.forward(ids[17:18, :211], lens[17:18]).cpu().numpy()
    m.close()
    assert 1 - _cos(batch[17:18], alone)[0] <= 1e-5


def test_refusals_before_any_forward(hip):
    from archi_amd._lib import HipBackendError
    from archi_amd.llama import HipLlama
    shape = LLAMA_SHAPES["ll-tiny-g1"]
    w = _weights("ll-tiny-g1", 24, 0.05)
    with pytest.raises(HipBackendError, match="sliding_window"):
        HipLlama(shape._replace(window=-1), w, device=0)
    with pytest.raises(HipBackendError, match="4 query heads"):
        HipLlama(shape._replace(q_heads=10), w, device=0)
    with pytest.raises(ValueError, match="attention 'full'"):
        HipLlama(shape._replace(attention="full"), w, device=0)
    m = HipLlama(shape, w, device=0)
    with pytest.raises(ValueError, match="pool 'last' or 'mean'"):
        m.forward(np.zeros((1, 32), np.int32), [3], pooling="cls")
    m.close()


def test_default_rope_table_is_the_one_create_built(hip):
    """A default-RoPE shape runs on the table ak_llama_create built from theta; handing it HF's own inverse frequencies afterwards
    (ak_llama_set_rope_inv_freq, what a llama3 shape always gets) moves no row by more than 1 - cos 1e-6."""
    import ctypes
    from archi_amd._lib import check
    from archi_amd.llama import rope_inv_freq
    m = _llama("ll-tiny-g2", 25)
    rng = np.random.default_rng(8)
    lens = np.array([200, 64, 33, 1], np.int32)
    ids = rng.integers(0, 1000, (4, 200)).astype(np.int32)
    a = m.forward(ids, lens).cpu().numpy()
    inv = np.ascontiguousarray(rope_inv_freq(m.shape), np.float32)
    check(m._lib.ak_llama_set_rope_inv_freq(m._h, ctypes.c_void_p(inv.ctypes.data)), "ak_llama_set_rope_inv_freq")
    b = m.forward(ids, lens).cpu().numpy()
    m.close()
    assert np.isfinite(a).all() and (1 - _cos(a, b)).max() <= 1e-6


@pytest.mark.parametrize("dialect,shape", [("mistral", "ll-win"), ("llama", "ll-l3")])
def test_text_end_to_end(hip, tmp_path, dialect, shape):
    """Checkpoint directory (config.json of the dialect, safetensors, tokenizer.json, lasttoken Pooling, Normalize) -> ArchiHipEmbeddings,
    against the float32 CPU model on the same ids; the top-10 of a query wherever the CPU scores are separated by more than 1e-3."""
    from archi_amd.embeddings import ArchiHipEmbeddings
    from tests.llama_ref import hf_model, reference, write_checkpoint
    w = _weights(shape, 31, 0.05)
    d = write_checkpoint(str(tmp_path / shape), shape, w, dialect=dialect, max_seq_length=64)
    emb = ArchiHipEmbeddings(d)
    assert emb.dimensions == 256 and emb.pooling == "last" and emb.normalize and emb.max_seq_length == 64
    assert emb.encoder.shape == LLAMA_SHAPES[shape]
    docs = ["Muon chambers measure the momentum of tracks.", "Résumé: the µ-metal shield — “good enough” at σ = 3.",
            "Für die Kalibrierung wird eine Quelle verwendet.", "The beam energy was 6.8 TeV per proton.", "日本語のテキスト", "short",
            "Η ενέργεια του δέσμου " * 12, "trigger decision at 40 MHz", "The detector readout chain digitises every channel.",
            "A calorimeter stops the particle and measures its energy.", "Tracks that leave the calorimeter are muons.",
            "The quick brown fox jumps over the lazy dog " * 6]
    got = np.asarray(emb.embed_documents(docs), np.float32)
    ids, lens = emb.tokenizer.encode_batch_array([t.replace("\n", " ") for t in docs], emb.max_seq_length)
    assert lens.max() == 64 and (ids[np.arange(len(lens)), 0] == ids[0, 0]).all()      # truncated to max_seq_length; <s> in front
    model = hf_model(shape, w, dialect)
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
    # the caller's statement that the checkpoint was trained without the causal mask, and the pooling override
    sub = np.flatnonzero(lens >= 5)
    for kw, attention, pooling in (({"attention": "bidirectional", "pooling": "mean"}, "bidirectional", "mean"),
                                   ({"attention": "bidirectional", "pooling": "last"}, "bidirectional", "last"), ({"pooling": "mean"}, "causal", "mean")):
        e2 = ArchiHipEmbeddings(d, model_kwargs=kw)
        assert e2.pooling == pooling and e2.encoder.shape.attention == attention and e2.encoder.window == (0 if attention == "bidirectional" else LLAMA_SHAPES[shape].window)
        got2 = np.asarray(e2.embed_documents(docs), np.float32)
        want2 = reference(model, ids, lens, attention=attention, pooling=pooling)
        assert 1 - _cos(got2, want2).min() <= COS_BAR, kw
        assert (1 - _cos(got2[sub], got[sub])).min() > 10 * COS_BAR, kw      # and it is another embedding than the causal last-token one
        e2.encoder.close()
