"""GPU tests of the ModernBERT path (ak_mbert_*: csrc/mbert.hip, the windowed k_attn_long of attn_long.hip, k_gemm MODE 8): the
fixtures of tests/golden/make_modernbert_fixtures.py (float32 transformers.ModernBertModel on the CPU) at the bar stored in each
fixture, the base shape at full depth and the large shape's width, the invariances the other families have, the entry points'
refusals, and text end to end through ArchiHipEmbeddings and ArchiHipVectorStore.

The bar of a fixture is, per figure, the larger of the project's bf16 encoder bar (1 - cos 3e-4, max |d| 3e-3) and the error of
ModernBertModel itself run all in bf16 on the CPU against its float32 self on the same rows; no margin on top.
Measured on MI355X (worst row of each fixture, 1 - cos / max |d|): see DESIGN.md section 9."""
import ctypes
import glob
import os

import numpy as np
import pytest

from archi_amd.modernbert import MODERNBERT_SHAPES, random_modernbert_weights

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIX = sorted(os.path.basename(p)[len("modernbert_"):-4] for p in glob.glob(os.path.join(GOLDEN, "modernbert_*.npz")))
FULL_SHAPE_COS_TOL = 1e-3          # the decoder's full-shape bar (tests/test_decoder_gpu.py)


def _load(name):
    from tests.golden.make_modernbert_fixtures import load
    return load(name)


def _model(shape, seed, std=0.1):
    from archi_amd.modernbert import HipModernBert
    w = random_modernbert_weights(shape, seed=seed, std=std)
    return HipModernBert(shape, w, device=0), w


def _report(got, want, what):
    from tests.modernbert_ref import cos_gap
    gap, dmax = float(cos_gap(got, want).max()), float(np.abs(got - want).max())
    print(f"{what}: 1 - cos max {gap:.3e}, max |d| {dmax:.3e}")
    return gap, dmax


def test_fixtures_present():
    assert len(FIX) >= 6, FIX
    lens = np.concatenate([_load(n)["lens"] for n in FIX])
    for n in (1, 64, 65, 129, 130, 512, 513, 8192):
        assert n in lens, n
    assert {_load(n)["pooling"] for n in FIX} == {"cls", "mean"}
    types = {MODERNBERT_SHAPES[_load(n)["shape_name"]][10] for n in FIX}
    assert any(set(t) == {1} for t in types) and any(set(t) == {0} for t in types) and any(set(t) == {0, 1} for t in types)


@pytest.mark.parametrize("name", FIX)
def test_model_matches_fixture(hip, name):
    c = _load(name)
    m, _ = _model(c["shape_name"], c["seed"], c["std"])
    got = m.forward(c["ids"], c["lens"], pooling=c["pooling"]).cpu().numpy()
    m.close()
    gap, dmax = _report(got, c["expected"], f"{name} (bar {c['bar_cos']:.3e} / {c['bar_abs']:.3e})")
    assert gap <= c["bar_cos"] and dmax <= c["bar_abs"], (gap, dmax)


@pytest.mark.parametrize("name", FIX)
def test_provider_matches_fixture(hip, name):
    """The same rows through ArchiHipEmbeddings.embed_token_arrays: length-sorted tiles, one S per tile."""
    from archi_amd.embeddings import ArchiHipEmbeddings
    c = _load(name)
    emb = ArchiHipEmbeddings(c["shape_name"], model_kwargs={"synthetic_seed": c["seed"], "synthetic_std": c["std"]},
                             encode_kwargs={"batch_tokens": 1024})
    assert emb.pooling == c["pooling"] and emb.normalize and emb.dimensions == c["expected"].shape[1] and emb.max_seq_length == 8192
    got = emb.embed_token_arrays(c["ids"], c["lens"])
    emb.encoder.close()
    gap, dmax = _report(got, c["expected"], f"{name} through the provider")
    assert gap <= c["bar_cos"] and dmax <= c["bar_abs"], (gap, dmax)


def test_base_shape_full_depth(hip):
    """ModernBERT-base (22 layers, hidden 768, intermediate 1152, vocab 50368), seeded weights at the project's std 0.02, a ragged
    batch of rows up to 512 tokens against float32 ModernBertModel on the CPU; the decoder's full-shape bar."""
    from tests.modernbert_ref import hf_model, reference_embed
    shape = MODERNBERT_SHAPES["nomic-ai/modernbert-embed-base"]
    m, w = _model(shape, 5, std=0.02)
    lens = np.array([512, 301, 130, 64, 7], np.int32)
    rng = np.random.RandomState(5)
    ids = np.zeros((len(lens), 512), np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.randint(3, shape[0], size=n)
    got = m.forward(ids, lens, pooling="mean").cpu().numpy()
    m.close()
    want = reference_embed(hf_model(shape, w), ids, lens, "mean")
    gap, _ = _report(got, want, "ModernBERT-base, 22 layers")
    assert gap <= FULL_SHAPE_COS_TOL, gap


def test_large_width_two_layer_cut(hip):
    """Hidden 1024 / intermediate 2624 (2 I = 5248 is no multiple of 256: Wi is padded to 5376 rows and mlp.Wo to 2688 columns at
    create), 16 heads, one global and one sliding layer."""
    from tests.modernbert_ref import PROJECT_BAR_ABS, PROJECT_BAR_COS, hf_model, reference_embed
    shape = MODERNBERT_SHAPES["modernbert-large-cut2"]
    m, w = _model(shape, 6, std=0.02)
    lens = np.array([300, 257, 130, 33], np.int32)
    rng = np.random.RandomState(6)
    ids = np.zeros((len(lens), 300), np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.randint(3, shape[0], size=n)
    for pooling in ("mean", "cls"):
        got = m.forward(ids, lens, pooling=pooling).cpu().numpy()
        want = reference_embed(hf_model(shape, w), ids, lens, pooling)
        gap, dmax = _report(got, want, f"large width, 2 layers, {pooling}")
        assert gap <= PROJECT_BAR_COS and dmax <= PROJECT_BAR_ABS, (gap, dmax)
    m.close()


def test_large_batch_on_the_wide_gemm_tiles(hip):
    """64 x 512 tokens at the large width: every GEMM of the layer -- MODE 0, MODE 2 and the GeGLU MODE 8 over the padded Wi -- runs on
    the 256 x 256 phased tile (>= 256 tiles); sampled rows against float32 ModernBertModel, the rest finite and unit length."""
    from tests.modernbert_ref import PROJECT_BAR_ABS, PROJECT_BAR_COS, hf_model, reference_embed
    shape = MODERNBERT_SHAPES["modernbert-large-cut2"]
    m, w = _model(shape, 7, std=0.02)
    B, S = 64, 512
    ids = np.random.RandomState(7).randint(3, shape[0], size=(B, S)).astype(np.int32)
    lens = np.full(B, S, np.int32)
    lens[1], lens[B - 1] = 333, 130
    got = m.forward(ids, lens, pooling="mean").cpu().numpy()
    m.close()
    assert np.isfinite(got).all() and np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 1e-5
    rows = [0, 1, 31, B - 1]
    want = reference_embed(hf_model(shape, w), ids[rows], lens[rows], "mean")
    gap, dmax = _report(got[rows], want, "large width, 64 x 512 on the wide tiles")
    assert gap <= PROJECT_BAR_COS and dmax <= PROJECT_BAR_ABS, (gap, dmax)


def test_invariances(hip):
    c = _load("mix_mean")
    m, _ = _model(c["shape_name"], c["seed"], c["std"])
    ids, lens = c["ids"], c["lens"]
    S = (ids.shape[1] + 31) // 32 * 32
    a = m.forward(ids, lens, S=S).cpu().numpy()
    assert np.array_equal(a, m.forward(ids, lens, S=S).cpu().numpy())                        # two runs
    junk = ids.copy()
    for i, n in enumerate(lens):
        junk[i, n:] = 777                                                                     # ids behind a row's length
    assert np.array_equal(a, m.forward(junk, lens, S=S).cpu().numpy())
    for i in range(len(lens)):                                                                # a row alone at the same S
        assert np.array_equal(a[i:i + 1], m.forward(ids[i:i + 1], lens[i:i + 1], S=S).cpu().numpy()), i
    unnorm = m.forward(ids, lens, normalise=False).cpu().numpy()
    assert np.allclose(unnorm / np.linalg.norm(unnorm, axis=1, keepdims=True), a, atol=1e-6)
    assert np.array_equal(m.forward(ids[:2], [0, 5], S=S).cpu().numpy()[0], np.zeros(a.shape[1], np.float32))   # an empty row
    m.close()


def test_short_rows_local_equals_global_given_one_theta(hip):
    """Rows of at most 65 tokens: every key is inside the window (|q - k| <= 64), so a local-only model equals the global-only
    model holding the same weights when both thetas are equal."""
    from archi_amd.modernbert import HipModernBert
    base = MODERNBERT_SHAPES["modernbert-tiny-local"]
    w = random_modernbert_weights(base, seed=21, std=0.1)
    loc = HipModernBert(base[:7] + (10000.0, 10000.0) + base[9:], w, device=0)
    glo = HipModernBert(base[:7] + (10000.0, 10000.0, base[9], (1, 1, 1)) + base[11:], w, device=0)
    lens = np.array([65, 64, 33, 1], np.int32)
    rng = np.random.RandomState(21)
    ids = rng.randint(3, base[0], size=(4, 65)).astype(np.int32)
    a, b = loc.forward(ids, lens).cpu().numpy(), glo.forward(ids, lens).cpu().numpy()
    assert np.array_equal(a, b)
    lens2 = np.array([67, 64], np.int32)                                                      # ... and past 65 tokens the window shows
    ids2 = rng.randint(3, base[0], size=(2, 67)).astype(np.int32)
    a2, b2 = loc.forward(ids2, lens2).cpu().numpy(), glo.forward(ids2, lens2).cpu().numpy()
    assert not np.array_equal(a2[0], b2[0]) and np.array_equal(a2[1], b2[1])
    loc.close(); glo.close()


def test_refusals_through_the_abi(hip):
    import torch
    from archi_amd import _lib
    from archi_amd._lib import MBERT_MAX_LAYERS, AkModernBertConfig
    from archi_amd.modernbert import HipModernBert
    lib = _lib.load()
    m, _ = _model("modernbert-tiny-global", 3)
    out = torch.empty((1, 128), dtype=torch.float32, device="cuda")
    for S, what in ((48, "multiple of 32"), (8224, "multiple of 32"), (0, "multiple of 32")):
        stage = torch.zeros((1, max(S, 1) + 1), dtype=torch.int32, device="cuda")
        rc = lib.ak_mbert_forward_lens(m._h, stage.data_ptr(), S + 1, stage.data_ptr() + 4 * S, S + 1, 1, S, 0, 1, out.data_ptr(), None)
        assert rc != 0 and what in _lib.last_error(), (S, rc, _lib.last_error())
    stage = torch.zeros((1, 33), dtype=torch.int32, device="cuda")
    assert lib.ak_mbert_forward_lens(m._h, stage.data_ptr(), 33, stage.data_ptr() + 128, 33, 1, 32, 7, 1, out.data_ptr(), None) != 0
    assert "pooling" in _lib.last_error()
    types = (ctypes.c_int * MBERT_MAX_LAYERS)(1, 1)
    arr = (ctypes.c_void_p * len(m._ptrs))(*m._ptrs)

    def create(cfg, n):
        h = ctypes.c_void_p()
        rc = lib.ak_mbert_create(ctypes.byref(cfg), arr, n, ctypes.byref(h))
        assert rc != 0 and not h.value, rc
        return _lib.last_error()

    ok = dict(vocab_size=1000, hidden=128, layers=2, heads=2, intermediate=192, max_position=8192, norm_eps=1e-5,
              global_rope_theta=160000.0, local_rope_theta=10000.0, half_window=64, layer_global=types)
    n = len(m._ptrs)
    assert "head size" in create(AkModernBertConfig(**dict(ok, heads=4)), n)                  # head size 32
    assert "weight pointers" in create(AkModernBertConfig(**ok), n - 1)
    assert "half_window" in create(AkModernBertConfig(**dict(ok, half_window=0)), n)
    assert "multiple of 64" in create(AkModernBertConfig(**dict(ok, intermediate=200)), n)
    assert "multiple of 128" in create(AkModernBertConfig(**dict(ok, hidden=192, heads=3)), n)
    with pytest.raises(ValueError, match="multiple of 32"):
        m.forward_lens(torch.zeros((1, 49), dtype=torch.int32, device="cuda"), 1, 48, out)
    m.close()


def test_text_end_to_end(hip, tmp_path):
    """Checkpoint directory (save_pretrained + BPE tokenizer.json + sentence-transformers files, mean pooling + Normalize) ->
    ArchiHipEmbeddings -> ArchiHipVectorStore, against the same directory through transformers' fast tokenizer + float32
    ModernBertModel on the CPU: the embeddings at the bf16 bar, the CPU top-k ids wherever the CPU scores are separated by > 1e-3."""
    from archi_amd.embeddings import ArchiHipEmbeddings
    from archi_amd.vectorstore import ArchiHipVectorStore
    from tests.modernbert_ref import CORPUS, PROJECT_BAR_ABS, PROJECT_BAR_COS, TEXTS, hf_tokenizer, reference_embed, write_checkpoint
    d = str(tmp_path / "modernbert")
    model = write_checkpoint(d, "modernbert-tiny-256", seed=4, std=0.05, pooling="mean", max_seq_length=128)
    emb = ArchiHipEmbeddings(d)
    assert emb.dimensions == 256 and emb.pooling == "mean" and emb.normalize and emb.max_seq_length == 128
    rng = np.random.default_rng(9)
    words = " ".join(CORPUS).split()
    docs = list(TEXTS) + [" ".join(rng.choice(words, rng.integers(3, 90))) for _ in range(40)]
    got = np.asarray(emb.embed_documents(docs), np.float32)
    tok = hf_tokenizer(os.path.join(d, "tokenizer.json"))

    def cpu(texts):
        toks = tok([x.replace("\n", " ") for x in texts], truncation=True, max_length=128)["input_ids"]
        ids = np.zeros((len(toks), 128), np.int32)
        for i, t in enumerate(toks):
            ids[i, :len(t)] = t
        return reference_embed(model, ids, [len(t) for t in toks], "mean")

    want = cpu(docs)
    gap, dmax = _report(got, want, "documents")
    assert gap <= PROJECT_BAR_COS and dmax <= PROJECT_BAR_ABS, (gap, dmax)
    query = "search_query: which trigger of the muon detector failed? σ µs"
    q_want = cpu([query])[0]
    store = ArchiHipVectorStore(None, emb, collection_name="modernbert_e2e", distance_metric="cosine")
    store.add_texts(docs, metadatas=[{"i": i} for i in range(len(docs))])
    k = 10
    res = store.similarity_search_with_score(query, k=k)
    got_ids = [int(doc.metadata["i"]) for doc, _ in res]
    cpu_scores = 1 - want @ q_want
    order = np.argsort(cpu_scores, kind="stable")
    checked = 0
    for rank in range(k):
        sep_prev = rank == 0 or cpu_scores[order[rank]] - cpu_scores[order[rank - 1]] > 1e-3
        sep_next = cpu_scores[order[rank + 1]] - cpu_scores[order[rank]] > 1e-3
        if sep_prev and sep_next:
            checked += 1
            assert got_ids[rank] == int(order[rank]), (got_ids, order[:k], cpu_scores[order[:k + 1]])
    assert checked >= 3, checked
    emb.encoder.close()
