"""GPU tests of the EmbeddingGemma path (ak_gemma_*: csrc/gemma.hip, the head-256 grouped-query k_attn_gqa of attn_gqa.hip, k_gemm
MODE 9): the fixtures of tests/golden/make_gemma_fixtures.py (float32 transformers.Gemma3TextModel on the CPU, bidirectional) at the
bar stored in each fixture, the base shape at full depth and on the wide GEMM tiles, the invariances the other families have, the Dense
head present and absent, the entry points' refusals, and text end to end through ArchiHipEmbeddings and ArchiHipVectorStore.

The bar of a fixture is, per figure, the larger of the project's bf16 encoder bar (1 - cos 3e-4, max |d| 3e-3) and the error of
Gemma3TextModel itself run all in bf16 on the CPU against its float32 self on the same rows; no margin on top.
Measured on MI355X (worst row of each fixture, 1 - cos / max |d|): see DESIGN.md section 9."""
import ctypes
import glob
import os

import numpy as np
import pytest

from archi_amd.gemma import GEMMA_SHAPES, random_gemma_weights

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIX = sorted(os.path.basename(p)[len("gemma_"):-4] for p in glob.glob(os.path.join(GOLDEN, "gemma_*.npz")))
FULL_SHAPE_COS_TOL = 1e-3          # the family bar at full depth (tests/test_decoder_gpu.py, tests/test_modernbert_gpu.py)


def _load(name):
    from tests.golden.make_gemma_fixtures import load
    return load(name)


def _model(shape, seed, std=0.1, dense=True):
    from archi_amd.gemma import HipGemma
    w = random_gemma_weights(shape, seed=seed, std=std)
    return HipGemma(shape, w, device=0, dense=dense), w


def _report(got, want, what):
    from tests.gemma_ref import cos_gap
    gap, dmax = float(cos_gap(got, want).max()), float(np.abs(got - want).max())
    print(f"{what}: 1 - cos max {gap:.3e}, max |d| {dmax:.3e}")
    return gap, dmax


def _ids(shape, seed, lens, width):
    rng = np.random.RandomState(seed)
    ids = np.zeros((len(lens), width), np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.randint(3, shape[0], size=n)
    return ids


def test_fixtures_present():
    assert set(FIX) >= {"tiny", "g2", "global", "local"}, FIX
    lens = set(_load("tiny")["lens"].tolist())
    assert lens == {1, 32, 33, 34, 65, 66, 97, 130, 300, 513, 1024, 2048}
    types = {GEMMA_SHAPES[_load(n)["shape_name"]][13] for n in FIX}
    assert any(set(t) == {1} for t in types) and any(set(t) == {0} for t in types) and any(set(t) == {0, 1} for t in types)
    assert {len(GEMMA_SHAPES[_load(n)["shape_name"]][14]) for n in FIX} == {0, 1, 2}          # no, one and two Dense modules


@pytest.mark.parametrize("name", FIX)
def test_model_matches_fixture(hip, name):
    c = _load(name)
    m, _ = _model(c["shape_name"], c["seed"], c["std"])
    got = m.forward(c["ids"], c["lens"]).cpu().numpy()
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
    assert emb.pooling == "mean" and emb.normalize and emb.dimensions == c["expected"].shape[1] and emb.max_seq_length == 2048
    got = emb.embed_token_arrays(c["ids"], c["lens"])
    emb.encoder.close()
    gap, dmax = _report(got, c["expected"], f"{name} through the provider")
    assert gap <= c["bar_cos"] and dmax <= c["bar_abs"], (gap, dmax)


def test_base_shape_full_depth(hip):
    """EmbeddingGemma-300m's stack at full depth (24 layers, 5 sliding : 1 full, hidden 768, intermediate 1152, 3 query heads on 1 kv
    head, window 512, the two Dense modules), seeded weights at the project's std 0.02, a ragged batch of rows up to 512 tokens against
    float32 Gemma3TextModel on the CPU at the family bar. Every dimension is the released model's but the vocabulary (2000 rows, not
    262144: the table's height changes no kernel's path, and 200 M random numbers would make this the slowest test of the suite)."""
    from tests.gemma_ref import dense_matrices, hf_model, reference_embed
    shape = GEMMA_SHAPES["gm-base-24"]
    assert shape[1:] == GEMMA_SHAPES["google/embeddinggemma-300m"][1:]
    m, w = _model(shape, 5, std=0.02)
    lens = np.array([512, 301, 130, 64, 7], np.int32)
    ids = _ids(shape, 5, lens, 512)
    got = m.forward(ids, lens).cpu().numpy()
    m.close()
    want = reference_embed(hf_model(shape, w), ids, lens, dense_matrices(shape, w))
    gap, _ = _report(got, want, "EmbeddingGemma stack, 24 layers")
    assert gap <= FULL_SHAPE_COS_TOL, gap


def test_base_width_on_the_wide_gemm_tiles(hip):
    """8 x 512 tokens at the base width, one sliding and one full layer: wherever the launcher's rule picks the wide tile it runs (QKV
    N = 1280, gate / up N = 2304); sampled rows against float32 Gemma3TextModel, the rest finite and of unit length."""
    from tests.gemma_ref import PROJECT_BAR_ABS, PROJECT_BAR_COS, dense_matrices, hf_model, reference_embed
    shape = GEMMA_SHAPES["gm-base-cut2"]
    m, w = _model(shape, 7, std=0.02)
    B, S = 8, 512
    ids = np.random.RandomState(7).randint(3, shape[0], size=(B, S)).astype(np.int32)
    lens = np.full(B, S, np.int32)
    lens[1], lens[B - 1] = 333, 130
    got = m.forward(ids, lens).cpu().numpy()
    m.close()
    assert np.isfinite(got).all() and np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 1e-5
    rows = [0, 1, B - 1]
    want = reference_embed(hf_model(shape, w), ids[rows], lens[rows], dense_matrices(shape, w))
    gap, dmax = _report(got[rows], want, "base width, 8 x 512")
    assert gap <= PROJECT_BAR_COS and dmax <= PROJECT_BAR_ABS, (gap, dmax)


def test_invariances(hip):
    """Two runs and junk behind a row's length: bit for bit. A row alone against the row in a ragged batch, at the batch's S and at its
    own: within the fixture's bar of each other (in fact bit for bit at the same S; at another S the pad blocks are skipped alike)."""
    from tests.gemma_ref import cos_gap
    c = _load("tiny")
    m, _ = _model(c["shape_name"], c["seed"], c["std"])
    keep = np.flatnonzero(c["lens"] <= 513)
    ids, lens = c["ids"][keep, :544], c["lens"][keep]
    S = 544
    a = m.forward(ids, lens, S=S).cpu().numpy()
    assert np.array_equal(a, m.forward(ids, lens, S=S).cpu().numpy())                        # two runs
    junk = ids.copy()
    for i, n in enumerate(lens):
        junk[i, n:] = 777                                                                     # ids behind a row's length
    assert np.array_equal(a, m.forward(junk, lens, S=S).cpu().numpy())
    for i in range(len(lens)):
        alone = m.forward(ids[i:i + 1], lens[i:i + 1], S=S).cpu().numpy()                     # a row alone at the same S
        own = m.forward(ids[i:i + 1, :lens[i]], lens[i:i + 1]).cpu().numpy()                  # ... and at its own S
        for other in (alone, own):
            assert float(cos_gap(other, a[i:i + 1]).max()) <= c["bar_cos"] and float(np.abs(other - a[i]).max()) <= c["bar_abs"], i
    unnorm = m.forward(ids, lens, normalise=False).cpu().numpy()
    assert np.allclose(unnorm / np.linalg.norm(unnorm, axis=1, keepdims=True), a, atol=1e-6)
    assert np.array_equal(m.forward(ids[:2], [0, 5], S=S).cpu().numpy()[0], np.zeros(a.shape[1], np.float32))   # an empty row
    m.close()


def test_without_the_dense_head(hip):
    """The plain Gemma3 text model (no Dense module), mean pooled, against the reference without the head; and with the head the same
    rows are the reference's with it (the fixture test) -- the two differ."""
    from tests.gemma_ref import hf_model, reference_embed
    c = _load("tiny")
    m, w = _model(c["shape_name"], c["seed"], c["std"], dense=False)
    keep = np.flatnonzero(c["lens"] <= 300)
    ids, lens = c["ids"][keep, :320], c["lens"][keep]
    got = m.forward(ids, lens).cpu().numpy()
    m.close()
    assert got.shape[1] == GEMMA_SHAPES[c["shape_name"]][1]
    want = reference_embed(hf_model(c["shape_name"], w), ids, lens, ())
    gap, dmax = _report(got, want, "tiny without the Dense head")
    assert gap <= c["bar_cos"] and dmax <= c["bar_abs"], (gap, dmax)
    assert float(np.abs(got - c["expected"][keep]).max()) > 10 * c["bar_abs"]


def test_refusals_before_any_gpu_work(hip):
    import torch
    from archi_amd import _lib
    from archi_amd._lib import GEMMA_MAX_LAYERS, AkGemmaConfig
    from archi_amd.embeddings import ArchiHipEmbeddings
    for precision in ("f32", "bf16x3"):
        with pytest.raises(ValueError, match="bf16 only"):
            ArchiHipEmbeddings("gm-tiny", model_kwargs={"synthetic_seed": 1, "precision": precision})
    lib = _lib.load()
    m, _ = _model("gm-global", 3)
    D = m.out_dim
    out = torch.empty((1, D), dtype=torch.float32, device="cuda")
    for S, what in ((48, "multiple of 32"), (2080, "multiple of 32"), (0, "multiple of 32")):
        stage = torch.zeros((1, max(S, 1) + 1), dtype=torch.int32, device="cuda")
        rc = lib.ak_gemma_forward_lens(m._h, stage.data_ptr(), S + 1, stage.data_ptr() + 4 * S, S + 1, 1, S, 0, 1, out.data_ptr(), None)
        assert rc != 0 and what in _lib.last_error(), (S, rc, _lib.last_error())
    stage = torch.zeros((1, 33), dtype=torch.int32, device="cuda")
    assert lib.ak_gemma_forward_lens(m._h, stage.data_ptr(), 33, stage.data_ptr() + 128, 33, 1, 32, 1, 1, out.data_ptr(), None) != 0
    assert "pooling" in _lib.last_error()                                                     # cls pooling
    types = (ctypes.c_int * GEMMA_MAX_LAYERS)(1, 1)
    arr = (ctypes.c_void_p * len(m._ptrs))(*m._ptrs)

    def create(n=len(m._ptrs), **change):
        ok = dict(vocab_size=1000, hidden=384, layers=2, q_heads=3, kv_heads=1, head_dim=256, intermediate=384, max_position=2048, rms_eps=1e-6,
                  global_rope_theta=1e6, local_rope_theta=1e4, query_pre_attn_scalar=128.0, half_window=32, attn_softcap=0.0, final_softcap=0.0,
                  rope_type=0, activation=0, attention_bias=0, n_dense=1, dense_out=(ctypes.c_int * 2)(384, 0), layer_global=types)
        ok.update(change)
        h = ctypes.c_void_p()
        rc = lib.ak_gemma_create(ctypes.byref(AkGemmaConfig(**ok)), arr, n, ctypes.byref(h))
        assert rc != 0 and not h.value, (change, rc)
        return _lib.last_error()

    assert "head_dim" in create(head_dim=128)
    assert "kv_heads" in create(q_heads=3, kv_heads=2)
    assert "group" in create(q_heads=5, kv_heads=1)
    assert "hidden" in create(hidden=192)
    assert "hidden" in create(hidden=1152)
    assert "intermediate" in create(intermediate=200)
    assert "softcap" in create(attn_softcap=50.0)
    assert "softcap" in create(final_softcap=30.0)
    assert "rope_type" in create(rope_type=1)
    assert "activation" in create(activation=1)
    assert "attention_bias" in create(attention_bias=1)
    assert "half_window" in create(half_window=0)
    assert "layers" in create(layers=65)
    assert "weight pointers" in create(n=len(m._ptrs) - 1)
    with pytest.raises(ValueError, match="multiple of 32"):
        m.forward_lens(torch.zeros((1, 49), dtype=torch.int32, device="cuda"), 1, 48, out)
    with pytest.raises(ValueError, match="pool"):
        m.forward_lens(torch.zeros((1, 33), dtype=torch.int32, device="cuda"), 1, 32, out, pooling="cls")
    assert lib.ak_gemma_set_rope_inv_freq(m._h, None, m._inv_freq[1].ctypes.data) != 0 and "NULL" in _lib.last_error()
    m.close()


def test_rope_tables_from_hf_frequencies_or_from_the_thetas(hip):
    """The handle replaces ak_gemma_create's tables (from the thetas) by the tables of HF's own inverse frequencies, which differ in one
    frequency of 128 by 1 ulp: setting the same frequencies again changes nothing, bit for bit; setting the host routine's correctly
    rounded ones moves a long row by far less than the bar (the choice is about parity of the table, not about what a test can see)."""
    from tests.gemma_ref import cos_gap
    c = _load("tiny")
    m, _ = _model(c["shape_name"], c["seed"], c["std"])
    keep = np.flatnonzero(c["lens"] == 1024)
    ids, lens = c["ids"][keep, :1024], c["lens"][keep]
    a = m.forward(ids, lens).cpu().numpy()
    hip.ak_gemma_set_rope_inv_freq(m._h, m._inv_freq[0].ctypes.data, m._inv_freq[1].ctypes.data)
    assert np.array_equal(a, m.forward(ids, lens).cpu().numpy())
    e = np.arange(0, 256, 2, dtype=np.float32) / np.float32(256)
    host = [(np.float32(1) / np.power(np.float64(t), e.astype(np.float64)).astype(np.float32)).astype(np.float32) for t in (1e6, 1e4)]
    assert all((h != f).sum() == 1 for h, f in zip(host, m._inv_freq))
    assert hip.ak_gemma_set_rope_inv_freq(m._h, host[0].ctypes.data, host[1].ctypes.data) == 0
    b = m.forward(ids, lens).cpu().numpy()
    m.close()
    gap = float(cos_gap(a, b).max())
    print(f"tables from the thetas against tables from HF's frequencies, 1024-token row: 1 - cos {gap:.3e}, max |d| {np.abs(a - b).max():.3e}")
    assert gap <= 0.1 * c["bar_cos"]


def test_text_end_to_end(hip, tmp_path):
    """Checkpoint directory (config.json model_type gemma3_text, safetensors, BPE tokenizer.json adding <bos> / <eos>, the
    sentence-transformers files with 2_Dense / 3_Dense and Normalize) -> ArchiHipEmbeddings -> ArchiHipVectorStore, against the same
    directory through transformers' fast tokenizer + float32 Gemma3TextModel on the CPU: the embeddings at the bf16 bar, the CPU top-k
    ids wherever the CPU scores are separated by > 1e-3."""
    from archi_amd.embeddings import ArchiHipEmbeddings
    from archi_amd.vectorstore import ArchiHipVectorStore
    from tests.gemma_ref import CORPUS, PROJECT_BAR_ABS, PROJECT_BAR_COS, TEXTS, hf_tokenizer, reference_embed, write_checkpoint
    d = str(tmp_path / "embeddinggemma")
    model, dense = write_checkpoint(d, "gm-tiny", seed=4, std=0.05, max_seq_length=128)
    emb = ArchiHipEmbeddings(d)
    assert emb.dimensions == 384 and emb.pooling == "mean" and emb.normalize and emb.max_seq_length == 128
    rng = np.random.default_rng(9)
    words = " ".join(CORPUS).split()
    docs = list(TEXTS) + [" ".join(rng.choice(words, rng.integers(3, 90))) for _ in range(40)]
    got = np.asarray(emb.embed_documents(docs), np.float32)
    tok = hf_tokenizer(os.path.join(d, "tokenizer.json"))

    def cpu(texts):
        toks = tok([x.replace("\n", " ") for x in texts], truncation=True, max_length=128)["input_ids"]
        assert all(t[0] == 2 and t[-1] == 1 for t in toks)                                    # <bos> ... <eos>
        ids = np.zeros((len(toks), 128), np.int32)
        for i, t in enumerate(toks):
            ids[i, :len(t)] = t
        return reference_embed(model, ids, [len(t) for t in toks], dense)

    want = cpu(docs)
    gap, dmax = _report(got, want, "documents")
    assert gap <= PROJECT_BAR_COS and dmax <= PROJECT_BAR_ABS, (gap, dmax)
    query = "task: search result | query: which trigger of the muon detector failed? σ µs"
    q_want = cpu([query])[0]
    store = ArchiHipVectorStore(None, emb, collection_name="gemma_e2e", distance_metric="cosine")
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
