"""GPU tests of the T5 path (ak_t5_*: csrc/t5.hip, the biased k_attn_long_relbias of attn_long.hip, k_gemm MODE 10 / MODE 9): the
fixtures of tests/golden/make_t5_fixtures.py (float32 transformers.T5EncoderModel on the CPU) at the bar stored in each fixture, the
invariances the other families have, the entry points' refusals, and text end to end through ArchiHipEmbeddings and
ArchiHipVectorStore.

The bar of a fixture is, per figure, the larger of the project's bf16 encoder bar (1 - cos 3e-4, max |d| 3e-3) and the error of
T5EncoderModel itself run all in bf16 on the CPU against its float32 self on the same rows; no margin on top.
Measured on MI355X (worst row of each fixture, 1 - cos / max |d|): see DESIGN.md section 9."""
import ctypes

import numpy as np
import pytest

from archi_amd.t5 import T5_SHAPES, random_t5_weights
from tests.golden import make_t5_fixtures as fx

pytestmark = pytest.mark.gpu
FIX = sorted(fx.CASES)


def _model(shape, seed, std=0.05, bias_std=2.0):
    from archi_amd.t5 import HipT5
    w = random_t5_weights(shape, seed=seed, std=std, bias_std=bias_std)
    return HipT5(shape, w, device=0), w


def _report(got, want, what):
    from tests.t5_ref import cos_gap
    gap, dmax = float(cos_gap(got, want).max()), float(np.abs(got - want).max())
    print(f"{what}: 1 - cos max {gap:.3e}, max |d| {dmax:.3e}")
    return gap, dmax


@pytest.mark.parametrize("name", FIX)
def test_model_matches_fixture(hip, name):
    c = fx.load(name)
    m, _ = _model(c["shape_name"], c["seed"], c["std"], c["bias_std"])
    got = m.forward(c["ids"], c["lens"], pooling=c["pooling"]).cpu().numpy()
    m.close()
    gap, dmax = _report(got, c["expected"], f"{name} worst / bar: (bar {c['bar_cos']:.3e} / {c['bar_abs']:.3e})")
    assert gap <= c["bar_cos"] and dmax <= c["bar_abs"], (gap, dmax)


@pytest.mark.parametrize("name", FIX)
def test_provider_matches_fixture(hip, name):
    """The same rows through ArchiHipEmbeddings.embed_token_arrays: length-sorted tiles, one S per tile."""
    from archi_amd.embeddings import ArchiHipEmbeddings
    c = fx.load(name)
    emb = ArchiHipEmbeddings(c["shape_name"], model_kwargs={"synthetic_seed": c["seed"], "synthetic_std": c["std"], "synthetic_bias_std": c["bias_std"]},
                             encode_kwargs={"batch_tokens": 1024 if name != "base_cut2" else 16384})
    assert emb.pooling == c["pooling"] and emb.normalize and emb.dimensions == c["expected"].shape[1] and emb.max_seq_length == 8192
    got = emb.embed_token_arrays(c["ids"], c["lens"])
    emb.encoder.close()
    gap, dmax = _report(got, c["expected"], f"{name} through the provider (bar {c['bar_cos']:.3e} / {c['bar_abs']:.3e})")
    assert gap <= c["bar_cos"] and dmax <= c["bar_abs"], (gap, dmax)


def test_invariances(hip):
    from tests.t5_ref import cos_gap
    c = fx.load("tiny_gated")
    m, _ = _model(c["shape_name"], c["seed"], c["std"], c["bias_std"])
    ids, lens = c["ids"], c["lens"]
    S = (ids.shape[1] + 31) // 32 * 32
    a = m.forward(ids, lens, S=S).cpu().numpy()
    assert np.array_equal(a, m.forward(ids, lens, S=S).cpu().numpy())                        # two runs
    junk = ids.copy()
    for i, n in enumerate(lens):
        junk[i, n:] = 777                                                                     # ids behind a row's length
    assert np.array_equal(a, m.forward(junk, lens, S=S).cpu().numpy())
    i = list(lens).index(129)                                                                 # the row of 129 tokens alone
    alone = m.forward(ids[i:i + 1, :129], lens[i:i + 1]).cpu().numpy()
    gap = float(cos_gap(alone, a[i:i + 1]).max())
    print(f"row of 129 tokens alone (S = 160) against itself in the batch (S = {S}): 1 - cos {gap:.3e}")
    assert gap <= 1e-5
    unnorm = m.forward(ids, lens, normalise=False).cpu().numpy()
    assert np.allclose(unnorm / np.linalg.norm(unnorm, axis=1, keepdims=True), a, atol=1e-6)
    assert np.array_equal(m.forward(ids[:2], [0, 5], S=S).cpu().numpy()[0], np.zeros(a.shape[1], np.float32))   # an empty row
    cls = m.forward(ids, lens, pooling="cls", S=S).cpu().numpy()
    assert not np.allclose(cls[0], a[0], atol=1e-3) and np.abs(np.linalg.norm(cls, axis=1) - 1).max() <= 1e-5
    m.close()


def test_refusals_through_the_abi(hip):
    import torch
    from archi_amd import _lib
    from archi_amd._lib import AkT5Config
    lib = _lib.load()
    m, _ = _model("t5-tiny-relu", 3)
    out = torch.empty((1, 128), dtype=torch.float32, device="cuda")
    for S, what in ((48, "multiple of 32"), (8224, "multiple of 32"), (0, "multiple of 32")):
        stage = torch.zeros((1, max(S, 1) + 1), dtype=torch.int32, device="cuda")
        rc = lib.ak_t5_forward_lens(m._h, stage.data_ptr(), S + 1, stage.data_ptr() + 4 * S, S + 1, 1, S, 0, 1, out.data_ptr(), None)
        assert rc != 0 and what in _lib.last_error(), (S, rc, _lib.last_error())
    stage = torch.zeros((1, 33), dtype=torch.int32, device="cuda")
    assert lib.ak_t5_forward_lens(m._h, stage.data_ptr(), 33, stage.data_ptr() + 128, 33, 1, 32, 7, 1, out.data_ptr(), None) != 0
    assert "pooling" in _lib.last_error()
    arr = (ctypes.c_void_p * len(m._ptrs))(*m._ptrs)

    def create(n, **change):
        ok = dict(vocab_size=1000, hidden=128, layers=2, heads=2, head_dim=64, d_ff=192, gated=0, max_distance=128, ln_eps=1e-6, n_dense=0)
        ok.update(change)
        h = ctypes.c_void_p()
        rc = lib.ak_t5_create(ctypes.byref(AkT5Config(**ok)), arr, n, ctypes.byref(h))
        assert rc != 0 and not h.value, rc
        return _lib.last_error()

    n = len(m._ptrs)
    assert n == 3 + 8 * 2
    assert "head_dim" in create(n, head_dim=32, heads=4)                                      # head size 32
    assert "heads * 64" in create(n, heads=4)
    assert "multiple of 128" in create(n, hidden=192, heads=3)
    assert "<= 1024" in create(n, hidden=1152, heads=18)
    assert "d_ff" in create(n, d_ff=200)
    assert "max_distance" in create(n, max_distance=0)
    assert "ln_eps" in create(n, ln_eps=0.0)
    assert "weight pointers" in create(n - 1)
    assert "weight pointers" in create(n, gated=1)                                            # the gated layer holds one matrix more
    assert "AK_MBERT_MAX_LAYERS" in create(n, layers=65)
    assert "n_dense" in create(n, n_dense=3)
    with pytest.raises(ValueError, match="multiple of 32"):
        m.forward_lens(torch.zeros((1, 49), dtype=torch.int32, device="cuda"), 1, 48, out)
    with pytest.raises(ValueError, match="pooling"):
        m.forward(np.zeros((1, 4), np.int32), [4], pooling="last")
    m.close()


def test_text_end_to_end(hip, tmp_path):
    """Checkpoint directory (T5EncoderModel safetensors, a small Unigram tokenizer.json whose post-processor appends </s>, 1_Pooling,
    2_Dense, Normalize) -> ArchiHipEmbeddings (BpeTokenizer) -> ArchiHipVectorStore, against the same directory through tokenizers +
    float32 T5EncoderModel + pooling + Dense + normalise on the CPU: the embeddings at the bf16 bar, the CPU top-k ids wherever the CPU
    scores are separated by > 1e-3 (the decoder suite's rule), embed_query equal to the matching embed_documents row."""
    from archi_amd.decoder import BpeTokenizer
    from archi_amd.embeddings import ArchiHipEmbeddings
    from archi_amd.vectorstore import ArchiHipVectorStore
    from tests import t5_ref as tr
    from tests.decoder_ref import CORPUS
    shape = T5_SHAPES["t5-tiny-gated"][:12] + ((96,),)
    w = random_t5_weights(shape, seed=4, std=0.05, bias_std=2.0)
    d = tr.write_checkpoint(str(tmp_path / "t5"), shape, w, pooling="mean", max_seq_length=128, corpus=CORPUS)
    model, dense = tr.hf_model(shape, w), tr.dense_tail(w)
    emb = ArchiHipEmbeddings(d)
    assert emb.dimensions == 96 and emb.pooling == "mean" and emb.normalize and emb.max_seq_length == 128
    assert isinstance(emb.tokenizer, BpeTokenizer)
    rng = np.random.default_rng(9)
    words = " ".join(CORPUS).split()
    docs = list(CORPUS) + ["run " * 40, "", "tier-2 tier-2 storage"] + [" ".join(rng.choice(words, rng.integers(3, 90))) for _ in range(40)]
    got = np.asarray(emb.embed_documents(docs), np.float32)
    tok = tr.hf_tokenizer(d)

    def cpu(texts):
        toks = tok([x.replace("\n", " ") for x in texts], truncation=True, max_length=128)["input_ids"]
        assert all(t[-1] == 1 for t in toks)                                                  # </s> closes every row
        ids = np.zeros((len(toks), 128), np.int32)
        for i, t in enumerate(toks):
            ids[i, :len(t)] = t
        return tr.reference(model, ids, [len(t) for t in toks], "mean", dense)

    want = cpu(docs)
    gap, dmax = _report(got, want, "documents")
    assert gap <= tr.PROJECT_BAR_COS and dmax <= tr.PROJECT_BAR_ABS, (gap, dmax)
    query = "what is the σ of the beam spot in the muon chambers?"
    assert np.array_equal(np.asarray(emb.embed_query(docs[3]), np.float32), got[3])
    q_want = cpu([query])[0]
    store = ArchiHipVectorStore(None, emb, collection_name="t5_e2e", distance_metric="cosine")
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
