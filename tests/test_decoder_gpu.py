"""GPU tests of the HIP Qwen3 decoder (archi_amd.decoder.HipDecoder, ak_decoder_*): the fixtures of
tests/golden/make_decoder_fixtures.py (float32 transformers.Qwen3Model on the CPU) at the BERT suite's bf16 bar, the full
Qwen3-Embedding-0.6B shape against the same reference, padding / determinism / batching invariances, and text end to end through
ArchiHipEmbeddings and ArchiHipVectorStore."""
import glob
import os

import numpy as np
import pytest

from archi_amd.decoder import QWEN3_SHAPES, random_qwen3_weights

pytestmark = pytest.mark.gpu
FIX = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "decoder_*.npz")))
COS_TOL, ABS_TOL = 1e-4, 2e-3

_WEIGHTS = {}


def _weights(shape, seed):
    if (shape, seed) not in _WEIGHTS:
        _WEIGHTS[(shape, seed)] = random_qwen3_weights(shape, seed=seed)
    return _WEIGHTS[(shape, seed)]


def _decoder(shape, seed):
    from archi_amd.decoder import HipDecoder
    return HipDecoder(QWEN3_SHAPES[shape], _weights(shape, seed), device=0)


def _cos(got, want):
    return (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))


def test_fixtures_present():
    assert len(FIX) >= 4


@pytest.mark.parametrize("path", FIX, ids=[os.path.basename(p) for p in FIX])
def test_decoder_matches_qwen3_fixture(hip, path):
    z = np.load(path)
    dec = _decoder(str(z["shape"]), int(z["seed"]))
    got = dec.forward(z["ids"], z["lens"]).cpu().numpy()
    want = z["expected"]
    cos = _cos(got, want)
    print(f"{os.path.basename(path)}: 1 - cos max {1 - cos.min():.2e}, max |d| {np.abs(got - want).max():.2e}")
    assert 1 - cos.min() <= COS_TOL, f"min cosine {cos.min()}"
    assert np.abs(got - want).max() <= ABS_TOL, f"max abs diff {np.abs(got - want).max()}"
    dec.close()


def test_decoder_06b_shape_against_hf(hip):
    """The full Qwen3-Embedding-0.6B shape (28 layers, 16 / 8 heads), seeded weights, a ragged batch up to 256 tokens, against
    float32 Qwen3Model on the CPU."""
    from tests.decoder_ref import hf_model, reference
    shape = "Qwen/Qwen3-Embedding-0.6B"
    w = _weights(shape, 5)
    rng = np.random.default_rng(5)
    lens = np.array([256, 1, 77, 200, 31, 128], np.int32)
    ids = np.zeros((len(lens), 256), np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.integers(0, QWEN3_SHAPES[shape][0], n)
    dec = _decoder(shape, 5)
    got = dec.forward(ids, lens).cpu().numpy()
    dec.close()
    want = reference(hf_model(shape, w), ids, lens)
    cos = _cos(got, want)
    print(f"0.6B: 1 - cos per row {np.array2string(1 - cos, precision=2)}, max |d| {np.abs(got - want).max():.2e}")
    assert 1 - cos.min() <= 1e-3, f"min cosine {cos.min()}"


def test_ids_past_length_do_not_matter(hip):
    dec = _decoder("qwen3-tiny-g2", 21)
    rng = np.random.default_rng(3)
    S = 160
    lens = np.array([160, 1, 33, 100, 64, 7], np.int32)
    ids = np.zeros((len(lens), S), np.int32)
    noisy = rng.integers(0, 1000, (len(lens), S)).astype(np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = noisy[i, :n]
    a = dec.forward(ids, lens).cpu().numpy()
    b = dec.forward(noisy, lens).cpu().numpy()
    assert np.isfinite(a).all()
    assert np.array_equal(a, b)
    dec.close()


def test_decoder_deterministic(hip):
    dec = _decoder("qwen3-tiny-g4", 22)
    rng = np.random.default_rng(4)
    lens = rng.integers(1, 257, 24).astype(np.int32)
    ids = rng.integers(0, 1000, (24, 256)).astype(np.int32)
    a = dec.forward(ids, lens).cpu().numpy()
    b = dec.forward(ids, lens).cpu().numpy()
    assert np.array_equal(a, b)
    dec.close()


def test_row_alone_vs_in_batch(hip):
    dec = _decoder("qwen3-tiny-g2", 23)
    rng = np.random.default_rng(6)
    lens = rng.integers(1, 385, 64).astype(np.int32)
    lens[17] = 211
    ids = rng.integers(0, 1000, (64, 384)).astype(np.int32)
    batch = dec.forward(ids, lens).cpu().numpy()
    alone = dec.forward(ids[17:18, :211], lens[17:18]).cpu().numpy()
    assert 1 - _cos(batch[17:18], alone)[0] <= 1e-5
    dec.close()


def test_text_end_to_end(hip, tmp_path):
    """Checkpoint directory -> ArchiHipEmbeddings (tokenizer.json, lasttoken pooling, Normalize) -> ArchiHipVectorStore, against
    the float32 CPU path on the same ids."""
    from archi_amd.embeddings import ArchiHipEmbeddings
    from archi_amd.vectorstore import ArchiHipVectorStore
    from tests.decoder_ref import hf_model, reference, write_checkpoint
    shape = "qwen3-tiny-g2"
    w = _weights(shape, 31)
    d = write_checkpoint(str(tmp_path / "qwen3"), QWEN3_SHAPES[shape], w, max_seq_length=64)
    emb = ArchiHipEmbeddings(d)
    assert emb.dimensions == 256 and emb.pooling == "last" and emb.normalize
    docs = ["Muon chambers measure the momentum of tracks.", "Résumé: the µ-metal shield — “good enough” at σ = 3.",
            "Für die Kalibrierung wird eine Quelle verwendet.", "The beam energy was 6.8 TeV per proton.",
            "日本語のテキスト", "short", "Η ενέργεια του δέσμου " * 12, "trigger decision at 40 MHz"]
    got = np.asarray(emb.embed_documents(docs), np.float32)
    ids, lens = emb.tokenizer.encode_batch_array([t.replace("\n", " ") for t in docs], emb.max_seq_length)
    model = hf_model(shape, w)
    want = reference(model, ids, lens)
    assert 1 - _cos(got, want).min() <= COS_TOL
    query = "Instruct: Given a physics question, retrieve relevant passages\nQuery:what is the beam energy?"
    q = np.asarray(emb.embed_query(query), np.float32)
    qi, ql = emb.tokenizer.encode_batch_array([query.replace("\n", " ")], emb.max_seq_length)
    q_want = reference(model, qi, ql)[0]
    assert 1 - float(q @ q_want / (np.linalg.norm(q) * np.linalg.norm(q_want))) <= COS_TOL

    store = ArchiHipVectorStore(None, emb, distance_metric="cosine")
    store.add_texts(docs, metadatas=[{"i": i} for i in range(len(docs))])
    k = 4
    res = store.similarity_search_with_score(query, k=k)
    got_ids = [doc.metadata["i"] for doc, _ in res]
    cpu_scores = 1 - want @ q_want / (np.linalg.norm(want, axis=1) * np.linalg.norm(q_want))
    order = np.argsort(cpu_scores, kind="stable")
    # the CPU top-k ids wherever the CPU scores are separated by more than 1e-3
    for rank in range(k):
        sep_prev = rank == 0 or cpu_scores[order[rank]] - cpu_scores[order[rank - 1]] > 1e-3
        sep_next = cpu_scores[order[rank + 1]] - cpu_scores[order[rank]] > 1e-3
        if sep_prev and sep_next:
            assert str(got_ids[rank]) == str(order[rank]), (got_ids, order[:k], cpu_scores[order[:k + 1]])
