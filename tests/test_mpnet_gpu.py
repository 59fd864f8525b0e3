"""GPU tests of the MPNet path (all-mpnet-base-v2 and its family): the BERT encoder with MPNet's relative-position bias
(ak_encoder_set_rel_bias; the bias inside k_attn_s / k_attn_d / k_attn, k32m_attn and k3_attn), its offset positions and its
tokenizer. The fixtures of tests/golden/make_mpnet_fixtures.py (float32 transformers.MPNetModel on the CPU) at the encoder's bars,
the split-bf16 mode on the GEMM tiles, bit-identity of an all-zero table with no table, batching / length-0 / forward_lens
invariances, and text end to end through ArchiHipEmbeddings and ArchiHipVectorStore."""
import glob
import os

import numpy as np
import pytest

from archi_amd.encoder import MPNET_SHAPES, mpnet_rel_bias_table, random_mpnet_weights

pytestmark = pytest.mark.gpu
FIX = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "mpnet_*.npz")))
F32_ABS_TOL, F32_COS_TOL = 1e-5, 1e-6          # the encoder's parity bar (test_encoder_gpu.py)
BF16_COS_TOL, BF16_ABS_TOL = 3e-4, 3e-3        # the stated hidden-768 bf16 tolerance
EPS = 1e-5

_WEIGHTS = {}


def _weights(shape, seed):
    if (shape, seed) not in _WEIGHTS:
        _WEIGHTS[(shape, seed)] = random_mpnet_weights(shape, seed=seed)
    return _WEIGHTS[(shape, seed)]


def _encoder(shape, seed, precision="bf16", table="real"):
    """HipEncoder of random_mpnet_weights(shape, seed); table: "real" (the seeded bias), "zero" (an all-zero table) or None."""
    from archi_amd.encoder import HipEncoder
    vocab, H, L, heads, I, max_pos = MPNET_SHAPES[shape][:6]
    w, rel, _ = _weights(shape, seed)
    n_rel = max_pos - 2
    tab = None
    if table == "real":
        tab = mpnet_rel_bias_table(rel, n_rel)
    elif table == "zero":
        tab = np.zeros((heads, 2 * n_rel - 1), np.float32)
    return HipEncoder(vocab, H, L, heads, I, n_rel, w, ln_eps=EPS, device=0, precision=precision, rel_bias=tab)


def _cos(got, want):
    return (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))


def _check(got, want, precision, what):
    cos, dmax = _cos(got, want), np.abs(got - want).max()
    print(f"{what} [{precision}]: 1 - cos max {1 - cos.min():.2e}, max |d| {dmax:.2e}")
    if precision == "bf16":
        assert 1 - cos.min() <= BF16_COS_TOL and dmax <= BF16_ABS_TOL, (1 - cos.min(), dmax)
    else:
        assert 1 - cos.min() <= F32_COS_TOL and dmax <= F32_ABS_TOL, (1 - cos.min(), dmax)


def test_fixtures_present():
    assert len(FIX) >= 4


@pytest.mark.parametrize("precision", ["bf16", "f32", "bf16x3"])
@pytest.mark.parametrize("path", FIX, ids=[os.path.basename(p) for p in FIX])
def test_encoder_matches_mpnet_fixture(hip, path, precision):
    z = np.load(path)
    enc = _encoder(str(z["shape"]), int(z["seed"]), precision)
    ids, lens = z["ids"], z["lens"]
    mask = (np.arange(ids.shape[1])[None, :] < lens[:, None]).astype(np.int32)
    got = enc.forward(ids, mask, pooling="mean", normalise=True).cpu().numpy()
    _check(got, z["expected"], precision, os.path.basename(path))
    enc.close()


def test_split_bf16_large_batch_on_the_gemm_tiles(hip):
    """16 384 tokens at hidden 768: the split-bf16 mode's GEMM-tile form (launch_attn_x3_split) against float32 MPNetModel on
    sampled rows (a row's embedding does not depend on its neighbours)."""
    from tests.mpnet_ref import hf_embed, hf_model, pad_rows
    shape, seed, B, S = "mpnet-cut2", 31, 32, 512
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, S + 1, B)
    lens[0] = S
    toks = [rng.integers(5, MPNET_SHAPES[shape][0], n).tolist() for n in lens]
    ids, mask = pad_rows(toks, S)
    enc = _encoder(shape, seed, "bf16x3")
    got = enc.forward(ids, mask, pooling="mean", normalise=True).cpu().numpy()
    enc.close()
    pick = np.array([0, 1, B // 2, B - 1])
    model, _ = hf_model(shape, seed)
    width = int(lens[pick].max())
    want = hf_embed(model, ids[pick][:, :width], mask[pick][:, :width])
    _check(got[pick], want, "bf16x3", "B=32 S=512")


@pytest.mark.parametrize("precision", ["bf16", "f32", "bf16x3"])
def test_zero_bias_table_is_bit_identical_to_no_table(hip, precision):
    """The bias kernels with an all-zero table give the bits of the kernels without one (both head sizes, padded rows)."""
    rng = np.random.default_rng(5)
    for shape, S in (("mpnet-cut2", 512), ("mpnet-tiny-hd32", 128)):
        B = 3
        ids = rng.integers(5, MPNET_SHAPES[shape][0], (B, S)).astype(np.int32)
        mask = (np.arange(S)[None, :] < np.array([S, S // 2 + 3, 1])[:, None]).astype(np.int32)
        outs = []
        for table in ("zero", None):
            enc = _encoder(shape, 41, precision, table=table)
            outs.append(enc.forward(ids, mask, pooling="mean", normalise=True).cpu().numpy())
            enc.close()
        assert np.array_equal(outs[0], outs[1]), (shape, np.abs(outs[0] - outs[1]).max())


@pytest.mark.parametrize("precision", ["bf16", "f32", "bf16x3"])
def test_row_alone_equals_the_row_in_a_batch_and_lens_entry_point(hip, precision):
    """A row embedded alone gives the row of the batch; a length-0 row embeds to zeros; forward_lens (lengths, garbage past them)
    gives the bits of forward on the explicit mask."""
    import torch
    shape = "mpnet-tiny-hd32"
    enc = _encoder(shape, 43, precision)
    rng = np.random.default_rng(7)
    B, S = 9, 256
    lens = rng.integers(1, S + 1, B).astype(np.int32)
    lens[0], lens[1], lens[2] = S, 1, 0
    stage = rng.integers(5, MPNET_SHAPES[shape][0], (B, S + 1)).astype(np.int32)
    stage[:, S] = lens
    mask = (np.arange(S)[None, :] < lens[:, None]).astype(np.int32)
    want = enc.forward(stage[:, :S] * mask, mask, pooling="mean", normalise=True).cpu().numpy()
    out = torch.zeros((B, enc.hidden), dtype=torch.float32, device="cuda")
    enc.forward_lens(torch.from_numpy(stage).cuda(), B, S, out, pooling="mean", normalise=True)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.all(want[2] == 0.0)
    i = 3
    w = (int(lens[i]) + 31) // 32 * 32
    alone = enc.forward(stage[i:i + 1, :w] * mask[i:i + 1, :w], mask[i:i + 1, :w], pooling="mean", normalise=True).cpu().numpy()
    d = np.abs(alone - want[i:i + 1]).max()
    assert d <= (1e-3 if precision == "bf16" else 1e-6), d
    enc.close()


def test_sequence_longer_than_the_table_is_refused(hip):
    from archi_amd._lib import HipBackendError
    from archi_amd.encoder import HipEncoder
    vocab, H, L, heads, I, max_pos = MPNET_SHAPES["mpnet-tiny-hd32"][:6]
    w, rel, _ = _weights("mpnet-tiny-hd32", 43)
    enc = HipEncoder(vocab, H, L, heads, I, 512, w, ln_eps=EPS, device=0, rel_bias=mpnet_rel_bias_table(rel, 64))
    ids = np.full((1, 96), 7, np.int32)
    with pytest.raises((HipBackendError, RuntimeError), match="n_rel"):
        enc.forward(ids, np.ones_like(ids))
    enc.close()


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_text_end_to_end(hip, tmp_path, precision):
    """Checkpoint directory -> ArchiHipEmbeddings (MPNet tokenizer, mean pooling, Normalize) -> ArchiHipVectorStore, against
    float32 MPNetModel on the CPU: f32 gives the CPU top-10 and scores within 1e-5; bf16 the CPU ids wherever the CPU scores are
    separated by more than 1e-3."""
    from archi_amd.embeddings import ArchiHipEmbeddings
    from archi_amd.vectorstore import ArchiHipVectorStore
    from tests.mpnet_ref import TEXTS, hf_embed, hf_tokenizer, pad_rows, write_checkpoint
    d = str(tmp_path / "mpnet")
    model = write_checkpoint(d, "mpnet-tiny-hd32", seed=3, max_seq_length=128)
    emb = ArchiHipEmbeddings(d, model_kwargs={"precision": precision})
    assert emb.dimensions == 256 and emb.pooling == "mean" and emb.normalize and emb.max_seq_length == 128
    rng = np.random.default_rng(9)
    words = ["the", "muon", "detector", "calibration", "run", "grid", "beam", "trigger", "jet", "energy", "data", "tier",
             "site", "job", "failed", ".", ","]
    docs = list(TEXTS) + [" ".join(rng.choice(words, rng.integers(3, 60))) for _ in range(40)]
    got = np.asarray(emb.embed_documents(docs), np.float32)
    tok = hf_tokenizer(os.path.join(d, "vocab.txt"))
    toks = [t[:127] + [t[-1]] if len(t) > 128 else t for t in (tok(x)["input_ids"] for x in docs)]
    ids, mask = pad_rows(toks, max(len(t) for t in toks))
    want = hf_embed(model, ids, mask)
    _check(got, want, precision, "documents")
    query = "which trigger failed on the muon detector grid?"
    qt = tok(query)["input_ids"]
    q_want = hf_embed(model, *pad_rows([qt], len(qt)))[0]

    store = ArchiHipVectorStore(None, emb, collection_name=f"mpnet_e2e_{precision}", distance_metric="cosine")
    store.add_texts(docs, metadatas=[{"i": i} for i in range(len(docs))])
    k = 10
    res = store.similarity_search_with_score(query, k=k)
    got_ids = [int(doc.metadata["i"]) for doc, _ in res]
    got_scores = np.array([s for _, s in res], np.float64)
    cpu_scores = 1 - want @ q_want / (np.linalg.norm(want, axis=1) * np.linalg.norm(q_want))
    order = np.argsort(cpu_scores, kind="stable")
    if precision == "f32":
        assert got_ids == [int(o) for o in order[:k]], (got_ids, order[:k])
        assert np.abs(got_scores - (1 - cpu_scores[order[:k]])).max() <= 1e-5      # the store returns the cosine similarity
        return
    for rank in range(k):
        sep_prev = rank == 0 or cpu_scores[order[rank]] - cpu_scores[order[rank - 1]] > 1e-3
        sep_next = cpu_scores[order[rank + 1]] - cpu_scores[order[rank]] > 1e-3
        if sep_prev and sep_next:
            assert got_ids[rank] == int(order[rank]), (got_ids, order[:k], cpu_scores[order[:k + 1]])


@pytest.mark.parametrize("precision", ["bf16", "f32", "bf16x3"])
def test_named_shape_with_synthetic_seed(hip, precision):
    from archi_amd.embeddings import ArchiHipEmbeddings
    emb = ArchiHipEmbeddings("sentence-transformers/all-mpnet-base-v2", model_kwargs={"synthetic_seed": 0, "precision": precision})
    assert emb.dimensions == 768 and emb.max_seq_length == 384 and emb.pooling == "mean"
    v = np.asarray(emb.embed_documents(["the muon detector", "a second text about beams " * 30]), np.float32)
    assert v.shape == (2, 768) and np.isfinite(v).all()
    assert np.allclose(np.linalg.norm(v, axis=1), 1.0, atol=1e-5)
