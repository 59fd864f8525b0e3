"""GPU tests of the XLM-RoBERTa path: the BERT encoder with positions from the ids (ak_encoder_set_positions_from_ids: k_positions,
then k_embed / k32_embed / k3_embed read the position rows). The fixtures of tests/golden/make_xlmr_fixtures.py (float32
transformers.XLMRobertaModel on the CPU, literal pad ids inside rows) at the encoder's bars, the first hidden-1024 coverage, HF's
shifted positions on rows holding <pad>, forward_lens / batching / determinism invariances, the entry point's refusals, and text end
to end through ArchiHipEmbeddings and ArchiHipVectorStore."""
import glob
import os

import numpy as np
import pytest

from archi_amd.encoder import XLMR_SHAPES, random_xlmr_weights

pytestmark = pytest.mark.gpu
FIX = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "xlmr_*.npz")))
F32_ABS_TOL, F32_COS_TOL = 1e-5, 1e-6          # the encoder's parity bar (test_encoder_gpu.py, test_mpnet_gpu.py)
BF16_COS_TOL, BF16_ABS_TOL = 3e-4, 3e-3        # the stated hidden-768 bf16 tolerance
EPS = 1e-5
PAD = 1

_WEIGHTS = {}


def _weights(shape, seed):
    if (shape, seed) not in _WEIGHTS:
        _WEIGHTS[(shape, seed)] = random_xlmr_weights(shape, seed=seed)
    return _WEIGHTS[(shape, seed)]


def _encoder(shape, seed, precision="bf16", positions=True):
    from archi_amd.encoder import HipEncoder
    vocab, H, L, heads, I, max_pos = XLMR_SHAPES[shape][:6]
    return HipEncoder(vocab, H, L, heads, I, max_pos, _weights(shape, seed), ln_eps=EPS, device=0, precision=precision,
                      positions_from_ids=PAD if positions else None)


def _cos(got, want):
    return (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))


def _check(got, want, precision, what, bf16=(BF16_COS_TOL, BF16_ABS_TOL)):
    cos, dmax = _cos(got, want), np.abs(got - want).max()
    print(f"{what} [{precision}]: 1 - cos max {1 - cos.min():.2e}, max |d| {dmax:.2e}")
    if precision == "bf16":
        assert 1 - cos.min() <= bf16[0] and dmax <= bf16[1], (1 - cos.min(), dmax)
    else:
        assert 1 - cos.min() <= F32_COS_TOL and dmax <= F32_ABS_TOL, (1 - cos.min(), dmax)


def _mask(ids, lens):
    return (np.arange(ids.shape[1])[None, :] < np.asarray(lens)[:, None]).astype(np.int32)


def test_fixtures_present():
    assert len(FIX) >= 4


@pytest.mark.parametrize("precision", ["bf16", "f32", "bf16x3"])
@pytest.mark.parametrize("path", FIX, ids=[os.path.basename(p) for p in FIX])
def test_encoder_matches_xlmr_fixture(hip, path, precision):
    z = np.load(path)
    enc = _encoder(str(z["shape"]), int(z["seed"]), precision)
    ids, lens = z["ids"], z["lens"]
    got = enc.forward(ids, _mask(ids, lens), pooling=str(z["pooling"]), normalise=True).cpu().numpy()
    _check(got, z["expected"], precision, os.path.basename(path))
    enc.close()


def _rows(rng, lens, S, vocab, pads=2):
    toks = [rng.integers(4, vocab, n).tolist() for n in lens]
    for t in toks:
        if len(t) > 8:
            for j in rng.choice(np.arange(1, len(t)), pads, replace=False):
                t[j] = PAD
    from tests.xlmr_ref import pad_rows
    return pad_rows(toks, S)


# bf16 at hidden 1024: stated from test_hidden_1024_bf16_holds_its_stated_tolerance_on_seeds below
BF16_1024 = (3e-4, 3e-3)


@pytest.mark.parametrize("precision", ["bf16", "f32", "bf16x3"])
def test_hidden_1024_two_layer_cut(hip, precision):
    """The first hidden-1024 coverage: a two-layer cut of the bge-m3 / multilingual-e5-large layer (16 heads of 64) against float32
    XLMRobertaModel, ragged rows with literal pad ids, cls and mean pooling."""
    from tests.xlmr_ref import hf_embed, hf_model
    shape, seed = "xlmr-1024-cut2", 71
    rng = np.random.default_rng(seed)
    ids, mask = _rows(rng, [160, 1, 77, 130], 160, 1000)
    model, _ = hf_model(shape, seed)
    enc = _encoder(shape, seed, precision)
    for pooling in ("cls", "mean"):
        got = enc.forward(ids, mask, pooling=pooling, normalise=True).cpu().numpy()
        _check(got, hf_embed(model, ids, mask, pooling=pooling), precision, f"hidden 1024 {pooling}", bf16=BF16_1024)
    enc.close()


def test_hidden_1024_bf16_holds_its_stated_tolerance_on_seeds(hip):
    from tests.xlmr_ref import hf_embed, hf_model
    worst = 0.0
    for seed in (81, 82, 83):
        rng = np.random.default_rng(seed)
        ids, mask = _rows(rng, [128, 64, 17], 128, 1000)
        model, _ = hf_model("xlmr-1024-cut2", seed)
        enc = _encoder("xlmr-1024-cut2", seed, "bf16")
        got = enc.forward(ids, mask, pooling="cls", normalise=True).cpu().numpy()
        enc.close()
        want = hf_embed(model, ids, mask, pooling="cls")
        _check(got, want, "bf16", f"seed {seed}", bf16=BF16_1024)
        worst = max(worst, float(1 - _cos(got, want).min()))
    print(f"hidden 1024 bf16 worst 1 - cos over seeds {worst:.2e}")


@pytest.mark.parametrize("precision", ["f32", "bf16x3", "bf16"])
def test_literal_pad_takes_hf_shifted_positions(hip, precision):
    """Rows holding the pad id (a text with a literal <pad>) get HF's positions -- the pad at padding_idx, the tokens behind it one
    place earlier -- and differ clearly from the offset scheme's."""
    from tests.xlmr_ref import hf_embed, hf_model, offset_positions
    shape, seed = "xlmr-tiny-hd64", 91
    rng = np.random.default_rng(seed)
    ids, mask = _rows(rng, [96, 60, 33], 96, 1000, pads=3)
    model, _ = hf_model(shape, seed)
    enc = _encoder(shape, seed, precision)
    got = enc.forward(ids, mask, pooling="mean", normalise=True).cpu().numpy()
    enc.close()
    want = hf_embed(model, ids, mask, pooling="mean")
    off = hf_embed(model, ids, mask, pooling="mean", position_ids=offset_positions(ids))
    _check(got, want, precision, "literal <pad>")
    assert np.abs(got - off).max() > 10 * BF16_ABS_TOL


@pytest.mark.parametrize("precision", ["bf16", "f32", "bf16x3"])
def test_lens_entry_point_batching_and_determinism(hip, precision):
    """forward_lens (lengths, garbage past them -- pad ids included) gives the bits of forward on the explicit mask; a row alone
    equals the row in the batch; two runs are bit-identical; a length-0 row embeds to zeros."""
    import torch
    shape = "xlmr-tiny-hd32"
    enc = _encoder(shape, 93, precision)
    rng = np.random.default_rng(7)
    B, S = 9, 256
    lens = rng.integers(1, S + 1, B).astype(np.int32)
    lens[0], lens[1], lens[2] = S, 1, 0
    stage = rng.integers(0, 1000, (B, S + 1)).astype(np.int32)        # ids 0 .. 3 too: <s>, <pad>, </s>, <unk> anywhere
    stage[:, S] = lens
    mask = _mask(stage[:, :S], lens)
    want = enc.forward(stage[:, :S] * mask, mask, pooling="mean", normalise=True).cpu().numpy()
    outs = []
    for _ in range(2):
        out = torch.zeros((B, enc.hidden), dtype=torch.float32, device="cuda")
        enc.forward_lens(torch.from_numpy(stage).cuda(), B, S, out, pooling="mean", normalise=True)
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0], want)
    assert np.all(want[2] == 0.0)
    for i in (3, 4):
        w = (int(lens[i]) + 31) // 32 * 32
        alone = enc.forward(stage[i:i + 1, :w] * mask[i:i + 1, :w], mask[i:i + 1, :w], pooling="mean", normalise=True).cpu().numpy()
        assert 1 - _cos(alone, want[i:i + 1]).min() <= 1e-5
        assert np.abs(alone - want[i:i + 1]).max() <= (1e-3 if precision == "bf16" else 1e-6)
    enc.close()


def test_entry_point_refusals(hip):
    from archi_amd import _lib
    from archi_amd._lib import HipBackendError
    from archi_amd.encoder import HipEncoder, mpnet_rel_bias_table
    enc = _encoder("xlmr-tiny-hd64", 95, "bf16")
    lib = _lib.load()
    assert lib.ak_encoder_set_positions_from_ids(enc._h, PAD, 128) != 0            # set twice
    assert "already" in _lib.last_error()
    ids = np.full((1, 96), 7, np.int32)
    enc.forward(ids, np.ones_like(ids))
    enc.close()
    vocab, H, L, heads, I, max_pos = XLMR_SHAPES["xlmr-long-hd64"][:6]
    w = _weights("xlmr-long-hd64", 95)
    from archi_amd._lib import check
    for precision in ("f32", "bf16x3"):                                            # rows over 512 tokens: bf16 only
        enc = HipEncoder(vocab, H, L, heads, I, max_pos, w, ln_eps=EPS, device=0, precision=precision)
        try:
            with pytest.raises(HipBackendError, match="bf16 at head size 64"):
                check(lib.ak_encoder_set_positions_from_ids(enc._h, PAD, 8192), "ak_encoder_set_positions_from_ids")
            check(lib.ak_encoder_set_positions_from_ids(enc._h, PAD, 512), "ak_encoder_set_positions_from_ids")
        finally:
            enc.close()
    enc = HipEncoder(vocab, H, L, heads, I, 514, dict(w, pos_emb=w["pos_emb"][:514]), ln_eps=EPS, device=0,
                     rel_bias=mpnet_rel_bias_table(np.zeros((32, heads), np.float32), 512))
    assert lib.ak_encoder_set_positions_from_ids(enc._h, PAD, 512) != 0             # not combined with a relative-position bias
    assert "relative-position bias" in _lib.last_error()
    enc.close()


@pytest.mark.parametrize("precision", ["f32", "bf16x3", "bf16"])
def test_text_end_to_end(hip, tmp_path, precision):
    """Checkpoint directory (save_pretrained + tokenizer.json + sentence-transformers files) -> ArchiHipEmbeddings -> ArchiHipVectorStore,
    against float32 XLMRobertaModel on the CPU over transformers' fast tokenizer: f32 / bf16x3 give the CPU top-10 ids and scores
    within 1e-5; bf16 the CPU ids wherever the CPU scores are separated by more than 1e-3."""
    from archi_amd.embeddings import ArchiHipEmbeddings
    from archi_amd.vectorstore import ArchiHipVectorStore
    from tests.xlmr_ref import CORPUS, TEXTS, hf_embed, hf_tokenizer, pad_rows, write_checkpoint
    d = str(tmp_path / "xlmr")
    model = write_checkpoint(d, "xlmr-tiny-hd64", seed=3, pooling="cls", max_seq_length=128)
    emb = ArchiHipEmbeddings(d, model_kwargs={"precision": precision})
    assert emb.dimensions == 256 and emb.pooling == "cls" and emb.normalize and emb.max_seq_length == 128
    rng = np.random.default_rng(9)
    words = " ".join(CORPUS).split()
    docs = list(TEXTS) + [" ".join(rng.choice(words, rng.integers(3, 60))) for _ in range(40)]
    got = np.asarray(emb.embed_documents(docs), np.float32)
    tok = hf_tokenizer(os.path.join(d, "tokenizer.json"))
    toks = tok([x.replace("\n", " ") for x in docs], truncation=True, max_length=128)["input_ids"]
    ids, mask = pad_rows(toks, max(len(t) for t in toks))
    want = hf_embed(model, ids, mask, pooling="cls")
    _check(got, want, precision, "documents")
    query = "welcher Trigger ist am Myon-Detektor fehlgeschlagen? σ µs"
    qt = tok(query)["input_ids"]
    q_want = hf_embed(model, *pad_rows([qt], len(qt)), pooling="cls")[0]

    store = ArchiHipVectorStore(None, emb, collection_name=f"xlmr_e2e_{precision}", distance_metric="cosine")
    store.add_texts(docs, metadatas=[{"i": i} for i in range(len(docs))])
    k = 10
    res = store.similarity_search_with_score(query, k=k)
    got_ids = [int(doc.metadata["i"]) for doc, _ in res]
    got_scores = np.array([s for _, s in res], np.float64)
    cpu_scores = 1 - want @ q_want / (np.linalg.norm(want, axis=1) * np.linalg.norm(q_want))
    order = np.argsort(cpu_scores, kind="stable")
    if precision != "bf16":
        assert got_ids == [int(o) for o in order[:k]], (got_ids, order[:k])
        assert np.abs(got_scores - (1 - cpu_scores[order[:k]])).max() <= 1e-5
        return
    for rank in range(k):
        sep_prev = rank == 0 or cpu_scores[order[rank]] - cpu_scores[order[rank - 1]] > 1e-3
        sep_next = cpu_scores[order[rank + 1]] - cpu_scores[order[rank]] > 1e-3
        if sep_prev and sep_next:
            assert got_ids[rank] == int(order[rank]), (got_ids, order[:k], cpu_scores[order[:k + 1]])


def test_named_shape_with_synthetic_seed(hip):
    from archi_amd.embeddings import ArchiHipEmbeddings
    emb = ArchiHipEmbeddings("intfloat/multilingual-e5-base", model_kwargs={"synthetic_seed": 0})
    assert emb.dimensions == 768 and emb.max_seq_length == 512 and emb.pooling == "mean"
    assert emb.encoder.positions_from_ids == PAD
    v = np.asarray(emb.embed_documents(["the muon detector", "ein zweiter Text über Strahlen " * 30]), np.float32)
    assert v.shape == (2, 768) and np.isfinite(v).all()
    assert np.allclose(np.linalg.norm(v, axis=1), 1.0, atol=1e-5)


# ---- rows longer than 512 tokens (bf16, head size 64: csrc/attn_long.hip) ----------------------------------------------------

LONG = "xlmr-long-hd64"
LONG_LENS = [8192, 4100, 1000, 513, 64, 1]


def _long_batch(seed, S=8192, lens=LONG_LENS):
    rng = np.random.default_rng(seed)
    return _rows(rng, lens, S, 1000, pads=3)


def _hf_rows(model, ids, lens, pooling):
    """float32 XLMRobertaModel, each row alone at its own length (SDPA: memory-efficient at 8192 tokens)."""
    from tests.xlmr_ref import hf_embed
    out = []
    for row, n in zip(ids, lens):
        out.append(hf_embed(model, row[None, :n], np.ones((1, n), np.int32), pooling=pooling)[0])
    return np.stack(out)


def test_long_rows_match_hf(hip):
    """One batch of lengths {8192, 4100, 1000, 513, 64, 1} (literal pad ids inside) at S = 8192 against float32 XLMRobertaModel."""
    from tests.xlmr_ref import hf_model
    seed = 101
    ids, mask = _long_batch(seed)
    enc = _encoder(LONG, seed, "bf16")
    assert enc.max_seq == 8192
    model, _ = hf_model(LONG, seed)
    model.config._attn_implementation = "sdpa"
    for pooling in ("cls", "mean"):
        got = enc.forward(ids, mask, pooling=pooling, normalise=True).cpu().numpy()
        _check(got, _hf_rows(model, ids, LONG_LENS, pooling), "bf16", f"long rows {pooling}")
    enc.close()


def test_long_rows_batching_determinism_and_lens(hip):
    """A row alone equals the same row in the batch (1 - cos <= 1e-5); two runs are bit-identical; forward_lens with garbage past
    each row's length gives the bits of forward on the explicit mask."""
    import torch
    seed = 103
    ids, mask = _long_batch(seed)
    enc = _encoder(LONG, seed, "bf16")
    a = enc.forward(ids, mask, pooling="mean", normalise=True).cpu().numpy()
    b = enc.forward(ids, mask, pooling="mean", normalise=True).cpu().numpy()
    assert np.array_equal(a, b)
    B, S = ids.shape
    rng = np.random.default_rng(seed)
    stage = rng.integers(0, 1000, (B, S + 1)).astype(np.int32)
    stage[:, :S] = np.where(mask == 1, ids, stage[:, :S])
    stage[:, S] = LONG_LENS
    out = torch.zeros((B, enc.hidden), dtype=torch.float32, device="cuda")
    enc.forward_lens(torch.from_numpy(stage).cuda(), B, S, out, pooling="mean", normalise=True)
    want = enc.forward(ids * mask, mask, pooling="mean", normalise=True).cpu().numpy()
    assert np.array_equal(out.cpu().numpy(), want)
    for i in (1, 2, 3):
        w = (LONG_LENS[i] + 31) // 32 * 32
        alone = enc.forward(ids[i:i + 1, :w], mask[i:i + 1, :w], pooling="mean", normalise=True).cpu().numpy()
        assert 1 - _cos(alone, a[i:i + 1]).min() <= 1e-5, i
    enc.close()


def test_short_tiles_are_bit_identical_with_and_without_long_max_seq(hip):
    """A tile of S <= 512 runs the kernels it ran before whatever the encoder's max_seq: the same weights with the 8194-row table
    (max_seq 8192) and with its first 514 rows (max_seq 512) give the same bits."""
    from archi_amd.encoder import HipEncoder
    seed = 105
    vocab, H, L, heads, I, max_pos = XLMR_SHAPES[LONG][:6]
    w = _weights(LONG, seed)
    ids, mask = _rows(np.random.default_rng(seed), [256, 100, 7, 255], 256, 1000)
    outs = []
    for mp in (max_pos, 514):
        enc = HipEncoder(vocab, H, L, heads, I, mp, dict(w, pos_emb=w["pos_emb"][:mp]), ln_eps=EPS, device=0, positions_from_ids=PAD)
        assert enc.max_seq == mp - 2
        outs.append(enc.forward(ids, mask, pooling="cls", normalise=True).cpu().numpy())
        enc.close()
    assert np.array_equal(outs[0], outs[1])


def test_hidden_1024_large_batch_on_the_gemm_tiles(hip):
    """16 x 512 = 8192 tokens at hidden 1024 in bf16: the lazy-LayerNorm wide-tile GEMMs (N = 1024 / 3072 / 4096) that ingestion
    tiles of bge-m3 / multilingual-e5-large take, against float32 XLMRobertaModel on sampled rows."""
    from tests.xlmr_ref import hf_embed, hf_model
    shape, seed = "xlmr-1024-cut2", 107
    ids, mask = _rows(np.random.default_rng(seed), [512] + list(np.random.default_rng(seed).integers(1, 513, 15)), 512, 1000)
    enc = _encoder(shape, seed, "bf16")
    got = enc.forward(ids, mask, pooling="cls", normalise=True).cpu().numpy()
    enc.close()
    pick = np.array([0, 1, 7, 15])
    model, _ = hf_model(shape, seed)
    width = int(mask[pick].sum(1).max())
    _check(got[pick], hf_embed(model, ids[pick][:, :width], mask[pick][:, :width], pooling="cls"), "bf16", "hidden 1024 16 x 512",
           bf16=BF16_1024)


def test_split_bf16_large_batch_on_the_gemm_tiles(hip):
    """32 x 512 = 16 384 tokens in bf16x3: the split mode's GEMM-tile path, whose embedding kernel (k3_embed) reads the position rows,
    against float32 XLMRobertaModel on sampled rows (pad ids inside them)."""
    from tests.xlmr_ref import hf_embed, hf_model
    shape, seed = "xlmr-tiny-hd64", 109
    lens = [512] + list(np.random.default_rng(seed).integers(1, 513, 31))
    ids, mask = _rows(np.random.default_rng(seed), lens, 512, 1000)
    enc = _encoder(shape, seed, "bf16x3")
    got = enc.forward(ids, mask, pooling="mean", normalise=True).cpu().numpy()
    enc.close()
    pick = np.array([0, 1, 16, 31])
    model, _ = hf_model(shape, seed)
    width = int(mask[pick].sum(1).max())
    _check(got[pick], hf_embed(model, ids[pick][:, :width], mask[pick][:, :width], pooling="mean"), "bf16x3", "bf16x3 32 x 512")


def test_bge_m3_named_shape_routes_long_rows(hip):
    """The provider on a long-row shape: a text longer than 512 tokens is embedded whole, equal to the encoder's own row."""
    from archi_amd.embeddings import ArchiHipEmbeddings
    emb = ArchiHipEmbeddings(LONG, model_kwargs={"synthetic_seed": 5, "tokenizer_file": os.path.join(os.path.dirname(__file__), "golden",
                                                                                                          "xlmr_tokenizer.json")})
    assert emb.max_seq_length == 8192 and emb.encoder.max_seq == 8192
    text = "Die Kalibrierung des Myon-Detektors σ = 0.5 µs " * 150
    toks = emb.tokenizer.encode(text, emb.max_seq_length)
    assert 512 < len(toks) < 8192
    v = np.asarray(emb.embed_documents([text, "short"]), np.float32)
    S = (len(toks) + 31) // 32 * 32
    ids = np.full((1, S), PAD, np.int32)
    ids[0, :len(toks)] = toks
    want = emb.encoder.forward(ids, (np.arange(S) < len(toks))[None].astype(np.int32), pooling=emb.pooling, normalise=True).cpu().numpy()
    assert 1 - _cos(v[:1], want).min() <= 1e-6 and np.isfinite(v).all()
