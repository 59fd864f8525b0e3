"""GPU suite of the batch hybrid query (csrc/lexical_batch.hip) and of the coalescing of concurrent hybrid_search calls. Every
comparison is exact equality, on texts and float64 score bits:

  - hybrid_search_batch against a loop of hybrid_search and against the reference's formula over ALL rows (test_lexical_gpu.Brute);
  - the splits inside the call (33 queries, the pair budget, the term table's capacity) against the unsplit call, with out_info
    showing the extra passes; a 16-query batch is one statistics pass, one score pass and one scan;
  - collections below the MFMA scan's size and an empty one;
  - 8 reader threads + 1 writer with the coalescer on and off: every answer is the brute force of a state the collection was in;
  - 16 queries as one batch are not slower than the 16 single calls.
"""
import threading
import time
import zlib

import numpy as np
import pytest

from archi_amd import _lib
from archi_amd import vectorstore as vs
from archi_amd.lexical import DeviceBm25
from archi_amd.vectorstore import ArchiHipHybridVectorStore
from oracle import knn_oracle as ko
from tests.test_lexical_gpu import Brute, add_both, same

pytestmark = pytest.mark.gpu
N, DIM, PER = 6000, 64, 50


class KeyEmb:
    """A unit vector per text, keyed by the text."""

    def __init__(self, dim):
        self.dim = dim

    def embed_documents(self, texts):
        raise AssertionError("vectors are handed in; queries go through embed_query")

    def vector(self, text):
        return ko.gen_rows(zlib.crc32(text.encode()) & 0x7fffffff, 1, 0, 1, self.dim, True, "f32")[0]

    def embed_query(self, text):
        return [float(x) for x in self.vector(text)]


def corpus6000():
    rng = np.random.default_rng(61)
    vec = ko.gen_rows(61, 0, 0, N, DIM, True, "f32").copy()
    vocab = np.array([f"w{i}" for i in range(500)])
    words = rng.integers(0, 500, size=(N, 6))
    common = rng.random(N) < 0.3
    texts = [" ".join(vocab[words[i]]) + (" detector" if common[i] else "") + (" muon" if i % 397 == 0 else "") + f" #{i}" for i in range(N)]
    texts[10] = ""                                                  # 0 words
    texts[11] = "... !!!"                                           # 0 words
    texts[12] = "lonely"                                            # 1 word
    texts[13] = "w1 w2 w3 detector w1"                              # an even number of distinct words
    texts[14] = "w1 w2 w3 detector muon"                            # an odd number
    texts[15] = " ".join(f"v{i}" for i in range(150)) + " detector w7"        # more than 128 distinct words (the lane loop's stride)
    texts[16] = " ".join(f"v{i}" for i in range(129))
    texts[4321] = "solo31 w9 w9"                                    # the row only query 31 matches
    vec[397 * 3] = 0.0                                              # a zero-vector row that holds 'muon'
    metas = [{"source": "git" if (i // PER) % 4 == 0 else "web"} for i in range(N)]
    return texts, vec, metas


def queries32():
    rng = np.random.default_rng(62)
    long_q = " ".join(f"w{i}" for i in rng.permutation(500)[:70].tolist())             # more than 64 distinct words
    qs = ["detector muon", "nosuchword zzz", "", long_q, "w3 w17 detector", "w3 w17 detector", "muon w5 lonely", "w5 v3 muon",
          "v100 v128 v149", "w1 w1 w2 w1"]
    qs += [f"w{20 + i} w{300 + i}" + (" detector" if i % 5 == 0 else "") for i in range(32 - len(qs) - 1)]
    qs.append("solo31")                                             # query index 31: bit 31 of the rows' masks
    assert len(qs) == 32 and len(set(qs)) == 31
    return qs


WORLDS = {}


@pytest.fixture(scope="module", autouse=True)
def fresh(hip):
    vs.reset_collections()
    yield
    WORLDS.clear()
    vs.reset_collections()


def world(dtype, metric, sign):
    """The 6000-row collection of one (dtype, metric, sign), two documents deleted; built once per module."""
    key = (dtype, metric, sign)
    if key not in WORLDS:
        texts, vec, metas = corpus6000()
        emb = KeyEmb(DIM)
        db = DeviceBm25(sign=sign)
        sd = ArchiHipHybridVectorStore({"hip": {"dtype": dtype, "capacity": N}}, emb, collection_name=f"lexb_{dtype}_{metric}", distance_metric=metric,
                                       bm25=db)
        add_both((sd,), texts, vec, metas, 0, N, per=PER)
        live = np.ones(N, bool)
        for doc in (3, 41):                                         # some rows deleted
            assert sd.delete(document_id=doc) is True
            live[(doc - 1) * PER: doc * PER] = False
        WORLDS[key] = dict(store=sd, emb=emb, db=db, texts=texts, live=live, git=np.array([m["source"] == "git" for m in metas]),
                           brute=Brute(texts, vec, metric, dtype, sign=sign), singles={})
    return WORLDS[key]


def singles(w, queries, k, **kwargs):
    """[hybrid_search(q) for q in queries] as (text, score) lists; computed once per argument set and shared."""
    key = (tuple(queries), k, repr(sorted(kwargs.items())))
    if key not in w["singles"]:
        w["singles"][key] = [[(d.page_content, s) for d, s in w["store"].hybrid_search(q, k=k, **kwargs)] for q in queries]
    return w["singles"][key]


def index_batch(w, queries, k, ws=0.7, wb=0.3):
    """HipIndex.hybrid_search_batch below the store -> (per query the merged (ids, scores), info)."""
    sd, db = w["store"], w["db"]
    col = sd._collection()
    with sd.table.lock:
        terms = [db.device_query(q, sd.table, col.index) for q in queries]
        also = np.fromiter(sd.table.suspects, np.int64, len(sd.table.suspects))
    qs = np.stack([w["emb"].vector(q) for q in queries])
    legs, info = col.index.hybrid_search_batch(qs, terms, db.k1, db.b, db.sign, ws, wb, also, k)
    merged = []
    for hi, hc, si, sdist in legs:
        c = np.concatenate([hc, (1.0 - sdist.astype(np.float64)) * ws + 0 * wb])
        i = np.concatenate([hi, si]).astype(np.int64)
        nan = c != c
        o = np.lexsort((i, -np.where(nan, 0.0, c), ~nan))[:k]
        merged.append((i[o].tolist(), c[o].tobytes()))
    return merged, info


@pytest.mark.parametrize("dtype,metric,sign,kwargs", [("bf16", "cosine", 1.0, {}), ("f32", "l2", -1.0, {"filter": {"source": "git"}}),
                                                      ("f16", "inner_product", 1.0, {})])
def test_batch_equals_single_calls_and_the_formula_over_all_rows(dtype, metric, sign, kwargs):
    w = world(dtype, metric, sign)
    sd, br, queries, k = w["store"], w["brute"], queries32(), 10
    assert sd._collection().index.scan_plan(32, k)["fast"]                     # the MFMA scan serves the scan leg
    allowed = w["git"] if kwargs else np.ones(N, bool)
    got = sd.hybrid_search_batch(queries, k=k, **kwargs)
    want = singles(w, queries, k, **kwargs)
    assert len(got) == 32
    for j, q in enumerate(queries):
        assert same(got[j], want[j]), (j, q[:40])
        assert same(got[j], br.top(q, w["emb"].vector(q), k, 0.7, 0.3, w["live"], allowed)), (j, q[:40])
    if not kwargs:                                                             # bit 31: the row only the last query matches leads its list
        assert got[31][1 if metric == "cosine" else 0][0].page_content == w["texts"][4321]
    if metric == "cosine":
        assert all(g[0][1] != g[0][1] for g in got)                            # the zero-vector row's NaN ranks first for every query
    # other weights, among them a negative BM25 weight
    for ws, wb in ((0.5, 0.5), (1.0, 0.0), (0.7, -0.3)):
        got = sd.hybrid_search_batch(queries[:8], k=k, semantic_weight=ws, bm25_weight=wb, **kwargs)
        for j, q in enumerate(queries[:8]):
            assert same(got[j], singles(w, queries[:8], k, semantic_weight=ws, bm25_weight=wb, **kwargs)[j]), (j, ws, wb)
            assert same(got[j], br.top(q, w["emb"].vector(q), k, ws, wb, w["live"], allowed)), (j, ws, wb)
    if dtype == "f16":
        # k larger than |U|: a batch whose words are all rare
        rare = ["muon", "solo31", "nosuchword", "", "lonely muon"]
        k2 = 40
        merged, info = index_batch(w, rare, k2)
        assert 0 < info["union_rows"] < k2 and info["hit_rows"] >= info["union_rows"]
        got = sd.hybrid_search_batch(rare, k=k2)
        for j, q in enumerate(rare):
            assert len(got[j]) == k2 and same(got[j], singles(w, rare, k2)[j]), (j, q)
            assert same(got[j], br.top(q, w["emb"].vector(q), k2, 0.7, 0.3, w["live"], np.ones(N, bool))), (j, q)


def test_splits_inside_the_call_give_the_unsplit_lists_and_show_their_passes():
    w = world("bf16", "cosine", 1.0)
    queries = queries32() + ["w77 detector w78"]
    k = 10
    want, base = index_batch(w, queries, k)                                     # 33 queries: two sub-batches
    assert (base["sub_batches"], base["stats_passes"], base["score_passes"], base["scans"]) == (2, 2, 2, 2)
    assert base["union_rows"] > 1500 and base["pairs"] >= 32 * 1500
    texts_of = singles(w, queries, k)
    got = w["store"].hybrid_search_batch(queries, k=k)
    for j in range(33):
        assert same(got[j], texts_of[j]), j
    unsplit, one = index_batch(w, queries[:32], k)
    assert unsplit == want[:32]
    assert (one["sub_batches"], one["stats_passes"], one["score_passes"], one["scans"]) == (1, 1, 1, 1)
    try:
        # the pair budget below Q x |U|: the hit leg runs in query groups, the statistics pass and the scan stay shared
        budget = 5 * one["hit_rows"] + 3
        assert budget < 32 * one["hit_rows"]
        _lib.debug_set("AK_LEX_BATCH_PAIRS", str(budget))
        got, info = index_batch(w, queries[:32], k)
        assert got == unsplit
        assert (info["sub_batches"], info["stats_passes"], info["scans"], info["score_passes"]) == (1, 1, 1, 7)      # groups of 5 queries
        assert info["pairs"] == one["pairs"] and info["union_rows"] == one["union_rows"]
        _lib.debug_set("AK_LEX_BATCH_PAIRS", "1")                               # below |U| itself: one query at a time
        got, info = index_batch(w, queries[:8], k)
        assert got == unsplit[:8] and info["score_passes"] == 8 and info["stats_passes"] == 1 and info["scans"] == 1
        _lib.debug_set("AK_LEX_BATCH_PAIRS", None)
        # a union larger than the term table (forced down to 16 terms): sub-batches by terms; the 70-word query alone does not
        # fit and goes through the single-query passes
        _lib.debug_set("AK_LEX_BATCH_TERMS", "16")
        got, info = index_batch(w, queries[:32], k)
        assert got == unsplit
        assert info["sub_batches"] >= 3 and info["stats_passes"] == info["sub_batches"] + 1 == info["scans"]
    finally:
        _lib.debug_set("AK_LEX_BATCH_PAIRS", None)
        _lib.debug_set("AK_LEX_BATCH_TERMS", None)
    got, info = index_batch(w, queries[:32], k)
    assert got == unsplit and info["sub_batches"] == 1


def test_a_16_query_batch_is_one_statistics_pass_one_score_pass_and_one_scan():
    w = world("bf16", "cosine", 1.0)
    queries = queries32()[:16]
    ix = w["store"]._collection().index
    ix.profile(True)
    try:
        merged, info = index_batch(w, queries, 10)
    finally:
        ix.profile(False)
    assert min(info[s] for s in ("stats_ns", "score_ns", "hit_ns", "scan_ns")) > 0
    assert (info["stats_passes"], info["score_passes"], info["scans"], info["sub_batches"]) == (1, 1, 1, 1)
    assert info["n"] == int(w["live"].sum()) and info["hit_rows"] == info["union_rows"] + 1 and info["pairs"] == 16 * info["hit_rows"]
    assert info["own_hit_rows"] >= info["union_rows"] > 1500 and info["arena_entries"] > 6 * N * 0.9
    texts_of = singles(w, queries32(), 10)
    got = w["store"].hybrid_search_batch(queries, k=10)
    assert all(same(got[j], texts_of[j]) for j in range(16))


def test_batch_below_the_fast_path_and_on_an_empty_collection():
    emb = KeyEmb(DIM)
    sd = ArchiHipHybridVectorStore({"hip": {"dtype": "f32", "capacity": 512}}, emb, collection_name="lexb_small", bm25=DeviceBm25())
    queries = ["detector muon", "", "nosuchword", "w3 w17 detector", "muon"]
    assert sd.hybrid_search_batch(queries, k=5) == [[] for _ in queries]          # no collection yet
    texts, vec, metas = corpus6000()
    add_both((sd,), texts, vec, metas, 0, 300, per=PER)                            # 300 rows: the exact path serves the scan leg
    br = Brute(texts[:300], vec[:300], "cosine", "f32")
    live = np.ones(300, bool)
    got = sd.hybrid_search_batch(queries, k=7)
    for j, q in enumerate(queries):
        assert same(got[j], [(d.page_content, s) for d, s in sd.hybrid_search(q, k=7)]), q
        assert same(got[j], br.top(q, emb.vector(q), 7, 0.7, 0.3, live, live)), q
    for doc in range(1, 300 // PER + 1):                                           # every row deleted: the semantic fallback, empty
        sd.delete(document_id=doc)
    assert sd.hybrid_search_batch(queries, k=5) == [[] for _ in queries] == [sd.hybrid_search(q, k=5) for q in queries]


@pytest.mark.parametrize("coalesce", ["1", "0"])
def test_concurrent_hybrid_searches_equal_the_brute_force_of_a_state_the_collection_was_in(coalesce):
    """8 threads call hybrid_search (filtered: the mask pins one layout, as in the one-snapshot test of test_lexical_gpu.py) while a
    ninth adds and deletes the rows of another document. The collection is in one of two states; every answer must be the brute
    force of one of them. Whether calls were coalesced depends on arrival times and is not asserted (the native harness pins the
    grouping); with AK_COALESCE=0 every call runs alone and the answers obey the same rule."""
    n, extra, k = 5000, 50, 10
    texts, vec, metas = corpus6000()
    texts, vec, metas = texts[: n + extra], vec[: n + extra], [dict(m) for m in metas[: n + extra]]
    for i in range(n, n + extra):
        texts[i] = f"detector muon w3 visitor #{i}"
        metas[i] = {"source": "web"}
    emb = KeyEmb(DIM)
    sd = ArchiHipHybridVectorStore({"hip": {"dtype": "bf16", "capacity": 8192}}, emb, collection_name="lexb_race" + coalesce, bm25=DeviceBm25())
    add_both((sd,), texts, vec, metas, 0, n, per=PER)
    queries = [f"detector muon w{3 + j} visitor" for j in range(8)]
    br = Brute(texts, vec, "cosine", "bf16")
    web = np.array([m["source"] == "web" for m in metas])
    states = []
    for with_extra in (False, True):
        live = np.ones(n + extra, bool)
        live[n:] = with_extra
        states.append([br.top(q, emb.vector(q), k, 0.7, 0.3, live, web) for q in queries])
    assert states[0] != states[1]
    errors, searches = [], [0] * 8
    stop = threading.Event()

    def reader(j):
        try:
            while not stop.is_set():
                got = [(d.page_content, s) for d, s in sd.hybrid_search(queries[j], k=k, filter={"source": "web"})]
                ok = [len(got) == k and all(g[0] == w_[0] and (g[1] == w_[1] or (g[1] != g[1] and w_[1] != w_[1])) for g, w_ in zip(got, st[j]))
                      for st in states]
                assert any(ok), (j, got[:3], states[0][j][:3], states[1][j][:3])
                searches[j] += 1
        except Exception as e:      # noqa: BLE001
            errors.append(repr(e))
            stop.set()

    _lib.debug_set("AK_COALESCE", coalesce)
    try:
        threads = [threading.Thread(target=reader, args=(j,)) for j in range(8)]
        for t in threads:
            t.start()
        try:
            for cycle in range(12):
                sd.add_texts_batch([(texts[n:], [dict(m) for m in metas[n:]], 9000 + cycle, vec[n:])])
                while sum(searches) < 16 * (2 * cycle + 1) and not stop.is_set():
                    time.sleep(0.0005)
                assert sd.delete(document_id=9000 + cycle) is True
                while sum(searches) < 16 * (2 * cycle + 2) and not stop.is_set():
                    time.sleep(0.0005)
        finally:
            stop.set()
            for t in threads:
                t.join()
    finally:
        _lib.debug_set("AK_COALESCE", None)
    assert not errors, errors[:3]
    assert min(searches) > 0 and sum(searches) >= 16 * 24
    # afterwards: the first state again, through the batch call too
    got = sd.hybrid_search_batch(queries, k=k, filter={"source": "web"})
    assert all(same(got[j], states[0][j]) for j in range(8))


def test_a_batch_of_16_is_not_slower_than_16_single_calls():
    """60 000 rows x 128, warm: the median of 5 hybrid_search_batch calls of 16 distinct queries against the median of 5 loops of
    the 16 single hybrid_search calls (the single path is untouched by the batch call). batch <= loop is what makes the batch
    worth having; both times are printed."""
    n, dim = 60_000, 128
    rng = np.random.default_rng(12)
    vec = ko.gen_rows(616, 0, 0, n, dim, True, "f32")
    vocab = np.array([f"w{i}" for i in range(2000)])
    words = rng.integers(0, 2000, size=(n, 6))
    common = rng.random(n) < 0.3
    texts = [" ".join(vocab[words[i]]) + (" detector" if common[i] else "") + (" muon" if i % 977 == 0 else "") for i in range(n)]
    emb = KeyEmb(dim)
    sd = ArchiHipHybridVectorStore({"hip": {"dtype": "bf16", "capacity": 1 << 16}}, emb, collection_name="lexb_speed", bm25=DeviceBm25())
    for lo in range(0, n, 20000):
        sd.add_texts_batch([(texts[a: a + PER], [{"source": "web"} for _ in range(PER)], 1 + a // PER, vec[a: a + PER]) for a in range(lo, lo + 20000, PER)])
    queries = [f"detector w{i} w{i + 1000}" + (" muon" if i % 4 == 0 else "") for i in range(16)]

    def loop():
        return [sd.hybrid_search(q, k=10) for q in queries]

    def batch():
        return sd.hybrid_search_batch(queries, k=10)

    def median_ms(fn):
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3
    want, got = loop(), batch()                                                 # warm: lists attached, workspaces grown
    loop(), batch()
    for j in range(16):
        assert same(got[j], [(d.page_content, s) for d, s in want[j]]), j
    loop_ms, batch_ms = median_ms(loop), median_ms(batch)
    print(f"hybrid on {n} x {dim}, 16 distinct queries (30 % of the rows match 'detector'), medians of 5: 16 single calls {loop_ms:.2f} ms, "
          f"one batch call {batch_ms:.2f} ms ({loop_ms / batch_ms:.1f}x)")
    assert batch_ms <= loop_ms, (batch_ms, loop_ms)
