"""GPU suite of the device BM25 / hybrid query (csrc/lexical.hip, archi_amd/lexical.py). Every comparison is exact equality.

  - HipIndex.lex_scores / DeviceBm25.scores_arrays against HostBm25.scores_arrays on twin stores: the same hit positions and the
    same float64 bits, through growth, tombstone reclaim, deletes, compaction, a vacuum and an in-place text change;
  - hybrid_search with DeviceBm25 against the HostBm25 twin and against the reference's formula evaluated over ALL rows (scalar
    BM25 from scratch with math.log, the oracle's distances; postgres_vectorstore.py:435-457);
  - one writer against 8 readers; the 300k-chunk collection of test_store_scale_gpu.py, with the time of a warm query.
"""
import math
import re
import threading
import time

import numpy as np
import pytest

from archi_amd import vectorstore as vs
from archi_amd.lexical import DeviceBm25
from archi_amd.vectorstore import ArchiHipHybridVectorStore, HostBm25
from oracle import knn_oracle as ko
from tests import lexical_ref as lr

pytestmark = pytest.mark.gpu
TOK = re.compile(r"\w+")


@pytest.fixture(autouse=True)
def fresh(hip):
    vs.reset_collections()
    yield
    vs.reset_collections()


class Emb:
    """Queries embed to a fixed unit vector; a query that starts with 'zerovec' to the zero vector."""

    def __init__(self, dim, seed=99):
        self.q = ko.gen_rows(seed, 1, 0, 1, dim, True, "f32")[0]

    def embed_documents(self, texts):
        raise AssertionError("vectors are handed in")

    def vector(self, text):
        return np.zeros_like(self.q) if text.startswith("zerovec") else self.q

    def embed_query(self, text):
        return [float(x) for x in self.vector(text)]


def same(got, want):
    """== on (page_content, score), with NaN equal to NaN."""
    got = [(d.page_content, s) for d, s in got]
    assert len(got) == len(want), (len(got), len(want))
    for j, ((gt, gs), (wt, ws)) in enumerate(zip(got, want)):
        assert gt == wt and (gs == ws or (gs != gs and ws != ws)), (j, got[j], want[j])
    return True


class Brute:
    """The reference's formula over all rows: combined = (1.0 - distance) * w_s + COALESCE(bm25, 0) * w_b, ORDER BY combined DESC
    (NaN first), id; scalar BM25 from scratch, the oracle's distances on the stored values."""

    def __init__(self, texts, vec, metric, dtype, k1=1.2, b=0.75, sign=1.0):
        self.texts, self.metric, self.k1, self.b, self.sign = texts, metric, k1, b, sign
        self.stored = ko.round_through(np.asarray(vec, np.float32), dtype)
        self.toks = [TOK.findall(t.lower()) for t in texts]
        self._dist = {}

    def distances(self, qv):
        key = qv.tobytes()
        if key not in self._dist:
            self._dist[key] = np.array([ko.distance(self.metric, self.stored[i], qv) for i in range(len(self.texts))])
        return self._dist[key]

    def bm25(self, query, live):
        idx = np.flatnonzero(live)
        lens = np.array([len(self.toks[i]) for i in idx], np.float64)
        out = np.zeros(len(self.texts))
        if not len(idx):
            return out
        avg = int(lens.sum()) / len(idx)
        acc = np.zeros(len(idx))
        for w in dict.fromkeys(TOK.findall(query.lower())):
            tf = np.array([self.toks[i].count(w) for i in idx], np.float64)
            df = int((tf > 0).sum())
            if not df:
                continue
            idf = math.log(1.0 + (len(idx) - df + 0.5) / (df + 0.5))
            with np.errstate(invalid="ignore", divide="ignore"):
                c = idf * tf * (self.k1 + 1.0) / (tf + self.k1 * ((1.0 - self.b) + self.b * lens / avg))
            acc = acc + np.where(tf > 0, c, 0.0)
        hit = np.zeros(len(idx), bool)
        for w in set(TOK.findall(query.lower())):
            hit |= np.array([w in self.toks[i] for i in idx])
        out[idx] = np.where(hit, self.sign * acc, 0.0)
        return out

    def top(self, query, qv, k, ws, wb, live, allowed):
        d = self.distances(np.asarray(qv, np.float32))
        comb = (1.0 - d) * ws + self.bm25(query, live) * wb
        ids = np.flatnonzero(live & allowed)
        c = comb[ids]
        nan = c != c
        order = np.lexsort((ids, -np.where(nan, 0.0, c), ~nan))[:k]
        return [(self.texts[i], float(s)) for i, s in zip(ids[order].tolist(), c[order].tolist())]


def corpus(n, dim, seed, per=50):
    rng = np.random.default_rng(seed)
    vec = ko.gen_rows(seed, 0, 0, n, dim, True, "f32").copy()
    vocab = np.array([f"w{i}" for i in range(500)])
    words = rng.integers(0, 500, size=(n, 6))
    common = rng.random(n) < 0.3
    texts = [" ".join(vocab[words[i]]) + (" detector" if common[i] else "") + (" muon" if i % 397 == 0 else "") + f" #{i}" for i in range(n)]
    metas = [{"source": "git" if (i // per) % 4 == 0 else "web"} for i in range(n)]
    return texts, vec, metas


def twin_stores(dtype, metric, capacity, dim, sign=1.0, names=("lexh", "lexd")):
    emb = Emb(dim)
    hb, db = HostBm25(sign=sign), DeviceBm25(sign=sign)
    sh = ArchiHipHybridVectorStore({"hip": {"dtype": dtype, "capacity": capacity}}, emb, collection_name=names[0], distance_metric=metric, bm25=hb)
    sd = ArchiHipHybridVectorStore({"hip": {"dtype": dtype, "capacity": capacity}}, emb, collection_name=names[1], distance_metric=metric, bm25=db)
    return emb, hb, db, sh, sd


def add_both(stores, texts, vec, metas, lo, hi, per=50):
    for s in stores:
        s.add_texts_batch([(texts[a: min(a + per, hi)], [dict(m) for m in metas[a: min(a + per, hi)]], 1 + a // per, vec[a: min(a + per, hi)])
                           for a in range(lo, hi, per)])


def scores_equal(hb, db, sh, sd, queries):
    th, td = sh.table, sd.table
    db.use_index(sd._collection().index)
    for q in queries:
        hp, hs = hb.scores_arrays(q, th)
        dp, ds = db.scores_arrays(q, td)
        assert np.array_equal(hp, dp), (q[:40], len(hp), len(dp))
        assert np.array_equal(hs, ds) and ds.dtype == np.float64, (q[:40], np.flatnonzero(hs != ds)[:5])
        assert hb.scores(q, th) == db.scores(q, td)
    return True


def test_lex_scores_equal_host_bm25_through_growth_reclaim_deletes_compaction_and_text_changes():
    n, dim, per = 20000, 64, 50
    more = 14000
    texts, vec, metas = corpus(n + more, dim, 21)
    rng = np.random.default_rng(5)
    long_q = " ".join(f"w{i}" for i in rng.permutation(500)[:199].tolist()) + " detector"
    queries = ["detector muon", "w3 w3 w17 nosuchword w3", "muon", "nosuchword", "", long_q, "again detector"]
    for sign in (1.0, -1.0):
        vs.reset_collections()
        emb, hb, db, sh, sd = twin_stores("f32", "cosine", 4096, dim, sign=sign)       # small first reservation: the buffers grow
        add_both((sh, sd), texts, vec, metas, 0, n)
        ix = sd._collection().index
        assert ix.allocated_rows >= n > 4096
        assert scores_equal(hb, db, sh, sd, queries)                                    # 20 000 rows, the 200-term query among them
        info = ix.lex_info()
        assert info["rows_attached"] == n and info["entries"] > 6 * n * 0.9 and info["arena_bytes"] >= 8 * info["entries"]
        if sign < 0:
            continue                                                                    # the lifecycle below once
        # deletes
        for s in (sh, sd):
            for doc in (3, 4, 77, 200, 201, 202):
                assert s.delete(document_id=doc) is True
        assert scores_equal(hb, db, sh, sd, queries)
        assert ix.lex_info()["rows_attached"] == n - 6 * per
        # adds that do not fit: tombstones are reclaimed or the buffers grow, and slots are renumbered
        for s in (sh, sd):
            for doc in range(1, 120):
                s.delete(document_id=doc)
        slots0, epoch0 = ix.layout()
        dead = slots0 - ix.count()
        assert dead > slots0 // 8 and ix.allocated_rows - slots0 < more           # the add below does not fit: tombstones are reclaimed
        add_both((sh, sd), texts, vec, metas, n, n + more)
        slots1, epoch1 = ix.layout()
        assert epoch1 != epoch0 and slots1 == slots0 - dead + more == ix.count()
        assert scores_equal(hb, db, sh, sd, queries)
        # the 70 000-repeat row and an empty text
        for s in (sh, sd):
            s.add_texts(["again " * 70000, "", "... !!!"], [{"source": "web"} for _ in range(3)], document_id=9000,
                        embeddings=ko.gen_rows(8, 3, 0, 3, dim, True, "f32"))
        assert scores_equal(hb, db, sh, sd, queries)
        hp, hs = db.scores_arrays("again", sd.table)
        assert len(hp) == 1 and hs[0] != 0.0
        # compaction: the arena shrinks to the live rows' entries
        for s in (sh, sd):
            s.delete(document_id=300)
        before = ix.lex_info()
        live_entries = sum(len(set(TOK.findall(sd.table.text_at(p).lower()))) for p in np.flatnonzero(sd.table._alive[: sd.table.positions]).tolist())
        assert before["entries"] > live_entries
        for s in (sh, sd):
            with s.table.lock:
                s._collection().index.compact()
        after = ix.lex_info()
        assert after["entries"] == live_entries and after["rows_attached"] == len(sd.table) == ix.count() == ix.slots
        assert after["arena_bytes"] < before["arena_bytes"] and 8 * live_entries <= after["arena_bytes"] <= 8 * (live_entries + ix.slots)
        assert scores_equal(hb, db, sh, sd, queries)
        # a text changed in place, then a vacuum of the table: text_epoch starts the lists over
        gen0 = ix.lex_info()["generation"]
        for s in (sh, sd):
            s.table.update_row(int(s.table.live_rids()[5]), text="muon muon rewritten in place detector")
        assert scores_equal(hb, db, sh, sd, queries)
        assert ix.lex_info()["generation"] != gen0
        for s in (sh, sd):
            s.table.vacuum()
        assert scores_equal(hb, db, sh, sd, queries)
        # the scorer lives on while the store object is re-created per request; lists that are not the scorer's are replaced
        sd2 = ArchiHipHybridVectorStore({"hip": {"dtype": "f32", "capacity": 4096}}, emb, collection_name="lexd", bm25=db)
        assert scores_equal(hb, db, sh, sd2, queries[:3])
        other = DeviceBm25()
        assert scores_equal(HostBm25(), other, sh, sd2, queries[:3])
        assert scores_equal(hb, db, sh, sd2, queries[:3])


def test_lex_attach_contract_and_direct_lists():
    """The C ABI below the scorer: lists attached directly, held to the doc-major reference; errors attach nothing."""
    from archi_amd import HipBackendError
    from archi_amd.index import HipIndex
    rng = np.random.default_rng(9)
    n, dim = 6000, 64
    ix = HipIndex(dim, 1024, dtype="bf16", metric="cosine")
    ids = (np.arange(n, dtype=np.int64) * 3 + 11)
    ix.add(ko.gen_rows(4, 0, 0, n, dim, True, "f32"), ids=ids)
    lists = [np.unique(rng.integers(6, 2_000_000_000, size=int(c))) for c in rng.integers(0, 150, size=n)]
    lists[7] = lists[7][:1] if len(lists[7]) else np.array([9])
    cnt = np.array([len(x) for x in lists])
    ro = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    terms = np.concatenate(lists).astype(np.int32)
    terms[ro[7]] = 2_147_483_647                                           # the largest term id
    shared = rng.choice(n, size=2500, replace=False)                       # a term many rows hold: put 5 at the front of their lists
    for r in shared.tolist():
        if cnt[r]:
            terms[ro[r]] = 5
    tfs = rng.integers(1, 9, size=len(terms)).astype(np.int32)
    tfs[ro[7]] = 70000
    dl = np.array([int(tfs[ro[r]: ro[r + 1]].sum()) for r in range(n)], np.int32)
    ix.lex_clear(41)
    with pytest.raises(HipBackendError, match="generation"):
        ix.lex_attach(ids, ro, terms, tfs, dl, 40)
    bad = ids.copy()
    bad[-1] = 5                                                            # an unknown id: nothing is attached
    with pytest.raises(HipBackendError, match="not a live row"):
        ix.lex_attach(bad, ro, terms, tfs, dl, 41)
    unsorted = terms.copy()
    r2 = int(np.flatnonzero(cnt >= 2)[0])
    unsorted[ro[r2]: ro[r2] + 2] = unsorted[ro[r2]: ro[r2] + 2][::-1]
    with pytest.raises(HipBackendError, match="ascend"):
        ix.lex_attach(ids, ro, unsorted, tfs, dl, 41)
    assert ix.lex_info() == {"generation": 41, "rows_attached": 0, "entries": 0, "arena_bytes": 0}
    half = n // 2
    ix.lex_attach(ids[:half], ro[: half + 1], terms[: ro[half]], tfs[: ro[half]], dl[:half], 41)
    ix.lex_attach(ids[half:], ro[half:] - ro[half], terms[ro[half]:], tfs[ro[half]:], dl[half:], 41)
    assert ix.lex_info()["rows_attached"] == n and ix.lex_info()["entries"] == len(terms)
    ix.remove(ids[100:400])
    alive = np.ones(n, bool)
    alive[100:400] = False
    some = terms[ro[2000]: ro[2000] + 3].tolist() + terms[ro[4000]: ro[4000] + 2].tolist()
    for q, k1, b, sign in (([5], 1.2, 0.75, 1.0), ([2_147_483_647, 5, 5], 1.2, 0.75, -1.0), (some + [5, 123], 0.9, 0.4, 1.0), ([123456], 1.2, 0.75, 1.0)):
        bm, hit, info = ix.lex_scores(q, k1, b, sign)
        rows, sc = lr.doc_major_scores(ro, terms, tfs, dl, alive, q, k1, b, sign)
        slots = ix.lookup(ids[rows])
        assert np.array_equal(np.sort(slots), np.flatnonzero(hit)) and np.array_equal(bm[slots], sc), q
        assert info["n"] == n - 300 and info["sum_len"] == int(dl[alive].sum()) and info["hits"] == len(rows)
        assert not bm[hit == 0].any()
    # avg == 0: every length 0 with lists present -- the length term drops out of the norm
    ix.lex_clear(42)
    zero = np.zeros(n, np.int32)
    live_ids = ids[alive]
    keep = np.flatnonzero(alive)
    ro2 = np.concatenate([[0], np.cumsum(cnt[keep])]).astype(np.int64)
    t2 = np.concatenate([terms[ro[r]: ro[r + 1]] for r in keep.tolist()])
    f2 = np.concatenate([tfs[ro[r]: ro[r + 1]] for r in keep.tolist()])
    ix.lex_attach(live_ids, ro2, t2, f2, zero[: len(keep)], 42)
    bm, hit, info = ix.lex_scores([5], 1.2, 0.75, 1.0)
    rows, sc = lr.doc_major_scores(ro2, t2, f2, zero[: len(keep)], np.ones(len(keep), bool), [5])
    slots = ix.lookup(live_ids[rows])
    assert info["sum_len"] == 0 and len(rows) > 1000 and np.array_equal(bm[slots], sc) and np.array_equal(np.sort(slots), np.flatnonzero(hit))
    ix.close()


@pytest.mark.parametrize("dtype,metric", [("f32", "cosine"), ("bf16", "cosine"), ("f32", "l2"), ("bf16", "l2"), ("f32", "inner_product"),
                                          ("bf16", "inner_product")])
def test_hybrid_search_device_equals_host_twin_and_the_formula_over_all_rows(dtype, metric):
    n, dim, per, k = 20000, 64, 50, 10
    texts, vec, metas = corpus(n, dim, 33)
    vec[397 * 3] = 0.0                     # a zero-vector row that is a BM25 hit ('muon') ...
    vec[1001] = 0.0                        # ... and one that is not: both NaN under cosine, ranked first
    assert "muon" in texts[397 * 3] and "muon" not in texts[1001] and "detector" not in texts[1001]
    emb, hb, db, sh, sd = twin_stores(dtype, metric, n, dim)
    add_both((sh, sd), texts, vec, metas, 0, n)
    soft = 1 + 397 * 6 // per                                                # the document of a 'muon' row
    for s in (sh, sd):
        s.table.register_document(soft, is_deleted=True)
    br = Brute(texts, vec, metric, dtype)
    live = np.ones(n, bool)
    everything = np.ones(n, bool)
    git = np.array([m["source"] == "git" for m in metas])
    not_soft = np.ones(n, bool)
    not_soft[(soft - 1) * per: soft * per] = False

    def check(query, kk, ws, wb, kwargs, allowed):
        got_d = sd.hybrid_search(query, k=kk, semantic_weight=ws, bm25_weight=wb, **kwargs)
        got_h = sh.hybrid_search(query, k=kk, semantic_weight=ws, bm25_weight=wb, **kwargs)
        want = br.top(query, emb.vector(query), kk, ws, wb, live, allowed)
        assert same(got_d, [(d.page_content, s) for d, s in got_h]), (query, ws, wb, kwargs)
        assert same(got_d, want), (query, ws, wb, kwargs)
        return got_d

    for ws, wb in ((0.7, 0.3), (0.5, 0.5), (1.0, 0.0), (0.0, 1.0)):
        for kwargs, allowed in (({}, not_soft), ({"filter": {"source": "git"}}, git & not_soft), ({"include_deleted": True}, everything),
                                ({"filter": {"source": "web"}, "include_deleted": True}, ~git)):
            got = check("detector muon", k, ws, wb, kwargs, allowed)
            if metric == "cosine" and "filter" not in kwargs:
                assert [s != s for _, s in got[:2]] == [True, True] and got[0][0].page_content == texts[1001] and got[2][1] == got[2][1]
    few = check("muon", 100, 0.7, 0.3, {"filter": {"source": "git"}}, git & not_soft)          # k larger than the number of hits
    assert len(few) == 100 and sum("muon" in d.page_content for d, _ in few) < 30
    check("nosuchword", k, 0.7, 0.3, {}, not_soft)                                               # no hit at all: the scan leg alone
    check("zerovec detector", k, 0.7, 0.3, {}, not_soft)                                         # a zero query vector
    check("zerovec detector", k, 0.5, 0.5, {"filter": {"source": "git"}}, git & not_soft)
    # rows leave and arrive between queries
    for s in (sh, sd):
        s.delete(document_id=2)
    live[per: 2 * per] = False
    check("detector muon", k, 0.7, 0.3, {}, not_soft)
    check("w3 w17 detector", 50, 0.5, 0.5, {"filter": {"source": "git"}}, git & not_soft)


def test_hybrid_search_on_an_empty_collection_and_with_sign():
    dim = 64
    emb, hb, db, sh, sd = twin_stores("f32", "cosine", 4096, dim, sign=-1.0)
    assert sd.hybrid_search("detector", k=5) == [] == sh.hybrid_search("detector", k=5)         # no collection yet
    texts, vec, metas = corpus(6000, dim, 44)
    add_both((sh, sd), texts, vec, metas, 0, 6000)
    br = Brute(texts, vec, "cosine", "f32", sign=-1.0)
    live = np.ones(6000, bool)
    for ws, wb in ((0.7, 0.3), (0.2, 0.8)):
        got = sd.hybrid_search("detector muon w5", k=12, semantic_weight=ws, bm25_weight=wb)
        assert same(got, [(d.page_content, s) for d, s in sh.hybrid_search("detector muon w5", k=12, semantic_weight=ws, bm25_weight=wb)])
        assert same(got, br.top("detector muon w5", emb.q, 12, ws, wb, live, live))
    for s in (sh, sd):                                                                           # every row deleted: the semantic fallback, empty
        for doc in range(1, 6000 // 50 + 1):
            s.delete(document_id=doc)
    assert sd.hybrid_search("detector", k=5) == [] == sh.hybrid_search("detector", k=5)


def test_filtered_hybrid_readers_see_one_snapshot_while_a_writer_moves_the_index():
    """One writer (add batches, delete documents, soft-delete, one compaction) against 8 readers calling a filtered hybrid_search
    with the device scorer: no exception, no chunk of a filtered-out document, none of a document soft-deleted or deleted before
    the search started."""
    rng = np.random.default_rng(5)
    d = 64
    queries = ko.gen_rows(17, 1, 0, 8, d, True, "f32")

    class QEmb:
        def embed_documents(self, texts):
            raise AssertionError("vectors are handed in")

        def embed_query(self, text):
            return [float(x) for x in queries[int(text.rsplit("q", 1)[1])]]

    s = ArchiHipHybridVectorStore({"hip": {"dtype": "f32", "capacity": 512}}, QEmb(), collection_name="lexrace", bm25=DeviceBm25())
    state, gone_docs = {}, set()
    lock = threading.Lock()

    def ingest(doc, kind, n):
        x = rng.standard_normal((n, d)).astype(np.float32)
        s.add_texts([f"{kind} {doc} {i} detector" if i % 2 else f"{kind} {doc} {i} tracker w{i}" for i in range(n)],
                    metadatas=[{"source": kind, "doc": doc} for _ in range(n)], document_id=doc, embeddings=x / np.linalg.norm(x, axis=1, keepdims=True))
        state[doc] = kind

    for doc in range(40):
        ingest(doc, "web" if doc % 2 else "git", 60)
    stop = threading.Event()
    errors, searches = [], [0]

    def reader(j):
        try:
            while not stop.is_set():
                with lock:
                    gone_before = set(gone_docs)
                res = s.hybrid_search(f"detector tracker w3 q{j}", k=10, filter={"source": "web"})
                for doc_, _ in res:
                    assert doc_.metadata["source"] == "web", f"filtered-out chunk returned: {doc_.page_content!r}"
                    assert doc_.metadata["doc"] not in gone_before, f"chunk of a deleted document {doc_.metadata['doc']} returned"
                assert len(res) == 10
                searches[0] += 1
        except Exception as e:      # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=reader, args=(j,)) for j in range(8)]
    for t in threads:
        t.start()
    nxt = 40
    try:
        for cycle in range(40):
            ingest(nxt, "web" if cycle % 3 else "git", 50); nxt += 1
            if cycle % 4 == 1:
                victim = int(rng.choice(sorted(state)))
                s.delete(document_id=victim); del state[victim]
                with lock:
                    gone_docs.add(victim)
            if cycle % 5 == 2:
                web = [x for x in sorted(state) if state[x] == "web" and x not in gone_docs]
                if len(web) > 6:
                    sdel = int(rng.choice(web))
                    s.table.register_document(sdel, is_deleted=True)
                    with lock:
                        gone_docs.add(sdel)
            if cycle == 20:
                with s.table.lock:
                    s._collection().index.compact()
            time.sleep(0.002)
    finally:
        stop.set()
        for t in threads:
            t.join()
    assert not errors, errors[:3]
    assert searches[0] > 50
    # afterwards: every live row has its list, and the answer is the host scorer's on the same table
    res = s.hybrid_search("detector tracker w3 q0", k=10, filter={"source": "web"})
    assert s._collection().index.lex_info()["rows_attached"] == len(s.table)
    s._bm25 = HostBm25()
    assert same(res, [(d_.page_content, sc) for d_, sc in s.hybrid_search("detector tracker w3 q0", k=10, filter={"source": "web"})])


def test_hybrid_search_on_the_large_collection_equals_brute_force_and_halves_the_host_time():
    """The 300k-chunk collection of test_store_scale_gpu.py (same seeds and texts; a query word matches a third of it). Answers equal
    the brute force before and after 5 000 more rows and a document delete; the warm device query against the warm HostBm25 query
    on the twin store, medians of 20 after 3 warm-ups, in this process: device <= host / 2. The host path makes at least six passes
    over the ~100 k hits and uploads an 800 KB id list and a 300 KB mask per query; none of that is left on the device path. Both
    medians are printed before the assertion."""
    n, dim, per = 300_000, 64, 50
    rng = np.random.default_rng(11)
    vec = ko.gen_rows(515, 0, 0, n + 5000, dim, True, "f32")
    vocab = np.array([f"w{i}" for i in range(2000)])
    common = rng.random(n + 5000) < 0.33
    words = rng.integers(0, 2000, size=(n + 5000, 6))
    texts = [" ".join(vocab[words[i]]) + (" detector" if common[i] else "") + (" muon" if i % 977 == 0 else "") for i in range(n + 5000)]
    emb = Emb(dim)
    hb, db = HostBm25(), DeviceBm25()
    sh = ArchiHipHybridVectorStore({"hip": {"dtype": "f32", "capacity": 1 << 19}}, emb, collection_name="hyh", bm25=hb)
    sd = ArchiHipHybridVectorStore({"hip": {"dtype": "f32", "capacity": 1 << 19}}, emb, collection_name="hyd", bm25=db)
    for store in (sh, sd):
        for lo in range(0, n, 20000):
            store.add_texts_batch([(texts[a: a + per], [{"source": "web" if (a // per) % 4 else "git"} for _ in range(per)], 1 + a // per, vec[a: a + per])
                                   for a in range(lo, lo + 20000, per)])
    toks = [TOK.findall(t.lower()) for t in texts]
    dist = np.array([ko.distance("cosine", vec[i], emb.q) for i in range(n + 5000)])

    def brute(query, k, ws, wb, live, allowed):
        idx = np.flatnonzero(live)
        lens = np.array([len(toks[i]) for i in idx], np.float64)
        avg = int(lens.sum()) / len(idx)
        bmv = np.zeros(len(idx))
        for w in dict.fromkeys(TOK.findall(query.lower())):
            tf = np.array([toks[i].count(w) for i in idx], np.float64)
            df = int((tf > 0).sum())
            if not df:
                continue
            idf = math.log(1.0 + (len(idx) - df + 0.5) / (df + 0.5))
            c = idf * tf * (1.2 + 1.0) / (tf + 1.2 * ((1.0 - 0.75) + 0.75 * lens / avg))
            bmv = bmv + np.where(tf > 0, c, 0.0)
        comb = (1.0 - dist[idx]) * ws + bmv * wb
        ok = allowed[idx]
        order = np.lexsort((idx[ok], -comb[ok]))[:k]
        return [(texts[i], float(c)) for i, c in zip(idx[ok][order].tolist(), comb[ok][order].tolist())]

    live = np.zeros(n + 5000, bool)
    live[:n] = True
    everything = np.ones(n + 5000, bool)
    git = np.array([((a // per) % 4) == 0 for a in range(n + 5000)])
    t0 = time.perf_counter()
    first = sd.hybrid_search("detector muon", k=10)                     # attaches the lists of the 300k rows
    first_s = time.perf_counter() - t0
    sh.hybrid_search("detector muon", k=10)
    assert same(sd.hybrid_search("detector muon", k=10, semantic_weight=0.7, bm25_weight=0.3), brute("detector muon", 10, 0.7, 0.3, live, everything))
    assert same(first, brute("detector muon", 10, 0.7, 0.3, live, everything))
    assert same(sd.hybrid_search("detector muon", k=10, semantic_weight=0.5, bm25_weight=0.5, filter={"source": "git"}),
                brute("detector muon", 10, 0.5, 0.5, live, git))

    def median_ms(store):
        for _ in range(3):
            store.hybrid_search("detector muon", k=10)
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            store.hybrid_search("detector muon", k=10)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3

    host_ms, dev_ms = median_ms(sh), median_ms(sd)
    print(f"hybrid on {n} chunks (a third match 'detector'): first device query incl. list attach {first_s:.1f} s; warm query, median of 20: "
          f"HostBm25 {host_ms:.2f} ms, DeviceBm25 {dev_ms:.2f} ms ({host_ms / dev_ms:.1f}x)")
    # more rows arrive, a document leaves: the lists follow without starting over
    gen = sd._collection().index.lex_info()["generation"]
    for store in (sh, sd):
        store.add_texts_batch([(texts[n: n + 5000], [{"source": "web" if (x // per) % 4 else "git"} for x in range(n, n + 5000)], 900_000, vec[n: n + 5000])])
        store.delete(document_id=1 + 977 * 3 // per)
    live[n:] = True
    d0 = (977 * 3 // per) * per
    live[d0: d0 + per] = False
    got = sd.hybrid_search("detector muon", k=10, semantic_weight=0.7, bm25_weight=0.3)
    assert same(got, brute("detector muon", 10, 0.7, 0.3, live, everything))
    assert same(got, [(d.page_content, s) for d, s in sh.hybrid_search("detector muon", k=10, semantic_weight=0.7, bm25_weight=0.3)])
    assert sd._collection().index.lex_info()["generation"] == gen
    assert dev_ms <= host_ms / 2, (dev_ms, host_ms)
