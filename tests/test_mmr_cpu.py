"""CPU suite of the max-marginal-relevance search: the ABI entry point exists, the reference restatement (tests/mmr_ref.py) agrees
with an independent restatement of LangChain's published helper and has the contract's properties, and the store's host logic
(ArchiHipVectorStore.max_marginal_relevance_search*) on an oracle-backed index."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from archi_amd import vectorstore as vs
from archi_amd.vectorstore import ArchiHipVectorStore
from oracle import knn_oracle as ko
from tests.fake_index import OracleIndex
from tests.mmr_ref import MmrOracleIndex, mmr_search_ref, mmr_select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def fresh():
    vs.reset_collections()
    yield
    vs.reset_collections()


# ---- ABI -------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_exported():
    import __graft_entry__ as ge
    ge.build()
    from archi_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    assert re.search(r"\bint ak_index_mmr_search\s*\(", hdr)
    assert "ak_index_mmr_search" in {name for name, _, _ in _lib.SYMBOLS}
    so = os.path.join(ROOT, "archi_amd", "lib", "libarchi_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert re.search(r"\bT ak_index_mmr_search\b", exported)
    assert _lib.load().ak_abi_version() == 5 == _lib.ABI_VERSION


def test_mmr_kernels_have_no_spills_and_no_scratch():
    from scripts.kernel_resources import HIPCC, kernel_resources
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    keys = ("SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]")
    seen = {name: {key: use[key] for key in keys if key in use} for name, use in kernel_resources("mmr.hip").items()}
    assert sum("k_mmr_gram" in n for n in seen) == 3 and sum("k_mmr_select" in n for n in seen) == 1 and len(seen) == 4, sorted(seen)
    for n, res in seen.items():
        assert len(res) == 3 and all(v == 0 for v in res.values()), (n, res)


# ---- mmr_ref against LangChain's helper, restated independently --------------------------------
def _langchain_mmr(query, cands, lam, k):
    """maximal_marginal_relevance of langchain_core.vectorstores.utils as published [upstream, not in tree], in numpy float64:
    cosine similarities by matrix product, first pick = argmax similarity to the query, then argmax of
    lam * sim_to_query - (1 - lam) * max sim to the selected. Also returns the smallest gap between the best and the second-best
    score over all steps."""
    q = np.asarray(query, np.float64)
    x = np.asarray(cands, np.float64)
    xn = x / np.linalg.norm(x, axis=1, keepdims=True)
    sim_q = xn @ (q / np.linalg.norm(q))
    gram = xn @ xn.T
    order = np.sort(sim_q)[::-1]
    margin = order[0] - order[1]
    picked = [int(np.argmax(sim_q))]
    while len(picked) < min(k, len(x)):
        score = lam * sim_q - (1.0 - lam) * gram[:, picked].max(axis=1)
        score[picked] = -np.inf
        top = np.sort(score)[::-1]
        margin = min(margin, top[0] - top[1])
        picked.append(int(np.argmax(score)))
    return picked, margin


@pytest.mark.parametrize("seed,n,dim,k,lam", [(1, 24, 16, 6, 0.5), (2, 40, 32, 8, 0.25), (3, 16, 8, 5, 0.75), (4, 30, 24, 10, 0.0),
                                              (5, 20, 16, 4, 1.0), (6, 64, 48, 12, 0.6)])
def test_reference_agrees_with_langchains_helper(seed, n, dim, k, lam):
    rows = ko.gen_rows(seed, 0, 0, n, dim, True, "f32")
    q = ko.gen_rows(seed, 1, 0, 1, dim, True, "f32")[0]
    ids = np.arange(100, 100 + n)
    gi, gd, gc, gr = mmr_search_ref(rows, ids, None, q, k, n, lam)
    ci, _, _ = ko.search(rows, q[None], n, "cosine", ids=ids)           # the candidates in rank order
    want, margin = _langchain_mmr(q, rows[ci[0] - 100], lam, k)
    assert margin > 1e-4, margin        # float32-chain vs float64-BLAS similarities differ by ~1e-7: no step is a coin toss
    assert gr[0].tolist() == want and gc[0] == k
    assert gi[0].tolist() == ci[0][want].tolist()


# ---- properties of the reference --------------------------------------------------------------
def _corpus(seed, n, dim):
    return ko.gen_rows(seed, 0, 0, n, dim, True, "f32"), ko.gen_rows(seed, 1, 0, 3, dim, True, "f32")


def test_lambda_one_is_the_plain_topk():
    rows, q = _corpus(11, 50, 16)
    ids = np.arange(50) * 3
    gi, gd, gc, gr = mmr_search_ref(rows, ids, None, q, 7, 20, 1.0)
    oi, od, _ = ko.search(rows, q, 7, "cosine", ids=ids)
    assert np.array_equal(gi, oi) and np.array_equal(gd, od) and gr.tolist() == [list(range(7))] * 3 and gc.tolist() == [7] * 3


def test_copies_are_spread_over_distinct_groups():
    base, q = _corpus(12, 16, 32)
    rows = np.repeat(base, 8, axis=0)                                  # 8 identical copies of each of 16 distinct rows
    ids = np.arange(128)
    plain, _, _ = ko.search(rows, q, 8, "cosine", ids=ids)
    gi, _, gc, _ = mmr_search_ref(rows, ids, None, q, 8, 128, 0.5)
    for qi in range(3):
        assert len(set((plain[qi] // 8).tolist())) == 1               # the plain top 8 is one paragraph eight times
        assert gc[qi] == 8 and len(set((gi[qi] // 8).tolist())) == 8


def test_ties_go_to_the_lower_rank():
    # four candidates: rank 0, then two identical rows (ranks 1 and 2: equal dq, equal similarity to every row), then another
    e = np.eye(4, dtype=np.float32)
    rows = np.stack([e[0], e[0] * 0.6 + e[1] * 0.8, e[0] * 0.6 + e[1] * 0.8, e[0] * 0.5 + e[2]])
    dq = [ko.distance("cosine", r, e[0]) for r in rows]
    assert dq[1] == dq[2]
    for lam in (0.0, 0.3, 1.0):
        picks = mmr_select(rows, dq, 4, lam)
        assert picks.index(1) < picks.index(2), (lam, picks)


def test_a_nan_candidate_is_picked_after_every_finite_one():
    rows, q = _corpus(13, 6, 8)
    rows[2] = 0.0                                                       # zero row: NaN distance to everything
    gi, gd, gc, gr = mmr_search_ref(rows, np.arange(6), None, q[:1], 6, 6, 0.5)
    assert gc[0] == 6 and gi[0, 5] == 2 and math.isnan(gd[0, 5]) and gr[0, 5] == 5      # ranked last, picked last
    assert not np.isnan(gd[0, :5]).any()
    # and with two of them: the lower rank (the lower id) first
    rows[4] = 0.0
    gi, gd, _, _ = mmr_search_ref(rows, np.arange(6), None, q[:1], 6, 6, 0.5)
    assert gi[0, 4:].tolist() == [2, 4] and np.isnan(gd[0, 4:]).all() and not np.isnan(gd[0, :4]).any()


def test_fewer_candidates_than_k_pads():
    rows, q = _corpus(14, 5, 8)
    alive = np.array([1, 1, 0, 1, 0], np.uint8)
    gi, gd, gc, gr = mmr_search_ref(rows, np.arange(5), alive, q, 4, 10, 0.5)
    assert gc.tolist() == [3, 3, 3] and (gi[:, 3] == -1).all() and np.isnan(gd[:, 3]).all() and (gr[:, 3] == -1).all()
    assert all(set(r[:3].tolist()) == {0, 1, 3} for r in gi)
    ei, ed, ec, er = mmr_search_ref(np.zeros((0, 8), np.float32), np.zeros(0, np.int64), None, q, 4, 10, 0.5)
    assert ec.tolist() == [0, 0, 0] and (ei == -1).all() and np.isnan(ed).all() and (er == -1).all()


# ---- the store on the oracle-backed index ------------------------------------------------------
DIM = 16


class TextEmb:
    """One vector per distinct text: copies of a text are copies of a row."""

    @staticmethod
    def _vec(text):
        return [float(x) for x in ko.gen_rows(77, 5, sum(text.encode()) * 131 + len(text), 1, DIM, True, "f32")[0]]

    def embed_documents(self, texts):
        return [self._vec(t) for t in texts]

    def embed_query(self, text):
        return self._vec(text)


def mmr_factory(dim, capacity, dtype, metric, shards=1):
    return MmrOracleIndex(dim, capacity, dtype=dtype, metric=metric)


def plain_factory(dim, capacity, dtype, metric, shards=1):
    return OracleIndex(dim, capacity, dtype=dtype, metric=metric)


def _store(factory=mmr_factory, metric="cosine", name="mmr"):
    return ArchiHipVectorStore({"hip": {"dtype": "f32"}}, TextEmb(), collection_name=name, distance_metric=metric, index_factory=factory)


TEXTS = [f"paragraph {i // 4}" for i in range(24)] + [f"note {i}" for i in range(12)]      # six paragraphs four times, twelve notes


def test_store_returns_documents_and_scores_in_pick_order():
    s = _store()
    s.add_texts(TEXTS, metadatas=[{"n": i} for i in range(len(TEXTS))])
    col = s._collection()
    # a query (not a text of the corpus) whose nearest chunk is one of the four-fold paragraphs
    q = next(c for c in (f"question {i}" for i in range(50)) if s.similarity_search(c, k=1)[0].page_content.startswith("paragraph"))
    top = s.similarity_search(q, k=1)[0].page_content
    qv = np.asarray(TextEmb().embed_query(q), np.float32)
    ids, dist, cnt = col.index.mmr_search(qv[None], 4, fetch_k=20, lambda_mult=0.5)
    assert cnt[0] == 4
    want = [(col.table.text_at(col.table.pos(int(i))), 1.0 - float(d)) for i, d in zip(ids[0], dist[0])]
    got = s.max_marginal_relevance_search_by_vector_with_score(qv.tolist(), k=4, fetch_k=20, lambda_mult=0.5)
    assert [(d.page_content, sc) for d, sc in got] == want
    assert [d.page_content for d in s.max_marginal_relevance_search(q, k=4, fetch_k=20, lambda_mult=0.5)] == [t for t, _ in want]
    assert [d.page_content for d in s.max_marginal_relevance_search_by_vector(qv.tolist(), k=4)] == [t for t, _ in want]
    # what the feature is for: the plain top 4 is one paragraph four times, the MMR answer holds it once
    assert [d.page_content for d in s.similarity_search(q, k=4)] == [top] * 4
    assert got[0][0].page_content == top and len({d.page_content for d, _ in got}) == 4
    # lambda_mult = 1: the plain search, scores included
    plain = s.similarity_search_with_score(q, k=4)
    same = s.max_marginal_relevance_search_by_vector_with_score(qv.tolist(), k=4, fetch_k=20, lambda_mult=1.0)
    assert [(d.page_content, d.metadata, sc) for d, sc in same] == [(d.page_content, d.metadata, sc) for d, sc in plain]


def test_store_filter_and_include_deleted():
    s = _store()
    s.add_texts(TEXTS[:24], metadatas=[{"source": "web" if i % 2 else "git"} for i in range(24)], document_id=1)
    s.add_texts(TEXTS[24:], metadatas=[{"source": "web"} for _ in TEXTS[24:]], document_id=2)
    col, qv = s._collection(), np.asarray(TextEmb().embed_query("note 3"), np.float32)
    t = col.table

    def expect(mask):
        ids, dist, cnt = col.index.mmr_search(qv[None], 5, fetch_k=20, lambda_mult=0.5, row_filter=mask)
        return [(t.text_at(t.pos(int(i))), 1.0 - float(d)) for i, d in zip(ids[0, :cnt[0]], dist[0, :cnt[0]])]

    web = s.max_marginal_relevance_search_by_vector_with_score(qv.tolist(), k=5, filter={"source": "web"})
    assert len(web) == 5 and all(d.metadata["source"] == "web" for d, _ in web)
    mask = s._where(col, {"source": "web"}, False)[0]
    assert mask is not None and [(d.page_content, sc) for d, sc in web] == expect(mask)
    t.register_document(2, is_deleted=True)                           # soft delete: the notes leave the answer ...
    gone = s.max_marginal_relevance_search_by_vector_with_score(qv.tolist(), k=5)
    assert len(gone) == 5 and not any(d.page_content.startswith("note") for d, _ in gone)
    assert [(d.page_content, sc) for d, sc in gone] == expect(s._where(col, {}, False)[0])
    back = s.max_marginal_relevance_search_by_vector_with_score(qv.tolist(), k=5, include_deleted=True)      # ... unless asked for
    assert back[0][0].page_content == "note 3" and [(d.page_content, sc) for d, sc in back] == expect(None)


def test_store_raises_fetch_k_to_k_and_refuses_by_name():
    s = _store()
    s.add_texts(TEXTS)
    col = s._collection()
    seen, orig = [], col.index.mmr_search

    def spy(queries, k, **kw):
        seen.append((k, kw["fetch_k"], kw["lambda_mult"]))
        return orig(queries, k, **kw)
    col.index.mmr_search = spy
    assert len(s.max_marginal_relevance_search("note 1", k=9, fetch_k=3, lambda_mult=0.25)) == 9
    assert seen == [(9, 9, 0.25)]
    with pytest.raises(ValueError, match="128"):
        s.max_marginal_relevance_search("note 1", k=4, fetch_k=129)
    with pytest.raises(ValueError, match="128"):
        s.max_marginal_relevance_search("note 1", k=200)
    with pytest.raises(ValueError, match="lambda_mult"):
        s.max_marginal_relevance_search("note 1", lambda_mult=1.5)
    assert seen == [(9, 9, 0.25)]                                     # nothing reached the index
    assert s.max_marginal_relevance_search("note 1", k=0) == []
    l2 = _store(metric="l2", name="mmr_l2")
    l2.add_texts(TEXTS[:4])
    with pytest.raises(NotImplementedError, match="cosine"):
        l2.max_marginal_relevance_search("note 1")
    bare = _store(factory=plain_factory, name="mmr_bare")
    bare.add_texts(TEXTS[:4])
    with pytest.raises(NotImplementedError, match="OracleIndex has no mmr_search"):
        bare.max_marginal_relevance_search("note 1")


def test_hybrid_store_inherits_the_methods():
    from archi_amd.vectorstore import ArchiHipHybridVectorStore
    for name in ("max_marginal_relevance_search", "max_marginal_relevance_search_by_vector",
                 "max_marginal_relevance_search_by_vector_with_score"):
        assert getattr(ArchiHipHybridVectorStore, name) is getattr(ArchiHipVectorStore, name)


def test_store_searches_again_when_a_picked_row_vanishes_before_its_text_is_read():
    s = _store()
    texts = [f"note {i}" for i in range(20)]
    s.add_texts(texts, ids=[f"id-{i}" for i in range(20)])
    col = s._collection()
    orig, calls = col.index.mmr_search, []

    def racing(queries, k, **kw):
        out = orig(queries, k, **kw)
        calls.append(out[0][0].tolist())
        if len(calls) == 1:                                            # a writer deletes the second pick between the scan and the read
            victim = col.table.text_at(col.table.pos(int(out[0][0, 1])))
            assert s.delete(ids=[f"id-{victim.split()[1]}"])
            calls.append(victim)
        return out
    col.index.mmr_search = racing
    got = [d.page_content for d in s.max_marginal_relevance_search("note 7", k=5, fetch_k=12)]
    assert len(calls) == 3 and calls[1] not in got and len(got) == 5 and got[0] == "note 7"
    assert got == [col.table.text_at(col.table.pos(i)) for i in calls[2]]
