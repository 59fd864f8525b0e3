"""GPU suite of ak_index_mmr_search (csrc/mmr.hip, csrc/index.hip): ids, float64 distance bits and ranks equal to the CPU
restatement tests/mmr_ref.py, which is fed the rows read back with fetch()."""
import ctypes
import threading

import numpy as np
import pytest

from oracle import knn_oracle as ko
from tests.mmr_ref import MmrOracleIndex, mmr_search_ref

pytestmark = pytest.mark.gpu


def _index(rows, dtype, ids=None, metric="cosine", capacity=None):
    from archi_amd.index import HipIndex
    ix = HipIndex(rows.shape[1], capacity or max(len(rows), 1), dtype=dtype, metric=metric)
    if len(rows):
        ix.add(rows, ids=ids)
    return ix


def _stored(ix, ids):
    """(rows by slot as stored, ids by slot, alive by slot) of an index whose live ids are `ids`."""
    n = ix.slots
    rows = ix.fetch(np.arange(n)) if n else np.zeros((0, ix.dim), np.float32)
    slots = ix.lookup(ids)
    by_slot = np.full(n, -1, np.int64)
    alive = np.zeros(n, np.uint8)
    by_slot[slots[slots >= 0]] = np.asarray(ids)[slots >= 0]
    alive[slots[slots >= 0]] = 1
    return rows, by_slot, alive


def _same(got, want):
    gi, gd, gc, gr = got
    wi, wd, wc, wr = want
    assert np.array_equal(gi, wi), (gi, wi)
    # float64 bits; a NaN (padding, a zero row's distance) must be a NaN in the same place -- its sign and payload are not part of
    # the contract (0.0 / 0.0 is -NaN on the oracle's CPU, the library emits the canonical NaN)
    nan = np.isnan(wd)
    assert np.array_equal(np.isnan(gd), nan) and np.array_equal(gd.view(np.uint64)[~nan], wd.view(np.uint64)[~nan]), (gd, wd)
    assert np.array_equal(gc, wc) and np.array_equal(gr, wr), (gc, wc, gr, wr)


# ---- below the MFMA scan: scalar path (dim % 8 != 0), panel path, partial last panel ---------------
@pytest.mark.parametrize("dtype,dim", [("f32", 100), ("bf16", 384), ("f16", 72)])
def test_small_index_every_shape(dtype, dim):
    n = 300
    rows = ko.gen_rows(21, 0, 0, n, dim, True, "f32")
    ids = np.arange(n, dtype=np.int64) * 7 + 3
    q = ko.gen_rows(21, 1, 0, 3, dim, True, "f32")
    ix = _index(rows, dtype, ids)
    try:
        srows, sids, alive = _stored(ix, ids)
        cache = {}
        for k, fk in ((1, 1), (4, 20), (10, 64), (5, 127), (128, 128)):
            for lam in (0.0, 0.25, 0.5, 1.0):
                want = mmr_search_ref(srows, sids, alive, q, k, fk, lam, cache=cache)
                _same(ix.mmr_search(q, k, fetch_k=fk, lambda_mult=lam, return_rank=True), want)
                one = ix.mmr_search(q[0], k, fetch_k=fk, lambda_mult=lam, return_rank=True)        # nq = 1
                _same(one, tuple(a[:1] for a in want))
                if lam == 1.0:                        # the free cross-check: the plain search, bit for bit
                    si, sd, sc = ix.search(q, k)
                    assert np.array_equal(one[0], si[:1]) and np.array_equal(one[1].view(np.uint64), sd[:1].view(np.uint64))
    finally:
        ix.close()


# ---- on the MFMA scan -------------------------------------------------------------------------------
def test_candidates_from_the_fast_path():
    from archi_amd.index import HipIndex
    n, dim, nq = 8192, 128, 33
    ix = HipIndex(dim, n, dtype="bf16", metric="cosine")
    try:
        ix.generate(seed=31, n=n, normalise=True)                      # generated rows: the id map is built lazily by the first call
        corpus = ko.gen_rows(31, 0, 0, n, dim, True, "bf16")
        q = ko.gen_rows(31, 1, 0, nq, dim, True, "f32")
        assert np.array_equal(ix.fetch(np.arange(0, n, 997)), corpus[::997])
        got = ix.mmr_search(q, 10, fetch_k=64, lambda_mult=0.5, return_rank=True, return_stats=True)
        st = got[4]
        assert st["reranked"] > 0 and st["certified"] + st["exact_reruns"] == nq and st["certified"] > 0      # the MFMA scan ran
        _same(got[:4], mmr_search_ref(corpus, np.arange(n), None, q, 10, 64, 0.5))
        assert (got[3][:, 1:] != np.arange(1, 10)).any()               # and the pick is not the plain order
    finally:
        ix.close()


def test_every_pair_block_of_one_query():
    from archi_amd.index import HipIndex
    n, dim = 4096, 768
    ix = HipIndex(dim, n, dtype="f16", metric="cosine")
    try:
        ix.generate(seed=32, n=n, normalise=True)
        corpus = ko.gen_rows(32, 0, 0, n, dim, True, "f16")
        q = ko.gen_rows(32, 1, 0, 1, dim, True, "f32")
        _same(ix.mmr_search(q, 128, fetch_k=128, lambda_mult=0.5, return_rank=True),
              mmr_search_ref(corpus, np.arange(n), None, q, 128, 128, 0.5))
    finally:
        ix.close()


# ---- duplicates and degenerate rows -----------------------------------------------------------------
def test_copies_and_a_zero_row():
    dim = 64
    base = ko.gen_rows(41, 0, 0, 16, dim, True, "f32")
    rows = np.repeat(base, 8, axis=0)
    q = ko.gen_rows(41, 1, 0, 2, dim, True, "f32")
    ix = _index(rows, "bf16", np.arange(128))
    try:
        srows, sids, alive = _stored(ix, np.arange(128))
        got = ix.mmr_search(q, 8, fetch_k=128, lambda_mult=0.5, return_rank=True)
        _same(got, mmr_search_ref(srows, sids, alive, q, 8, 128, 0.5))
        assert all(len(set((r // 8).tolist())) == 8 for r in got[0])     # 8 distinct groups, where search() returns one 8 times
        assert all(len(set((r // 8).tolist())) == 1 for r in ix.search(q, 8)[0])
    finally:
        ix.close()
    few = ko.gen_rows(42, 0, 0, 12, 40, True, "f32")
    few[5] = 0.0                                                          # NaN distance: ranks last, picked last
    ix = _index(few, "f32", np.arange(12))
    try:
        srows, sids, alive = _stored(ix, np.arange(12))
        q = ko.gen_rows(42, 1, 0, 1, 40, True, "f32")
        got = ix.mmr_search(q, 12, fetch_k=12, lambda_mult=0.5, return_rank=True)
        _same(got, mmr_search_ref(srows, sids, alive, q, 12, 12, 0.5))
        assert got[0][0, 11] == 5 and np.isnan(got[1][0, 11]) and got[3][0, 11] == 11 and not np.isnan(got[1][0, :11]).any()
    finally:
        ix.close()


# ---- few rows, none ----------------------------------------------------------------------------------
def test_fewer_rows_than_fetch_k_and_an_empty_index():
    rows = ko.gen_rows(51, 0, 0, 7, 48, True, "f32")
    q = ko.gen_rows(51, 1, 0, 2, 48, True, "f32")
    ix = _index(rows, "f16", np.arange(7) + 10, capacity=16)
    try:
        srows, sids, alive = _stored(ix, np.arange(7) + 10)
        got = ix.mmr_search(q, 10, fetch_k=20, lambda_mult=0.5, return_rank=True)
        _same(got, mmr_search_ref(srows, sids, alive, q, 10, 20, 0.5))
        assert got[2].tolist() == [7, 7] and (got[0][:, 7:] == -1).all() and np.isnan(got[1][:, 7:]).all() and (got[3][:, 7:] == -1).all()
    finally:
        ix.close()
    ix = _index(np.zeros((0, 48), np.float32), "bf16", capacity=16)
    try:
        gi, gd, gc, gr = ix.mmr_search(q, 4, fetch_k=20, return_rank=True)
        assert gc.tolist() == [0, 0] and (gi == -1).all() and np.isnan(gd).all() and (gr == -1).all()
    finally:
        ix.close()


# ---- mask and lifecycle ---------------------------------------------------------------------------------
def test_mask_stale_mask_remove_and_compact():
    from archi_amd import StaleFilterError
    n, dim = 200, 64
    rows = ko.gen_rows(61, 0, 0, n, dim, True, "f32")
    q = ko.gen_rows(61, 1, 0, 2, dim, True, "f32")
    ids = np.arange(n, dtype=np.int64) + 1000
    ix = _index(rows, "bf16", ids, capacity=512)
    try:
        srows, sids, alive = _stored(ix, ids)
        mask = np.zeros(n, np.uint8)
        mask[[3, 50, 51, 120, 199]] = 1                                   # a mask leaving 5 rows
        slots, epoch = ix.layout()
        got = ix.mmr_search(q, 4, fetch_k=20, lambda_mult=0.5, row_filter=mask, filter_epoch=epoch, return_rank=True)
        _same(got, mmr_search_ref(srows, sids, alive & mask, q, 4, 20, 0.5))
        assert set(got[0].ravel().tolist()) <= {1003, 1050, 1051, 1120, 1199}
        got = ix.mmr_search(q, 8, fetch_k=20, lambda_mult=0.5, row_filter=mask, return_rank=True)
        assert got[2].tolist() == [5, 5]
        _same(got, mmr_search_ref(srows, sids, alive & mask, q, 8, 20, 0.5))
        ix.add(ko.gen_rows(62, 0, 0, 1, dim, True, "f32"), ids=[5000])    # the layout moves on: the old mask is refused
        with pytest.raises(StaleFilterError):
            ix.mmr_search(q, 4, fetch_k=20, row_filter=mask, filter_epoch=epoch)
        # removed rows never appear, before and after compact()
        first = ix.mmr_search(q, 10, fetch_k=30, lambda_mult=0.5)[0]
        victims = np.unique(first[:, :5].ravel())
        assert ix.remove(victims) == len(victims)
        live = np.setdiff1d(np.append(ids, 5000), victims)
        for compacted in (False, True):
            if compacted:
                assert ix.compact() == len(victims)
            srows, sids, alive = _stored(ix, live)
            got = ix.mmr_search(q, 10, fetch_k=30, lambda_mult=0.5, return_rank=True)
            _same(got, mmr_search_ref(srows, sids, alive, q, 10, 30, 0.5))
            assert not np.isin(got[0], victims).any()
    finally:
        ix.close()


# ---- concurrency ------------------------------------------------------------------------------------------
def test_eight_threads_on_one_index():
    n, dim = 400, 128
    rows = ko.gen_rows(71, 0, 0, n, dim, True, "f32")
    qs = ko.gen_rows(71, 1, 0, 8, dim, True, "f32")
    ix = _index(rows, "bf16", np.arange(n))
    try:
        srows, sids, alive = _stored(ix, np.arange(n))
        cache = {}
        want = [mmr_search_ref(srows, sids, alive, qs[t:t + 1], 6, 40, 0.5, cache=cache) for t in range(8)]
        got, errs = [None] * 8, []

        def work(t):
            try:
                for _ in range(5):
                    got[t] = ix.mmr_search(qs[t], 6, fetch_k=40, lambda_mult=0.5, return_rank=True)
                    _same(got[t], want[t])
            except BaseException as e:                                    # noqa: B036 -- reported by the main thread
                errs.append((t, e))
        threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errs, errs
    finally:
        ix.close()


# ---- the store ------------------------------------------------------------------------------------------------
def test_store_on_the_real_index_equals_the_store_on_the_oracle_index():
    from archi_amd import vectorstore as vs
    from archi_amd.vectorstore import ArchiHipVectorStore
    dim = 64

    class Emb:
        @staticmethod
        def _vec(text):
            return [float(x) for x in ko.gen_rows(81, 5, sum(text.encode()) * 131 + len(text), 1, dim, True, "f32")[0]]

        def embed_documents(self, texts):
            return [self._vec(t) for t in texts]

        def embed_query(self, text):
            return self._vec(text)

    texts = [f"paragraph {i // 4}" for i in range(40)] + [f"note {i}" for i in range(24)]
    metas = [{"source": "web" if i % 3 else "git"} for i in range(len(texts))]
    vs.reset_collections()
    try:
        real = ArchiHipVectorStore({"hip": {"dtype": "bf16"}}, Emb(), collection_name="mmr_real")
        fake = ArchiHipVectorStore({"hip": {"dtype": "bf16"}}, Emb(), collection_name="mmr_fake",
                                   index_factory=lambda d, c, dtype, metric, shards=1: MmrOracleIndex(d, c, dtype=dtype, metric=metric))
        for s in (real, fake):
            s.add_texts(texts, metadatas=[dict(m) for m in metas])
        for query in ("question 1", "question 2", "note 5"):
            for kw in ({}, {"filter": {"source": "web"}}, {"k": 6, "fetch_k": 30, "lambda_mult": 0.25}):
                a = real.max_marginal_relevance_search_by_vector_with_score(Emb._vec(query), **kw)
                b = fake.max_marginal_relevance_search_by_vector_with_score(Emb._vec(query), **kw)
                # (the rest of the metadata names the collection and the row's random chunk id)
                assert [(d.page_content, d.metadata["source"], sc) for d, sc in a] == [(d.page_content, d.metadata["source"], sc) for d, sc in b]
                assert len(a) == kw.get("k", 4)
    finally:
        vs.reset_collections()


# ---- refusals ----------------------------------------------------------------------------------------------------
def test_refusals_return_an_error_and_leave_the_outputs_untouched():
    from archi_amd import HipBackendError, _lib
    rows = ko.gen_rows(91, 0, 0, 50, 32, True, "f32")
    q = np.ascontiguousarray(ko.gen_rows(91, 1, 0, 1, 32, True, "f32"))
    lib = _lib.load()

    def raw(ix, k, fk, lam):
        oi, od = np.full(256, 77, np.int64), np.full(256, 7.5, np.float64)
        orr, oc, st = np.full(256, 77, np.int32), np.full(1, 77, np.int32), np.full(4, 77, np.int64)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = lib.ak_index_mmr_search(ix._h, P(q), 1, k, fk, lam, 0, None, 0, 0, P(oi), P(od), P(orr), P(oc), P(st))
        untouched = (oi == 77).all() and (od == 7.5).all() and (orr == 77).all() and (oc == 77).all() and (st == 77).all()
        return rc, untouched, _lib.last_error()

    ix = _index(rows, "bf16", np.arange(50))
    try:
        for k, fk, lam, word in ((0, 10, 0.5, "k must be"), (5, 4, 0.5, "fetch_k must be >= k"), (5, 129, 0.5, "128"),
                                 (5, 10, -0.1, "lambda_mult"), (5, 10, 1.5, "lambda_mult"), (5, 10, float("nan"), "lambda_mult")):
            rc, untouched, msg = raw(ix, k, fk, lam)
            assert rc != 0 and untouched and word in msg, (k, fk, lam, rc, msg)
        with pytest.raises(HipBackendError, match="fetch_k"):
            ix.mmr_search(q, 5, fetch_k=200)
        rc, untouched, _ = raw(ix, 5, 10, 0.5)                            # and the same call with good arguments does write
        assert rc == 0 and not untouched
    finally:
        ix.close()
    for metric, name in (("l2", "l2"), ("inner_product", "inner_product")):
        ix = _index(rows, "bf16", np.arange(50), metric=metric)
        try:
            rc, untouched, msg = raw(ix, 5, 10, 0.5)
            assert rc != 0 and untouched and "cosine" in msg and name in msg, (rc, msg)
        finally:
            ix.close()
