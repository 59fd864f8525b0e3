"""GPU suite of ak_index_group_search (csrc/group.hip, csrc/index.hip): ids, group keys, sizes and counts equal, and float64
distance bits equal, to the CPU restatement tests/group_ref.py, which is fed the rows read back with fetch()."""
import ctypes
import threading

import numpy as np
import pytest

from oracle import knn_oracle as ko
from tests.group_ref import GroupOracleIndex, group_search_ref

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
    gi, gd, gg, gs, gc = got[:5]
    wi, wd, wg, ws, wc = want
    assert np.array_equal(gc, wc), (gc, wc)
    assert np.array_equal(gg, wg), (gg, wg)
    assert np.array_equal(gs, ws), (gs, ws)
    assert np.array_equal(gi, wi), (gi, wi)
    # float64 bits; a NaN (padding, a zero row's distance) must be a NaN in the same place -- its sign and payload are not part of
    # the contract (0.0 / 0.0 is -NaN on the oracle's CPU, the library emits the canonical NaN)
    nan = np.isnan(wd)
    assert np.array_equal(np.isnan(gd), nan) and np.array_equal(gd.view(np.uint64)[~nan], wd.view(np.uint64)[~nan]), (gd, wd)


def _first(want, nq=1):
    return tuple(a[:nq] for a in want)


# ---- 1. below the MFMA scan: scalar row loads (dim % 8 != 0) and 16-byte ones, every dtype and metric ---------------
@pytest.mark.parametrize("metric", ["cosine", "l2", "inner_product"])
@pytest.mark.parametrize("dtype,dim", [("f32", 100), ("bf16", 384), ("f16", 72)])
def test_small_index_every_shape(dtype, dim, metric):
    n = 300
    rng = np.random.default_rng(dim)
    rows = ko.gen_rows(21, 0, 0, n, dim, True, "f32")
    if metric != "cosine":
        rows = rows * (0.5 + rng.random((n, 1), dtype=np.float32))        # norms that matter
    ids = np.arange(n, dtype=np.int64) * 7 + 3
    groups = rng.integers(0, 40, n).astype(np.int32)
    groups[rng.random(n) < 0.1] = -(1 + rng.integers(0, 3))               # some rows are groups by themselves
    q = ko.gen_rows(21, 1, 0, 3, dim, True, "f32")
    ix = _index(rows, dtype, ids, metric=metric)
    try:
        srows, sids, alive = _stored(ix, ids)
        for k in (1, 4, 32):
            for g in (1, 3, 8):
                want = group_search_ref(srows, sids, alive, groups, q, k, g, metric)
                _same(ix.group_search(q, k, g, row_group=groups), want)
                _same(ix.group_search(q[0], k, g, row_group=groups), _first(want))           # nq = 1
    finally:
        ix.close()


# ---- 2. on the MFMA scan -----------------------------------------------------------------------------------------------
def test_groups_from_the_fast_path():
    from archi_amd.index import HipIndex
    n, dim, nq = 8192, 128, 33
    ix = HipIndex(dim, n, dtype="bf16", metric="cosine")
    try:
        ix.generate(seed=31, n=n, normalise=True)                      # generated rows: the id map is built lazily by the first call
        corpus = ko.gen_rows(31, 0, 0, n, dim, True, "bf16")
        q = ko.gen_rows(31, 1, 0, nq, dim, True, "f32")
        assert np.array_equal(ix.fetch(np.arange(0, n, 997)), corpus[::997])
        groups = (np.arange(n) % 24).astype(np.int32)                  # 24 groups among the 40 rows of round 1: collapses by pigeonhole
        got = ix.group_search(q, 10, 2, row_group=groups, return_stats=True)
        st = got[5]
        assert st["reranked"] > 0 and st["certified"] + st["exact_reruns"] == nq and st["certified"] > 0      # the MFMA scan ran
        assert st["searches"] >= 1 and st["rounds"] >= nq and st["member_rows"] > 0
        _same(got, group_search_ref(corpus, np.arange(n), None, groups, q, 10, 2))
        assert (got[3][:, :10] == 2).all() and (got[4] == 10).all()
    finally:
        ix.close()


def test_one_query_32_groups_of_8_at_dim_768():
    from archi_amd.index import HipIndex
    n, dim = 4096, 768
    ix = HipIndex(dim, n, dtype="f16", metric="cosine")
    try:
        ix.generate(seed=32, n=n, normalise=True)
        corpus = ko.gen_rows(32, 0, 0, n, dim, True, "f16")
        q = ko.gen_rows(32, 1, 0, 1, dim, True, "f32")
        groups = (np.arange(n) % 100).astype(np.int32)
        got = ix.group_search(q, 32, 8, row_group=groups)
        _same(got, group_search_ref(corpus, np.arange(n), None, groups, q, 32, 8))
        assert got[4][0] == 32 and (got[3] == 8).all()
    finally:
        ix.close()


# ---- 3. rounds: one group holds more of the nearest rows than a round fetches --------------------------------------------
@pytest.fixture(scope="module")
def skewed():
    """200 copies of one row (ids 0 .. 199, key 7777) ahead of 8192 generated rows in groups of 16; query 0 is that row."""
    n, dim = 8192, 128
    corpus = ko.gen_rows(33, 0, 0, n, dim, True, "bf16")
    hot = ko.gen_rows(33, 2, 0, 1, dim, True, "bf16")
    rows = np.concatenate([np.repeat(hot, 200, axis=0), corpus])
    ids = np.arange(len(rows), dtype=np.int64)
    groups = np.concatenate([np.full(200, 7777), np.arange(n) // 16]).astype(np.int32)
    q = np.concatenate([hot, ko.gen_rows(33, 1, 0, 1, dim, True, "f32")])
    plain = ko.search(rows, q[:1], 128, "cosine", ids=ids)[0][0]
    assert (groups[plain] == 7777).all()                              # the precondition: round 1 of query 0 is one group
    refs = {}

    def ref(k, g):
        if (k, g) not in refs:
            refs[(k, g)] = group_search_ref(rows, ids, None, groups, q, k, g)
        return refs[(k, g)]
    return rows, ids, groups, q, ref


def test_a_query_whose_first_round_is_one_group_runs_more_rounds(skewed):
    rows, ids, groups, q, ref = skewed
    ix = _index(rows, "bf16", ids)
    try:
        got = ix.group_search(q, 10, 2, row_group=groups, return_stats=True)
        st = got[5]
        assert st["multi_round_queries"] >= 1 and st["rounds"] > len(q) and st["searches"] > 1, st
        _same(got, ref(10, 2))
        assert got[2][0, 0] == 7777 and got[0][0, 0].tolist() == [0, 1]      # ties by id
    finally:
        ix.close()


def test_a_narrow_fetch_forces_many_rounds(skewed):
    from archi_amd import _lib
    rows, ids, groups, q, ref = skewed
    ix = _index(rows, "bf16", ids)
    try:
        _lib.debug_set("AK_GROUP_FETCH", "4")
        got = ix.group_search(q, 32, 1, row_group=groups, return_stats=True)
        st = got[5]
        assert st["multi_round_queries"] == len(q) and st["rounds"] >= len(q) * 8, st      # 4 rows a round: at least 8 rounds for 32 groups
        _same(got, ref(32, 1))
        _same(ix.group_search(q, 32, 3, row_group=groups), ref(32, 3))
    finally:
        _lib.debug_set("AK_GROUP_FETCH", None)
        ix.close()


# ---- 4. a group larger than any list ------------------------------------------------------------------------------------------
def test_a_group_of_6000_rows():
    from archi_amd.index import HipIndex
    n, dim = 8192, 128
    ix = HipIndex(dim, n, dtype="bf16", metric="cosine")
    try:
        ix.generate(seed=34, n=n, normalise=True)
        corpus = ko.gen_rows(34, 0, 0, n, dim, True, "bf16")
        q = ko.gen_rows(34, 1, 0, 3, dim, True, "f32")
        rng = np.random.default_rng(34)
        groups = (100 + np.arange(n) // 8).astype(np.int32)
        groups[rng.permutation(n)[:6000]] = 5                           # one key on 6000 of the 8192 rows
        got = ix.group_search(q, 5, 8, row_group=groups, return_stats=True)
        _same(got, group_search_ref(corpus, np.arange(n), None, groups, q, 5, 8))
        assert got[5]["member_rows"] >= 3 * 6000 and (got[2] == 5).any()
    finally:
        ix.close()


# ---- 5. degenerate data ---------------------------------------------------------------------------------------------------------
def test_copies_zero_rows_few_groups_and_the_identities():
    dim = 64
    base = ko.gen_rows(41, 0, 0, 16, dim, True, "f32")
    rows = np.repeat(base, 8, axis=0)                                  # 8 copies of 16 rows: ties broken by id across groups
    rows[40:48] = 0.0                                                    # a whole group of zero rows (NaN under cosine) ...
    rows[3] = 0.0                                                        # ... and one zero row inside another group
    n = len(rows)
    ids = np.arange(n, dtype=np.int64)
    q = ko.gen_rows(41, 1, 0, 2, dim, True, "f32")
    ix = _index(rows, "bf16", ids)
    try:
        srows, sids, alive = _stored(ix, ids)
        across = (ids % 8).astype(np.int32)                             # every group holds one copy of every row
        within = (ids // 8).astype(np.int32)                            # every group is one row 8 times; group 5 is all NaN
        for groups in (across, within):
            for k, g in ((4, 3), (32, 8), (8, 1)):
                _same(ix.group_search(q, k, g, row_group=groups), group_search_ref(srows, sids, alive, groups, q, k, g))
        got = ix.group_search(q, 32, 8, row_group=within)
        assert got[4].tolist() == [16, 16] and (got[2][:, 15] == 5).all() and np.isnan(got[1][:, 15]).all()      # NaN last, still a group
        assert (got[2][:, 16:] == -1).all() and (got[3][:, 16:] == 0).all()                                        # fewer groups than k
        # every key negative, group_size 1: search(), bit for bit
        gi, gd, gg, gs, gc = ix.group_search(q, 20, 1, row_group=np.full(n, -3, np.int32))
        si, sd, sc = ix.search(q, 20)
        assert np.array_equal(gi[:, :, 0], si) and np.array_equal(gd[:, :, 0].view(np.uint64), sd.view(np.uint64))
        assert (gg == -3).all() and (gs == 1).all() and (gc == 20).all()
        # one single group: its members are search()'s first rows
        gi, gd, gg, gs, gc = ix.group_search(q, 4, 8, row_group=np.full(n, 11, np.int32))
        si, sd, sc = ix.search(q, 8)
        assert np.array_equal(gi[:, 0, :], si) and np.array_equal(gd[:, 0, :].view(np.uint64), sd.view(np.uint64))
        assert gc.tolist() == [1, 1] and (gg[:, 0] == 11).all() and (gs[:, 0] == 8).all() and (gi[:, 1:] == -1).all()
        # every row filtered out
        gi, gd, gg, gs, gc = ix.group_search(q, 4, 2, row_group=across, row_filter=np.zeros(n, np.uint8))
        assert gc.tolist() == [0, 0] and (gi == -1).all() and np.isnan(gd).all() and (gg == -1).all() and (gs == 0).all()
    finally:
        ix.close()
    ix = _index(np.zeros((0, 48), np.float32), "bf16", capacity=16)        # an empty index
    try:
        gi, gd, gg, gs, gc = ix.group_search(ko.gen_rows(41, 1, 0, 2, 48, True, "f32"), 4, 2, row_group=np.zeros(0, np.int32))
        assert gc.tolist() == [0, 0] and (gi == -1).all() and np.isnan(gd).all() and (gg == -1).all() and (gs == 0).all()
    finally:
        ix.close()


# ---- 6. masks and writers -----------------------------------------------------------------------------------------------------
def test_mask_tombstones_stale_keys_and_compact():
    from archi_amd import StaleFilterError, _lib
    n, dim = 200, 64
    rows = ko.gen_rows(61, 0, 0, n, dim, True, "f32")
    q = np.ascontiguousarray(ko.gen_rows(61, 1, 0, 2, dim, True, "f32"))
    ids = np.arange(n, dtype=np.int64) + 1000
    groups = (np.arange(n) % 13).astype(np.int32)
    ix = _index(rows, "bf16", ids, capacity=512)
    try:
        srows, sids, alive = _stored(ix, ids)
        slots, epoch = ix.layout()
        free = ix.group_search(q, 5, 3, row_group=groups, filter_epoch=epoch)
        _same(free, group_search_ref(srows, sids, alive, groups, q, 5, 3))
        mask = np.ones(n, np.uint8)
        mask[free[0][:, 0, 0] - 1000] = 0                                 # the best group's best row leaves, for both queries
        got = ix.group_search(q, 5, 3, row_group=groups, row_filter=mask, filter_epoch=epoch)
        _same(got, group_search_ref(srows, sids, alive & mask, groups, q, 5, 3))
        assert not np.isin(got[0], free[0][:, 0, 0]).any()
        ix.add(ko.gen_rows(62, 0, 0, 1, dim, True, "f32"), ids=[5000])    # the layout moves on: the old keys are refused ...
        with pytest.raises(StaleFilterError):
            ix.group_search(q, 5, 3, row_group=groups, filter_epoch=epoch)
        oi, od = np.full(2 * 5 * 3, 77, np.int64), np.full(2 * 5 * 3, 7.5, np.float64)      # ... and nothing is written
        og, os_, oc, st = np.full(10, 77, np.int32), np.full(10, 77, np.int32), np.full(2, 77, np.int32), np.full(8, 77, np.int64)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)                   # noqa: E731
        rc = _lib.load().ak_index_group_search(ix._h, P(q), 2, 5, 3, 0, P(groups), None, n, epoch, P(oi), P(od), P(og), P(os_), P(oc), P(st))
        assert rc == _lib.ERR_STALE_FILTER
        assert (oi == 77).all() and (od == 7.5).all() and (og == 77).all() and (os_ == 77).all() and (oc == 77).all() and (st == 77).all()
        # removed rows never appear, before and after compact(); the key array is rebuilt for each layout
        victims = np.unique(free[0][:, :2, 0].ravel())
        assert ix.remove(victims) == len(victims)
        live = np.setdiff1d(np.append(ids, 5000), victims)
        for compacted in (False, True):
            if compacted:
                assert ix.compact() == len(victims)
            srows, sids, alive = _stored(ix, live)
            keys = np.where(sids >= 0, sids % 13, -1).astype(np.int32)
            got = ix.group_search(q, 6, 4, row_group=keys)
            _same(got, group_search_ref(srows, sids, alive, keys, q, 6, 4))
            assert not np.isin(got[0], victims).any()
    finally:
        ix.close()


# ---- 7. re-entrancy ----------------------------------------------------------------------------------------------------------------
def test_eight_threads_on_one_index():
    n, dim = 400, 128
    rows = ko.gen_rows(71, 0, 0, n, dim, True, "f32")
    qs = ko.gen_rows(71, 1, 0, 8, dim, True, "f32")
    groups = (np.arange(n) % 37).astype(np.int32)
    shapes = [(1 + (3 * t) % 32, 1 + t % 8) for t in range(8)]            # a different (k, group_size) per thread
    ix = _index(rows, "bf16", np.arange(n))
    try:
        srows, sids, alive = _stored(ix, np.arange(n))
        serial = [ix.group_search(qs[t:t + 2], k, g, row_group=groups) for t, (k, g) in enumerate(shapes)]
        _same(serial[3], group_search_ref(srows, sids, alive, groups, qs[3:5], *shapes[3]))
        errs = []

        def work(t):
            try:
                for _ in range(20):
                    _same(ix.group_search(qs[t:t + 2], *shapes[t], row_group=groups), serial[t])
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


# ---- 8. the store ----------------------------------------------------------------------------------------------------------------------
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

    vs.reset_collections()
    try:
        real = ArchiHipVectorStore({"hip": {"dtype": "bf16"}}, Emb(), collection_name="grp_real")
        fake = ArchiHipVectorStore({"hip": {"dtype": "bf16"}}, Emb(), collection_name="grp_fake",
                                   index_factory=lambda d, c, dtype, metric, shards=1: GroupOracleIndex(d, c, dtype=dtype, metric=metric))
        for s in (real, fake):
            for d in range(6):
                s._collection(dim).table.register_document(d + 1, resource_hash=f"h{d}", display_name=f"doc {d}")
                s.add_texts([f"page {'x' * (5 * d)} part {j}" for j in range(8)],
                            metadatas=[{"source": "web" if j % 3 else "git", "resource_hash": f"h{d}"} for j in range(8)], document_id=d + 1)
            s.add_texts([f"note {j}" for j in range(10)], metadatas=[{"source": "web"} for _ in range(10)])
            s._collection().table.register_document(3, is_deleted=True)
        strip = lambda res: [(v, [(d.page_content, d.metadata["source"], sc) for d, sc in mem]) for v, mem in res]      # noqa: E731
        for query in ("question 1", "note 5", "page xxxxx part 2"):
            for kw in ({}, {"k": 5, "group_size": 3}, {"k": 5, "group_size": 3, "filter": {"source": "web"}},
                       {"k": 32, "group_size": 8, "group_by": "resource_hash"}, {"k": 3, "group_size": 2, "include_deleted": True}):
                a = real.search_groups_by_vector(Emb._vec(query), **kw)
                b = fake.search_groups_by_vector(Emb._vec(query), **kw)
                assert strip(a) == strip(b) and len(a) == min(kw.get("k", 4), 5 + 10 + (1 if kw.get("include_deleted") else 0))
                if not kw.get("include_deleted"):
                    assert 3 not in [v for v, _ in a] and "h2" not in [v for v, _ in a]
    finally:
        vs.reset_collections()
