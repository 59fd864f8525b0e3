"""CPU suite of the grouped search: the ABI entry point exists and refuses its limits by name, the reference restatement
(tests/group_ref.py) agrees with an independent brute-force numpy grouping and has the contract's two identities, and the store's
host logic (ArchiHipVectorStore.search_groups* / similarity_search_by_document*) on an oracle-backed index."""
import os
import re
import subprocess

import numpy as np
import pytest

from archi_amd import vectorstore as vs
from archi_amd.vectorstore import ArchiHipVectorStore
from oracle import knn_oracle as ko
from tests.fake_index import OracleIndex
from tests.group_ref import GroupOracleIndex, group_search_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def fresh():
    vs.reset_collections()
    yield
    vs.reset_collections()


def _same(a, b):
    """float64 arrays: equal bits, a NaN where the other has a NaN (its sign is not compared)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


# ---- ABI -------------------------------------------------------------------------------------
def _lib():
    import __graft_entry__ as ge
    ge.build()
    from archi_amd import _lib
    return _lib


def test_entry_point_is_declared_bound_and_exported():
    _lib_ = _lib()
    hdr = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    assert re.search(r"\bint ak_index_group_search\s*\(", hdr)
    assert "ak_index_group_search" in {name for name, _, _ in _lib_.SYMBOLS}
    so = os.path.join(ROOT, "archi_amd", "lib", "libarchi_hip.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert re.search(r"\bT ak_index_group_search\b", exported)
    assert _lib_.load().ak_abi_version() == 5 == _lib_.ABI_VERSION


@pytest.mark.parametrize("k,g,mode,word", [(0, 1, 0, "k must"), (33, 1, 0, "k must"), (4, 0, 0, "group_size"), (4, 9, 0, "group_size"),
                                           (4, 2, 2, "FAST_ONLY")])
def test_limits_are_refused_by_name_before_anything_else(k, g, mode, word):
    """The limits come before the handle is looked at or the device bound: a NULL handle is enough to see them refused."""
    _lib_ = _lib()
    lib = _lib_.load()
    rc = lib.ak_index_group_search(None, None, 1, k, g, mode, None, None, 0, 0, None, None, None, None, None, None)
    assert rc == -1 and word in _lib_.last_error() and "ak_index_group_search" in _lib_.last_error()


def test_fetch_switch_takes_1_to_128_only():
    _lib_ = _lib()
    try:
        for good in ("1", "4", "128"):
            _lib_.debug_set("AK_GROUP_FETCH", good)
        for bad in ("129", "-1"):
            with pytest.raises(_lib_.HipBackendError):
                _lib_.debug_set("AK_GROUP_FETCH", bad)
    finally:
        _lib_.debug_set("AK_GROUP_FETCH", None)


def test_group_kernels_have_no_spills_and_no_scratch():
    from scripts.kernel_resources import HIPCC, kernel_resources
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    keys = ("SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]")
    seen = {name: {key: use[key] for key in keys if key in use} for name, use in kernel_resources("group.hip").items()}
    for kernel, copies in (("k_group_collapse", 1), ("k_group_exclude", 1), ("k_group_members", 2), ("k_group_dist", 3),
                           ("k_group_select", 1), ("k_group_init", 1)):
        assert sum(kernel in n for n in seen) == copies, (kernel, sorted(seen))
    for n, res in seen.items():
        assert len(res) == 3 and all(v == 0 for v in res.values()), (n, res)


# ---- group_ref against a brute-force numpy grouping -------------------------------------------
def _brute(rows, ids, alive, groups, q, k, g, metric):
    """Independent of ko.search and of group_walk: numpy distances, one lexsort, then per group a boolean selection."""
    d = ko.distances_numpy(rows, q, metric)
    live = np.flatnonzero(alive)
    dd = d[live]
    order = live[np.lexsort((ids[live], np.where(np.isnan(dd), 0.0, dd), np.isnan(dd)))]
    name = np.where(groups >= 0, groups.astype(np.int64), -1 - np.arange(len(groups), dtype=np.int64))      # one name per group
    names = name[order]
    _, first = np.unique(names, return_index=True)
    out = []
    for f in np.sort(first)[:k]:
        mem = order[names == names[f]][:g]
        out.append((int(groups[order[f]]), [int(i) for i in ids[mem]], d[mem]))
    return out


@pytest.mark.parametrize("seed,n,dim,k,g,metric", [(1, 60, 16, 5, 3, "cosine"), (2, 90, 24, 32, 8, "l2"), (3, 40, 8, 4, 1, "inner_product"),
                                                   (4, 120, 32, 10, 2, "cosine")])
def test_reference_agrees_with_brute_force_grouping(seed, n, dim, k, g, metric):
    rng = np.random.default_rng(seed)
    rows = ko.gen_rows(seed, 0, 0, n, dim, metric == "cosine", "f32")
    rows[n // 2: n // 2 + 6] = rows[3]                                   # copies across groups: ties broken by id
    rows[7] = 0.0                                                        # NaN under cosine
    rows[n - 1] = 0.0
    ids = rng.permutation(n).astype(np.int64) * 3 + 10
    alive = (rng.random(n) > 0.15).astype(np.uint8)
    groups = rng.integers(0, 12, n).astype(np.int32)
    groups[rng.random(n) < 0.2] = -5                                     # rows that are groups by themselves
    qs = ko.gen_rows(seed, 1, 0, 3, dim, True, "f32")
    gi, gd, gg, gs, gc = group_search_ref(rows, ids, alive, groups, qs, k, g, metric)
    for qi in range(3):
        want = _brute(rows, ids, alive, groups, qs[qi], k, g, metric)
        assert gc[qi] == len(want)
        for w, (key, mids, md) in enumerate(want):
            assert gg[qi, w] == key and gs[qi, w] == len(mids)
            assert gi[qi, w, :len(mids)].tolist() == mids and _same(gd[qi, w, :len(mids)], md)
            assert (gi[qi, w, len(mids):] == -1).all() and np.isnan(gd[qi, w, len(mids):]).all()
        assert (gg[qi, len(want):] == -1).all() and (gs[qi, len(want):] == 0).all() and (gi[qi, len(want):] == -1).all()


def _corpus(seed, n, dim):
    return ko.gen_rows(seed, 0, 0, n, dim, True, "f32"), ko.gen_rows(seed, 1, 0, 3, dim, True, "f32")


def test_every_key_negative_and_size_one_is_the_plain_topk():
    rows, q = _corpus(21, 50, 16)
    rows[5] = 0.0
    ids = np.arange(50) * 3
    gi, gd, gg, gs, gc = group_search_ref(rows, ids, None, np.full(50, -1, np.int32), q, 7, 1)
    oi, od, _ = ko.search(rows, q, 7, "cosine", ids=ids)
    assert np.array_equal(gi[:, :, 0], oi) and _same(gd[:, :, 0], od) and (gg == -1).all() and (gs == 1).all() and gc.tolist() == [7] * 3


def test_one_group_holds_the_plain_topk_as_its_members():
    rows, q = _corpus(22, 50, 16)
    ids = np.arange(50) + 100
    gi, gd, gg, gs, gc = group_search_ref(rows, ids, None, np.full(50, 9, np.int32), q, 4, 8)
    oi, od, _ = ko.search(rows, q, 8, "cosine", ids=ids)
    assert gc.tolist() == [1] * 3 and (gg[:, 0] == 9).all() and (gs[:, 0] == 8).all()
    assert np.array_equal(gi[:, 0, :], oi) and _same(gd[:, 0, :], od) and (gi[:, 1:] == -1).all() and (gg[:, 1:] == -1).all()


def test_nan_rows_rank_last_and_still_form_a_group():
    rows, q = _corpus(23, 12, 8)
    rows[2] = rows[9] = 0.0
    groups = np.array([0, 0, 7, 1, 1, 2, 2, 3, 3, 7, 4, 4], np.int32)
    gi, gd, gg, gs, gc = group_search_ref(rows, np.arange(12), None, groups, q[:1], 32, 8)
    assert gc[0] == 6 and gg[0, 5] == 7 and gi[0, 5, :2].tolist() == [2, 9] and np.isnan(gd[0, 5, :2]).all() and gs[0, 5] == 2
    assert not np.isnan(gd[0, :5, 0]).any()
    ei, ed, eg, es, ec = group_search_ref(np.zeros((0, 8), np.float32), np.zeros(0, np.int64), None, np.zeros(0, np.int32), q, 4, 2)
    assert ec.tolist() == [0, 0, 0] and (ei == -1).all() and np.isnan(ed).all() and (eg == -1).all() and (es == 0).all()


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


def group_factory(dim, capacity, dtype, metric, shards=1):
    return GroupOracleIndex(dim, capacity, dtype=dtype, metric=metric)


def plain_factory(dim, capacity, dtype, metric, shards=1):
    return OracleIndex(dim, capacity, dtype=dtype, metric=metric)


def _store(factory=group_factory, metric="cosine", name="grp"):
    return ArchiHipVectorStore({"hip": {"dtype": "f32"}}, TextEmb(), collection_name=name, distance_metric=metric, index_factory=factory)


def _txt(d, j):
    """Chunk j of document d: texts of different documents differ in length, so no two texts share TextEmb's vector."""
    return f"page {'x' * (7 * d)}{d} part {j}"


def _fill(s):
    """Four documents of six chunks (resource_hash h0 .. h3, a `lang` key on documents 1 and 2 only) and five chunks without one."""
    for d in range(4):
        s._collection(DIM).table.register_document(d + 1, resource_hash=f"h{d}", display_name=f"doc {d}")
        s.add_texts([_txt(d, j) for j in range(6)],
                    metadatas=[dict({"resource_hash": f"h{d}", "part": j}, **({"lang": "en" if d == 1 else "de"} if d in (1, 2) else {}))
                               for j in range(6)], document_id=d + 1)
    s.add_texts([f"loose note {j}" for j in range(5)], metadatas=[{"part": j} for j in range(5)])
    return s


def _flat_plain(s, q, **kw):
    return s.similarity_search_by_vector_with_score(TextEmb().embed_query(q), k=64, **kw)


def test_store_groups_by_document_in_the_plain_searchs_order():
    s = _fill(_store())
    q = _txt(2, 3)
    plain = _flat_plain(s, q)
    assert len(plain) == 29
    t = s._collection().table
    doc_of = {(d.page_content): t.document_id_at(t.pos(r)) for r in t.live_rids().tolist() for d in [s._document(t, t.pos(r))]}
    want, seen = [], {}
    for d, sc in plain:                                                 # the definition, on the store's own plain result
        doc = doc_of[d.page_content]
        name = ("doc", doc) if doc is not None else ("row", d.page_content)
        if name not in seen:
            seen[name] = (doc, [])
            want.append(seen[name])
        if len(seen[name][1]) < 3:
            seen[name][1].append((d.page_content, sc))
    got = s.search_groups(q, k=6, group_size=3)
    assert [(v, [(d.page_content, sc) for d, sc in mem]) for v, mem in got] == [(v, m) for v, m in want[:6]]
    assert got[0][0] == 3 and got[0][1][0][0].page_content == q and got[0][1][0][0].metadata["display_name"] == "doc 2"
    assert any(v is None and len(mem) == 1 for v, mem in got) or all(v is not None for v, _ in got)
    # rows without a document: each a group of its own, value None, one member whatever group_size is
    everything = s.search_groups(q, k=32, group_size=8)
    assert len(everything) == 4 + 5 and sum(v is None for v, _ in everything) == 5
    assert all(len(mem) == (1 if v is None else 6) for v, mem in everything)
    # the flat lists: group rank, then row rank
    flat = s.similarity_search_by_document_with_score(q, k=6, chunks_per_document=3)
    assert [(d.page_content, sc) for d, sc in flat] == [pair for _, m in want[:6] for pair in m]
    assert [d.page_content for d in s.similarity_search_by_document(q, k=6, chunks_per_document=3)] == [d.page_content for d, _ in flat]
    assert [d.page_content for d in s.similarity_search_by_document(q, k=3)] == [m[0][0] for _, m in want[:3]]
    by_vec = s.search_groups_by_vector(TextEmb().embed_query(q), k=6, group_size=3)
    assert [(v, [(d.page_content, sc) for d, sc in mem]) for v, mem in by_vec] == [(v, m) for v, m in want[:6]]


def test_store_groups_by_a_metadata_key():
    s = _fill(_store())
    q = _txt(1, 0)
    by_doc = s.search_groups(q, k=32, group_size=8)
    by_hash = s.search_groups(q, k=32, group_size=8, group_by="resource_hash")
    # every document has its own resource_hash: the same groups, named by the hash
    strip = lambda res: [[(d.page_content, sc) for d, sc in mem] for _, mem in res]      # noqa: E731
    assert strip(by_hash) == strip(by_doc)
    assert [v for v, _ in by_hash if v is not None] == [f"h{v - 1}" for v, _ in by_doc if v is not None]
    assert sum(v is None for v, _ in by_hash) == 5
    # a key only some rows carry: two groups, every other row a group by itself
    by_lang = s.search_groups(q, k=32, group_size=8, group_by="lang")
    named = [(v, len(mem)) for v, mem in by_lang if v is not None]
    assert sorted(named) == [("de", 6), ("en", 6)] and sum(v is None for v, _ in by_lang) == 29 - 12 == len(by_lang) - 2
    assert all(len(mem) == 1 for v, mem in by_lang if v is None)


def test_store_filter_and_soft_deleted_documents():
    s = _fill(_store())
    q = _txt(3, 1)
    t = s._collection().table
    odd = s.search_groups(q, k=8, group_size=8, filter={"part": 1})
    assert len(odd) == 5 and all(len(mem) == 1 and mem[0][0].metadata["part"] == 1 for _, mem in odd)
    assert [mem[0][0].page_content for _, mem in odd] == [d.page_content for d, _ in _flat_plain(s, q, filter={"part": 1})]
    t.register_document(4, is_deleted=True)                             # document 4 ("page 3 ...") is soft-deleted
    left = s.search_groups(q, k=32, group_size=8)
    assert 4 not in [v for v, _ in left] and len(left) == 3 + 5
    assert not any(d.page_content.startswith(_txt(3, 0)[:-1]) for _, mem in left for d, _ in mem)
    back = s.search_groups(q, k=32, group_size=8, include_deleted=True)
    assert back[0][0] == 4 and back[0][1][0][0].page_content == q and len(back) == 9
    assert s.similarity_search_by_document(q, k=2, chunks_per_document=2)[0].page_content != q


def test_key_array_is_cached_until_the_table_or_the_layout_moves():
    s = _fill(_store())
    col = s._collection()
    t = col.table
    with t.lock:
        epoch = col.index.layout()[1]
        a = s._group_keys(col, "document_id", epoch)
        assert s._group_keys(col, "document_id", epoch) is a           # the same object: cached
        b = s._group_keys(col, "resource_hash", epoch)
        assert b is not a and s._group_keys(col, "resource_hash", epoch) is b and s._group_keys(col, "document_id", epoch) is a
    keys, values = a
    assert keys.dtype == np.int32 and len(keys) == col.index.layout()[0] and (keys >= 0).sum() == 24 and (keys == -1).sum() == 5
    s.add_texts([_txt(0, 6)], metadatas=[{"resource_hash": "h0"}], document_id=1)      # a writer: table version and layout move
    with t.lock:
        epoch2 = col.index.layout()[1]
        c = s._group_keys(col, "document_id", epoch2)
    assert epoch2 != epoch and c is not a and len(c[0]) == len(keys) + 1 and c[0][-1] == keys[0]
    assert not any(k[3:] == ("group_by", "document_id") and k[2] == epoch for k in t.where_cache)
    t.register_document(2, is_deleted=True)                             # documents change: dropped again
    with t.lock:
        assert s._group_keys(col, "document_id", epoch2) is not c
    # the added chunk took chunk index 0 of its document (an upsert): the old slot is a tombstone whose key is -1 now
    assert c[0][0] == -1 and (c[0] >= 0).sum() == 24
    members = [d.page_content for d, _ in s.search_groups(_txt(0, 6), k=1, group_size=8)[0][1]]
    assert len(members) == 6 and members[0] == _txt(0, 6) and _txt(0, 0) not in members


def test_store_refuses_limits_and_the_sharded_index_by_name():
    s = _fill(_store())
    for bad in (0, 33):
        with pytest.raises(ValueError, match="k = "):
            s.search_groups(_txt(0, 0), k=bad)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="group_size"):
            s.search_groups(_txt(0, 0), group_size=bad)
        with pytest.raises(ValueError, match="group_size"):
            s.similarity_search_by_document(_txt(0, 0), chunks_per_document=bad)
    bare = _store(factory=plain_factory, name="grp_bare")
    bare.add_texts(["a", "b"])
    with pytest.raises(NotImplementedError, match="OracleIndex has no group_search"):
        bare.search_groups("a")
    from archi_amd.sharded import ShardedHipIndex
    assert not hasattr(ShardedHipIndex, "group_search")                  # what the store's refusal keys on
    assert _store(name="grp_empty").search_groups("a") == []


def test_hybrid_store_inherits_the_methods():
    from archi_amd.vectorstore import ArchiHipHybridVectorStore
    for name in ("search_groups", "search_groups_by_vector", "similarity_search_by_document", "similarity_search_by_document_with_score"):
        assert getattr(ArchiHipHybridVectorStore, name) is getattr(ArchiHipVectorStore, name)


def test_store_rebuilds_stale_keys_and_searches_again_when_a_row_vanishes():
    s = _fill(_store())
    col = s._collection()
    orig, calls = col.index.group_search, []

    def racing(queries, k, g, **kw):
        calls.append(kw["filter_epoch"])
        if len(calls) == 1:                                              # a writer adds a row between the key array and the scan
            s.add_texts(["late note"], metadatas=[{"part": 9}])
        out = orig(queries, k, g, **kw)                                  # call 1 raises StaleFilterError: no mask, stale keys
        if len(calls) == 2:                                              # a writer deletes the best chunk before its text is read
            victim = int(out[0][0, 0, 0])
            col.table.kill(victim)
            col.table.version += 1
            col.index.remove([victim])
        return out
    col.index.group_search = racing
    got = s.search_groups(_txt(1, 4), k=3, group_size=2)
    assert len(calls) == 3 and calls[0] != calls[1] == calls[2]
    assert len(got) == 3 and _txt(1, 4) not in [d.page_content for _, mem in got for d, _ in mem]
    col.index.group_search = orig                                        # the answer is the later state's, whole
    strip = lambda res: [(v, [(d.page_content, sc) for d, sc in mem]) for v, mem in res]      # noqa: E731
    assert strip(got) == strip(s.search_groups(_txt(1, 4), k=3, group_size=2))
