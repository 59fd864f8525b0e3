"""CPU suite of the device BM25 / hybrid query (csrc/lexical.hip, archi_amd/lexical.py): the new entry points are declared, bound and
exported; the CSR encoding is HostBm25's postings transposed; the doc-major reference the kernels restate equals HostBm25 bit for
bit; DeviceBm25 refuses an index without the lexical entry points; the new kernels compile without spills or scratch."""
import os
import re
import subprocess

import numpy as np
import pytest

from archi_amd.chunktable import ChunkTable
from archi_amd.lexical import DeviceBm25, encode_rows
from archi_amd.vectorstore import HostBm25
from tests import lexical_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ak_index_lex_attach", "ak_index_lex_clear", "ak_index_lex_info", "ak_index_lex_scores", "ak_index_hybrid_search")


def test_lexical_entry_points_are_declared_bound_and_exported_by_both_libraries():
    import __graft_entry__ as ge
    ge.build()
    from archi_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    bound = {n for n, *_ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in bound and hasattr(lib, name), name
    for so in ("libarchi_hip.so", "libarchi_hip_dbg.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "archi_amd", "lib", so)], stdout=subprocess.PIPE,
                             check=True).stdout.decode()
        exported = set(re.findall(r"\b(ak_[a-z0-9_]+)\b", out))
        assert set(NEW) <= exported, (so, set(NEW) - exported)
    assert _lib.ABI_VERSION == 5 and lib.ak_abi_version() == 5 and "#define AK_ABI_VERSION 5" in hdr
    import archi_amd
    assert archi_amd.DeviceBm25 is DeviceBm25


def _table(texts, dead=()):
    t = ChunkTable()
    for i, tx in enumerate(texts):
        t.append(t.next_id, i // 3, i % 3, tx, {})
    for i in dead:
        t.kill(int(t._ids[i]))
    return t


def _transposed(bm, npos):
    """HostBm25's postings as per-position lists [(term id, tf)] ascending in term id."""
    rows = [[] for _ in range(npos)]
    for tid in range(len(bm._ppos)):
        for p, tf in zip(bm._ppos[tid], bm._ptf[tid]):
            rows[p].append((tid, tf))
    return [sorted(r) for r in rows]


def test_csr_encoding_is_host_bm25_postings_transposed():
    texts = ["muon detector muon", "", "Größe naïve x_1 42 ÉCOLE", "the The THE größe", " ".join(["again"] * 70000), "... !!! ---",
             "dead on arrival muon", "x_1 42 naïve tail"]
    t = _table(texts, dead=(6,))
    bm = HostBm25()
    bm._sync(t)
    terms = {}
    rids, ro, te, tf, dl = encode_rows(t, 0, t.positions, terms)
    assert terms == bm._terms                                             # the same numbering: first appearance
    live = [p for p in range(t.positions) if t._alive[p]]
    assert rids.tolist() == [int(t._ids[p]) for p in live] and 6 not in live
    want = _transposed(bm, t.positions)
    for j, p in enumerate(live):
        got = list(zip(te[ro[j]: ro[j + 1]].tolist(), tf[ro[j]: ro[j + 1]].tolist()))
        assert got == want[p], p
        assert dl[j] == bm._dlen[p]
        assert all(a < b for a, b in zip(te[ro[j]: ro[j + 1]][:-1], te[ro[j]: ro[j + 1]][1:]))
    assert ro[0] == 0 and ro[-1] == len(te) == len(tf) and te.dtype == np.int32 and tf.dtype == np.int32 and ro.dtype == np.int64
    j = live.index(4)
    assert tf[ro[j]: ro[j + 1]].tolist() == [70000] and dl[j] == 70000     # a tf no 16-bit field holds
    j = live.index(2)
    words = {w: i for w, i in terms.items()}
    assert sorted(te[ro[j]: ro[j + 1]].tolist()) == sorted(words[w] for w in ("größe", "naïve", "x_1", "42", "école"))
    assert dl[live.index(1)] == 0 and ro[live.index(1)] == ro[live.index(1) + 1]       # an empty text: an empty list
    # a later range continues the dictionary
    t.append(t.next_id, 9, 0, "muon brandnew", {})
    r2 = encode_rows(t, len(texts), t.positions, terms)
    assert r2[2].tolist() == sorted([terms["muon"], terms["brandnew"]]) and terms["brandnew"] == len(terms) - 1


def _zipf_table(n, seed, empty=False):
    rng = np.random.default_rng(seed)
    vocab = np.array([f"w{i}" for i in range(3000)])
    p = 1.0 / np.arange(1, 3001) ** 1.1
    p /= p.sum()
    t = ChunkTable()
    for lo in range(0, n, 50):
        lens = rng.integers(0, 40, size=50)
        texts = ["" if empty else " ".join(vocab[rng.choice(3000, size=int(m), p=p)]) for m in lens]
        t.append_block(lo // 50, texts, [{} for _ in texts])
    return t, rng


def _check_against_host(t, bm, enc, queries, sign):
    rids, ro, te, tf, dl, terms = enc
    pos_of_row = np.searchsorted(t._ids[: t.positions], rids)
    alive = t._alive[pos_of_row]
    for q in queries:
        hpos, hsc = bm.scores_arrays(q, t)
        qt = [terms[w] for w in re.findall(r"\w+", q.lower()) if w in terms]
        rows, sc = lr.doc_major_scores(ro, te, tf, dl, alive, qt, bm.k1, bm.b, sign)
        assert np.array_equal(pos_of_row[rows], hpos), q[:40]
        assert np.array_equal(sc, hsc) and sc.dtype == np.float64, q[:40]          # the same float64 bits
    return True


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_doc_major_reference_equals_host_bm25_bit_for_bit(sign):
    t, rng = _zipf_table(5000, 7)
    for doc in rng.choice(100, size=17, replace=False).tolist():           # deletes: whole documents and single rows
        for rid in t.rids_of_document(doc):
            t.kill(rid)
    for rid in rng.choice(t.live_rids(), size=200, replace=False).tolist():
        t.kill(int(rid))
    t.append(t.next_id, 900, 0, "onlyhere onlyhere w0", {})
    t.kill(t.next_id - 1)                                                   # a term whose postings are all dead
    bm = HostBm25(sign=sign)
    terms = {}
    enc = encode_rows(t, 0, t.positions, terms) + (terms,)
    long_q = " ".join(f"w{i}" for i in rng.permutation(3000)[:200].tolist())
    assert len(set(long_q.split())) == 200
    queries = ["w0", "w1 w17 w400", "w3 w3 w2 w3 nosuchword w2", "onlyhere", "onlyhere w5", "nosuchword", "", long_q, "w2999 w0 w1500"]
    assert _check_against_host(t, bm, enc, queries, sign)
    hpos, _ = bm.scores_arrays(long_q, t)
    assert len(hpos) > 1000 and len(bm.scores_arrays("onlyhere", t)[0]) == 0


def test_doc_major_reference_when_every_row_is_empty():
    t, _ = _zipf_table(500, 3, empty=True)
    bm = HostBm25()
    terms = {}
    enc = encode_rows(t, 0, t.positions, terms) + (terms,)
    assert terms == {} and int(enc[4].sum()) == 0
    assert _check_against_host(t, bm, enc, ["w0", "", "w1 w2"], 1.0)
    # avg == 0 with lists present (only reachable through lex_attach directly): the length term drops out of the norm
    rows, sc = lr.doc_major_scores(np.array([0, 1, 1]), np.array([5]), np.array([3]), np.array([0, 0]), np.array([True, True]), [5])
    import math
    assert rows.tolist() == [0] and sc.tolist() == [((math.log(1.0 + (2 - 1 + 0.5) / (1 + 0.5)) * 3.0) * (1.2 + 1.0)) / (3.0 + 1.2 * (1.0 - 0.75))]


def test_device_bm25_refuses_an_index_without_lexical_entry_points():
    from archi_amd import HipBackendError
    from archi_amd import vectorstore as vs
    from archi_amd.vectorstore import ArchiHipHybridVectorStore
    from tests.fake_index import OracleIndex

    class Emb:
        def embed_documents(self, texts):
            return [[1.0, 0.0, 0.0, float(i)] for i in range(len(texts))]

        def embed_query(self, text):
            return [1.0, 0.0, 0.0, 0.5]

    vs.reset_collections()
    store = ArchiHipHybridVectorStore({"hip": {"dtype": "f32"}}, Emb(), collection_name="lexcpu", bm25=DeviceBm25(),
                                      index_factory=lambda dim, capacity, dtype, metric, shards=1: OracleIndex(dim, capacity, dtype=dtype, metric=metric))
    store.add_texts(["muon detector", "tracker alignment"], [{}, {}])
    with pytest.raises(HipBackendError, match="HostBm25"):
        store.hybrid_search("muon", k=2)
    with pytest.raises(HipBackendError, match="HostBm25"):
        DeviceBm25().scores("muon", store._collection().table)
    vs.reset_collections()


def test_lexical_kernels_have_no_spills_and_no_scratch():
    """-Rpass-analysis=kernel-resource-usage on lexical.hip with the library's flags: every kernel of the file reports 0 spilled
    registers and 0 bytes of scratch."""
    from scripts.kernel_resources import HIPCC, kernel_resources
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    keys = ("SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]")
    seen = {name: {key: use[key] for key in keys if key in use} for name, use in kernel_resources("lexical.hip").items()}
    kernels = ("k_lex_stats", "k_lex_compact", "k_lex_also", "k_lex_score", "k_lex_combine", "k_lex_emit", "k_lex_gather", "k_lex_scatter")
    assert all(any(k in n for n in seen) for k in kernels) and len(seen) == len(kernels), sorted(seen)
    for n, res in seen.items():
        assert len(res) == 3 and all(v == 0 for v in res.values()), (n, res)
