"""CPU suite of the batch hybrid query (csrc/lexical_batch.hip, the generic coalescer of csrc/coalesce.h):
  - the evaluation the batch call uses -- ONE scan mask for all queries, every query's exact distances over the union U of the
    batch's matching rows, +0.0 for a row of U without a term of the query -- stated in numpy (tests/lexical_batch_ref.py) and held
    to the all-rows formula;
  - the entry point is declared, bound and exported by both libraries, ABI version 5;
  - the new kernels compile without spills or scratch;
  - hybrid_search_batch on the CPU store equals a loop of hybrid_search, and raises what hybrid_search raises;
  - the coalescer with hybrid requests under ThreadSanitizer and AddressSanitizer / UBSan (a stand-alone child process)."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import knn_oracle as ko
from tests import lexical_batch_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, DIM, K = 2000, 32, 10


@pytest.fixture(scope="module")
def world():
    """A seeded 2000-row corpus as CSR lists (rows of 0, 1, 2 and > 128 distinct terms; a term in 30 % of the rows and a rare one),
    dead rows, a WHERE mask, a zero-vector row, 7 queries with their oracle distances. Built once, never changed."""
    rng = np.random.default_rng(2024)
    COMMON, RARE = 7, 9
    lists = []
    for r in range(R):
        kind = r % 10
        n = 0 if kind == 0 else 1 if kind == 1 else 2 if kind == 2 else 150 if r % 400 == 3 else int(rng.integers(3, 9))
        t = set((rng.integers(20, 600, size=n) if n < 100 else rng.permutation(np.arange(20, 900))[:n]).tolist())
        if kind >= 3 and rng.random() < 0.3:
            t.add(COMMON)
        if r % 397 == 5:
            t.add(RARE)
        lists.append(sorted(t))
    assert {len(x) for x in lists} >= {0, 1, 2} and max(len(x) for x in lists) > 128
    ro = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    terms = np.concatenate([np.asarray(x, np.int32) for x in lists])
    tfs = rng.integers(1, 5, size=len(terms)).astype(np.int32)
    dl = np.array([int(tfs[ro[r]: ro[r + 1]].sum()) for r in range(R)], np.int32)
    vec = ko.gen_rows(77, 0, 0, R, DIM, True, "f32").copy()
    ZERO = 1234                                           # a zero-vector row: NaN under cosine, ranked first; the store lists it as `also`
    vec[ZERO] = 0.0
    alive = np.ones(R, bool)
    alive[rng.choice(R, size=150, replace=False)] = False
    alive[ZERO] = True
    allowed = rng.random(R) < 0.6
    allowed[ZERO] = True
    long_q = rng.permutation(np.arange(20, 900))[:70].tolist()             # more than 64 distinct terms
    queries = [[COMMON, RARE], [RARE, 33, COMMON], [], [5000, 5001], [33, 33, 41, 33], [COMMON, RARE], long_q]
    qv = ko.gen_rows(78, 1, 0, len(queries), DIM, True, "f32")
    dist = np.array([[ko.distance("cosine", vec[r], qv[q]) for r in range(R)] for q in range(len(queries))])
    assert dist[0][ZERO] != dist[0][ZERO]
    return dict(ro=ro, terms=terms, tfs=tfs, dl=dl, alive=alive, allowed=allowed, queries=queries, dist=dist, zero=ZERO, bm={})


def _bm(world, sign):
    if sign not in world["bm"]:
        got = [br.bm25_rows(world["ro"], world["terms"], world["tfs"], world["dl"], world["alive"], q, 1.2, 0.75, sign) for q in world["queries"]]
        world["bm"][sign] = (np.array([g[0] for g in got]), np.array([g[1] for g in got]))
    return world["bm"][sign]


def _same_bits(a, b):
    return a.shape == b.shape and bool(np.all((a == b) | ((a != a) & (b != b)))) and bool(np.all(np.signbit(a) == np.signbit(b)))


@pytest.mark.parametrize("sign,w_b,w_s", list(itertools.product((1.0, -1.0), (0.3, 0.0, -0.3), (0.7, 0.0))))
def test_two_leg_batch_scheme_equals_the_all_rows_formula(world, sign, w_b, w_s):
    """The batch evaluation, merged per query, against the statement over all rows: with a WHERE mask and without, with the
    zero-vector row as `also`. w_s > 0: the same ids and the same float64 bits. w_s == 0 makes every row without a term tie at
    (1 - d) * 0 + 0 * w_b, and the statement's tie order (id) is not the scan's (distance) -- for the single-query call as for the
    batch; there the scores must still be equal position by position, every returned row must carry its own all-rows score bit for
    bit, and ids and bits must agree wherever the score is not the tied one at the cut (+0.0 and -0.0 tie)."""
    bms, hits = _bm(world, sign)
    dist, alive = world["dist"], world["alive"]
    for allowed in (world["allowed"], np.ones(R, bool)):
        U, legs = br.two_leg_batch(dist, bms, hits, alive, allowed, [world["zero"], 5, -3, R + 7], K, w_s, w_b)
        assert U[world["zero"]] and U.sum() > 100 and not U[~alive].any() and not U[~allowed].any()
        for q in range(len(dist)):
            gi, gc = br.merge(legs[q][0], legs[q][1], K, w_s, w_b)
            wi, wc = br.all_rows_topk(dist[q], bms[q], alive, allowed, K, w_s, w_b)
            comb_all = (1.0 - dist[q]) * w_s + bms[q] * w_b
            assert _same_bits(gc, comb_all[gi]), (q, gc)                     # every returned row carries the statement's score, bit for bit
            assert gi[0] == world["zero"] and gc[0] != gc[0] and len(set(gi.tolist())) == K
            if w_s > 0:
                assert np.array_equal(gi, wi) and _same_bits(gc, wc), (q, gi, wi)
                continue
            assert np.all((gc == wc) | ((gc != gc) & (wc != wc))), (q, gc, wc)
            free = wc != wc[-1]                                              # +0.0 and -0.0 tie
            assert np.array_equal(gi[free], wi[free]) and _same_bits(gc[free], wc[free]), (q, gi, wi)
    # rows move between the legs, the union does not care: a batch of one query is the single call's scheme
    for q in (0, 2, 6):
        _, one = br.two_leg_batch(dist[q: q + 1], bms[q: q + 1], hits[q: q + 1], alive, world["allowed"], [world["zero"]], K, w_s, w_b)
        _, many = br.two_leg_batch(dist, bms, hits, alive, world["allowed"], [world["zero"]], K, w_s, w_b)
        a = br.merge(one[0][0], one[0][1], K, w_s, w_b)
        b = br.merge(many[q][0], many[q][1], K, w_s, w_b)
        assert np.all((a[1] == b[1]) | (a[1] != a[1])) and (w_s == 0 or (np.array_equal(a[0], b[0]) and _same_bits(a[1], b[1])))


def test_batch_entry_point_is_declared_bound_and_exported_by_both_libraries():
    import __graft_entry__ as ge
    ge.build()
    from archi_amd import _lib
    from archi_amd.index import HipIndex
    from archi_amd.vectorstore import ArchiHipHybridVectorStore
    name = "ak_index_hybrid_search_batch"
    hdr = open(os.path.join(ROOT, "include", "archi_knn.h")).read()
    lib = _lib.load()
    assert re.search(r"\bint %s\(" % name, hdr)
    assert name in {n for n, *_ in _lib.SYMBOLS} and hasattr(lib, name)
    for so in ("libarchi_hip.so", "libarchi_hip_dbg.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "archi_amd", "lib", so)], stdout=subprocess.PIPE,
                             check=True).stdout.decode()
        assert name in set(re.findall(r"\b(ak_[a-z0-9_]+)\b", out)), so
    assert _lib.ABI_VERSION == 5 and lib.ak_abi_version() == 5 and "#define AK_ABI_VERSION 5" in hdr
    assert callable(HipIndex.hybrid_search_batch) and callable(ArchiHipHybridVectorStore.hybrid_search_batch)
    # the switches of the batch call and of the coalescer are the library's own: ak_debug_set knows them
    for switch in ("AK_LEX_BATCH_PAIRS", "AK_LEX_BATCH_TERMS", "AK_COALESCE"):
        _lib.debug_set(switch, "1")
        _lib.debug_set(switch, None)
    # the table's capacity in the kernels' file is the one the header states
    src = open(os.path.join(ROOT, "archi_amd", "csrc", "lexical_batch.hip")).read()
    assert re.search(r"constexpr int LEX_BT_CAP = 2048;", src) and "2048 distinct terms" in hdr


def test_batch_kernels_have_no_spills_and_no_scratch():
    """-Rpass-analysis=kernel-resource-usage on lexical_batch.hip with the library's flags: every kernel of the file reports 0
    spilled registers and 0 bytes of scratch."""
    from scripts.kernel_resources import HIPCC, kernel_resources
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    keys = ("SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]")
    seen = {name: {key: use[key] for key in keys if key in use} for name, use in kernel_resources("lexical_batch.hip").items()}
    kernels = ("k_lex_stats_b", "k_lex_compact_b", "k_lex_also_b", "k_lex_score_b", "k_lex_spread", "k_lex_combine_b", "k_lex_emit_b")
    assert all(any(k in n for n in seen) for k in kernels) and len(seen) == len(kernels), sorted(seen)
    for n, res in seen.items():
        assert len(res) == 3 and all(v == 0 for v in res.values()), (n, res)


class _Emb:
    """A vector per text, seeded by the text."""

    def embed_documents(self, texts):
        return [self.embed_query(t) for t in texts]

    def embed_query(self, text):
        rng = np.random.default_rng(sum(text.encode()) + 7 * len(text))
        v = rng.standard_normal(8)
        return [float(x) for x in (v / np.linalg.norm(v)).astype(np.float32)]


def test_hybrid_search_batch_on_the_cpu_store_equals_a_loop_of_hybrid_search():
    from archi_amd import vectorstore as vs
    from archi_amd.vectorstore import ArchiHipHybridVectorStore, HostBm25
    from tests.fake_index import OracleIndex

    def factory(dim, capacity, dtype, metric, shards=1):
        return OracleIndex(dim, capacity, dtype=dtype, metric=metric)
    vs.reset_collections()
    try:
        store = ArchiHipHybridVectorStore({"hip": {"dtype": "f32"}}, _Emb(), collection_name="lexbcpu", bm25=HostBm25(), index_factory=factory)
        texts = [f"chunk {i} " + ("muon " if i % 3 == 0 else "") + ("detector " if i % 2 else "") + f"w{i % 11}" for i in range(120)]
        store.add_texts(texts, [{"source": "git" if i % 4 == 0 else "web"} for i in range(120)])
        queries = ["muon detector", "", "nosuchword", "w3 muon w3", "muon detector", "detector w5 chunk"]
        for kwargs in ({}, {"filter": {"source": "git"}}, {"semantic_weight": 0.2, "bm25_weight": 0.8}):
            got = store.hybrid_search_batch(queries, k=7, **kwargs)
            want = [store.hybrid_search(q, k=7, **kwargs) for q in queries]
            assert len(got) == len(queries)
            for g, w in zip(got, want):
                assert [(d.page_content, s) for d, s in g] == [(d.page_content, s) for d, s in w] and len(g) == 7
        assert store.hybrid_search_batch([], k=3) == []
        with pytest.raises(ValueError, match="semantic_weight"):
            store.hybrid_search_batch(queries, k=3, semantic_weight=-0.1)
        none = ArchiHipHybridVectorStore({"hip": {"dtype": "f32"}}, _Emb(), collection_name="lexbcpu", index_factory=factory)
        with pytest.raises(RuntimeError, match="BM25 index"):
            none.hybrid_search_batch(queries, k=3)
        # a device scorer on an index without the lexical entry points raises, as hybrid_search does: no fallback
        from archi_amd import HipBackendError
        from archi_amd.lexical import DeviceBm25
        dev = ArchiHipHybridVectorStore({"hip": {"dtype": "f32"}}, _Emb(), collection_name="lexbcpu", bm25=DeviceBm25(), index_factory=factory)
        with pytest.raises(HipBackendError, match="HostBm25"):
            dev.hybrid_search_batch(queries, k=3)
    finally:
        vs.reset_collections()


@pytest.mark.parametrize("target,binary", [("tsan-hybrid", "hybrid_coalesce_tsan"), ("asan-hybrid", "hybrid_coalesce_asan")])
def test_hybrid_coalescer_under_sanitizers(target, binary):
    """tests/native/hybrid_coalesce_main.cpp, a stand-alone program: the generic coalescer (csrc/coalesce.h) with hybrid requests
    and a stand-in for the batch call, 32 threads, under -fsanitize=thread and -fsanitize=address,undefined. It pins the grouping
    key (calls that differ in k, any weight or BM25 parameter -- by one bit --, or the filter's pointer, length or epoch are never
    served together; equal ones are), that every request is served once with its own rows, that a group's error reaches all its
    members and nobody else, and that no request is touched after its owner left. A report or a wrong answer exits non-zero."""
    import shutil
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    csrc = os.path.join(ROOT, "archi_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, target], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    p = subprocess.run([os.path.join(csrc, "build", binary)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.startswith("ok:") and "Sanitizer" not in out, out[-3000:]
    # the search coalescer's own harness still builds from the same header, unchanged
    assert "using Coalescer = CoalescerT<SearchReq>;" in open(os.path.join(csrc, "coalesce.h")).read()
