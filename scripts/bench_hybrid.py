"""hybrid_search with the BM25 index in HBM (archi_amd.lexical.DeviceBm25, csrc/lexical.hip) against the host scorer (HostBm25).

Shape A: the 300k-chunk collection of tests/test_store_scale_gpu.py end to end through ArchiHipHybridVectorStore.hybrid_search (a
query word matches a third of the rows), twin stores, p50 / p99 of the whole query for both scorers.
Shape B: 1M x 384 f32 generated rows with synthetic lists attached through HipIndex.lex_attach (Zipf vocabulary of 200k terms,
80-160 distinct terms per row), one-term queries matching about 0.1 %, 10 % and 60 % of the rows, through HipIndex.hybrid_search.
The host scorer is not run on shape B: it needs the 1M texts in a ChunkTable.
Per query: HIP-event times of the statistics pass, the score pass (with the host's idf step between them), the hit leg's re-rank
+ select and the scan leg; for the two list passes the algorithmic bytes (entries read + per-slot arrays) and GB/s against the
8 TB/s nominal HBM rate. Every shape checks sampled answers against the brute-force formula (scalar BM25 with math.log, the oracle's
distances over all rows); exit status 1 on a mismatch. Prints ONE JSON line.

    python scripts/bench_hybrid.py [--shape a|b|ab] [--queries 50] [--rows-b 1000000]

--batch: the batch call and the coalescing of concurrent calls on shape A's collection (device scorer only), 32 distinct queries
with distinct vectors. For Q = 1, 4, 16, 32: hybrid_search_batch of Q queries against the loop of Q hybrid_search calls, the two
alternating in one job after a warm-up, medians; per-query p50 / p99 and queries per second; stage times, |U|, the sum of the
queries' own hit counts and the hit leg's share from out_info; GB/s of the list passes. Then 32 Python request threads calling
hybrid_search with the coalescer on and with AK_COALESCE=0, alternating. Every batch answer is checked against the single call's.
The JSON line also goes to profiles/hybrid_batch_bench.json.

    python scripts/bench_hybrid.py --batch [--queries 20] [--rows-a 300000]
"""
import argparse
import json
import math
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_GBS = 8000.0
TOK = re.compile(r"\w+")
SLOT_BYTES_STATS = 1 + 8 + 4 + 4          # alive, offset, count, length per slot
SLOT_BYTES_SCORE = 8 + 8 + 4 + 4 + 8      # list entry, offset, count, length, score per listed row


def pct(ms):
    a = np.sort(np.asarray(ms))
    return {"p50_ms": round(float(np.percentile(a, 50)), 3), "p99_ms": round(float(np.percentile(a, 99)), 3)}


def stage_report(infos, n_slots, arena_entries, hit_entries):
    t = np.median(np.asarray([i[6:10] for i in infos], np.float64), axis=0) / 1e6      # ms
    hits = int(infos[0][2])
    b_stats = arena_entries * 8 + n_slots * SLOT_BYTES_STATS
    b_score = hit_entries * 8 + hits * SLOT_BYTES_SCORE
    out = {"stats_pass_ms": round(t[0], 4), "score_pass_ms": round(t[1], 4), "hit_leg_ms": round(t[2], 4), "scan_leg_ms": round(t[3], 4),
           "hit_rows": hits, "stats_pass_bytes": int(b_stats), "score_pass_bytes": int(b_score)}
    if t[0] > 0:
        out["stats_pass_gbs"] = round(b_stats / t[0] / 1e6, 1)
        out["stats_pass_hbm_share"] = round(b_stats / t[0] / 1e6 / HBM_GBS, 4)
    if t[1] > 0:
        out["score_pass_gbs"] = round(b_score / t[1] / 1e6, 1)
        out["score_pass_hbm_share"] = round(b_score / t[1] / 1e6 / HBM_GBS, 4)
    return out


def order_top(ids, comb, k):
    nan = comb != comb
    o = np.lexsort((ids, -np.where(nan, 0.0, comb), ~nan))[:k]
    return ids[o], comb[o]


def shape_a(args):
    from archi_amd import vectorstore as vs
    from archi_amd.lexical import DeviceBm25
    from archi_amd.vectorstore import ArchiHipHybridVectorStore, HostBm25
    from oracle import knn_oracle as ko
    n, dim, per = 300_000, 64, 50
    rng = np.random.default_rng(11)
    vec = ko.gen_rows(515, 0, 0, n, dim, True, "f32")
    vocab = np.array([f"w{i}" for i in range(2000)])
    common = rng.random(n + 5000) < 0.33
    words = rng.integers(0, 2000, size=(n + 5000, 6))
    texts = [" ".join(vocab[words[i]]) + (" detector" if common[i] else "") + (" muon" if i % 977 == 0 else "") for i in range(n)]
    qv = ko.gen_rows(99, 1, 0, 1, dim, True, "f32")[0]

    class Emb:
        def embed_query(self, text):
            return [float(x) for x in qv]

    vs.reset_collections()
    stores = {}
    for name, bm in (("host", HostBm25()), ("device", DeviceBm25())):
        s = ArchiHipHybridVectorStore({"hip": {"dtype": "f32", "capacity": 1 << 19}}, Emb(), collection_name="bench_" + name, bm25=bm)
        for lo in range(0, n, 20000):
            s.add_texts_batch([(texts[a: a + per], [{"source": "web" if (a // per) % 4 else "git"} for _ in range(per)], 1 + a // per, vec[a: a + per])
                               for a in range(lo, lo + 20000, per)])
        stores[name] = s
    res = {"rows": n, "dim": dim, "dtype": "f32", "query": "detector muon", "k": 10}
    lat = {}
    for name, s in stores.items():
        for _ in range(3):
            s.hybrid_search("detector muon", k=10)
        ms = []
        for _ in range(args.queries):
            t0 = time.perf_counter()
            s.hybrid_search("detector muon", k=10)
            ms.append((time.perf_counter() - t0) * 1e3)
        lat[name] = ms
        res[name] = pct(ms)
    res["speedup_p50"] = round(res["host"]["p50_ms"] / res["device"]["p50_ms"], 2)
    # stage times of the device query
    sd = stores["device"]
    col = sd._collection()
    ix, bm = col.index, sd._bm25
    ix.profile(True)
    terms = bm.device_query("detector muon", col.table, ix)
    infos = [ix.hybrid_search(qv, terms, bm.k1, bm.b, bm.sign, 0.7, 0.3, [], 10)[4] for _ in range(20)]
    ix.profile(False)
    toks = [set(TOK.findall(t.lower())) for t in texts]
    hit_entries = sum(len(t) for t in toks if "detector" in t or "muon" in t)
    res["stages"] = stage_report(infos, ix.slots, int(ix.lex_info()["arena_bytes"]) // 8, hit_entries)
    # check: the brute-force formula over all rows, with and without a filter
    lens = np.array([len(TOK.findall(t.lower())) for t in texts], np.float64)
    avg = int(lens.sum()) / n
    bmv = np.zeros(n)
    for w in ("detector", "muon"):
        tf = np.array([t.lower().split().count(w) for t in texts], np.float64)
        df = int((tf > 0).sum())
        idf = math.log(1.0 + (n - df + 0.5) / (df + 0.5))
        bmv = bmv + np.where(tf > 0, idf * tf * (1.2 + 1.0) / (tf + 1.2 * ((1.0 - 0.75) + 0.75 * lens / avg)), 0.0)
    dist = np.array([ko.distance("cosine", vec[i], qv) for i in range(n)])
    ok = True
    ids = np.arange(n)
    git = (ids // per) % 4 == 0
    for ws, wb, kw, allowed in ((0.7, 0.3, {}, np.ones(n, bool)), (0.5, 0.5, {"filter": {"source": "git"}}, git)):
        comb = (1.0 - dist) * ws + bmv * wb
        wi, wc = order_top(ids[allowed], comb[allowed], 10)
        want = [(texts[i], float(c)) for i, c in zip(wi.tolist(), wc.tolist())]
        for s in stores.values():
            got = [(d.page_content, sc) for d, sc in s.hybrid_search("detector muon", k=10, semantic_weight=ws, bm25_weight=wb, **kw)]
            ok = ok and got == want
    res["check_ok"] = bool(ok)
    vs.reset_collections()
    return res, ok


def synth_lists(rng, rows, vocab, cdf):
    """Zipf draws -> per row 80-160 distinct term ids ascending (fewer when 200 draws hold fewer), tf 1-4."""
    draws = np.searchsorted(cdf, rng.random((rows, 200))).astype(np.int32)
    np.minimum(draws, vocab - 1, out=draws)
    draws.sort(axis=1)
    first = np.ones(draws.shape, bool)
    first[:, 1:] = draws[:, 1:] != draws[:, :-1]
    rank = np.cumsum(first, axis=1)
    want = rng.integers(80, 161, size=(rows, 1))
    keep = first & (rank <= want)
    cnt = keep.sum(axis=1)
    terms = draws[keep]
    tfs = rng.integers(1, 5, size=len(terms)).astype(np.int32)
    ro = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    dl = np.add.reduceat(tfs, ro[:-1]).astype(np.int32)
    return ro, terms, tfs, dl


def shape_b(args):
    from archi_amd.index import HipIndex
    from oracle import knn_oracle as ko
    n, dim, vocab, k = args.rows_b, 384, 200_000, 10
    ix = HipIndex(dim, n, dtype="f32", metric="cosine")
    ix.generate(seed=1234, n=n, normalise=True)
    p = 1.0 / np.arange(1, vocab + 1)
    cdf = np.cumsum(p / p.sum())
    rng = np.random.default_rng(5)
    ix.lex_clear(7)
    parts, t0 = [], time.perf_counter()
    for lo in range(0, n, 100_000):
        rows = min(100_000, n - lo)
        ro, te, tf, dl = synth_lists(rng, rows, vocab, cdf)
        ix.lex_attach(np.arange(lo, lo + rows, dtype=np.int64), ro, te, tf, dl, 7)
        parts.append((ro, te, tf, dl))
    attach_s = time.perf_counter() - t0
    cnt = np.concatenate([np.diff(x[0]) for x in parts])
    terms = np.concatenate([x[1] for x in parts])
    tfs = np.concatenate([x[2] for x in parts])
    dl = np.concatenate([x[3] for x in parts]).astype(np.float64)
    row_of = np.repeat(np.arange(n), cnt)
    df = np.bincount(terms, minlength=vocab)
    info = ix.lex_info()
    res = {"rows": n, "dim": dim, "dtype": "f32", "vocab": vocab, "entries": int(info["entries"]), "arena_bytes": int(info["arena_bytes"]),
           "entries_per_row": round(info["entries"] / n, 1), "attach_s": round(attach_s, 1), "k": k, "queries": []}
    qs = ko.gen_rows(4321, 1, 0, 4, dim, True, "f32")
    corpus = ko.gen_rows(1234, 0, 0, n, dim, True, "f32")
    ids = np.arange(n, dtype=np.int64)
    avg = int(dl.sum()) / n
    ok = True
    for target in (0.001, 0.10, 0.60):
        t = int(np.argmin(np.abs(df / n - target)))
        q = qs[0]
        ix.profile(False)
        for _ in range(3):
            ix.hybrid_search(q, [t], 1.2, 0.75, 1.0, 0.7, 0.3, [], k)
        ms = []
        for _ in range(args.queries):
            t0 = time.perf_counter()
            ix.hybrid_search(q, [t], 1.2, 0.75, 1.0, 0.7, 0.3, [], k)
            ms.append((time.perf_counter() - t0) * 1e3)
        ix.profile(True)
        infos = [ix.hybrid_search(q, [t], 1.2, 0.75, 1.0, 0.7, 0.3, [], k)[4] for _ in range(20)]
        sel = terms == t
        hit_rows = row_of[sel]
        entry = {"term": t, "match_share": round(float(df[t]) / n, 4)}
        entry.update(pct(ms))
        entry.update(stage_report(infos, n, int(info["arena_bytes"]) // 8, int(cnt[hit_rows].sum())))
        # check: BM25 of the hit rows in the scalar formulation, the oracle's distances (hits one by one, the rest by its top-k)
        tf = tfs[sel].astype(np.float64)
        idf = math.log(1.0 + (n - int(df[t]) + 0.5) / (int(df[t]) + 0.5))
        bm = 0.0 + idf * tf * (1.2 + 1.0) / (tf + 1.2 * ((1.0 - 0.75) + 0.75 * dl[hit_rows] / avg))
        hd = np.array([ko.distance("cosine", corpus[r], q) for r in hit_rows.tolist()])
        alive = np.ones(n, np.uint8)
        alive[hit_rows] = 0
        si, sdist, sc = ko.search(corpus, q[None, :], k, "cosine", ids=ids, alive=alive)
        m = int(sc[0])
        c_id = np.concatenate([hit_rows, si[0, :m]])
        c_sc = np.concatenate([(1.0 - hd) * 0.7 + bm * 0.3, (1.0 - sdist[0, :m]) * 0.7 + 0 * 0.3])
        wi, wc = order_top(c_id, c_sc, k)
        hi, hc, gi, gd, _ = ix.hybrid_search(q, [t], 1.2, 0.75, 1.0, 0.7, 0.3, [], k)
        gi_all, gc_all = order_top(np.concatenate([hi, gi]), np.concatenate([hc, (1.0 - gd) * 0.7 + 0 * 0.3]), k)
        good = bool(np.array_equal(gi_all, wi) and np.array_equal(gc_all, wc))
        entry["check_ok"] = good
        ok = ok and good
        res["queries"].append(entry)
    ix.close()
    return res, ok


def batch_mode(args):
    import threading
    import zlib
    from archi_amd import _lib
    from archi_amd import vectorstore as vs
    from archi_amd.lexical import DeviceBm25
    from archi_amd.vectorstore import ArchiHipHybridVectorStore
    from oracle import knn_oracle as ko
    n, dim, per, k = args.rows_a, 64, 50, 10
    rng = np.random.default_rng(11)
    vec = ko.gen_rows(515, 0, 0, n, dim, True, "f32")
    vocab = np.array([f"w{i}" for i in range(2000)])
    common = rng.random(n) < 0.33
    words = rng.integers(0, 2000, size=(n, 6))
    texts = [" ".join(vocab[words[i]]) + (" detector" if common[i] else "") + (" muon" if i % 977 == 0 else "") for i in range(n)]

    class Emb:
        def embed_query(self, text):
            return [float(x) for x in ko.gen_rows(zlib.crc32(text.encode()) & 0x7fffffff, 1, 0, 1, dim, True, "f32")[0]]

    vs.reset_collections()
    s = ArchiHipHybridVectorStore({"hip": {"dtype": "f32", "capacity": 1 << 19}}, Emb(), collection_name="bench_batch", bm25=DeviceBm25())
    for lo in range(0, n, 20000):
        s.add_texts_batch([(texts[a: a + per], [{"source": "web" if (a // per) % 4 else "git"} for _ in range(per)], 1 + a // per, vec[a: a + per])
                           for a in range(lo, min(lo + 20000, n), per)])
    # half of the queries hold the frequent word (a third of the rows match), the rest only rare ones
    queries = [f"w{7 * i} w{7 * i + 1000}" + (" detector" if i % 2 == 0 else "") + (" muon" if i % 8 == 0 else "") for i in range(32)]
    col = s._collection()
    ix, bm = col.index, s._bm25
    for q in queries[:2]:
        s.hybrid_search(q, k=k)
    s.hybrid_search_batch(queries, k=k)
    flat = lambda r: [(d.page_content, sc) for d, sc in r]      # noqa: E731
    singles = [flat(s.hybrid_search(q, k=k)) for q in queries]
    ok = [flat(r) for r in s.hybrid_search_batch(queries, k=k)] == singles
    n_slots, arena = ix.slots, int(ix.lex_info()["arena_bytes"]) // 8
    res = {"rows": n, "dim": dim, "dtype": "f32", "k": k, "reps": args.queries, "batches": []}
    for Q in (1, 4, 16, 32):
        qs = queries[:Q]
        for _ in range(3):
            s.hybrid_search_batch(qs, k=k)
            [s.hybrid_search(q, k=k) for q in qs]
        tb, tl = [], []
        for _ in range(args.queries):                                # the two variants alternate
            t0 = time.perf_counter()
            s.hybrid_search_batch(qs, k=k)
            tb.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            [s.hybrid_search(q, k=k) for q in qs]
            tl.append((time.perf_counter() - t0) * 1e3)
        with s.table.lock:
            terms = [bm.device_query(q, col.table, ix) for q in qs]
        qv = np.asarray([Emb().embed_query(q) for q in qs], np.float32)
        ix.profile(True)
        infos = [ix.hybrid_search_batch(qv, terms, bm.k1, bm.b, bm.sign, 0.7, 0.3, [], k)[1] for _ in range(10)]
        ix.profile(False)
        st = {key: float(np.median([i[key] for i in infos])) / 1e6 for key in ("stats_ns", "score_ns", "hit_ns", "scan_ns")}
        info = infos[0]
        b_stats = arena * 8 + n_slots * (SLOT_BYTES_STATS + 4)
        total = sum(st.values())
        e = {"Q": Q, "batch_ms": pct(tb), "loop_ms": pct(tl), "speedup_p50": round(float(np.median(tl) / np.median(tb)), 2),
             "per_query_ms_batch": {key: round(v / Q, 4) for key, v in pct(tb).items()}, "per_query_ms_loop": {key: round(v / Q, 4) for key, v in pct(tl).items()},
             "qps_batch": round(Q / (np.median(tb) / 1e3), 1), "qps_loop": round(Q / (np.median(tl) / 1e3), 1),
             "stats_pass_ms": round(st["stats_ns"], 4), "score_pass_ms": round(st["score_ns"], 4), "hit_leg_ms": round(st["hit_ns"], 4),
             "scan_leg_ms": round(st["scan_ns"], 4), "hit_leg_share": round(st["hit_ns"] / total, 3) if total else None,
             "stats_pass_gbs": round(b_stats / st["stats_ns"] / 1e6, 1) if st["stats_ns"] else None,
             "union_rows": info["union_rows"], "own_hit_rows": info["own_hit_rows"], "pairs": info["pairs"],
             "union_over_own": round(info["union_rows"] / info["own_hit_rows"], 3) if info["own_hit_rows"] else None,
             "pairs_over_own": round(info["pairs"] / info["own_hit_rows"], 3) if info["own_hit_rows"] else None,
             "passes": [info["stats_passes"], info["score_passes"], info["scans"]]}
        res["batches"].append(e)

    # 32 request threads, each its own query, calling hybrid_search in a loop
    def threads_run(coalesce, seconds=1.0):
        _lib.debug_set("AK_COALESCE", coalesce)
        lat = [[] for _ in range(32)]
        stop = threading.Event()

        def run(j):
            while not stop.is_set():
                t0 = time.perf_counter()
                s.hybrid_search(queries[j], k=k)
                lat[j].append((time.perf_counter() - t0) * 1e3)
        ts = [threading.Thread(target=run, args=(j,)) for j in range(32)]
        t0 = time.perf_counter()
        for t in ts:
            t.start()
        time.sleep(seconds)
        stop.set()
        for t in ts:
            t.join()
        wall = time.perf_counter() - t0
        allms = np.concatenate([np.asarray(x) for x in lat])
        return len(allms) / wall, allms
    threads_run("1", 0.3), threads_run("0", 0.3)
    runs = {"1": [], "0": []}
    lats = {"1": [], "0": []}
    for _ in range(3):
        for c in ("1", "0"):
            qps, ms = threads_run(c)
            runs[c].append(qps)
            lats[c].append(ms)
    # how many calls shared an evaluation: the index-level call returns the group's size in info[10]
    _lib.debug_set("AK_COALESCE", "1")
    sizes = []
    with s.table.lock:
        tq = [bm.device_query(q, col.table, ix) for q in queries]
    qv = np.asarray([Emb().embed_query(q) for q in queries], np.float32)
    stop = threading.Event()

    def probe(j):
        while not stop.is_set():
            sizes.append(int(ix.hybrid_search(qv[j], tq[j], bm.k1, bm.b, bm.sign, 0.7, 0.3, [], k)[4][10]))
    ts = [threading.Thread(target=probe, args=(j,)) for j in range(32)]
    for t in ts:
        t.start()
    time.sleep(0.5)
    stop.set()
    for t in ts:
        t.join()
    _lib.debug_set("AK_COALESCE", None)
    sz = np.asarray(sizes)
    res["threads32"] = {"coalesced_qps": round(float(np.median(runs["1"])), 1), "uncoalesced_qps": round(float(np.median(runs["0"])), 1),
                        "coalesced": pct(np.concatenate(lats["1"])), "uncoalesced": pct(np.concatenate(lats["0"])),
                        "speedup": round(float(np.median(runs["1"]) / np.median(runs["0"])), 2),
                        "share_of_calls_served_in_a_group": round(float((sz > 0).mean()), 3), "median_group": int(np.median(sz[sz > 0])) if (sz > 0).any() else 0}
    ok = ok and [flat(s.hybrid_search(q, k=k)) for q in queries] == singles
    res["check_ok"] = bool(ok)
    vs.reset_collections()
    return res, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ab")
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--rows-a", type=int, default=300_000)
    ap.add_argument("--queries", type=int, default=50)
    ap.add_argument("--rows-b", type=int, default=1_000_000)
    args = ap.parse_args()
    from archi_amd import _lib
    _lib.init(0)
    if args.batch:
        res, ok = batch_mode(args)
        res = dict({"bench": "hybrid_batch", "hbm_nominal_gbs": HBM_GBS, "entry_bytes": 8}, **res)
        line = json.dumps(res)
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "hybrid_batch_bench.json"), "w") as f:
            f.write(line + "\n")
        print(line)
        sys.exit(0 if ok else 1)
    res = {"bench": "hybrid", "hbm_nominal_gbs": HBM_GBS, "entry_bytes": 8}
    ok = True
    if "a" in args.shape:
        res["shape_a"], good = shape_a(args)
        ok = ok and good
    if "b" in args.shape:
        res["shape_b"], good = shape_b(args)
        ok = ok and good
    res["check_ok"] = bool(ok)
    print(json.dumps(res))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
