"""Grouped search (HipIndex.group_search, csrc/group.hip) on generated collections: 4M x 768 bf16 and 1M x 384 f32, documents of 16
chunks ("even") and the same collection with one document holding the 200 chunks nearest to the queries ("skewed"), nq in
{1, 32, 1024} (the skewed collection: 1 and 32), k = 10, group_size in {1, 3}.

Per case, after a warm-up of every variant, the variants alternate in one job and their medians are reported:
    group1 / group3   ix.group_search(q, 10, 1 | 3, row_group=keys)                the new call
    search            ix.search(q, 10)                                             the plain search of the same process
    host              ix.search(q, k') with k' doubling from 16 until a numpy collapse of the returned rows by key yields 10 groups
                      or the rows run out: what a caller does today, and exact for the same reason the library's rounds are
Times are host clocks around calls that end in a device synchronise. In a run of their own (ak_index_profile on) the kernels are
timed with HIP events: k_group_collapse and the two passes of k_group_members from an even-collection call, k_group_exclude from a
skewed one (the event list of a call is [scan launches, collapse, (exclude, scan launches, collapse) per later round, members
count, members fill]; the number of scan launches per search is read from a plain search of the same width). The rounds come
from the call's stats. AK_GROUP_FETCH is swept over 16 / 32 / 64 / 128 for group1.

Self-check, sampled queries, exit status 1 on a mismatch: the definition of include/archi_knn.h is stated on ak_index_search, so
the groups must be the host variant's (ids, distance bits, keys), and a group's members must be ix.search(q, group_size) under a
mask that keeps that group's rows only. (tests/group_ref.py needs the complete ranking on the CPU: too slow at these sizes; the
GPU tests hold the library to it on small collections.) Prints ONE JSON line, also written to profiles/group_bench.json.

    python scripts/bench_group.py [--shapes 4000000x768xbf16,1000000x384xf32] [--nq 1,32,1024] [--reps 7] [--out profiles/group_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K = 10
CHUNKS = 16
HOT = 200


def host_variant(ix, q, keys_by_id, k):
    """Exact: the first k' rows of the ranking hold its first groups (the prefix property); k' doubles until there are k of them."""
    nq = len(q)
    out = [None] * nq
    todo = np.arange(nq)
    kk = 16
    while len(todo):
        ids, dist, cnt = ix.search(q[todo], kk)
        still = []
        for j, qi in enumerate(todo):
            m = int(cnt[j])
            key = keys_by_id[ids[j, :m]]
            _, first = np.unique(key, return_index=True)
            first = np.sort(first)
            if len(first) >= k or m < kk:
                out[qi] = (ids[j, first[:k]], dist[j, first[:k]], key[first[:k]])
            else:
                still.append(qi)
        todo = np.asarray(still, dtype=np.int64)
        kk *= 2
    return out


def p50(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4000000x768xbf16,1000000x384xf32")
    ap.add_argument("--nq", default="1,32,1024")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_bench.json"))
    args = ap.parse_args()
    from archi_amd import _lib
    from archi_amd.index import HipIndex
    from oracle import knn_oracle as ko

    report = {"k": K, "chunks_per_document": CHUNKS, "reps": args.reps, "shapes": [], "mismatches": 0}
    for shape in args.shapes.split(","):
        n, dim, dtype = shape.split("x")
        n, dim = int(n), int(dim)
        ix = HipIndex(dim, n, dtype=dtype, metric="cosine")
        ix.generate(seed=2024, n=n, normalise=True)            # ids = slots
        entry = {"rows": n, "dim": dim, "dtype": dtype, "cases": []}
        base = ko.gen_rows(4242, 1, 0, 1, dim, True, "f32")
        even = (np.arange(n) // CHUNKS).astype(np.int32)
        skew = even.copy()
        skew[ix.search(base, HOT)[0][0]] = n                   # one document holds the 200 chunks nearest to the base query
        for layout, keys in (("even", even), ("skewed", skew)):
            for nq in (int(x) for x in args.nq.split(",")):
                if layout == "skewed" and nq > 32:
                    continue
                if layout == "even":
                    q = ko.gen_rows(4242, 1, 0, nq, dim, True, "f32")
                else:                                          # every query next to the base query: they all meet the hot document
                    q = base + 0.01 * ko.gen_rows(4243, 1, 0, nq, dim, True, "f32")
                    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
                variants = {"group1": lambda: ix.group_search(q, K, 1, row_group=keys),
                            "group3": lambda: ix.group_search(q, K, 3, row_group=keys),
                            "search": lambda: ix.search(q, K),
                            "host": lambda: host_variant(ix, q, keys, K)}
                for fn in variants.values():                   # warm-up: code objects, scratch, the lazy id map
                    fn()
                    fn()
                rounds = args.reps if nq < 1024 else max(3, args.reps // 2)
                times = {name: [] for name in variants}
                for _ in range(rounds):                        # alternating
                    for name, fn in variants.items():
                        times[name] += p50(fn, 1)
                case = {"layout": layout, "nq": nq, "rounds_timed": rounds}
                for name, t in times.items():
                    case[f"{name}_p50_ms"] = round(float(np.median(t)), 4)
                    case[f"{name}_min_ms"] = round(float(np.min(t)), 4)
                g1 = ix.group_search(q, K, 1, row_group=keys, return_stats=True)
                g3 = ix.group_search(q, K, 3, row_group=keys, return_stats=True)
                case["stats_group1"], case["stats_group3"] = g1[5], g3[5]
                # the kernels, HIP events, in a run of their own
                fetch = min(max(4 * K, 16), 128)
                ix.profile(True)
                ix.profile_read()
                ix.search(q[:1] if layout == "skewed" else q, fetch)
                scan_launches = len(ix.profile_read())
                if layout == "even":
                    ev = []
                    for _ in range(5):
                        ix.profile_read()
                        ix.group_search(q, K, 3, row_group=keys)
                        ev.append([float(x) for x in ix.profile_read()[-3:]])
                    med = np.median(np.asarray(ev), axis=0)
                    case["collapse_kernel_ms"], case["members_count_kernel_ms"], case["members_fill_kernel_ms"] = (round(float(x), 5) for x in med)
                elif nq == 1 and g1[5]["rounds"] > 1:
                    ex = []
                    for _ in range(5):
                        ix.profile_read()
                        ix.group_search(q, K, 1, row_group=keys)
                        ev = ix.profile_read()
                        ex.append(float(ev[scan_launches + 1]))
                    case["exclude_kernel_ms"] = round(float(np.median(ex)), 5)
                ix.profile(False)
                # AK_GROUP_FETCH sweep
                if nq <= 32:
                    sweep = {}
                    try:
                        for f in (16, 32, 64, 128):
                            _lib.debug_set("AK_GROUP_FETCH", str(f))
                            ix.group_search(q, K, 1, row_group=keys)
                            t = p50(lambda: ix.group_search(q, K, 1, row_group=keys), rounds)
                            sweep[str(f)] = {"p50_ms": round(float(np.median(t)), 4),
                                             "rounds": ix.group_search(q, K, 1, row_group=keys, return_stats=True)[5]["rounds"]}
                    finally:
                        _lib.debug_set("AK_GROUP_FETCH", None)
                    case["fetch_sweep_group1"] = sweep
                # self-check on sampled queries
                host = host_variant(ix, q, keys, K)
                for qi in sorted({0, nq // 2, nq - 1}):
                    hi, hd, hk = host[qi]
                    c = len(hi)
                    ok = g1[4][qi] == c and np.array_equal(g1[0][qi, :c, 0], hi) and np.array_equal(g1[2][qi, :c], hk) and \
                        np.array_equal(g1[1][qi, :c, 0].view(np.uint64), hd.view(np.uint64)) and \
                        g3[4][qi] == c and np.array_equal(g3[2][qi, :c], hk)
                    for w in range(c if ok else 0):
                        mi, md, mc = ix.search(q[qi], 3, row_filter=(keys == hk[w]).astype(np.uint8))
                        m = int(mc[0])
                        ok = ok and g3[3][qi, w] == m and np.array_equal(g3[0][qi, w, :m], mi[0, :m]) and \
                            np.array_equal(g3[1][qi, w, :m].view(np.uint64), md[0, :m].view(np.uint64))
                    if not ok:
                        report["mismatches"] += 1
                        print(f"MISMATCH {shape} {layout} nq={nq} query {qi}", file=sys.stderr)
                entry["cases"].append(case)
                print(json.dumps(case), file=sys.stderr, flush=True)
        ix.close()
        report["shapes"].append(entry)
    line = json.dumps(report)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 1 if report["mismatches"] else 0


if __name__ == "__main__":
    sys.exit(main())
