"""Max-marginal-relevance search (HipIndex.mmr_search, csrc/mmr.hip) on generated collections: 1M x 384 f32 and 4M x 768 bf16,
nq in {1, 32, 1024}, (k, fetch_k) in {(4, 20), (10, 128)}, lambda_mult 0.5.

Per shape, after a warm-up of every variant, three variants alternate in one job and their medians are reported:
    mmr     ix.mmr_search(q, k, fetch_k)                                          the new call
    search  ix.search(q, fetch_k)                                                 the candidate search alone: what MMR adds on top
    host    ix.search(q, fetch_k) + ix.lookup + ix.fetch + numpy MMR per query    what a caller does today (LangChain's helper:
            float64 cosine by matrix product, argmax loop)
Times are host clocks around calls that end in a device synchronise. In a run of their own (ak_index_profile on) the two kernels
are timed with HIP events; the Gram kernel's LDS read rate follows from the bytes its chains read (computed from the shapes: every
lane of a pair block reads its two A rows and two B rows once) against 150 TB/s, the chip's aggregate ds_read_b128 rate. Sampled
queries are checked against tests/mmr_ref.py (the selection, fed the rows of the library's own candidate list read back with
fetch); exit status 1 on a mismatch. Device clocks and power as rocm-smi shows them at the end are noted. Prints ONE JSON line,
also written to profiles/mmr_bench.json.

    python scripts/bench_mmr.py [--shapes 1000000x384xf32,4000000x768xbf16] [--nq 1,32,1024] [--reps 15] [--out profiles/mmr_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LDS_PEAK_BPS = 150e12          # every CU streaming ds_read_b128
KF = ((4, 20), (10, 128))
LAM = 0.5


def numpy_mmr(query, cands, lam, k):
    """What a caller runs on the host today: LangChain's maximal_marginal_relevance, float64."""
    x = np.asarray(cands, np.float64)
    xn = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-300)
    q = np.asarray(query, np.float64)
    sim_q = xn @ (q / max(np.linalg.norm(q), 1e-300))
    picked = [int(np.argmax(sim_q))]
    red = xn @ xn[picked[0]]
    while len(picked) < min(k, len(x)):
        score = lam * sim_q - (1.0 - lam) * red
        score[picked] = -np.inf
        p = int(np.argmax(score))
        picked.append(p)
        red = np.maximum(red, xn @ xn[p])
    return picked


def host_variant(ix, q, k, fk):
    ids, dist, cnt = ix.search(q, fk)
    rows = ix.fetch(ix.lookup(ids.ravel())).reshape(len(q), fk, -1)
    return [ids[i][numpy_mmr(q[i], rows[i], LAM, k)] for i in range(len(q))]


def median_ms(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def gram_lds_bytes(nq, fk, dim, es):
    nb = (fk + 31) // 32
    return nq * (nb * (nb + 1) // 2) * 256 * 4 * dim * es      # blocks x lanes x (2 A rows + 2 B rows) x row bytes


def device_state():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--json"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                             timeout=30).stdout.decode()
        card = json.loads(out).get("card0", {})
        return {k: v for k, v in card.items() if any(w in k.lower() for w in ("sclk", "mclk", "power"))}
    except Exception as e:      # noqa: BLE001 -- a note, not a measurement
        return {"unavailable": str(e)[:80]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000000x384xf32,4000000x768xbf16")
    ap.add_argument("--nq", default="1,32,1024")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmr_bench.json"))
    args = ap.parse_args()
    from archi_amd import _lib
    from archi_amd.index import HipIndex
    from oracle import knn_oracle as ko
    from tests.mmr_ref import mmr_select

    report = {"lambda_mult": LAM, "reps": args.reps, "shapes": [], "mismatches": 0}
    for shape in args.shapes.split(","):
        n, dim, dtype = shape.split("x")
        n, dim = int(n), int(dim)
        es = 4 if dtype == "f32" else 2
        ix = HipIndex(dim, n, dtype=dtype, metric="cosine")
        ix.generate(seed=2024, n=n, normalise=True)
        entry = {"rows": n, "dim": dim, "dtype": dtype, "cases": []}
        for nq in (int(x) for x in args.nq.split(",")):
            q = ko.gen_rows(4242, 1, 0, nq, dim, True, "f32")
            for k, fk in KF:
                variants = {"mmr": lambda: ix.mmr_search(q, k, fetch_k=fk, lambda_mult=LAM),
                            "search": lambda: ix.search(q, fk),
                            "host": lambda: host_variant(ix, q, k, fk)}
                for fn in variants.values():          # warm-up: code objects, scratch, the lazy id map
                    fn()
                    fn()
                times = {name: [] for name in variants}
                rounds = args.reps if nq < 1024 else max(3, args.reps // 3)
                for _ in range(rounds):               # alternating
                    for name, fn in variants.items():
                        times[name] += median_ms(fn, 1)
                case = {"nq": nq, "k": k, "fetch_k": fk, "rounds": rounds}
                for name, t in times.items():
                    case[f"{name}_p50_ms"] = round(float(np.median(t)), 4)
                    case[f"{name}_min_ms"] = round(float(np.min(t)), 4)
                case["mmr_minus_search_ms"] = round(case["mmr_p50_ms"] - case["search_p50_ms"], 4)
                # the two kernels, HIP events, in a run of their own
                ix.profile(True)
                gram, select = [], []
                for _ in range(max(5, rounds)):
                    ix.profile_read()
                    ix.mmr_search(q, k, fetch_k=fk, lambda_mult=LAM)
                    ev = ix.profile_read()
                    gram.append(float(ev[-2]))
                    select.append(float(ev[-1]))
                ix.profile(False)
                case["gram_kernel_ms"] = round(float(np.median(gram)), 5)
                case["select_kernel_ms"] = round(float(np.median(select)), 5)
                lds = gram_lds_bytes(nq, fk, dim, es)
                case["gram_lds_read_bytes"] = lds
                if case["gram_kernel_ms"] > 0:
                    case["gram_lds_read_tbs"] = round(lds / (case["gram_kernel_ms"] * 1e-3) / 1e12, 3)
                    case["gram_lds_share_of_150tbs"] = round(lds / (case["gram_kernel_ms"] * 1e-3) / LDS_PEAK_BPS, 4)
                # sampled queries against the CPU restatement, fed the library's own candidates
                gi, gd, gc, gr = ix.mmr_search(q, k, fetch_k=fk, lambda_mult=LAM, return_rank=True)
                ci, cd, cc = ix.search(q, fk)
                for qi in sorted({0, nq // 2, nq - 1}):
                    m = int(cc[qi])
                    rows = ix.fetch(ix.lookup(ci[qi, :m]))
                    want = mmr_select(rows, cd[qi, :m], k, LAM)
                    ok = gr[qi, :len(want)].tolist() == want and gi[qi, :len(want)].tolist() == ci[qi][want].tolist() and \
                        np.array_equal(gd[qi, :len(want)], cd[qi][want]) and gc[qi] == len(want)
                    if not ok:
                        report["mismatches"] += 1
                        print(f"MISMATCH {shape} nq={nq} k={k} fetch_k={fk} query {qi}: got {gr[qi].tolist()} want {want}", file=sys.stderr)
                entry["cases"].append(case)
        ix.close()
        report["shapes"].append(entry)
    report["device"] = device_state()
    name = ctypes_name(_lib)
    report["gpu"] = name
    line = json.dumps(report)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 1 if report["mismatches"] else 0


def ctypes_name(_lib):
    import ctypes
    buf = ctypes.create_string_buffer(128)
    cu, hbm = ctypes.c_int(0), ctypes.c_int64(0)
    _lib.check(_lib.load().ak_device_info(buf, 128, ctypes.byref(cu), ctypes.byref(hbm)), "ak_device_info")
    return {"name": buf.value.decode(), "cus": cu.value, "hbm_bytes": hbm.value}


if __name__ == "__main__":
    sys.exit(main())
