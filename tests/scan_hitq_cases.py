"""Cases of the queued filter's GPU tests (tests/test_scan_hitq_gpu.py runs them on the product library, tests/scan_hitq_worker.py in a
child process on the dbg library under both arrangements). A case is a corpus, queries, the switches that shape its plan and what
becomes of the corpus before the search; build(name) makes it from a fixed seed, so both processes hold the same arrays."""
import numpy as np

K = 10
# tile P with the int8 plan wherever the shape allows, as tests/test_scan_split_gpu.py forces it
BASE_SWITCHES = {"AK_SCAN_CFG": "P", "AK_SCAN_I8": "2"}
ALL_SWITCHES = ("AK_SCAN_CFG", "AK_SCAN_I8", "AK_SEED_RATIO", "AK_SEED_DIV", "AK_SCAN_BLOCKS", "AK_SCAN_NOPRE")
CASES = ("tail-d256", "tail-d384", "seed-one-tile", "filtered-300", "one-query", "overflow")
OVERFLOW_EPS = 0.002          # length of the perturbation of query 0 in the overflow case, relative to the query


def unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def plant(rows, q, n):
    """Nearest neighbours where a drain that works on the wrong tile's row base, row mask or term parity loses them: the last row,
    the first row of the last (partial) tile, the first rows behind the first two tile boundaries, a row inside the partial tile."""
    last_tile = (n - 1) // 256 * 256
    at = np.array([n - 1, last_tile, 256, 512, min(n - 1, last_tile + 40)])[: len(q)]
    rows[at] = q[: len(at)]
    return at


def build(name):
    """-> dict(rows, q, switches, and per case: planted, ids, kill, row_filter)."""
    c = {"switches": dict(BASE_SWITCHES), "planted": None, "ids": None, "kill": None, "row_filter": None}
    if name in ("tail-d256", "tail-d384"):
        # 17 tiles, the last of 77 rows; two and three K-steps of 128 int8 elements: term parity and the tail mask in the drain
        rng = np.random.default_rng(3101)
        n, d, nq = 4173, int(name[-3:]), 70
        c["rows"], c["q"] = unit(rng, n, d), unit(rng, nq, d)
        c["planted"] = plant(c["rows"], c["q"], n)
    elif name == "seed-one-tile":
        # 257 tiles with a seeding pass of eight workgroups of ONE tile each
        rng = np.random.default_rng(3102)
        n, d, nq = 65613, 256, 256
        c["rows"], c["q"] = unit(rng, n, d), unit(rng, nq, d)
        c["planted"] = plant(c["rows"], c["q"], n)
        c["rows"][100] = c["q"][5]                                  # ... and a neighbour inside the seeding pass's rows
        c["planted"] = np.append(c["planted"], 100)
        c["switches"].update(AK_SEED_RATIO="1", AK_SEED_DIV="32")
    elif name == "filtered-300":
        # 300 queries (a padded second query group), 7000 removed rows and a 50 % row filter: the terms written with plain stores
        rng = np.random.default_rng(3103)
        n, d, nq = 70001, 256, 300
        c["rows"], c["q"] = unit(rng, n, d), unit(rng, nq, d)
        c["ids"] = rng.permutation(10 * n)[:n].astype(np.int64)
        c["kill"] = c["ids"][rng.permutation(n)[:7000]]
        c["row_filter"] = (rng.random(n) < 0.5).astype(np.uint8)
        c["switches"].update(AK_SCAN_BLOCKS="64")
    elif name == "one-query":
        # 255 padded columns whose threshold is +inf beside one that appends
        rng = np.random.default_rng(3105)
        n, d = 4173, 384
        c["rows"], c["q"] = unit(rng, n, d), unit(rng, 1, d)
        c["planted"] = plant(c["rows"], c["q"], n)
    elif name == "overflow":
        # rows ordered by increasing similarity to query 0 on eight workgroups of eight consecutive tiles, no pre-seeding, and 130
        # queries that are query 0 plus a small perturbation: (nearly) every row of a tile beats every query's running threshold, so a
        # wave queues far more than 64 entries per tile and compactions are raised tile after tile (overflow_premise below)
        rng = np.random.default_rng(3104)
        n, d, nq = 16384, 256, 130
        rows, q0 = unit(rng, n, d), unit(rng, 1, d)
        q = q0 + OVERFLOW_EPS * unit(rng, nq, d)
        q[0] = q0[0]
        c["q"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
        c["rows"] = rows[np.argsort(rows @ q0[0])]
        c["switches"].update(AK_SCAN_BLOCKS="8", AK_SCAN_NOPRE="1")
    else:
        raise KeyError(name)
    return c


def overflow_premise(stored, q, k=K, tiles_per_workgroup=8):
    """Lane-sites that MUST be queued, per (wave, tile), of the overflow case's waves that hold the first 64 queries -- the smallest
    count over all tiles of all workgroups, first tiles excluded (their thresholds are still -max: every lane-site is queued).
    While a workgroup filters tile t, a query's threshold is at most the k-th best APPROXIMATE score of the workgroup's earlier tiles
    minus 3 eps, and an approximate score is within eps of the exact one: a row whose exact similarity reaches the exact k-th best of
    the earlier tiles reaches the threshold. A lane-site is 8 rows of one query, so a wave (128 rows x 64 queries) queues at least
    such pairs / 8 entries per tile."""
    sim = stored.astype(np.float64) @ q[:64].astype(np.float64).T            # cosine of unit rows: the order of the scores
    worst = None
    for t in range(len(stored) // 256):
        first = t - t % tiles_per_workgroup
        if t == first:
            continue
        kth = np.sort(sim[first * 256: t * 256], axis=0)[-k]                   # per query, over the workgroup's earlier tiles
        for half in (0, 1):                                                    # the two wave rows of the tile
            must = int((sim[t * 256 + 128 * half: t * 256 + 128 * half + 128] >= kth).sum())
            worst = must // 8 if worst is None else min(worst, must // 8)
    return worst
