"""Cases and inputs of tests/test_rerank_panel_gpu.py, shared with its child (tests/rerank_panel_worker.py): small indexes, crafted
candidate arrays, and the numpy statement of the distance key.

A case is one index (dtype, metric, dim; 8 192 rows) and one candidate array cand [nq][kp]. The launch-level cases cover, between
them: the three stored types and the three metrics (all nine pairs at dim 768), dim 64 (one panel of a 16-bit row), 192 (three
panels: one super-panel; an f32 row has six), 768 and 4096 (the largest the panel kernel takes), kp 64 / 128 / 512, and nq 1 / 3 / 65
(every pair of kp and nq at dim 768). kp = 70 is what the lexical and the id-list callers pass: a list that is no multiple of a
wave's 64 candidates."""
import numpy as np

N_ROWS = 8192
KEY_INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_DIM = 4096                      # the panel kernel's largest row (TAIL_MAX_DIM)

DTYPES = ("bf16", "f16", "f32")
METRICS = ("cosine", "inner_product", "l2")


def _case(dtype, metric, dim, kp, nq, oracle=False):
    return {"name": f"{dtype}-{metric}-d{dim}-kp{kp}-q{nq}", "dtype": dtype, "metric": metric, "dim": dim, "kp": kp, "nq": nq,
            "oracle": oracle}


def _cases():
    out = []
    shapes = [(kp, nq) for kp in (64, 128, 512) for nq in (1, 3, 65)]
    pairs = [(d, m) for d in DTYPES for m in METRICS]
    for i, (d, m) in enumerate(pairs):                       # dim 768: every (dtype, metric) and every (kp, nq)
        kp, nq = shapes[i]
        out.append(_case(d, m, 768, kp, nq, oracle=nq <= 3))
    # the other dims: every dtype and every metric once per dim
    for dim, rot in ((64, 0), (192, 1), (MAX_DIM, 2)):
        for j, d in enumerate(DTYPES):
            kp, nq = shapes[(3 * j + rot * 4 + 1) % 9]
            out.append(_case(d, METRICS[(j + rot) % 3], dim, kp, nq, oracle=(dim != MAX_DIM and nq <= 3)))
    out.append(_case("bf16", "cosine", 768, 70, 3, oracle=True))
    out.append(_case("f32", "l2", 192, 512, 65, oracle=False))
    return out


CASES = _cases()
REFUSED = [("bf16", "cosine", MAX_DIM + 64), ("f32", "l2", 96)]      # dim above the query staging; dim % 64 != 0


def rows_and_queries(c):
    """Gaussian rows; unit length for cosine, lengths 0.25 .. 4 for the inner product and L2 (queries too)."""
    rng = np.random.default_rng(sum(map(ord, c["dtype"] + c["metric"])) * 7919 + c["dim"])
    x = rng.standard_normal((N_ROWS, c["dim"]), dtype=np.float32)
    q = rng.standard_normal((65, c["dim"]), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    if c["metric"] != "cosine":
        x *= rng.uniform(0.25, 4.0, size=(N_ROWS, 1)).astype(np.float32)
        q *= rng.uniform(0.25, 4.0, size=(65, 1)).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(q[:c["nq"]], dtype=np.float32)


def candidates(c):
    """cand [nq][kp]: random approximate-score bits above the row slot. Every list holds slot 0, the last slot and three rows that
    all queries share; the first list has KEY_INVALID in the middle and at its end; with three or more queries list 1 is all
    invalid and list 2 has one whole wave (64 entries) invalid and a wave with a single valid entry where kp allows."""
    nq, kp = c["nq"], c["kp"]
    rng = np.random.default_rng(1000 + kp * 131 + nq)
    slots = rng.integers(0, N_ROWS, size=(nq, kp), dtype=np.int64)
    slots[:, 0] = 0
    slots[:, kp - 1] = N_ROWS - 1
    slots[:, [5, 17, 40]] = [N_ROWS - 1, 4099, 77]
    hi = rng.integers(0, 0xFFFFFFFF, size=(nq, kp), dtype=np.int64)           # < 0xffffffff: never KEY_INVALID by accident
    cand = (hi.astype(np.uint64) << np.uint64(32)) | slots.astype(np.uint64)
    cand[0, [3, kp // 2, kp // 2 + 1]] = KEY_INVALID
    cand[0, kp - 6:] = KEY_INVALID
    if nq >= 3:
        cand[1, :] = KEY_INVALID
        if kp >= 128:
            cand[2, 64:128] = KEY_INVALID
        if kp >= 256:
            cand[2, 128:192] = KEY_INVALID
            cand[2, 150] = (np.uint64(12345) << np.uint64(32)) | np.uint64(N_ROWS - 1)
    return np.ascontiguousarray(cand)


def dist_key(d):
    """csrc/common.h dist_key in numpy: float64 distances -> ascending uint64 keys (-0.0 as +0.0, one NaN key above +inf)."""
    d = np.array(d, dtype=np.float64)                        # a copy
    d[d == 0.0] = 0.0
    u = d.view(np.uint64)
    neg = (u >> np.uint64(63)) != 0
    k = np.where(neg, ~u, u | np.uint64(0x8000000000000000))
    return np.where(np.isnan(d), np.uint64(0xFFF8000000000000), k)
