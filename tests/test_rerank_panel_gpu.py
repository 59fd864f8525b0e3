"""The panel re-rank kernel (csrc/exact.hip, k_rerank_panel): candidate rows fetched by neighbouring lanes, passed through
wave-private LDS images to the lanes that run the sequential float32 chains. It replaces the thread-per-candidate k_rerank behind
rerank(), which stays as the fallback and as the reference here.

Launch level (a child process on libarchi_hip_dbg.so, tests/rerank_panel_worker.py, through ak_kts_rr_rerank): the two kernels on
the same crafted candidate arrays, keys and ids equal bit for bit; for a subset, every key against the oracle's distance on the
stored row. Then through the search API in this process: the int8 plan's k' = 512 tail and the k' = 128 / 256 tails against
ko.search, each case asserting from the library's counters that candidates were re-ranked."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle import knn_oracle as ko
from tests import rerank_panel_cases as rc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_DEAD = []                   # the child ended badly: it is not started again
_RES = {}


def _child(tmp_path_factory):
    if "res" in _RES:
        return _RES["res"]
    assert not _DEAD, "not started: the child ended badly before"
    out = str(tmp_path_factory.mktemp("rerank_panel") / "launches.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AK_")}
    env["ARCHI_HIP_DBG"] = "1"
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "rerank_panel_worker.py"), out], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=300)
    except subprocess.TimeoutExpired:
        _DEAD.append(1)
        raise
    if p.returncode != 0:
        _DEAD.append(1)
    assert p.returncode == 0, f"exit {p.returncode}\n" + p.stderr.decode("utf-8", "replace")[-3000:]
    print(f"child: {time.time() - t0:.0f} s")
    _RES["res"] = np.load(out)
    return _RES["res"]


def test_case_list_is_what_the_issue_asks():
    cs = rc.CASES
    assert {(c["dtype"], c["metric"]) for c in cs if c["dim"] == 768} == {(d, m) for d in rc.DTYPES for m in rc.METRICS}
    assert {c["dim"] for c in cs} == {64, 192, 768, rc.MAX_DIM}
    assert {c["kp"] for c in cs} >= {64, 128, 512} and {c["nq"] for c in cs} == {1, 3, 65}
    assert {(c["kp"], c["nq"]) for c in cs if c["dim"] == 768} >= {(kp, nq) for kp in (64, 128, 512) for nq in (1, 3, 65)}
    for dim in (64, 192, rc.MAX_DIM):
        assert {c["dtype"] for c in cs if c["dim"] == dim} == set(rc.DTYPES)
        assert {c["metric"] for c in cs if c["dim"] == dim} == set(rc.METRICS)
    for c in cs:
        cand = rc.candidates(c)
        slots = (cand & np.uint64(0xFFFFFFFF)).astype(np.int64)
        ok = cand != rc.KEY_INVALID
        assert (slots[ok] < rc.N_ROWS).all()                                  # nothing the kernels could read out of bounds
        assert (ok & (slots == 0)).any() and (ok & (slots == rc.N_ROWS - 1)).any()
        inv0 = np.flatnonzero(~ok[0])
        assert inv0.size and inv0.min() < c["kp"] // 2 + 2 and inv0.max() == c["kp"] - 1 and ok[0].any()
        if c["nq"] >= 3:
            assert not ok[1].any()                                            # an all-invalid list
            assert all((ok[:, j] & (slots[:, j] == slots[0, j])).sum() >= 2 for j in (17, 40))   # one row under several queries
        if c["metric"] != "cosine":
            x, q = rc.rows_and_queries(c)
            n = np.linalg.norm(x, axis=1)
            assert n.min() < 0.5 and n.max() > 2.0                            # un-normalised lengths


@pytest.mark.parametrize("name", [c["name"] for c in rc.CASES])
def test_panel_kernel_equals_the_thread_per_candidate_kernel_bit_for_bit(tmp_path_factory, name):
    res = _child(tmp_path_factory)
    c = next(c for c in rc.CASES if c["name"] == name)
    cand = rc.candidates(c)
    ok, nk, oi, ni = res[f"{name}:old:keys"], res[f"{name}:new:keys"], res[f"{name}:old:ids"], res[f"{name}:new:ids"]
    assert np.array_equal(nk, ok), f"keys differ at {np.argwhere(nk != ok)[:5]}"
    assert np.array_equal(ni, oi), f"ids differ at {np.argwhere(ni != oi)[:5]}"
    # ... and the reference itself did the work: every entry written, invalid in -> invalid out, ids those of the slots
    inv = cand == rc.KEY_INVALID
    assert (ok[inv] == rc.KEY_INVALID).all() and (oi[inv] == -1).all()
    assert (ok[~inv] != rc.KEY_INVALID).all() and (ok[~inv] != np.uint64(0x5A5A5A5A5A5A5A5A)).all()
    assert np.array_equal(oi[~inv], (cand[~inv] & np.uint64(0xFFFFFFFF)).astype(np.int64) * 3 + 11)


@pytest.mark.parametrize("name", [c["name"] for c in rc.CASES if c["oracle"]])
def test_panel_kernel_keys_are_the_oracle_distances(tmp_path_factory, name):
    res = _child(tmp_path_factory)
    c = next(c for c in rc.CASES if c["name"] == name)
    rows, q = rc.rows_and_queries(c)
    stored = ko.round_through(rows, c["dtype"])
    cand = rc.candidates(c)
    want = np.full(cand.shape, rc.KEY_INVALID, dtype=np.uint64)
    for qi in range(c["nq"]):
        live = np.flatnonzero(cand[qi] != rc.KEY_INVALID)
        d = np.array([ko.distance(c["metric"], stored[int(s)], q[qi]) for s in (cand[qi, live] & np.uint64(0xFFFFFFFF))], dtype=np.float64)
        want[qi, live] = rc.dist_key(d)
    got = res[f"{name}:new:keys"]
    assert np.array_equal(got, want), f"keys differ from the oracle's at {np.argwhere(got != want)[:5]}"


def test_switch_reaches_the_old_kernel_and_refused_shapes_are_errors(tmp_path_factory):
    res = _child(tmp_path_factory)
    assert (int(res["choice:default"]), int(res["choice:old"]), int(res["choice:reset"])) == (1, 0, 1)
    # the search under AK_RERANK_OLD = 1: the int8 plan's tail (k' = 512) on the old kernel, the oracle's answers
    assert int(res["old_search:kprime"]) == 512 and int(res["old_search:reranked"]) > 0 and int(res["old_search:equal"]) == 1
    for i in range(len(rc.REFUSED)):
        assert int(res[f"refused{i}:rc"]) != 0 and "panel" in str(res[f"refused{i}:error"]), str(res[f"refused{i}:error"])
        assert int(res[f"refused{i}:untouched"]) == 1 and int(res[f"refused{i}:choice"]) == 0
        assert int(res[f"refused{i}:rc_old"]) == 0 and int(res[f"refused{i}:old_wrote"]) == 1


# ---- through the search API ------------------------------------------------------------------------------------------------------
def _gauss(rng, n, d, unit):
    x = rng.standard_normal((n, d)).astype(np.float32)
    if unit:
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x, dtype=np.float32)


@pytest.fixture
def switches():
    from archi_amd import _lib
    used = []

    def set_(name, value):
        used.append(name)
        _lib.debug_set(name, value)
    yield set_
    for name in used:
        _lib.debug_set(name, None)


def _hold_to_oracle(ix, stored, q, k, metric, kprime, alive=None, row_filter=None):
    """tests/test_scan_i8_gpu.py::_hold_to_oracle for any plan: fast_only and auto against ko.search -- ids, distance bits, counts --
    and `reranked` > 0 from the library's counters in both modes."""
    nq = len(q)
    assert ix.scan_plan(nq, k)["kprime"] == kprime, ix.scan_plan(nq, k)
    oi, od, oc = ko.search(stored, q, k, metric, alive=alive)
    gi, gd, gc, st = ix.search(q, k, mode="fast_only", row_filter=row_filter, return_stats=True)
    print(f"fast_only: certified {st['certified']} / {nq}, reranked {st['reranked']}")
    assert st["reranked"] > 0, st
    if st["certified"] == nq:
        assert np.array_equal(gi, oi) and np.array_equal(gd, od, equal_nan=True) and np.array_equal(gc, oc)
    ai, ad, ac, st2 = ix.search(q, k, mode="auto", row_filter=row_filter, return_stats=True)
    assert st2["reranked"] > 0, st2
    assert np.array_equal(ai, oi), f"ids differ: {np.argwhere(ai != oi)[:5]}"
    assert np.array_equal(ad, od, equal_nan=True) and np.array_equal(ac, oc)
    return st


@pytest.mark.parametrize("dtype,metric,d", [("bf16", "cosine", 256), ("f16", "inner_product", 384)])
def test_int8_plan_tail_matches_oracle(hip, switches, dtype, metric, d):
    from archi_amd.index import HipIndex
    switches("AK_SCAN_CFG", "P")
    switches("AK_SCAN_I8", "2")
    rng = np.random.default_rng(2101 + d)
    n, nq = 8192, 130
    rows, q = _gauss(rng, n, d, True), _gauss(rng, nq, d, True)
    if metric == "inner_product":
        rows[(np.arange(n) & 4) != 0] *= 4.0
    ix = HipIndex(d, n, dtype=dtype, metric=metric, device=0)
    ix.add(rows)
    stored = ko.round_through(rows, dtype)
    before = ix.i8_info()["searches"]
    st = _hold_to_oracle(ix, stored, q, 10, metric, 512)
    assert ix.i8_info()["searches"] == before + 2 and st["certified"] >= 0.9 * nq, (st, ix.i8_info())
    # fewer live rows than k': the lists reach the re-rank padded with invalid keys
    flt = np.zeros(n, dtype=np.uint8)
    flt[rng.permutation(n)[:300]] = 1
    st = _hold_to_oracle(ix, stored, q, 10, metric, 512, alive=flt, row_filter=flt)
    assert st["reranked"] <= 300 * nq
    ix.close()


@pytest.mark.parametrize("dtype,metric", [("f32", "l2"), ("bf16", "cosine")])
@pytest.mark.parametrize("k,kprime", [(20, 128), (64, 256)])
def test_wide_tails_match_oracle(hip, dtype, metric, k, kprime):
    from archi_amd.index import HipIndex
    rng = np.random.default_rng(2201 + k)
    n, d, nq = 8192, 192, 70
    unit = metric == "cosine"
    rows, q = _gauss(rng, n, d, unit), _gauss(rng, nq, d, unit)
    ix = HipIndex(d, n, dtype=dtype, metric=metric, device=0)
    ix.add(rows)
    stored = ko.round_through(rows, dtype)
    _hold_to_oracle(ix, stored, q, k, metric, kprime)
    flt = np.zeros(n, dtype=np.uint8)
    flt[rng.permutation(n)[:kprime - 28]] = 1                  # fewer live rows than k' (and, at k = 64, more than k)
    st = _hold_to_oracle(ix, stored, q, k, metric, kprime, alive=flt, row_filter=flt)
    assert st["reranked"] <= (kprime - 28) * nq
    ix.close()
