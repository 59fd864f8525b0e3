"""The int8 shadow with one scale per FILTER CLASS (csrc/shadow8_scale.h, k_shadow8) under the int8 tile's whole-tile filter on
bounds (scan.hip, tile_epilogue): classes that mix adopting rows with rows on their own scale, peaky rows, a shadow built after
removals, an append that lands inside a published class, classes with a zero row or a row with an infinity. Every case forces tile P
and AK_SCAN_I8 = 2 at D = 256 like tests/test_scan_i8_gpu.py, and the bar is that file's: ids and float8 distance bits equal to the
oracle's, `fast_only` certifying at least 0.9 of the queries on benign data, `auto` equal always, the int8 path counted."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import knn_oracle as ko

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture
def i8_on_p():
    from archi_amd import _lib
    _lib.debug_set("AK_SCAN_CFG", "P")
    _lib.debug_set("AK_SCAN_I8", "2")
    yield _lib.debug_set
    for name in ("AK_SCAN_CFG", "AK_SCAN_I8"):
        _lib.debug_set(name, None)


def _index(rows, dtype, metric, ids=None, capacity=None):
    from archi_amd.index import HipIndex
    ix = HipIndex(rows.shape[1], capacity or len(rows), dtype=dtype, metric=metric, device=0)
    ix.add(rows, ids=ids)
    return ix


def _hold_to_oracle(ix, stored, q, k, metric, ids=None, alive=None, row_filter=None, min_certified=0.9):
    nq = len(q)
    plan = ix.scan_plan(nq, k)
    assert plan["cfg_name"] == "256x256" and plan["kprime"] == 512, plan
    oi, od, oc = ko.search(stored, q, k, metric, ids=ids, alive=alive)
    before = ix.i8_info()["searches"]
    if min_certified > 0:
        gi, gd, gc, st = ix.search(q, k, mode="fast_only", row_filter=row_filter, return_stats=True)
        info = ix.i8_info()
        assert info["searches"] == before + 1 and info["rows"] == ix.slots, info
        print(f"certified {st['certified']} / {nq}, reranked {st['reranked']}, max rho8 {info['max_rho']:.5f}")
        assert st["certified"] >= min_certified * nq, st
        if st["certified"] == nq:
            assert np.array_equal(gi, oi) and np.array_equal(gd, od, equal_nan=True)
        before += 1
    ai, ad, ac = ix.search(q, k, mode="auto", row_filter=row_filter)
    info = ix.i8_info()
    assert info["searches"] >= before + 1 and info["rows"] == ix.slots, info
    assert np.array_equal(ai, oi), f"ids differ: {np.argwhere(ai != oi)[:5]}"
    assert np.array_equal(ad, od, equal_nan=True) and np.array_equal(ac, oc)
    return oi


@pytest.mark.parametrize("nq", [64, 300])
def test_classes_that_mix_long_and_short_rows(hip, i8_on_p, nq):
    """4173 x 256 f16, inner product, a last tile of 77 rows; 300 queries are a padded second group. Rows with row bit 0 set are 8
    times as long as the others, so every class holds both: the long rows share the class's term and the cap keeps the short
    ones on their own scales -- no class is uniform and the filter's bound is an upper bound only. Rows lean against and queries
    towards one common direction u (0.3 of their length, the rest orthogonal to u), which keeps the unplanted inner products
    below 8 (0.91 * 3.6 / 16 - 0.09) = 0.92: query i's nearest neighbour is planted on a long row (8 * 0.82) and another of its
    ten on the short row beside it (the query itself: 1.0), in the same 8-row site; every eighth query has the pair in the tail
    tile."""
    rng = np.random.default_rng(2301)
    n, d = 4173, 256
    u = np.full(d, 1.0 / 16.0, dtype=np.float32)

    def perp(m):
        x = rng.standard_normal((m, d)).astype(np.float32)
        x -= np.outer(x @ u, u)
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    lean = lambda x, sign: (np.sqrt(np.float32(0.91)) * x + sign * np.float32(0.3) * u).astype(np.float32)
    xq = perp(nq)
    rows, q = lean(perp(n), -1.0), lean(xq, 1.0)
    rows[(np.arange(n) & 1) != 0] *= 8.0
    i = np.arange(nq)
    planted = np.where(i % 8 == 7, 4096 + 2 * (i // 8) + 1, 2 * (i * 6) + 1)
    assert planted.max() < n and len(np.unique(planted)) == nq and (planted & 1).all()
    rows[planted] = 8.0 * lean(xq, -1.0)          # the query's own direction leaning the rows' way: far from every other query
    rows[planted - 1] = q
    ix = _index(rows, "f16", "inner_product")
    oi = _hold_to_oracle(ix, ko.round_through(rows, "f16"), q, 10, "inner_product")
    assert np.array_equal(oi[:, 0], planted) and (oi == (planted - 1)[:, None]).any(axis=1).all()       # the test's own premise
    ix.close()


def test_peaky_rows_on_cosine(hip, i8_on_p):
    """8192 x 256 bf16: one row in 64 has a single dominant component -- mild (its class's rows adopt its coarser scale) and
    strong (beyond the cap: the class's other rows keep their own) alternately. Neighbours are planted ON such rows (the first
    eight queries, peaky themselves) and BESIDE them, in the peaky row's class."""
    rng = np.random.default_rng(2302)
    n, d, nq = 8192, 256, 128
    rows, q = _unit(rng, n, d), _unit(rng, nq, d)
    peaky = np.arange(n // 64) * 64 + (np.arange(n // 64) * 5) % 32
    for j, p in enumerate(peaky):
        rows[p] *= 1.0 if j % 2 == 0 else 0.8
        rows[p, (2 * j) % d] += 0.22 if j % 2 == 0 else 0.45
        rows[p] /= np.linalg.norm(rows[p])
    q[:8] = rows[peaky[:8]] + 0.02 * _unit(rng, 8, d)
    beside = peaky[8:72] ^ 1                                   # the same 4-row group: the same class, the same site
    rows[beside] = q[8:72]
    planted = np.concatenate([peaky[:8], beside])
    ix = _index(rows, "bf16", "cosine")
    oi = _hold_to_oracle(ix, ko.round_through(rows, "bf16"), q, 10, "cosine")
    assert np.array_equal(oi[:72, 0], planted)
    ix.close()


def test_shadow_built_after_removals_with_a_row_filter(hip, i8_on_p):
    """16461 x 256 bf16, 130 queries: 3000 rows are removed BEFORE the first search, so the shadow is built over classes with
    removed rows (ea = 0: they keep their own scale and contribute nothing to the class's term); then a 50 % row filter on top."""
    rng = np.random.default_rng(2303)
    n, d, nq = 16461, 256, 130
    rows, q = _unit(rng, n, d), _unit(rng, nq, d)
    ids = rng.permutation(10 * n)[:n].astype(np.int64)
    planted = rng.permutation(n)[:nq]
    rows[planted] = q
    ix = _index(rows, "bf16", "cosine", ids=ids)
    kill = ids[np.setdiff1d(rng.permutation(n)[:3200], planted)[:3000]]
    assert ix.remove(kill) == 3000 and ix.i8_info()["builds"] == 0
    alive = np.isin(ids, kill, invert=True).astype(np.uint8)
    stored = ko.round_through(rows, "bf16")
    oi = _hold_to_oracle(ix, stored, q, 10, "cosine", ids=ids, alive=alive)
    assert np.array_equal(oi[:, 0], ids[planted]) and ix.i8_info()["builds"] == 1
    flt = (rng.random(n) < 0.5).astype(np.uint8)
    _hold_to_oracle(ix, stored, q, 10, "cosine", ids=ids, alive=alive & flt, row_filter=flt)
    ix.close()


def test_append_boundary_inside_a_class(hip, i8_on_p):
    """Build at n0 = 20013 (13 rows into a 32-row block), search, add 5000 rows whose first nineteen -- the rest of that block --
    are peakier than the published rows of their classes, search again: the published rows keep their codes and terms, the new
    rows take the class's term from them and from their own products, the block is mixed. Results stay the oracle's, the shadow
    is extended (builds == 1), and every query's nearest neighbour arrives with the second batch -- two of them in the mixed
    block."""
    rng = np.random.default_rng(2304)
    n0, d, nq, extra = 20013, 256, 64, 5000
    rows, q = _unit(rng, n0 + extra, d), _unit(rng, nq, d)
    first = np.arange(n0, n0 + 19)
    rows[first, np.arange(19) * 7] += 0.3
    rows[first] /= np.linalg.norm(rows[first], axis=1, keepdims=True)
    planted = n0 + 40 + np.arange(nq) * 70
    planted[0], planted[1] = n0 + 2, n0 + 7                    # rows 15 and 20 of the mixed block: one of either class
    rows[planted] = q
    # rows of the PUBLISHED part of the mixed block must stay findable after the append: the second neighbours of queries 2 and 3
    rows[n0 - 3] = q[2] + 0.3 * _unit(rng, 1, d)[0]
    rows[n0 - 9] = q[3] + 0.3 * _unit(rng, 1, d)[0]
    ids = np.arange(1, n0 + extra + 1, dtype=np.int64)
    ix = _index(rows[:n0], "bf16", "cosine", ids=ids[:n0], capacity=n0 + extra)
    stored = ko.round_through(rows, "bf16")
    oi = _hold_to_oracle(ix, stored[:n0], q, 10, "cosine", ids=ids[:n0])
    assert oi[2, 0] == ids[n0 - 3] and oi[3, 0] == ids[n0 - 9]
    assert ix.i8_info()["builds"] == 1 and ix.i8_info()["rows"] == n0
    ix.add(rows[n0:], ids=ids[n0:])
    oi = _hold_to_oracle(ix, stored, q, 10, "cosine", ids=ids)
    assert np.array_equal(oi[:, 0], ids[planted])
    assert oi[2, 1] == ids[n0 - 3] and oi[3, 1] == ids[n0 - 9]
    assert ix.i8_info()["builds"] == 1                         # extended, not rebuilt
    ix.close()


def test_classes_with_a_zero_row_and_a_row_with_an_infinity(hip, i8_on_p):
    """A row of zeros and a row with an infinity sit in the very 4-row groups that hold planted neighbours: they keep scale 0 and an
    all-zero shadow, contribute nothing to the class's term and have no finite score. `auto` mode only."""
    rng = np.random.default_rng(2305)
    n, d, nq = 8192, 256, 64
    rows, q = _unit(rng, n, d), _unit(rng, nq, d)
    planted = np.arange(nq) * 124 + 4 * (np.arange(nq) % 8)     # rows = 0 mod 4
    rows[planted] = q
    rows[planted[0::2] + 1] = 0.0
    rows[planted[1::2] + 1, np.arange(nq // 2) * 3] = np.inf
    ix = _index(rows, "bf16", "cosine")
    oi = _hold_to_oracle(ix, ko.round_through(rows, "bf16"), q, 10, "cosine", min_certified=0.0)
    assert np.array_equal(oi[:, 0], planted)
    ix.close()


def test_uniform_corpus_enters_no_site_without_a_hit():
    """libarchi_hip_dbg.so, a child process (one library per process): 8192 x 256 unit rows, 256 queries, the instrumented main
    pass. The CPU restatement (tests/test_shadow8_class_cpu.py) says every row of this corpus adopts its class's scale -- asserted
    first --, so the bound of every site is its exact maximum and the whole-tile filter enters a lane-site only where it appends:
    the wave counters of entered-and-empty lane-sites (high half of counter 5) are all 0 while sites were entered."""
    if not os.path.exists(os.path.join(ROOT, "archi_amd", "lib", "libarchi_hip_dbg.so")):
        pytest.fail("libarchi_hip_dbg.so not built (make -C archi_amd/csrc dbg)")
    from tests import test_shadow8_class_cpu as cpu
    n, d, nq = 8192, 256, 256
    stored = ko.gen_rows(1234, 0, 0, n, d, True, "bf16")
    assert cpu.quantise_rows(stored, cpu.cosine_ea(stored))["adopt"].all()
    code = (
        "import sys, json, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from archi_amd import _lib\n"
        "from archi_amd.index import HipIndex\n"
        "from oracle import knn_oracle as ko\n"
        "assert _lib.is_dbg_library()\n"
        f"n, d, nq = {n}, {d}, {nq}\n"
        "ix = HipIndex(d, n, dtype='bf16', metric='cosine', device=0)\n"
        "ix.generate(seed=1234, n=n, normalise=True)\n"
        "stored = ko.gen_rows(1234, 0, 0, n, d, True, 'bf16')\n"
        "q = ko.gen_rows(4321, 1, 0, nq, d, True, 'f32')\n"
        "oi, od, oc = ko.search(stored, q, 10, 'cosine')\n"
        "_lib.debug_set('AK_SCAN_CFG', 'P')\n"
        "_lib.debug_set('AK_SCAN_I8', '2')\n"
        "_lib.debug_set('AK_SCAN_DBG', '1')\n"
        "gi, gd, gc, st = ix.search(q, 10, mode='fast_only', return_stats=True)\n"
        "assert ix.i8_info()['searches'] == 1 and st['certified'] >= 0.9 * nq, (ix.i8_info(), st)\n"
        "ai, ad, ac = ix.search(q, 10, mode='auto')\n"
        "assert np.array_equal(ai, oi) and np.array_equal(ad, od)\n"
        "main = ix.debug_read()[1]\n"
        "main = main[main[:, 7] > 0]\n"
        "print('RESULT ' + json.dumps({'waves': len(main), 'entered_lane0': int((main[:, 5] & 0xffffffff).sum()), 'empty': int((main[:, 5] >> 32).sum())}))\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AK_")}
    env["ARCHI_HIP_DBG"] = "1"
    p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode("utf-8", "replace")[-3000:]
    res = json.loads([l for l in p.stdout.decode().splitlines() if l.startswith("RESULT ")][-1][7:])
    print(res)
    assert res["waves"] > 0 and res["entered_lane0"] > 0 and res["empty"] == 0, res
