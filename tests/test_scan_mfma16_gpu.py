"""The phased scan tiles on the 16x16x32 MFMA shape: a lane owns query columns 16c + (lane & 15) and corpus rows
16h + 4 * (lane >> 4) + j of a 32 x 32 block, the filter groups are the 8 rows a lane holds of a 32-row block per column, and
the group bound takes the row class lane >> 4 & 1. The shapes here are the smallest at which that mapping can go wrong; the
bar is the suite's: ids and float8 distances equal to the oracle's, with the fast path certified. Whatever shape a tile ships
with in the product library is what the forced-tile cases run; the last test holds BOTH shapes of every phased tile in
libarchi_hip_dbg.so (AK_SCAN_MFMA)."""
import os

import numpy as np
import pytest

from oracle import knn_oracle as ko

pytestmark = pytest.mark.gpu


def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture
def scan_cfg():
    from archi_amd import _lib
    yield lambda cfg: _lib.debug_set("AK_SCAN_CFG", cfg)
    _lib.debug_set("AK_SCAN_CFG", None)


def _index(rows, dtype, metric, ids=None):
    from archi_amd.index import HipIndex
    ix = HipIndex(rows.shape[1], len(rows), dtype=dtype, metric=metric, device=0)
    ix.add(rows, ids=ids)
    return ix


def _hold_to_oracle(ix, stored, q, k, metric, want_cfg, ids=None, alive=None, row_filter=None):
    nq = len(q)
    assert ix.scan_plan(nq, k)["cfg_name"] == want_cfg
    oi, od, oc = ko.search(stored, q, k, metric, ids=ids, alive=alive)
    gi, gd, gc, st = ix.search(q, k, mode="fast_only", row_filter=row_filter, return_stats=True)
    assert st["certified"] >= 0.9 * nq, st                 # the MFMA path really ran and certified
    ai, ad, ac = ix.search(q, k, mode="auto", row_filter=row_filter)
    assert np.array_equal(ai, oi), f"ids differ: {np.argwhere(ai != oi)[:5]}"
    assert np.array_equal(ad, od, equal_nan=True) and np.array_equal(ac, oc)
    if st["certified"] == nq:
        assert np.array_equal(gi, oi) and np.array_equal(gd, od, equal_nan=True)
    return oi


CFG_NAME = {"P": "256x256", "Q": "256x128 phased", "R": "256x192 phased"}


@pytest.mark.parametrize("cfg,nq", [("P", 256), ("Q", 128), ("R", 192)])
def test_every_row_position_and_query_column_is_a_top1_once(hip, cfg, nq, scan_cfg):
    """8192 x 128 (two K-tiles: the shortest rows the phased loop takes). Query j's nearest neighbour is a copy of the query at
    tile-row j of tile j mod 32, every other row a random unit vector: each (16-row block, lane >> 4, element) position and each
    (32-query block, 16-query block, lane & 15) column carries a top-1 exactly once."""
    rng = np.random.default_rng(1601)
    n, d = 8192, 128
    rows, q = _unit(rng, n, d), _unit(rng, nq, d)
    planted = (np.arange(nq) % 32) * 256 + np.arange(nq)
    rows[planted] = q
    scan_cfg(cfg)
    ix = _index(rows, "bf16", "cosine")
    oi = _hold_to_oracle(ix, ko.round_through(rows, "bf16"), q, 10, "cosine", CFG_NAME[cfg])
    assert np.array_equal(oi[:, 0], planted)               # the test's own premise
    ix.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("metric", ["l2", "inner_product"])
def test_group_bounds_that_differ_by_row_class(hip, dtype, metric, scan_cfg):
    """Un-normalised rows, those with row bit 2 set four times as long as the others: the two classes of per-block maxima differ,
    and a lane must take the class of ITS rows (lane >> 4 & 1). 200 queries: a padded last group."""
    rng = np.random.default_rng(1602)
    n, d, nq = 12288, 192, 200
    rows = _unit(rng, n, d)
    rows[(np.arange(n) & 4) != 0] *= 4.0
    q = _unit(rng, nq, d)
    scan_cfg("P")
    ix = _index(rows, dtype, metric)
    _hold_to_oracle(ix, ko.round_through(rows, dtype), q, 10, metric, CFG_NAME["P"])
    ix.close()


@pytest.mark.parametrize("k", [10, 33])
def test_tail_tile_row_filter_and_removed_rows(hip, k, scan_cfg):
    """n % 256 != 0 (the rows_left mask on the new row numbers), a 50 % WHERE mask (the non-DMA branch of the per-row terms) on
    top of removed rows; k = 33 runs the k' = 128 plan: slot layout, three-kernel tail."""
    rng = np.random.default_rng(1603)
    n, d, nq = 70001, 192, 70
    rows, q = _unit(rng, n, d), _unit(rng, nq, d)
    ids = rng.permutation(10 * n)[:n].astype(np.int64)
    scan_cfg("P")
    ix = _index(rows, "bf16", "cosine", ids=ids)
    stored = ko.round_through(rows, "bf16")
    kill = ids[rng.permutation(n)[:7000]]
    assert ix.remove(kill) == 7000
    alive = np.isin(ids, kill, invert=True).astype(np.uint8)
    flt = (rng.random(n) < 0.5).astype(np.uint8)
    _hold_to_oracle(ix, stored, q, k, "cosine", CFG_NAME["P"], ids=ids, alive=alive)
    _hold_to_oracle(ix, stored, q, k, "cosine", CFG_NAME["P"], ids=ids, alive=alive & flt, row_filter=flt)
    ix.close()


def test_compaction_on_a_sorted_corpus(hip, scan_cfg):
    """Rows ordered by increasing similarity to query 0: every tile beats its threshold, the append buffer fills and compacts again
    and again -- under this shape's append order (8-row groups, four columns per lane)."""
    rng = np.random.default_rng(1604)
    n, d, nq = 16384, 128, 130
    rows, q = _unit(rng, n, d), _unit(rng, nq, d)
    rows = rows[np.argsort(rows @ q[0])]
    scan_cfg("P")
    ix = _index(rows, "bf16", "cosine")
    _hold_to_oracle(ix, ko.round_through(rows, "bf16"), q, 10, "cosine", CFG_NAME["P"])
    ix.close()


def test_both_mfma_shapes_of_the_dbg_library_match_oracle():
    """libarchi_hip_dbg.so instantiates the phased tiles P, Q, R on both shapes; AK_SCAN_MFMA = 16 / 32 picks one. A child process
    loads that library (one library per process) and holds all six to the oracle on the ragged 70001 x 192 shard."""
    import subprocess, sys
    here = os.path.dirname(os.path.abspath(__file__))
    if not os.path.exists(os.path.join(os.path.dirname(here), "archi_amd", "lib", "libarchi_hip_dbg.so")):
        pytest.skip("libarchi_hip_dbg.so not built (make -C archi_amd/csrc dbg)")
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {os.path.dirname(here)!r})\n"
        "from archi_amd import _lib\n"
        "from archi_amd.index import HipIndex\n"
        "from oracle import knn_oracle as ko\n"
        "assert _lib.is_dbg_library()\n"
        "ix = HipIndex(192, 70001, dtype='bf16', metric='cosine', device=0)\n"
        "ix.generate(seed=1234, n=70001, normalise=True)\n"
        "stored = ko.gen_rows(1234, 0, 0, 70001, 192, True, 'bf16')\n"
        "q = ko.gen_rows(4321, 1, 0, 70, 192, True, 'f32')\n"
        "oi, od, oc = ko.search(stored, q, 10, 'cosine')\n"
        "for shape in ('16', '32'):\n"
        "    _lib.debug_set('AK_SCAN_MFMA', shape)\n"
        "    for cfg in ('P', 'Q', 'R'):\n"
        "        _lib.debug_set('AK_SCAN_CFG', cfg)\n"
        "        gi, gd, gc, st = ix.search(q, 10, mode='fast_only', return_stats=True)\n"
        "        assert st['certified'] == 70, (shape, cfg, st)\n"
        "        assert np.array_equal(gi, oi) and np.array_equal(gd, od), (shape, cfg)\n"
        "print('ok')\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AK_")}
    env["ARCHI_HIP_DBG"] = "1"
    p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and b"ok" in p.stdout, p.stderr.decode("utf-8", "replace")[-3000:]
