"""The int8 scan plan (AK_SCAN_I8): the phased 256 x 256 tile on v_mfma_i32_16x16x64_i8 over an int8 shadow of a 16-bit corpus,
an exact seed threshold, and a dense k' = 512 tail. The candidates come from integer dot products with one scale per row and
per query; ids and distances come from the exact re-rank, so the bar is the suite's: ids and float8 distance bits equal to the
oracle's. Every case forces tile P and AK_SCAN_I8 = 2 (the plan wherever the shape allows) and asserts from the library's own
counters that the int8 path ran; on benign data it must also certify by itself (fast_only), not through the fallback."""
import os

import numpy as np
import pytest

from oracle import knn_oracle as ko

pytestmark = pytest.mark.gpu


def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture
def i8_on_p():
    from archi_amd import _lib
    _lib.debug_set("AK_SCAN_CFG", "P")
    _lib.debug_set("AK_SCAN_I8", "2")
    yield _lib.debug_set
    for name in ("AK_SCAN_CFG", "AK_SCAN_I8", "AK_SEED_RATIO"):
        _lib.debug_set(name, None)


def _index(rows, dtype, metric, ids=None, capacity=None):
    from archi_amd.index import HipIndex
    ix = HipIndex(rows.shape[1], capacity or len(rows), dtype=dtype, metric=metric, device=0)
    ix.add(rows, ids=ids)
    return ix


def _hold_to_oracle(ix, stored, q, k, metric, ids=None, alive=None, row_filter=None, min_certified=0.9):
    nq = len(q)
    plan = ix.scan_plan(nq, k)
    assert plan["cfg_name"] == "256x256" and plan["kprime"] == 512, plan        # the int8 plan's tile and candidate count
    oi, od, oc = ko.search(stored, q, k, metric, ids=ids, alive=alive)
    before = ix.i8_info()["searches"]
    gi, gd, gc, st = ix.search(q, k, mode="fast_only", row_filter=row_filter, return_stats=True)
    info = ix.i8_info()
    assert info["searches"] == before + 1 and info["rows"] == ix.slots, info     # the int8 kernels ran, over a complete shadow
    print(f"certified {st['certified']} / {nq}, reranked {st['reranked']}, max rho8 {info['max_rho']:.5f}")
    assert st["certified"] >= min_certified * nq, st             # ... and certified by themselves
    ai, ad, ac = ix.search(q, k, mode="auto", row_filter=row_filter)
    assert np.array_equal(ai, oi), f"ids differ: {np.argwhere(ai != oi)[:5]}"
    assert np.array_equal(ad, od, equal_nan=True) and np.array_equal(ac, oc)
    if st["certified"] == nq:
        assert np.array_equal(gi, oi) and np.array_equal(gd, od, equal_nan=True)
    return oi, st


def test_every_row_position_and_query_column_is_a_top1_once(hip, i8_on_p):
    """8192 x 256 bf16 (two int8 K-steps: the shortest rows the plan takes), 256 queries. Query j's nearest neighbour is a copy of
    the query at tile-row j of tile j mod 32: each (row block, lane group, element) position and each query column carries a
    top-1 exactly once."""
    rng = np.random.default_rng(1801)
    n, d, nq = 8192, 256, 256
    rows, q = _unit(rng, n, d), _unit(rng, nq, d)
    planted = (np.arange(nq) % 32) * 256 + np.arange(nq)
    rows[planted] = q
    ix = _index(rows, "bf16", "cosine")
    oi, _ = _hold_to_oracle(ix, ko.round_through(rows, "bf16"), q, 10, "cosine")
    assert np.array_equal(oi[:, 0], planted)               # the test's own premise
    ix.close()


def test_every_position_f16_inner_product_three_k_steps(hip, i8_on_p):
    """The same planting at D = 384 (three K-steps) on f16 with the inner product and un-normalised rows: rows with row bit 2 set
    are four times as long as the others, so the two row classes of a block carry different scale-folded bounds. The planted
    row is the query scaled to the long class's length, the largest inner product a row of that length can have."""
    rng = np.random.default_rng(1802)
    n, d, nq = 8192, 384, 256
    rows, q = _unit(rng, n, d), _unit(rng, nq, d)
    rows[(np.arange(n) & 4) != 0] *= 4.0
    planted = (np.arange(nq) % 32) * 256 + np.arange(nq)
    rows[planted] = 4.0 * q
    ix = _index(rows, "f16", "inner_product")
    oi, _ = _hold_to_oracle(ix, ko.round_through(rows, "f16"), q, 10, "inner_product")
    assert np.array_equal(oi[:, 0], planted)
    ix.close()


@pytest.mark.parametrize("seeded", [False, True])
def test_tail_tile_row_filter_and_removed_rows(hip, i8_on_p, seeded):
    """n % 256 != 0, 300 queries (a padded second group), 7000 removed rows and a 50 % WHERE mask on top of them. seeded: the
    seeding pass and the exact seed threshold are switched on for this small shard (AK_SEED_RATIO = 1); otherwise the main
    pass starts from the 16-bit pre-seeding threshold converted to the int8 units."""
    rng = np.random.default_rng(1803)
    n, d, nq = 70001, 256, 300
    rows, q = _unit(rng, n, d), _unit(rng, nq, d)
    ids = rng.permutation(10 * n)[:n].astype(np.int64)
    if seeded:
        i8_on_p("AK_SEED_RATIO", "1")
    ix = _index(rows, "bf16", "cosine", ids=ids)
    assert (ix.scan_plan(nq, 10)["ns_seed"] > 0) == seeded
    stored = ko.round_through(rows, "bf16")
    kill = ids[rng.permutation(n)[:7000]]
    assert ix.remove(kill) == 7000
    alive = np.isin(ids, kill, invert=True).astype(np.uint8)
    flt = (rng.random(n) < 0.5).astype(np.uint8)
    _hold_to_oracle(ix, stored, q, 10, "cosine", ids=ids, alive=alive)
    _hold_to_oracle(ix, stored, q, 10, "cosine", ids=ids, alive=alive & flt, row_filter=flt)
    ix.close()


def test_shadow_follows_added_rows_and_is_rebuilt_when_rows_move(hip, i8_on_p):
    """Search (the shadow is built), add 5000 rows, search: the shadow is extended, the new rows are found. Remove rows and
    reclaim them so that every later row moves: the shadow is built anew for the new layout, and no answer comes from what the
    old shadow held at a slot."""
    rng = np.random.default_rng(1804)
    n, d, nq, extra = 20000, 256, 64, 5000
    rows, q = _unit(rng, n + extra, d), _unit(rng, nq, d)
    rows[n + np.arange(nq) * 70] = q                       # every query's nearest neighbour arrives with the second batch
    ids = np.arange(1, n + extra + 1, dtype=np.int64)
    ix = _index(rows[:n], "bf16", "cosine", ids=ids[:n], capacity=n + extra)
    stored = ko.round_through(rows, "bf16")
    _hold_to_oracle(ix, stored[:n], q, 10, "cosine", ids=ids[:n])
    assert ix.i8_info()["builds"] == 1 and ix.i8_info()["rows"] == n
    ix.add(rows[n:], ids=ids[n:])
    oi, _ = _hold_to_oracle(ix, stored, q, 10, "cosine", ids=ids)
    assert np.array_equal(oi[:, 0], ids[n + np.arange(nq) * 70])
    assert ix.i8_info()["builds"] == 1                     # extended, not rebuilt
    # rows move: the first 3000 leave and are reclaimed, every survivor gets a slot 3000 lower
    assert ix.remove(ids[:3000]) == 3000
    assert ix.compact() == 3000
    oi, _ = _hold_to_oracle(ix, stored[3000:], q, 10, "cosine", ids=ids[3000:])
    info = ix.i8_info()
    assert info["builds"] == 2 and info["rows"] == n + extra - 3000, info
    assert not np.isin(oi, ids[:3000]).any()
    ix.close()


def test_compaction_on_a_sorted_corpus(hip, i8_on_p):
    """Rows ordered by increasing similarity to query 0: every tile beats its threshold, the append buffer fills and compacts
    again and again."""
    rng = np.random.default_rng(1805)
    n, d, nq = 16384, 256, 130
    rows, q = _unit(rng, n, d), _unit(rng, nq, d)
    rows = rows[np.argsort(rows @ q[0])]
    ix = _index(rows, "bf16", "cosine")
    _hold_to_oracle(ix, ko.round_through(rows, "bf16"), q, 10, "cosine")
    ix.close()


def test_neighbours_closer_than_the_int8_resolution(hip, i8_on_p):
    """Query 0: 300 rows within one int8 step of each other around its nearest neighbour; query 1: a pile of 600 equal rows --
    more equal scores than k' holds. Such queries may lose the int8 certificate; in auto mode the answers stay the oracle's."""
    rng = np.random.default_rng(1806)
    n, d, nq = 16384, 256, 40
    rows, q = _unit(rng, n, d), _unit(rng, nq, d)
    step = np.abs(q[0]).max() / 127.0
    near = rng.permutation(n)[:900]
    rows[near[:300]] = q[0] + rng.uniform(-0.5, 0.5, size=(300, d)).astype(np.float32) * step
    rows[near[300:]] = q[1]
    ix = _index(rows, "bf16", "cosine")
    _hold_to_oracle(ix, ko.round_through(rows, "bf16"), q, 10, "cosine", min_certified=0.0)
    ix.close()


def test_int8_and_bf16_tile_p_of_the_dbg_library_match_oracle():
    """libarchi_hip_dbg.so carries the instrumented int8 instantiation beside the 16-bit ones: a child process (one library per
    process) holds tile P on both element types to the oracle on the ragged 70001-row shard."""
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
        "ix = HipIndex(256, 70001, dtype='bf16', metric='cosine', device=0)\n"
        "ix.generate(seed=1234, n=70001, normalise=True)\n"
        "stored = ko.gen_rows(1234, 0, 0, 70001, 256, True, 'bf16')\n"
        "q = ko.gen_rows(4321, 1, 0, 70, 256, True, 'f32')\n"
        "oi, od, oc = ko.search(stored, q, 10, 'cosine')\n"
        "_lib.debug_set('AK_SCAN_CFG', 'P')\n"
        "for i8, dbg in (('0', '0'), ('2', '0'), ('2', '1')):\n"
        "    _lib.debug_set('AK_SCAN_I8', i8)\n"
        "    _lib.debug_set('AK_SCAN_DBG', dbg if dbg == '1' else None)\n"
        "    gi, gd, gc, st = ix.search(q, 10, mode='fast_only', return_stats=True)\n"
        "    assert ix.i8_info()['searches'] == (0 if i8 == '0' else 1 + int(dbg)), (i8, dbg, ix.i8_info())\n"
        "    assert st['certified'] == 70, (i8, dbg, st)\n"
        "    assert np.array_equal(gi, oi) and np.array_equal(gd, od), (i8, dbg)\n"
        "print('ok')\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AK_")}
    env["ARCHI_HIP_DBG"] = "1"
    p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and b"ok" in p.stdout, p.stderr.decode("utf-8", "replace")[-3000:]


def test_the_plan_takes_int8_only_where_it_is_eligible(hip):
    """Library defaults (AK_SCAN_I8 = 1, no forced tile) on a big shard -- 1.1M x 768 bf16, 4297 tiles: batches of at least two
    256-query groups on cosine take the int8 plan; Q <= 256, l2, f32 corpora and small shards keep the plans they had."""
    from archi_amd.index import HipIndex
    n, d = 1_100_000, 768
    ix = HipIndex(d, n, dtype="bf16", metric="cosine", device=0)
    ix.generate(seed=7, n=n, normalise=True)
    for nq, kprime, tile in ((1024, 512, "256x256"), (512, 512, "256x256"), (256, 64, "256x256"), (128, 64, "256x128"), (32, 64, "256x32")):
        plan = ix.scan_plan(nq, 10)
        assert (plan["kprime"], plan["cfg_name"]) == (kprime, tile), (nq, plan)
    assert ix.scan_plan(1024, 33)["kprime"] == 128          # larger k: the slot-layout plans, untouched
    ix.close()
    for dtype, metric, rows, dim in (("bf16", "l2", n, d), ("f32", "cosine", n // 2, d), ("bf16", "cosine", 500_000, d),
                                     ("f16", "cosine", n, 384)):
        ix = HipIndex(dim, rows, dtype=dtype, metric=metric, device=0)
        ix.generate(seed=7, n=rows, normalise=True)
        assert ix.scan_plan(1024, 10)["kprime"] == 64, (dtype, metric, rows, dim)
        assert ix.i8_info() == {"rows": 0, "builds": 0, "searches": 0, "max_rho": 0.0}
        ix.close()
