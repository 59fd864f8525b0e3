"""The queued arrangement of the int8 tile's filter (ScanCfg::FILT = 2, tile_epilogue): a lane's sixteen bounds first, the lane-sites
that pass gathered into the wave's LDS queue behind a ballot per site, and the queue scored and appended once per tile, one lane per
entry -- or more often where a site's entries would not fit. It must append the keys the whole-tile arrangement appends, so the bar is
the suite's: ids and float8 distance bits equal to the oracle's through the search API with the int8 plan forced on tile P
(AK_SCAN_CFG = P, AK_SCAN_I8 = 2), on the library as it ships; and in a child process on libarchi_hip_dbg.so, `fast_only` ids,
distances and certificate flags equal under the whole-tile arrangement and the queue on both passes (AK_SCAN_HITQ = 4 / 3).

Shapes (tests/scan_hitq_cases.py): 4173 rows at two and three K-steps with a last tile of 77 rows and neighbours planted either side
of tile boundaries (term parity and the tail mask in the drain); a seeding pass of one tile per workgroup; 300 queries with removed
rows and a row filter; one query beside 255 padded columns; and a corpus sorted by similarity to 130 nearly equal queries, where a
wave queues far more than 64 entries per tile -- the drains before a site -- and compactions are raised tile after tile. The
instrumented kernels' counters show that the overflow case drained more often than once per tile and the sparse one did not."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import knn_oracle as ko
from tests import scan_hitq_cases as hc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def switches():
    from archi_amd import _lib

    def go(values):
        for name in hc.ALL_SWITCHES:
            _lib.debug_set(name, values.get(name))
    yield go
    for name in hc.ALL_SWITCHES:
        _lib.debug_set(name, None)


@pytest.fixture(scope="module")
def dbg_results():
    """{case: the worker's result}: one child process on the dbg library for all cases."""
    if not os.path.exists(os.path.join(ROOT, "archi_amd", "lib", "libarchi_hip_dbg.so")):
        pytest.fail("libarchi_hip_dbg.so not built (make -C archi_amd/csrc dbg)")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AK_")}
    env["ARCHI_HIP_DBG"] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scan_hitq_worker.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    out = p.stdout.decode("utf-8", "replace")
    assert p.returncode == 0 and out.rstrip().endswith("ok"), (out[-2000:], p.stderr.decode("utf-8", "replace")[-3000:])
    res = [json.loads(line[len("RESULT "):]) for line in out.splitlines() if line.startswith("RESULT ")]
    return {r["case"]: r for r in res}


def test_the_overflow_premise_holds_on_the_cpu():
    """No GPU in this one, but it is the GPU case's premise: at least 256 lane-sites per wave and tile MUST be queued -- four
    times the queue -- in every tile behind a workgroup's first."""
    c = hc.build("overflow")
    assert hc.overflow_premise(ko.round_through(c["rows"], "bf16"), c["q"]) >= 256


@pytest.mark.parametrize("name", hc.CASES)
def test_the_library_as_it_ships_equals_the_oracle(hip, switches, name):
    from archi_amd.index import HipIndex
    c = hc.build(name)
    switches(c["switches"])
    rows, q = c["rows"], c["q"]
    nq = len(q)
    ix = HipIndex(rows.shape[1], len(rows), dtype="bf16", metric="cosine", device=0)
    ix.add(rows, ids=c["ids"])
    plan = ix.scan_plan(nq, hc.K)
    assert plan["cfg_name"] == "256x256" and plan["kprime"] == 512, plan
    if name == "seed-one-tile":
        assert plan["ns_seed"] == 8 and plan["seed_rows"] == 8 * 256, plan
    if name == "overflow":
        assert plan["nslices"] == 8 and plan["ns_seed"] == 0, plan
    stored = ko.round_through(rows, "bf16")
    alive = None
    if c["kill"] is not None:
        assert ix.remove(c["kill"]) == len(c["kill"])
        alive = np.isin(c["ids"], c["kill"], invert=True).astype(np.uint8)
    if c["row_filter"] is not None:
        alive = alive & c["row_filter"]
    oi, od, oc = ko.search(stored, q, hc.K, "cosine", ids=c["ids"], alive=alive)
    before = ix.i8_info()["searches"]
    gi, gd, gc, st = ix.search(q, hc.K, mode="fast_only", row_filter=c["row_filter"], return_stats=True)
    assert ix.i8_info()["searches"] == before + 1                        # the int8 plan ran
    assert st["certified"] >= 0.9 * nq, st
    ai, ad, ac = ix.search(q, hc.K, mode="auto", row_filter=c["row_filter"])
    assert np.array_equal(ai, oi), f"ids differ: {np.argwhere(ai != oi)[:5]}"
    assert np.array_equal(ad, od, equal_nan=True) and np.array_equal(ac, oc)
    if st["certified"] == nq:
        assert np.array_equal(gi, oi) and np.array_equal(gd, od, equal_nan=True)
    if c["planted"] is not None:
        assert np.array_equal(oi[: len(c["planted"]), 0], c["planted"])   # the case's own premise
    ix.close()


@pytest.mark.parametrize("name", hc.CASES)
def test_queued_and_whole_tile_arrangements_agree_in_the_dbg_library(dbg_results, name):
    r = dbg_results[name]
    assert r["fast_only_equal"] == [True, True, True], r["fast_only_equal"]          # ids, distances, certificate flags
    assert r["instrumented_equal"] == [True, True, True]
    assert r["certified"][0] == r["certified"][1] >= 0.9 * len(hc.build(name)["q"]), r["certified"]
    assert r["auto_equals_oracle"]


def test_drains_per_tile_in_the_overflow_and_the_sparse_case(dbg_results):
    """Overflow: the workgroup's waves of wave columns 0 and 1 hold 64 real queries each, and by the premise every tile behind the
    first queues at least 256 of their lane-sites and the first all 1024 -- more drains than tiles. Sparse: one query is one column
    of one wave column, sixteen lane-sites per wave and tile at the most; the queue never fills, so a tile drains at most once."""
    m = dbg_results["overflow"]["counters"]["main"]
    tiles, drains, queued = np.array(m["tiles"]), np.array(m["drains"]), np.array(m["queued"])
    assert m["waves"] == 64 and (tiles == 8).all(), (m["waves"], tiles)
    real = np.isin(np.arange(64) % 4, (0, 1))                             # wave = wave row * 4 + wave column
    print("overflow: drains per wave", sorted(set(drains.tolist())), "queued per wave", sorted(set(queued.tolist())), "compactions", m["compactions"])
    assert (queued[real] >= 1024 + 7 * 256).all() and (drains[real] >= 16 + 7 * 4).all() and (drains[real] > tiles[real]).all()
    assert (drains[~real] <= tiles[~real]).all()                          # two real queries, or none
    assert m["compactions"] >= 8 * 130                                    # at least: every query's 256 appends of a first tile
    s = dbg_results["one-query"]["counters"]["main"]
    tiles, drains, queued = np.array(s["tiles"]), np.array(s["drains"]), np.array(s["queued"])
    print("sparse: tiles", int(tiles.sum()), "drains", int(drains.sum()), "queued", int(queued.sum()))
    assert queued.sum() > 0 and (queued <= 16 * tiles).all() and (drains <= tiles).all()
