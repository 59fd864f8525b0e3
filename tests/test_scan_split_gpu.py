"""The per-tile filter of the phased 16x16x32 tiles (P8, P, Q, R), whichever arrangement a tile ships on (ScanCfg::FILT). In the
whole-tile arrangement the thresholds and per-row terms a lane needs are read once per tile, the exact maxima of all its filter
groups are computed branch-free, and one branch skips the groups without a hit; site by site, every group computes its bound and
branches. What a tile appends must be the same under both, so the bar is the suite's: ids and
float8 distance bits equal to the oracle's through the search API, with the tile forced (AK_SCAN_CFG, AK_SCAN_I8 = 2 for the
int8 tile). The shapes are those at which tile state can go wrong: two and three K-steps per tile, one / two / several tiles
per workgroup (asserted from the plan the library reports), tail tiles with planted neighbours either side of a tile boundary,
row filters and removed rows, compactions in consecutive tiles, 300 queries and one. The last test holds both arrangements of
libarchi_hip_dbg.so (AK_SCAN_FILTER) to the oracle and to each other."""
import os

import numpy as np
import pytest

from oracle import knn_oracle as ko

pytestmark = pytest.mark.gpu

CFG_NAME = {"P8": "256x256", "P": "256x256", "Q": "256x128 phased", "R": "256x192 phased"}
QTILE = {"P8": 256, "P": 256, "Q": 128, "R": 192}
SWITCHES = ("AK_SCAN_CFG", "AK_SCAN_I8", "AK_SEED_RATIO", "AK_SEED_DIV", "AK_SCAN_BLOCKS")


def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture
def force():
    """force(tile, **switches): tile P8 is tile P with the int8 plan wherever the shape allows, the others run on 16 bits."""
    from archi_amd import _lib

    def go(tile, **kw):
        _lib.debug_set("AK_SCAN_CFG", "P" if tile == "P8" else tile)
        _lib.debug_set("AK_SCAN_I8", "2" if tile == "P8" else "0")
        for name, value in kw.items():
            _lib.debug_set(name, str(value))
    yield go
    for name in SWITCHES:
        _lib.debug_set(name, None)


def _index(rows, dtype, metric, ids=None):
    from archi_amd.index import HipIndex
    ix = HipIndex(rows.shape[1], len(rows), dtype=dtype, metric=metric, device=0)
    ix.add(rows, ids=ids)
    return ix


def _tiles_per_workgroup(plan, n):
    """(seeding pass, main pass): tiles of every slice, by the kernel's own split (tile t0 = tb + nt * slice / nslices)."""
    def split(nt, ns):
        return [nt * (s + 1) // ns - nt * s // ns for s in range(ns)]
    tb = plan["seed_rows"] // 256
    seed = split(tb, plan["ns_seed"]) if plan["ns_seed"] else []
    return seed, split((n + 255) // 256 - tb, plan["nslices"])


def _hold_to_oracle(ix, tile, stored, q, k, metric, ids=None, alive=None, row_filter=None, min_certified=0.9):
    nq = len(q)
    plan = ix.scan_plan(nq, k)
    assert plan["cfg_name"] == CFG_NAME[tile] and plan["kprime"] == (512 if tile == "P8" else 64), plan
    oi, od, oc = ko.search(stored, q, k, metric, ids=ids, alive=alive)
    before = ix.i8_info()["searches"]
    gi, gd, gc, st = ix.search(q, k, mode="fast_only", row_filter=row_filter, return_stats=True)
    assert ix.i8_info()["searches"] == before + (tile == "P8")          # the element type the case names is the one that ran
    assert st["certified"] >= min_certified * nq, st                     # ... and certified by itself
    ai, ad, ac = ix.search(q, k, mode="auto", row_filter=row_filter)
    assert np.array_equal(ai, oi), f"ids differ: {np.argwhere(ai != oi)[:5]}"
    assert np.array_equal(ad, od, equal_nan=True) and np.array_equal(ac, oc)
    if st["certified"] == nq:
        assert np.array_equal(gi, oi) and np.array_equal(gd, od, equal_nan=True)
    return oi


def _plant(rows, q, n):
    """Nearest neighbours at the places where a filter that works on the wrong tile's row base, row mask or term parity loses
    them: the last row, the first row of the last (partial) tile, the first rows of the tiles behind the first two tile
    boundaries, and a row inside the partial tile."""
    last_tile = (n - 1) // 256 * 256
    at = np.array([n - 1, last_tile, 256, 512, min(n - 1, last_tile + 40)])
    at = at[: len(q)]
    rows[at] = q[: len(at)]
    return at


# (tile, D): two and three K-steps per tile -- 128 int8 elements or 64 16-bit elements of a row per K-step
KS_CASES = [("P8", 256), ("P8", 384), ("P", 128), ("P", 192), ("Q", 128), ("Q", 192), ("R", 128), ("R", 192)]


@pytest.mark.parametrize("tile,d", KS_CASES)
@pytest.mark.parametrize("n,blocks,want", [(4096, 0, (2, 2)), (4173, 0, (2, 3)), (8269, 8, (4, 5))])
def test_two_three_and_more_tiles_per_workgroup_with_neighbours_at_the_tile_boundaries(hip, force, tile, d, n, blocks, want):
    """4096 rows: two tiles per workgroup; 4173: 17 tiles, the last one of 77 rows, two or three per workgroup; 8269 rows on eight
    workgroups per query group: four or five. 70 queries of which five have their nearest neighbour planted at a tile boundary."""
    rng = np.random.default_rng(2101)
    nq = 70
    rows, q = _unit(rng, n, d), _unit(rng, nq, d)
    planted = _plant(rows, q, n)
    force(tile, **({"AK_SCAN_BLOCKS": blocks} if blocks else {}))
    ix = _index(rows, "bf16", "cosine")
    seed, main = _tiles_per_workgroup(ix.scan_plan(nq, 10), n)
    assert not seed and (min(main), max(main)) == want, (seed, main)
    oi = _hold_to_oracle(ix, tile, ko.round_through(rows, "bf16"), q, 10, "cosine")
    assert np.array_equal(oi[: len(planted), 0], planted)               # the test's own premise
    ix.close()


@pytest.mark.parametrize("tile,d,nq", [("P8", 256, 256), ("Q", 128, 128)])
def test_one_tile_per_workgroup_in_the_seeding_pass(hip, force, tile, d, nq):
    """65 613 rows (257 tiles, the last of 77 rows) with the seeding pass switched on at 1/32 of the tiles: eight seeding
    workgroups per query group of ONE tile each, one or two tiles per workgroup in the main pass."""
    rng = np.random.default_rng(2102)
    n = 65613
    rows, q = _unit(rng, n, d), _unit(rng, nq, d)
    planted = _plant(rows, q, n)
    rows[100] = q[5]                                                     # ... and one inside the seeding pass's rows
    force(tile, AK_SEED_RATIO=1, AK_SEED_DIV=32)
    ix = _index(rows, "bf16", "cosine")
    seed, main = _tiles_per_workgroup(ix.scan_plan(nq, 10), n)
    assert seed == [1] * 8 and (min(main), max(main)) == (1, 2), (seed, main)
    oi = _hold_to_oracle(ix, tile, ko.round_through(rows, "bf16"), q, 10, "cosine")
    assert np.array_equal(oi[:6, 0], np.append(planted, 100))
    ix.close()


@pytest.mark.parametrize("tile,d", [("P8", 256), ("P", 128), ("R", 192)])
def test_row_filter_and_removed_rows_over_several_tiles_with_300_queries(hip, force, tile, d):
    """70 001 rows, 300 queries (a padded last query group), 7000 removed rows and a 50 % WHERE mask on top of them -- the branch
    of the per-tile terms that is written with plain stores -- on 32 workgroups per query group: eight or nine tiles each."""
    rng = np.random.default_rng(2103)
    n, nq = 70001, 300
    rows, q = _unit(rng, n, d), _unit(rng, nq, d)
    ids = rng.permutation(10 * n)[:n].astype(np.int64)
    nqg = -(-nq // QTILE[tile])
    force(tile, AK_SCAN_BLOCKS=32 * nqg)
    ix = _index(rows, "bf16", "cosine", ids=ids)
    seed, main = _tiles_per_workgroup(ix.scan_plan(nq, 10), n)
    assert not seed and min(main) >= 3, (seed, main)
    stored = ko.round_through(rows, "bf16")
    kill = ids[rng.permutation(n)[:7000]]
    assert ix.remove(kill) == 7000
    alive = np.isin(ids, kill, invert=True).astype(np.uint8)
    flt = (rng.random(n) < 0.5).astype(np.uint8)
    _hold_to_oracle(ix, tile, stored, q, 10, "cosine", ids=ids, alive=alive)
    _hold_to_oracle(ix, tile, stored, q, 10, "cosine", ids=ids, alive=alive & flt, row_filter=flt)
    ix.close()


def _sorted_corpus(seed, n, d, nq):
    rng = np.random.default_rng(seed)
    rows, q = _unit(rng, n, d), _unit(rng, nq, d)
    return rows[np.argsort(rows @ q[0])], q


@pytest.mark.parametrize("tile,d", [("P8", 256), ("P", 128), ("Q", 128), ("R", 128)])
def test_compactions_in_consecutive_tiles_at_two_k_steps(hip, force, tile, d):
    """Rows ordered by increasing similarity to query 0, eight workgroups per query group of eight consecutive tiles each: every
    row of every tile beats query 0's threshold, 256 appends per tile against a buffer that asks for a compaction from 64
    entries on, so requests are raised tile after tile, at the shortest K-loop between two of them."""
    n, nq = 16384, 130
    rows, q = _sorted_corpus(2104, n, d, nq)
    force(tile, AK_SCAN_BLOCKS=8 * -(-nq // QTILE[tile]))
    ix = _index(rows, "bf16", "cosine")
    seed, main = _tiles_per_workgroup(ix.scan_plan(nq, 10), n)
    assert not seed and main == [8] * 8, (seed, main)
    _hold_to_oracle(ix, tile, ko.round_through(rows, "bf16"), q, 10, "cosine")
    ix.close()


@pytest.mark.parametrize("tile,d", [("P8", 384), ("Q", 192)])
def test_a_single_query(hip, force, tile, d):
    """One query on a forced wide tile: 255 (127) padded columns whose threshold is +inf beside one that appends."""
    rng = np.random.default_rng(2105)
    n = 4173
    rows, q = _unit(rng, n, d), _unit(rng, 1, d)
    planted = _plant(rows, q, n)
    force(tile)
    ix = _index(rows, "bf16", "cosine")
    oi = _hold_to_oracle(ix, tile, ko.round_through(rows, "bf16"), q, 10, "cosine", min_certified=1.0)
    assert oi[0, 0] == planted[0]
    ix.close()


def test_both_filter_arrangements_of_the_dbg_library_match_oracle_and_each_other():
    """libarchi_hip_dbg.so instantiates P8, P, Q and R with both arrangements of the filter; AK_SCAN_FILTER = 1 (site by site) /
    2 (whole tile) picks one. A child process (one library per process) runs P8 and Q under both on the sorted corpus of the
    compaction test: each equals the oracle, the two equal each other, and the instrumented kernels' counters show that slow-path
    entries and compactions did occur under both."""
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
        "n, nq = 16384, 130\n"
        "for tile, d in (('P8', 256), ('Q', 128)):\n"
        "    rng = np.random.default_rng(2104)\n"
        "    rows = rng.standard_normal((n, d)).astype(np.float32); rows /= np.linalg.norm(rows, axis=1, keepdims=True)\n"
        "    q = rng.standard_normal((nq, d)).astype(np.float32); q /= np.linalg.norm(q, axis=1, keepdims=True)\n"
        "    rows = rows[np.argsort(rows @ q[0])]\n"
        "    ix = HipIndex(d, n, dtype='bf16', metric='cosine', device=0)\n"
        "    ix.add(rows)\n"
        "    oi, od, oc = ko.search(ko.round_through(rows, 'bf16'), q, 10, 'cosine')\n"
        "    _lib.debug_set('AK_SCAN_CFG', tile[0])\n"
        "    _lib.debug_set('AK_SCAN_I8', '2' if tile == 'P8' else '0')\n"
        "    _lib.debug_set('AK_SCAN_BLOCKS', str(8 * (2 if tile == 'Q' else 1)))\n"
        "    got = {}\n"
        "    for filt in ('1', '2'):\n"
        "        _lib.debug_set('AK_SCAN_FILTER', filt)\n"
        "        for dbg in (None, '1'):\n"
        "            _lib.debug_set('AK_SCAN_DBG', dbg)\n"
        "            gi, gd, gc, st = ix.search(q, 10, mode='fast_only', return_stats=True)\n"
        "            assert st['certified'] >= 0.9 * nq, (tile, filt, dbg, st)\n"
        "            ai, ad, ac = ix.search(q, 10, mode='auto')\n"
        "            assert np.array_equal(ai, oi) and np.array_equal(ad, od), (tile, filt, dbg)\n"
        "            got[(filt, dbg)] = (gi, gd, gc)\n"
        "        main = ix.debug_read()[1]\n"
        "        main = main[main[:, 7] > 0]\n"
        "        assert len(main) and (main[:, 7] == 8).all(), (tile, filt, main[:, 7])\n"
        "        assert main[:, 5].sum() > 0 and main[:, 6].sum() > 0, (tile, filt, main[:, 5].sum(), main[:, 6].sum())\n"
        "        print(tile, filt, 'slow-path entries', int(main[:, 5].sum()), 'compactions', int(main[:, 6].sum()))\n"
        "    first = got[('1', None)]\n"
        "    for key, val in got.items():\n"
        "        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first, val)), (tile, key)\n"
        "    assert _lib.load().ak_debug_set(b'AK_SCAN_FILTER', b'3') != 0\n"
        "    _lib.debug_set('AK_SCAN_FILTER', None)\n"
        "    ix.close()\n"
        "print('ok')\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AK_")}
    env["ARCHI_HIP_DBG"] = "1"
    p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    print(p.stdout.decode("utf-8", "replace"))
    assert p.returncode == 0 and b"ok" in p.stdout, p.stderr.decode("utf-8", "replace")[-3000:]
