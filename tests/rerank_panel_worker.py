"""Child of tests/test_rerank_panel_gpu.py: every launch-level case through ak_kts_rr_rerank (libarchi_hip_dbg.so; the parent sets
ARCHI_HIP_DBG=1), the thread-per-candidate kernel (which = 0) and the panel kernel (which = 1) on the same index and the same
candidate array. Writes keys and ids of both to an .npz; judges nothing but the return codes. Each launch runs once.

usage: rerank_panel_worker.py OUT.npz"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from archi_amd import _lib  # noqa: E402
from archi_amd.index import HipIndex  # noqa: E402
from oracle import knn_oracle as ko  # noqa: E402
from tests import rerank_panel_cases as rc  # noqa: E402


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _launch(lib, ix, q, cand, which):
    """(rc, keys, ids); the outputs are filled with a sentinel first, so an entry the kernel did not write shows."""
    dev = torch.device("cuda", 0)
    nq, kp = cand.shape
    qd = torch.from_numpy(q).to(dev)
    cd = torch.from_numpy(cand.view(np.int64)).to(dev)
    keys = torch.full((nq, kp), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    ids = torch.full((nq, kp), -777, dtype=torch.int64, device=dev)
    nb = torch.zeros(nq, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    r = lib.ak_kts_rr_rerank(ix._h, _ptr(qd), nq, kp, _ptr(cd), _ptr(keys), _ptr(ids), _ptr(nb), which, None)
    torch.cuda.synchronize()
    return r, keys.cpu().numpy().view(np.uint64), ids.cpu().numpy()


def main(out):
    lib = _lib.init(0)
    assert _lib.is_dbg_library()
    res = {}
    built = {}
    for c in rc.CASES:
        key = (c["dtype"], c["metric"], c["dim"])
        if key not in built:                                 # 19 small indexes, all kept to the end
            rows, _ = rc.rows_and_queries(c)
            ix = HipIndex(c["dim"], rc.N_ROWS, dtype=c["dtype"], metric=c["metric"], device=0)
            ix.add(rows, ids=np.arange(rc.N_ROWS, dtype=np.int64) * 3 + 11)
            built[key] = ix
        ix = built[key]
        _, q = rc.rows_and_queries(c)
        cand = rc.candidates(c)
        for which, tag in ((0, "old"), (1, "new")):
            r, keys, ids = _launch(lib, ix, q, cand, which)
            assert r == 0, (c["name"], tag, r, _lib.last_error())
            res[f"{c['name']}:{tag}:keys"] = keys
            res[f"{c['name']}:{tag}:ids"] = ids
    # the switch: what rerank() launches, and a search that goes through it (the int8 plan's tail) held to the oracle
    c = rc.CASES[0]
    ix = built[(c["dtype"], c["metric"], c["dim"])]
    res["choice:default"] = np.int64(lib.ak_kts_rr_choice(ix._h))
    _lib.debug_set("AK_RERANK_OLD", "1")
    res["choice:old"] = np.int64(lib.ak_kts_rr_choice(ix._h))
    _lib.debug_set("AK_SCAN_CFG", "P")
    _lib.debug_set("AK_SCAN_I8", "2")
    rows, _ = rc.rows_and_queries(c)
    q = ko.gen_rows(99, 1, 0, 130, c["dim"], True, "f32")
    gi, gd, gc, st = ix.search(q, 10, mode="auto", return_stats=True)
    oi, od, oc = ko.search(ko.round_through(rows, c["dtype"]), q, 10, c["metric"], ids=np.arange(rc.N_ROWS, dtype=np.int64) * 3 + 11)
    res["old_search:equal"] = np.int64(np.array_equal(gi, oi) and np.array_equal(gd, od) and np.array_equal(gc, oc))
    res["old_search:reranked"] = np.int64(st["reranked"])
    res["old_search:kprime"] = np.int64(ix.scan_plan(130, 10)["kprime"])
    for name in ("AK_RERANK_OLD", "AK_SCAN_CFG", "AK_SCAN_I8"):
        _lib.debug_set(name, None)
    res["choice:reset"] = np.int64(lib.ak_kts_rr_choice(ix._h))
    for ix in built.values():
        ix.close()
    # shapes the panel kernel does not take: which = 1 is an error, which = 0 runs
    for i, (dtype, metric, dim) in enumerate(rc.REFUSED):
        ix = HipIndex(dim, 256, dtype=dtype, metric=metric, device=0)
        ix.add(np.random.default_rng(5).standard_normal((256, dim), dtype=np.float32))
        q = np.random.default_rng(6).standard_normal((2, dim), dtype=np.float32)
        cand = np.arange(2 * 64, dtype=np.uint64).reshape(2, 64) % np.uint64(256)
        r1, keys, ids = _launch(lib, ix, q, cand, 1)
        res[f"refused{i}:rc"] = np.int64(r1)
        res[f"refused{i}:error"] = np.array(_lib.last_error())
        res[f"refused{i}:untouched"] = np.int64((ids == -777).all())
        res[f"refused{i}:choice"] = np.int64(lib.ak_kts_rr_choice(ix._h))
        r0, keys, ids = _launch(lib, ix, q, cand, 0)
        res[f"refused{i}:rc_old"] = np.int64(r0)
        res[f"refused{i}:old_wrote"] = np.int64((ids >= 0).all())
        ix.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
