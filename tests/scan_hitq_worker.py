"""Child process of tests/test_scan_hitq_gpu.py on libarchi_hip_dbg.so (one library per process): every case of
tests/scan_hitq_cases.py under the whole-tile arrangement (AK_SCAN_HITQ = 4) and under the queued one on both passes (3). Per case one
JSON line: whether `fast_only` ids, distances and certificate flags are equal under the two, whether `auto` under the queue equals the
oracle, and the instrumented kernels' counters of a queued run (entries queued, drains and tiles per wave, compactions)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from archi_amd import _lib
from archi_amd.index import HipIndex
from oracle import knn_oracle as ko
from tests import scan_hitq_cases as hc


def fast_only(ix, q, flt):
    """ids, distances, certificate flags of a device-resident `fast_only` search."""
    nq = len(q)
    tq = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    oi = torch.full((nq, hc.K), -1, dtype=torch.int64, device="cuda")
    od = torch.full((nq, hc.K), float("nan"), dtype=torch.float64, device="cuda")
    oc = torch.zeros((nq,), dtype=torch.int32, device="cuda")
    tf = torch.from_numpy(flt).cuda() if flt is not None else None
    ix.search_device(tq.data_ptr(), nq, hc.K, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), torch.cuda.current_stream().cuda_stream,
                     mode="fast_only", row_filter_ptr=tf.data_ptr() if tf is not None else 0)
    torch.cuda.synchronize()
    return oi.cpu().numpy(), od.cpu().numpy(), oc.cpu().numpy()


def counters(ix):
    out = {}
    for name, a in zip(("seed", "main"), ix.debug_read()):
        a = a[a[:, 7] > 0]
        out[name] = {"waves": len(a), "tiles": a[:, 7].tolist(), "queued": (a[:, 5] & 0xffffffff).tolist(), "drains": (a[:, 5] >> 32).tolist(),
                     "compactions": int(a[:, 6].sum())}
    return out


def main():
    assert _lib.is_dbg_library()
    for name in sys.argv[1:] or hc.CASES:
        c = hc.build(name)
        for sw in hc.ALL_SWITCHES:
            _lib.debug_set(sw, c["switches"].get(sw))
        rows, q = c["rows"], c["q"]
        ix = HipIndex(rows.shape[1], len(rows), dtype="bf16", metric="cosine", device=0)
        ix.add(rows, ids=c["ids"])
        stored = ko.round_through(rows, "bf16")
        alive = None
        if c["kill"] is not None:
            assert ix.remove(c["kill"]) == len(c["kill"])
            alive = np.isin(c["ids"], c["kill"], invert=True).astype(np.uint8)
        flt = c["row_filter"]
        if flt is not None:
            alive = alive & flt if alive is not None else flt
        oi, od, oc = ko.search(stored, q, hc.K, "cosine", ids=c["ids"], alive=alive)
        got = {}
        for hitq in ("4", "3"):
            _lib.debug_set("AK_SCAN_HITQ", hitq)
            before = ix.i8_info()["searches"]
            got[hitq] = fast_only(ix, q, flt)
            assert ix.i8_info()["searches"] == before + 1          # the int8 plan ran
        ai, ad, ac = ix.search(q, hc.K, mode="auto", row_filter=flt)
        _lib.debug_set("AK_SCAN_DBG", "1")
        instr = fast_only(ix, q, flt)
        cnt = counters(ix)
        _lib.debug_set("AK_SCAN_DBG", None)
        _lib.debug_set("AK_SCAN_HITQ", None)
        res = {"case": name,
               "plan": ix.scan_plan(len(q), hc.K),
               "fast_only_equal": [bool(np.array_equal(a, b, equal_nan=True)) for a, b in zip(got["4"], got["3"])],
               "instrumented_equal": [bool(np.array_equal(a, b, equal_nan=True)) for a, b in zip(got["3"], instr)],
               "certified": [int(got["4"][2].astype(bool).sum()), int(got["3"][2].astype(bool).sum())],
               "auto_equals_oracle": bool(np.array_equal(ai, oi) and np.array_equal(ad, od, equal_nan=True) and np.array_equal(ac, oc)),
               "counters": cnt}
        print("RESULT " + json.dumps(res), flush=True)
        ix.close()
    print("ok", flush=True)


if __name__ == "__main__":
    main()
