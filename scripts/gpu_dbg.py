"""Phase cycle counters of the scan kernel (AK_SCAN_DBG)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["AK_SCAN_DBG"] = "1"
import numpy as np, torch
from archi_amd.index import HipIndex
n, d, dtype, nq = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
ix = HipIndex(d, n, dtype=dtype, metric="cosine", device=0); ix.generate(seed=1234, n=n)
tmp = HipIndex(d, nq, dtype=dtype, metric="cosine", device=0); tmp.generate(seed=4321, n=nq, stream=1)
q = tmp.fetch(np.arange(nq)); tmp.close()
tq = torch.from_numpy(q).cuda(); k = 10
oi = torch.empty((nq, k), dtype=torch.int64, device="cuda"); od = torch.empty((nq, k), dtype=torch.float64, device="cuda")
oc = torch.empty((nq,), dtype=torch.int32, device="cuda")
for _ in range(3):
    ix.search_device(tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), torch.cuda.current_stream().cuda_stream)
torch.cuda.synchronize()
dbg = ix.debug_read()
names = ["k-loop", "filter", "sync", "compact", "final", "n_slow", "n_comp", "tiles"]
for li, lname in enumerate(("seed", "main")):
    a = dbg[li]; a = a[a[:, 7] > 0]
    if not len(a): continue
    print(f"{lname}: waves={len(a)} tiles/wave={a[:,7].mean():.1f}")
    # slot 5: slow-path entries of lane 0 (site-by-site and whole-tile filter); the queued filter of the int8 tile (AK_SCAN_HITQ, or
    # the pass ships on it) puts the wave's queued entries there and its drains in the high half
    drains = (a[:, 5] >> 32).astype(np.float64)
    a[:, 5] &= 0xffffffff
    stage = (a[:, 2] & 0xffffffff).astype(np.float64); wait = (a[:, 2] >> 32).astype(np.float64)
    a = a.astype(np.float64); a[:, 2] = 0             # (slot 2 packs the two parts of the k-loop printed below: not a phase of its own)
    tot = a[:, :5].sum(1).mean()
    for j in range(5):
        print(f"   {names[j]:8s} mean {a[:, j].mean()/1e3:9.1f} kcyc  ({100*a[:, j].mean()/tot:5.1f}%)  max {a[:, j].max()/1e3:9.1f}")
    print(f"   k-loop split: staging issue {stage.mean()/1e3:9.1f} kcyc, wait+barrier {wait.mean()/1e3:9.1f} kcyc, "
          f"fragments+MFMA {(a[:,0]-stage-wait).mean()/1e3:9.1f} kcyc; per k-step: "
          f"{stage.mean()/(a[:,7].mean()*int(sys.argv[2])//64):.0f} / {wait.mean()/(a[:,7].mean()*int(sys.argv[2])//64):.0f} / "
          f"{(a[:,0]-stage-wait).mean()/(a[:,7].mean()*int(sys.argv[2])//64):.0f} cycles")
    # the int8 tile's whole-tile filter (the main pass unless AK_SCAN_HITQ / AK_SCAN_FILTER say otherwise) has no drains: the high half
    # holds the WAVE's lane-sites that were entered and appended nothing -- 0 on a corpus whose filter classes all share one scale
    whole_tile_i8 = lname == "main" and dtype != "f32" and os.environ.get("AK_SCAN_HITQ", "") not in ("2", "3") \
        and os.environ.get("AK_SCAN_FILTER", "") in ("", "2") and ix.scan_plan(nq, k).get("kprime") == 512
    if whole_tile_i8:
        print(f"   slow-path entries/wave {a[:,5].mean():.1f} (lane 0, of {a[:,7].mean()*16:.0f} sites)  entered without a hit/wave "
              f"{drains.mean():.2f} (all lanes)  compactions/wave {a[:,6].mean():.1f}   total {tot/1e3:.0f} kcyc")
    elif drains.sum() > 0:
        print(f"   queued filter: entries/wave {a[:,5].mean():.1f} = {a[:,5].mean()/a[:,7].mean():.1f} per tile (of 1024 lane-sites), "
              f"drains/wave {drains.mean():.1f} = {drains.mean()/a[:,7].mean():.2f} per tile, max {(drains/a[:,7]).max():.2f}  "
              f"compactions/wave {a[:,6].mean():.1f}   total {tot/1e3:.0f} kcyc")
    else:
        print(f"   slow-path entries/wave {a[:,5].mean():.1f} (of {a[:,7].mean()*8:.0f} groups)  compactions/wave {a[:,6].mean():.1f}   total {tot/1e3:.0f} kcyc")
ix.close()
