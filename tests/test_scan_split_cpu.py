"""Register budget and instantiation sets of the scan kernels with the filter arrangement as a tile parameter (ScanCfg::FILT; no
GPU needed). The whole-tile arrangement holds 2 * NI thresholds and up to 64 registers of per-row terms across the maxima of a tile,
on top of 128 accumulators: every k_scan instantiation either library launches stays at 0 spilled vector registers and at most 8 bytes of
scratch per lane (the frame of the out-of-line compaction routine), the dbg library carries both arrangements of P, P8, Q and R,
and the product library carries one per tile and refuses the switch that picks between them."""
import os
import re
import subprocess

import pytest

from scripts.kernel_resources import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN = re.compile(r"void ak::k_scan<(true|false), ak::(ScanCfg<[^>]*>|CfgP8f?), (true|false), (true|false), (true|false)>")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from archi_amd import _lib
    return _lib


def _launched(extra_flags):
    """{(tile type, SEED): resources} of the k_scan instantiations a build launches outside the measurement ones (INSTR)."""
    res = kernel_resources("scan.hip", extra_flags=extra_flags)
    names = subprocess.run(["c++filt"] + list(res), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    out = {}
    for (_, r), name in zip(res.items(), names):
        m = SCAN.match(name)
        if m and m.group(4) == "false":
            out[(m.group(1), m.group(2), m.group(3), m.group(5))] = r
    return out


def _arrangements(tiles):
    """{tile geometry or 'P8': set of FILT values} of the 16x16x32 tiles among `tiles` (ScanCfg<WM, WN, MI, NI, ring, minw, phased,
    FILT, MFMA>; CfgP8 ships the arrangement of its base, CfgP8f is the other one)."""
    out = {}
    for t in tiles:
        if t.startswith("CfgP8"):
            out.setdefault("P8", set()).add(t)
            continue
        f = t[len("ScanCfg<"):-1].split(", ")
        if f[8] == "16":
            out.setdefault(tuple(f[:4]), set()).add(int(f[7]))
    return out


@pytest.mark.parametrize("library,flags", [("product", []), ("dbg", ["-DAK_DBG_KERNELS=1"])])
def test_no_launched_scan_kernel_spills_in_either_library(library, flags):
    got = _launched(flags)
    for key, r in got.items():
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] <= 8, (library, key, r)
    arr = _arrangements({k[1] for k in got if k[2] == "false"})
    geometries = {("2", "4", "4", "2"), ("2", "4", "4", "1"), ("4", "2", "2", "3")}          # P, Q, R
    assert set(arr) == geometries | {"P8"}, arr
    if library == "dbg":
        assert all(arr[g] == {0, 1} for g in geometries) and arr["P8"] == {"CfgP8", "CfgP8f"}, arr
    else:
        assert all(len(arr[g]) == 1 for g in geometries) and arr["P8"] == {"CfgP8"}, arr


def test_product_library_holds_one_arrangement_per_tile_and_refuses_the_switch(built):
    lib = os.path.join(ROOT, "archi_amd", "lib", "libarchi_hip.so")
    dbg = os.path.join(ROOT, "archi_amd", "lib", "libarchi_hip_dbg.so")

    def tiles(path):
        out = subprocess.run(["nm", "-C", path], stdout=subprocess.PIPE, text=True, check=True).stdout
        return {m.group(2) for m in SCAN.finditer(out)}

    arr = _arrangements(tiles(lib))
    assert len(arr) == 4 and all(len(v) == 1 for v in arr.values()) and arr["P8"] == {"CfgP8"}, arr
    arr = _arrangements(tiles(dbg))
    assert len(arr) == 4 and all(len(v) == 2 for v in arr.values()), arr
    set_switch = built.load().ak_debug_set
    assert set_switch(b"AK_SCAN_FILTER", b"1") != 0 and set_switch(b"AK_SCAN_FILTER", b"2") != 0
    assert set_switch(b"AK_SCAN_FILTER", b"0") == 0 and set_switch(b"AK_SCAN_FILTER", None) == 0
