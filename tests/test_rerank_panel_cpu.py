"""CPU-side checks of the panel re-rank kernel (csrc/exact.hip): what the compiler made of it, the switch, and the numpy statement
of the distance key that the GPU test compares with."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_panel_rerank_kernels_spill_nothing():
    """Every instantiation of k_rerank_panel (f32, bf16, f16): 0 spilled vector registers, no scratch, and at most 128 VGPRs, so
    that four waves per SIMD stay resident -- 24 parked uint4 are 96 of them. The thread-per-candidate kernel is still there."""
    from scripts.kernel_resources import kernel_resources
    res = kernel_resources("exact.hip")
    names = subprocess.run(["c++filt"] + list(res), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    panel, old = 0, 0
    for (_, r), name in zip(res.items(), names):
        if re.match(r"void ak::k_rerank<\d>", name):
            old += 1
        if not re.match(r"void ak::k_rerank_panel<\d>", name):
            continue
        print(name.split("(")[0], {k: r[k] for k in ("VGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")})
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)
        assert r["VGPRs"] + r["AGPRs"] <= 128 and r["Occupancy [waves/SIMD]"] >= 4, (name, r)
        panel += 1
    assert panel == 3 and old == 3, (panel, old)


def test_the_switch_is_in_the_table_and_in_the_product_library():
    """AK_RERANK_OLD: a numeric switch of the product library (0 = the panel kernel, the default), accepted by ak_debug_set."""
    from archi_amd import _lib
    src = open(os.path.join(ROOT, "archi_amd", "csrc", "index.hip")).read()
    assert re.search(r'\{"AK_RERANK_OLD", &Switches::rerank_old, 0, false, false, false\}', src)
    assert "rerank_old{0}" in open(os.path.join(ROOT, "archi_amd", "csrc", "switches.h")).read()
    lib = _lib.load()
    for v in (b"1", b"0", None):
        assert lib.ak_debug_set(b"AK_RERANK_OLD", v) == 0
    names = {n for n, _, _ in _lib.KTS_SYMBOLS if n.startswith("ak_kts_rr_")}
    assert names == {"ak_kts_rr_rerank", "ak_kts_rr_choice"}
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "archi_amd", "lib", "libarchi_hip_dbg.so")],
                         stdout=subprocess.PIPE, check=True).stdout.decode()
    assert set(re.findall(r"\b(ak_kts_rr_[a-z0-9_]+)\b", out)) == names


def test_numpy_dist_key_is_the_oracle_order():
    """tests/rerank_panel_cases.py dist_key: ascending with the distance, -0.0 as +0.0, NaN above +inf and below KEY_INVALID."""
    from tests import rerank_panel_cases as rc
    d = np.array([-np.inf, -2.5, -1e-300, -0.0, 0.0, 5e-324, 1.0, 1.0000000000000002, np.inf, np.nan])
    k = rc.dist_key(d)
    assert k[3] == k[4] and (np.diff(k[[0, 1, 2, 3, 5, 6, 7, 8, 9]].astype(object)) > 0).all()
    assert k[9] == np.uint64(0xFFF8000000000000) and k[9] < rc.KEY_INVALID and k[4] == np.uint64(1 << 63)
