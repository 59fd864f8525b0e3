"""The int8 plan's quantiser and error bound, restated in numpy (no GPU needed): one scale per row and per query
(max |x| / 127 in float32, round to nearest, clip to +-127), the per-row relative rounding error rho in double, and the
certificate's eps = 4 gamma + rho_q + rho_c + rho_q rho_c + 1e-6 (+ 4 gamma, cosine) with rho_c the MAXIMUM over the rows.
The restatement is tied to the library by one GPU-produced fixture (tests/golden/i8_quantiser_gpu.json: the max rho the build's
own kernel measured on the same generated rows). On 20 000 rows x 64 queries |exact - int8 score| <= eps must hold for every
pair -- the bound every threshold, the seed re-rank and the certificate of the plan rest on."""
import json
import os

import numpy as np

from oracle import knn_oracle as ko

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "i8_quantiser_gpu.json")


def quantise(x):
    """-> (int8 values as float32 [n, d], scale float32 [n], rho float64 [n]); the arithmetic of k_shadow8 / k_query_setup8."""
    x = np.asarray(x, dtype=np.float32)
    mx = np.abs(x).max(axis=1)
    s = (mx / np.float32(127.0)).astype(np.float32)
    inv = np.where(s > 0, np.float32(1.0) / np.where(s > 0, s, 1), 0).astype(np.float32)
    v = np.clip(np.rint((x * inv[:, None]).astype(np.float32)), -127.0, 127.0).astype(np.float32)
    d = x.astype(np.float64) - s.astype(np.float64)[:, None] * v.astype(np.float64)
    rho = np.sqrt((d * d).sum(axis=1) / (x.astype(np.float64) ** 2).sum(axis=1))
    return v, s, rho


def test_int8_scores_stay_within_eps_of_the_exact_scores_and_rho_matches_the_gpu():
    g = json.load(open(GOLDEN))
    n, d, nq = g["rows"], g["dim"], 64
    assert n == 20000
    rows = ko.gen_rows(g["seed"], 0, 0, n, d, True, "bf16")
    q = ko.gen_rows(4321, 1, 0, nq, d, True, "f32")
    a8, sr, rho_r = quantise(rows)
    q8, sq, rho_q = quantise(q)
    rho_c = float(np.float32(rho_r.max() * 1.0001) + np.float32(1e-9))          # rounded up as the kernel does
    print(f"row rho: median {np.median(rho_r):.5f} p99.9 {np.quantile(rho_r, 0.999):.5f} max {rho_r.max():.5f}; "
          f"GPU max {g['max_rho']:.5f}; query rho: median {np.median(rho_q):.5f} max {rho_q.max():.5f}")
    # float32 ulp at 0.014 is 9.3e-10 and the fixture is truncated to 1e-9: the two maxima agree to 3e-9
    assert abs(rho_c - g["max_rho"]) <= 3e-9, (rho_c, g["max_rho"])
    # the scan: integer dot product (exact), one float32 multiply by ea8 = scale * 1/|a|, true units through a = s_q / |q|
    na = (rows.astype(np.float64) ** 2).sum(axis=1)
    ea8 = (sr * (1.0 / np.sqrt(na)).astype(np.float32)).astype(np.float32)
    dot = a8.astype(np.float64) @ q8.astype(np.float64).T                        # integers below 2^53: exact
    assert np.abs(dot).max() < 2 ** 24                                           # ... and exact as float32 in the kernel's filter
    s8 = (dot.astype(np.float32) * ea8[:, None]).astype(np.float32)
    qn = np.sqrt((q.astype(np.float64) ** 2).sum(axis=1))
    approx = s8.astype(np.float64) * (sq.astype(np.float64) / qn)[None, :]
    exact = (rows.astype(np.float64) @ q.astype(np.float64).T) / np.sqrt(na)[:, None] / qn[None, :]
    gamma = d * 2.0 ** -24
    eps = 4 * gamma + rho_q + rho_c + rho_q * rho_c + 1e-6 + 4 * gamma           # per query, cosine (k_query_setup8)
    err = np.abs(exact - approx)
    worst = (err / eps[None, :]).max()
    sigma = 1.0 / np.sqrt(d)
    print(f"eps: median {np.median(eps):.5f} = {np.median(eps) / sigma:.2f} sigma; largest |error| / eps {worst:.3f}")
    assert (err <= eps[None, :]).all(), worst


def test_the_int8_scan_kernels_spill_nothing():
    """The launched instantiations of the int8 tile (seeding pass, main pass) hold the budget the 16-bit tiles are held to in
    tests/test_scan_resources_cpu.py: 0 spilled vector registers, at most 8 bytes of scratch per lane."""
    import re
    import subprocess
    from scripts.kernel_resources import kernel_resources
    res = kernel_resources("scan.hip")
    names = subprocess.run(["c++filt"] + list(res), stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    checked = 0
    for (_, r), name in zip(res.items(), names):
        m = re.match(r"void ak::k_scan<true, ak::CfgP8, false, (true|false), (true|false)>", name)
        if not m or m.group(1) == "true":          # INSTR: the measurement instantiation (dbg library only)
            continue
        assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] <= 8, (name, r)
        checked += 1
    assert checked == 2, checked
