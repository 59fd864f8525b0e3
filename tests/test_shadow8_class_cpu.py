"""The int8 shadow's CLASS quantiser (csrc/shadow8_scale.h, k_shadow8), without a GPU.

The rows of a filter class -- the 16 rows of a 32-row block with one value of row bit 2, the set k_group_bounds maximises over --
share one scan-side term ea8 = E wherever they can adopt it, so that the scan's per-site bound max(0, max dot) * E is the site's
exact maximum score and the int8 tile's filter needs no per-row arithmetic. Restated here in numpy on the 20 000 generated rows of
tests/test_scan_i8_cpu.py's recipe x 64 queries:
  * |exact - int8 score| <= eps for every pair, with rho_c the measured maximum against the scale the scan applies (ea8 / ea);
  * on every site of a class whose rows all adopted, the bound equals max(0, the site's maximum score) under array_equal -- the
    site's maximum itself wherever that is not negative, and 0 = fma(0, E, 0), below every threshold the scan runs at, elsewhere;
  * the pass rate and the true-hit rate of both quantisers at the main pass's 3.71 sigma threshold are printed.
The restatement is tied to the library by tests/golden/i8_class_quantiser_gpu.json: the max rho the build's own kernel measured
on those rows on an MI355X, compared as the per-row test compares its fixture. The scale rule itself is driven alone by
tests/native/shadow8_scale_main.cpp under AddressSanitizer / UBSan."""
import json
import os
import subprocess

import numpy as np

from oracle import knn_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "i8_class_quantiser_gpu.json")
F = np.float32
CAP = F(2.0)           # S8_CLASS_CAP


def cosine_ea(x):
    """k_row_stats on cosine: na = the float32 sum of squares in row order, ea = (float)(1 / sqrt((double)na)), 0 for a row
    without a finite positive norm."""
    x = np.asarray(x, dtype=F)
    na = np.add.accumulate((x * x).astype(F), axis=1, dtype=F)[:, -1]
    ok = (na > 0) & np.isfinite(na)
    return np.where(ok, (1.0 / np.sqrt(np.where(ok, na, 1).astype(np.float64))).astype(F), F(0)).astype(F)


def own_scales(x):
    x = np.asarray(x, dtype=F)
    bad = ~np.isfinite(x).all(axis=1)
    mx = np.abs(np.where(np.isfinite(x), x, 0)).max(axis=1).astype(F)
    return np.where(bad, F(0), mx / F(127.0)).astype(F)


def class_ids(n):
    r = np.arange(n)
    return (r // 32) * 2 + ((r >> 2) & 1)


def quantise_rows(x, ea, shared=True):
    """-> dict(v int8 values as float32, scale, ea8, adopt, rho float64): k_shadow8 with shadow8_scale.h's rule (shared=True), or
    with one scale per row as it was (shared=False)."""
    x = np.asarray(x, dtype=F)
    n = len(x)
    own = own_scales(x)
    pos = lambda a: (a > 0) & np.isfinite(a)
    with np.errstate(all="ignore"):
        p = (own * ea).astype(F)
        p = np.where(pos(own) & pos(ea) & pos(p), p, F(0)).astype(F)
        cls = class_ids(n)
        E = np.zeros(cls.max() + 1, dtype=F)
        np.maximum.at(E, cls, p)
        Er = E[cls]
        s_sh = (Er / np.where(ea > 0, ea, 1)).astype(F)
        adopt = (p > 0) & (Er >= p) & (Er <= (CAP * p).astype(F)) & pos(s_sh) if shared else np.zeros(n, dtype=bool)
        scale = np.where(adopt, np.maximum(s_sh, own), own).astype(F)
        ea8 = np.where(adopt, Er, (own * ea).astype(F)).astype(F)
        inv = np.where(scale > 0, F(1.0) / np.where(scale > 0, scale, 1), 0).astype(F)
        v = np.clip(np.rint((x * inv[:, None]).astype(F)), -127.0, 127.0).astype(F)
        v = np.where(np.isnan(v), F(0), v)
        applied = np.where(adopt, Er.astype(np.float64) / np.where(ea > 0, ea, 1).astype(np.float64), scale.astype(np.float64))
        d = x.astype(np.float64) - applied[:, None] * v.astype(np.float64)
        rho = np.sqrt((d * d).sum(axis=1) / (x.astype(np.float64) ** 2).sum(axis=1))
    return dict(v=v, scale=scale, ea8=ea8, adopt=adopt, rho=rho, own=own)


def quantise_queries(q):
    """k_query_setup8's quantiser: one scale per query (unchanged; tests/test_scan_i8_cpu.py restates it too)."""
    q = np.asarray(q, dtype=F)
    s = (np.abs(q).max(axis=1) / F(127.0)).astype(F)
    inv = (F(1.0) / s).astype(F)
    v = np.clip(np.rint((q * inv[:, None]).astype(F)), -127.0, 127.0).astype(F)
    d = q.astype(np.float64) - s.astype(np.float64)[:, None] * v.astype(np.float64)
    return v, s, np.sqrt((d * d).sum(axis=1) / (q.astype(np.float64) ** 2).sum(axis=1))


def site_view(a, nq):
    """[n, nq] (n a multiple of 32) -> [blocks, kq, query, 8]: the 8 rows {16 h + 4 kq + j} a lane of the 16x16 tile holds of one
    32-row block for one query column (scan.hip, tile_epilogue)."""
    nb = a.shape[0] // 32
    return a.reshape(nb, 2, 4, 4, nq).transpose(0, 2, 4, 1, 3).reshape(nb, 4, nq, 8)


def class_term(ea8):
    """k_group_bounds over ea8 -> [blocks, kq]: the class of lane group kq is row bit 2 = kq & 1."""
    g = ea8.reshape(-1, 4, 2, 4).transpose(0, 2, 1, 3).reshape(-1, 2, 16).max(axis=2)      # [blocks, half]
    return g[:, [0, 1, 0, 1]]


def test_class_quantiser_eps_exact_bounds_and_gpu_rho():
    g = json.load(open(GOLDEN))
    n, d, nq = g["rows"], g["dim"], 64
    assert n == 20000 and n % 32 == 0
    rows = ko.gen_rows(g["seed"], 0, 0, n, d, True, "bf16")
    q = ko.gen_rows(4321, 1, 0, nq, d, True, "f32")
    ea = cosine_ea(rows)
    new, old = quantise_rows(rows, ea), quantise_rows(rows, ea, shared=False)
    q8, sq, rho_q = quantise_queries(q)
    kept = int((~new["adopt"]).sum())
    ratio = new["scale"] / new["own"]
    print(f"rows that kept their own scale: {kept} of {n}; shared / own scale: median {np.median(ratio):.3f} "
          f"p99 {np.quantile(ratio, 0.99):.3f} max {ratio.max():.3f}")
    assert (new["scale"] >= new["own"]).all()                                     # the clip at +-127 stays dead code
    assert np.abs(new["v"]).max() <= 127
    rho_c = float(F(new["rho"].max() * 1.0001) + F(1e-9))                         # rounded up as the kernel does
    rho_old = float(F(old["rho"].max() * 1.0001) + F(1e-9))
    print(f"row rho, class scales: median {np.median(new['rho']):.5f} max {new['rho'].max():.5f}; per-row scales: median "
          f"{np.median(old['rho']):.5f} max {old['rho'].max():.5f}; GPU max {g['max_rho']:.5f}")
    # float32 ulp at 0.014 is 9.3e-10 and the fixture is truncated to 1e-9: the two maxima agree to 3e-9
    assert abs(rho_c - g["max_rho"]) <= 3e-9, (rho_c, g["max_rho"])
    # eps rests on the MAXIMUM rho. Sharing a scale does move it: rho is not monotone in a row's peak, so a flatter row of a peaky
    # class, quantised with the peaky row's coarser scale, can end above that row's own figure (+3.0 % on these rows, +0.9 % on the
    # benchmark's 10M). Held here: the growth stays a few per cent -- within the cap a row loses at most one bit, and the rows near
    # the maximum are the peaky ones, whose scale grows least.
    assert rho_c <= rho_old * 1.05, (rho_c, rho_old)

    # the scan: integer dot product (exact), one float32 multiply by ea8; true units through a = s_q / |q|
    dot = new["v"].astype(np.float64) @ q8.astype(np.float64).T
    assert np.abs(dot).max() < 2 ** 24
    dot = dot.astype(F)
    s8 = (dot * new["ea8"][:, None]).astype(F)
    qn = np.sqrt((q.astype(np.float64) ** 2).sum(axis=1))
    na = (rows.astype(np.float64) ** 2).sum(axis=1)
    approx = s8.astype(np.float64) * (sq.astype(np.float64) / qn)[None, :]
    exact = (rows.astype(np.float64) @ q.astype(np.float64).T) / np.sqrt(na)[:, None] / qn[None, :]
    gamma = d * 2.0 ** -24
    eps = 4 * gamma + rho_q + rho_c + rho_q * rho_c + 1e-6 + 4 * gamma           # per query, cosine (k_query_setup8)
    err = np.abs(exact - approx)
    print(f"eps: median {np.median(eps):.5f}; largest |error| / eps {(err / eps[None, :]).max():.3f}; largest |error| {err.max():.5f}")
    assert (err <= eps[None, :]).all()

    # the filter's bound of a site against the site's exact maximum
    uniform = new["adopt"].reshape(-1, 4, 2, 4).transpose(0, 2, 1, 3).reshape(-1, 2, 16).all(axis=2)[:, [0, 1, 0, 1]]      # [blocks, kq]
    assert uniform.all() == (kept == 0)
    gea = class_term(new["ea8"])
    dpos = np.maximum(site_view(dot, nq).max(axis=3), F(0))
    U = (dpos * gea[:, :, None]).astype(F)                                        # fma(dpos, gea, geb = 0)
    smax = site_view(s8, nq).max(axis=3)
    sel = np.broadcast_to(uniform[:, :, None], U.shape)
    assert sel.any()
    assert np.array_equal(U[sel], np.maximum(smax[sel], F(0)))
    nonneg = sel & (smax >= 0)
    assert np.array_equal(U[nonneg], smax[nonneg]) and nonneg.sum() > 0.9 * sel.sum()
    assert (U >= smax).all()                                                      # an upper bound on every site, uniform or not

    # pass rate and true-hit rate at the main pass's threshold (3.71 sigma, scan units of each query)
    thr = (3.71 / np.sqrt(d)) / (sq.astype(np.float64) / qn)
    for name, z in (("per-row scales", old), ("class scales", new)):
        dz = (z["v"].astype(np.float64) @ q8.astype(np.float64).T).astype(F)
        sz = (dz * z["ea8"][:, None]).astype(F)
        Uz = (np.maximum(site_view(dz, nq).max(axis=3), F(0)) * class_term(z["ea8"])[:, :, None]).astype(F)
        hit = site_view(sz, nq).max(axis=3) >= thr[None, None, :]
        passed = Uz >= thr[None, None, :]
        assert (passed | ~hit).all()
        print(f"{name}: lane-sites passing the bound {100 * passed.mean():.4f} %, with a true hit {100 * hit.mean():.4f} %")
        if z is new and kept == 0:
            assert np.array_equal(passed, hit)


def test_special_rows_and_the_cap_in_the_restatement():
    """The numpy restatement on classes the generated corpus does not hold: a zero row, a row with an infinity, a removed row
    (ea = 0) and a row the cap excludes keep their own scale; the others of their class share one ea8."""
    rng = np.random.default_rng(7)
    x = rng.standard_normal((64, 256)).astype(F)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[1] = 0
    x[9, 5] = np.inf
    x[17] *= 0
    x[17, 3] = 1.0                                   # one dominant component: own * ea = 1 / 127, far above the cap
    ea = cosine_ea(x)
    assert ea[1] == 0 and ea[9] == 0
    ea[3] = 0                                        # removed
    z = quantise_rows(x, ea)
    cls0 = np.array([8 * (m >> 2) + (m & 3) for m in range(16)])
    assert set(cls0) == set(np.nonzero(class_ids(32) == 0)[0])
    special = np.array([1, 9, 3])
    assert not z["adopt"][special].any() and z["adopt"][17]
    # the peaky row sets E; the plain rows are beyond the cap of it and keep their own scales
    others = np.setdiff1d(cls0, np.append(special, 17))
    assert not z["adopt"][others].any()
    assert z["adopt"][32:].all() and len(np.unique(z["ea8"][class_ids(64) == 2])) == 1
    assert (z["v"][1] == 0).all() and (z["v"][9] == 0).all()


def test_scale_rule_header_under_sanitizers():
    """csrc/shadow8_scale.h driven alone by tests/native/shadow8_scale_main.cpp (-fsanitize=address,undefined): special rows, the cap,
    an append into a partly published class (published values unchanged), shared scale >= own scale on a random sweep."""
    csrc = os.path.join(ROOT, "archi_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "asan-shadow8"])
    p = subprocess.run([os.path.join(csrc, "build", "shadow8_scale_asan")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode("utf-8", "replace")
    assert p.returncode == 0 and out.rstrip().splitlines()[-1] == "shadow8_scale: ok" and "Sanitizer" not in out, out[-3000:]
