"""What the CPU proves about tests/test_parity_kernels_gpu.py, on the very inputs of its cases:

  * an emulation of each kernel's documented rounding scheme (float32 accumulation, the three-term split product, the cubic-piece
    table, the order of the roundings) stays inside every bound and meets every structural check;
  * every listed defect, applied to the reference, lands outside -- on at least one case, and where it can only show on a class of
    cases, on every case of that class (the class is stated next to each);
  * the case lists sit where they are meant to: launch_gemm_x3w's tile rule, restated, puts each case on its tile;
  * the table of MODE 6, rebuilt from its description, is within the 4.9e-7 the comment in gemm.hip states of the exact GELU over |x| <= 8,
    and the split's dropped terms are within C_SPLIT of the absolute sum on every case.
The bounds are not touched here: a mutant that slips through means the case list is too weak."""
import math

import numpy as np
import pytest

from tests import kernel_refs as kr
from tests import parity_kernel_cases as pc
from tests import parity_kernel_refs as pr

F = np.float32


def _cached(fn):
    memo = {}

    def get(c, *a):
        key = (c["name"],) + a
        if key not in memo:
            memo[key] = fn(c, *a)
        return memo[key]
    return get


# ---- GEMM ------------------------------------------------------------------------------------------------------------------------------
@_cached
def _gemm(c):
    inp = pc.gemm_inputs(c)
    rb = pc.gemm_res_block(c, inp)
    exp = {"f32": pr.gemm_f32_expect(c["epi"], inp["x"], inp["w"], inp["bias"], rb), "x3": pr.gemm_x3_expect(c["epi"], inp["x"], inp["w"], inp["bias"], rb)}
    return inp, rb, exp


def _gemm_outside(c, which, Y):
    """True when Y, taken as the kernel's output allocation, fails the GPU test's checks."""
    want, bound = _gemm(c)[2][which]
    w = kr.Worst()
    touched = pc.gemm_check(c, Y, want, bound, w)
    return w.ratio > 1.0 or touched > 0


def test_emulated_gemms_stay_inside_the_bound_and_leave_the_sentinels():
    for c in pc.gemm_cases():
        inp, rb, _ = _gemm(c)
        for which, emu in (("f32", pr.emu_gemm_f32), ("x3", pr.emu_gemm_x3)):
            assert not _gemm_outside(c, which, pc.gemm_place(c, emu(c["epi"], inp["x"], inp["w"], inp["bias"], rb))), (c["name"], which)


def test_dropped_split_terms_are_within_the_derived_constant():
    for c in pc.gemm_cases():
        inp = _gemm(c)[0]
        drop = pr.split_drop(inp["x"], inp["w"])
        assert (drop <= pr.C_SPLIT * (np.abs(inp["x"].astype(np.float64)) @ np.abs(inp["w"].astype(np.float64)).T) + 1e-300).all(), c["name"]
        xh, xl, xr = pr.split3(inp["x"])
        x64 = np.abs(inp["x"].astype(np.float64))
        assert (np.abs(xl) <= pr.U * (1 + pr.U) * x64).all() and (np.abs(xr) <= pr.U ** 2 * x64).all(), c["name"]


def _round_bits(x, bits):
    """float32 x rounded to `bits` mantissa bits."""
    b = np.ascontiguousarray(x, F).view(np.uint32).astype(np.uint64)
    m = 23 - bits
    return (((b + (1 << (m - 1))) >> m) << m).astype(np.uint32).view(F)


def _gemm_mutant(c, which, mut):
    """The output allocation of the reference with one defect, or None where the defect cannot occur on this case."""
    inp, rb, _ = _gemm(c)
    T, N, K, epi = c["T"], c["N"], c["K"], c["epi"]
    x, w, b = inp["x"].astype(np.float64), inp["w"].astype(np.float64), inp["bias"].astype(np.float64)
    res = None if rb is None else rb.astype(np.float64)
    col0, gelu = None, kr.gelu64
    if mut in ("lo_hi", "hi_lo"):
        if which != "x3":
            return None
        xh, xl, _ = pr.split3(inp["x"])
        wh, wl, _ = pr.split3(inp["w"])
        y = xh @ wh.T + (xh @ wl.T if mut == "lo_hi" else xl @ wh.T) + b
    elif mut in ("x_bf16", "x_10bit", "w_bf16"):
        if which != "f32":
            return None
        if mut == "w_bf16":
            y = x @ kr.bf16_round(inp["w"]).astype(np.float64).T + b
        else:
            y = (kr.bf16_round(inp["x"]) if mut == "x_bf16" else _round_bits(inp["x"], 10)).astype(np.float64) @ w.T + b
    elif mut in ("skip_first", "skip_last"):
        x2 = x.copy()
        if mut == "skip_first":
            x2[:, :32] = 0.0
        else:
            x2[:, K - 32:] = 0.0
        y = x2 @ w.T + b
    elif mut == "last_from_prev":
        if K < 64:
            return None
        x2, w2 = x.copy(), w.copy()
        x2[:, K - 32:], w2[:, K - 32:] = x[:, K - 64:K - 32], w[:, K - 64:K - 32]
        y = x2 @ w2.T + b
    elif mut == "bias_tile0":
        if N <= 128:
            return None
        y = x @ w.T + b[np.arange(N) % 128]
    elif mut == "col0_ignored":
        if c["col0"] == 0:
            return None
        y, col0 = x @ w.T + b, 0
    elif mut == "res_ldc_N":
        if epi != 2 or c["ldc"] == N or T == 1:
            return None
        y = x @ w.T + b
        res = inp["res"].reshape(-1)[(np.arange(T)[:, None] * N + c["col0"] + np.arange(N)[None, :])].astype(np.float64)
    elif mut == "tile8_as_0":
        if T <= 1024:
            return None
        y = x @ w.T + b
        y[1024:] = y[:T - 1024]
    elif mut == "tanh_gelu":
        if epi != 1:
            return None
        y, gelu = x @ w.T + b, kr.gelu_tanh64
    else:
        raise KeyError(mut)
    out = gelu(y) if epi == 1 else (y + res if epi == 2 else y)
    return pc.gemm_place(c, out.astype(F), col0)


# (defect, launcher, the class of cases on every one of which it must show; None: every case on which it can occur)
GEMM_MUTANTS = [
    ("lo_hi", "x3", ("onehot", "cancel")), ("hi_lo", "x3", ("onehot", "cancel")),
    ("x_bf16", "f32", ("onehot", "cancel")), ("w_bf16", "f32", ("onehot", "cancel")), ("x_10bit", "f32", ("onehot",)),
    ("skip_first", "f32", ("random", "gelu", "cancel")), ("skip_last", "f32", ("random", "gelu", "cancel")),
    ("skip_first", "x3", ("random", "gelu", "cancel")), ("skip_last", "x3", ("random", "gelu", "cancel")),
    ("last_from_prev", "f32", ("random", "gelu", "cancel")), ("last_from_prev", "x3", ("random", "gelu", "cancel")),
    ("bias_tile0", "f32", None), ("bias_tile0", "x3", None), ("col0_ignored", "f32", None), ("col0_ignored", "x3", None),
    ("res_ldc_N", "f32", None), ("res_ldc_N", "x3", None), ("tile8_as_0", "f32", None), ("tile8_as_0", "x3", None),
    ("tanh_gelu", "f32", None), ("tanh_gelu", "x3", None),
]


@pytest.mark.parametrize("mut,which,classes", GEMM_MUTANTS)
def test_every_gemm_defect_lands_outside(mut, which, classes):
    caught, must = [], []
    for c in pc.gemm_cases():
        Y = _gemm_mutant(c, which, mut)
        if Y is None:
            continue
        hit = _gemm_outside(c, which, Y)
        caught.append(hit)
        if classes is None or c["cls"] in classes:
            must.append((c["name"], hit))
    assert must and any(caught), (mut, which)
    assert all(hit for _, hit in must), (mut, which, [n for n, hit in must if not hit])
    print(f"{mut} ({which}): caught on {sum(caught)} of {len(caught)} cases on which it can occur, on all {len(must)} of its class")


# ---- MODE 5 / 6 ------------------------------------------------------------------------------------------------------------------------
def test_case_lists_of_launch_gemm_x3w_select_what_they_are_meant_to():
    """launch_gemm_x3w's rule restated (pc.x3w_selection): the small shapes run the narrow tile by the launcher's choice and the wide one
    under AK_GEMM_BN=256; (4096, 4096) is the first shape of its kind on the wide tile by that choice (256 tiles), (3840, 4352) the last on
    the narrow one (255 wide tiles); (2560, 3328) gives a workgroup of the 256 a second narrow tile; every nvalid the issue lists occurs."""
    d = {c["name"]: pc.x3w_selection(c) for c in pc.x3w_cases("default")}
    sel = lambda T, N, mode=5: [v for c, v in ((c, d[c["name"]]) for c in pc.x3w_cases("default")) if (c["T"], c["N"], c["mode"]) == (T, N, mode)][0]
    assert all(not pc.x3w_selection(c)[0] for c in pc.x3w_cases("default") if c["T"] <= 512)
    assert all(pc.x3w_selection(c)[0] and c["N"] % 256 == 0 for c in pc.x3w_cases("wide")) and len(pc.x3w_cases("wide")) >= 4
    assert sel(4096, 4096) == (True, 256, 256) and sel(4096, 4096, 6) == (True, 256, 256)
    assert sel(3840, 4352) == (False, 15 * 34, 256) and (3840 // 256) * (4352 // 256) == 255
    assert sel(2560, 3328) == (False, 260, 256)
    for child in ("default", "wide"):
        for c in pc.x3w_cases(child):
            assert c["T"] % 256 == 0 and c["N"] % 128 == 0 and c["K1"] % 64 == 0, c["name"]
    nv = {(c["nvalid"], c["N"]) for c in pc.x3w_cases("default") if c["mode"] == 5}
    assert {(0, 128), (384, 512), (512, 512), (1152, 1280)} <= nv
    assert {c["mode"] for c in pc.x3w_cases("wide")} == {5, 6} and {c["K1"] for c in pc.x3w_cases("default")} >= {64, 128, 384}


def _x3w_small():
    return [c for child in ("default", "wide") for c in pc.x3w_cases(child) if c["T"] <= 512]


def _x3w_out(c, inp, mut=None):
    """The reference (float64, rounded once) as the launch's output buffer, with one defect or none."""
    xh, xl = pr.halves(inp["x2"])
    wh, wl = pr.halves(inp["w2"])
    b = inp["bias"].astype(np.float64)
    y = xh @ wh.T + (0.0 if mut == "hi_lo" else xl @ wh.T) + (0.0 if mut == "lo_hi" else xh @ wl.T) + xl @ wl.T + b
    N, nv = c["N"], pc.x3w_nvalid(c)
    if c["mode"] == 5:
        out = np.full((c["T"], N), pc.SENT, F)
        nv = nv // 128 * 128 if mut == "nvalid_128" else (N if mut == "nvalid_ignored" else nv)
        out[:, :nv] = y[:, :nv]
        return out
    g = (kr.gelu_tanh64(y) if mut == "tanh_gelu" else kr.gelu64(y)).astype(F)
    out = pr.split_rows(g)
    if mut == "lo_copy":
        out[:, N:] = out[:, :N]
    return out


def test_emulated_modes_5_and_6_stay_inside_and_their_defects_land_outside():
    muts = {"lo_hi": [], "hi_lo": [], "nvalid_128": [], "nvalid_ignored": [], "tanh_gelu": [], "lo_copy": []}
    for c in _x3w_small():
        inp = pc.x3w_inputs(c)
        w = kr.Worst()
        emu = pr.emu_gemm_x3w(c["mode"], inp["x2"], inp["w2"], inp["bias"])
        if c["mode"] == 5:
            emu[:, pc.x3w_nvalid(c):] = pc.SENT                      # (the columns the kernel leaves alone)
        assert pc.x3w_check(c, emu, inp, w) == 0 and w.ratio <= 1.0, (c["name"], str(w))
        w = kr.Worst()
        assert pc.x3w_check(c, _x3w_out(c, inp), inp, w) == 0 and w.ratio <= 1.0, (c["name"], str(w))
        for m in muts:
            if (m.startswith("nvalid") and (c["mode"] != 5 or pc.x3w_nvalid(c) == c["N"])) or (m == "nvalid_128" and pc.x3w_nvalid(c) % 128 == 0) or \
                    (m in ("tanh_gelu", "lo_copy") and c["mode"] != 6):
                continue
            w = kr.Worst()
            bad = pc.x3w_check(c, _x3w_out(c, inp, m), inp, w)
            muts[m].append((c["name"], bad > 0 or w.ratio > 1.0))
    for m, rows in muts.items():
        assert rows and all(hit for _, hit in rows), (m, [n for n, hit in rows if not hit])
        print(f"{m}: caught on all {len(rows)} cases on which it can occur")


def test_table_gelu_of_mode_6_is_within_the_stated_distance_of_the_exact_function():
    """gemm.hip: `Max |error| against the double-precision function over |x| <= 8: 4.9e-7` (the float32 evaluation, product rounding
    included); the interpolation itself is 1.4e-9. Both, on the table rebuilt from the description."""
    x = np.concatenate([np.linspace(-8.0, 8.0, 1 << 21), np.linspace(-6.0, 6.0, 384 * 64 + 1), [-8.0, 8.0, -6.0, 6.0, 0.0]]).astype(F)
    g = kr.gelu64(x.astype(np.float64))
    e64 = np.abs(pr.gelu_tab64(x.astype(np.float64)) - g)
    e32 = np.abs(pr.gelu_tab32(x).astype(np.float64) - g)
    inside = np.abs(x) < 6.0
    print(f"table GELU: float64 evaluation max |error| {e64.max():.3g} (inside [-6, 6): {(e64[inside] / np.maximum(np.abs(x[inside]), 1e-30)).max():.3g} |x|), "
          f"float32 evaluation {e32.max():.3g} at x = {float(x[np.argmax(e32)])!r}")
    assert (e64[inside] <= 1.4e-9 * np.abs(x[inside]) + 1e-18).all()
    assert e32.max() <= 4.9e-7
    y = x.astype(np.float64)[None, ::64]
    want, bound = pr.gelu_tab_bound(y, np.zeros_like(y))
    assert (np.abs(pr.gelu_tab32(x[None, ::64]).astype(np.float64) - want) <= bound).all()


# ---- gemm_ln_x3 and the row kernels ----------------------------------------------------------------------------------------------------
def _flagged(out32, out2, want, bound, name="m"):
    w = kr.Worst()
    mism = pc.split_out_check(name, out32, out2, want, bound, w) if out2 is not None else (w.add(out32, want, bound, name), 0)[1]
    return mism > 0 or w.ratio > 1.0


def _out2_mutants(out32):
    good = pr.split_rows(out32)
    H = out32.shape[1]
    lo_copy = good.copy()
    lo_copy[:, H:] = good[:, :H]
    stride = np.full(good.size + 2 * H, pc.SENT16, np.uint16)           # row t at t * H: the lo half lands in the next row's hi half
    for t in range(good.shape[0]):
        stride[t * H:t * H + 2 * H] = good[t]
    return {"out2_lo_copy_of_hi": lo_copy, "out2_row_stride_H": stride[:good.size].reshape(good.shape)}


def test_emulated_gemm_ln_x3_stays_inside_and_its_defects_land_outside():
    for c in pc.gemm_ln_x3_cases():
        inp = pc.gemm_ln_x3_inputs(c)
        want, bound = pc.gemm_ln_x3_expect(c, inp)
        K = c["K1"]
        acc = pr.emu_three_term(*(kr.bf16_value(a) for a in (inp["x2"][:, :K], inp["x2"][:, K:], inp["w2"][:, :K], inp["w2"][:, K:])), step=32)
        r = ((acc + inp["bias"]).astype(F) + inp["res"]).astype(F)
        out = kr.layernorm_emulate(r, inp["gamma"], inp["beta"], c["eps"])
        assert not _flagged(out, pr.split_rows(out), want, bound), c["name"]
        for mut in (dict(eps_mode="outside"), dict(ddof=1)):
            if "ddof" in mut and c["K1"] > 384:          # (1 / (2 H) relative: below the accumulation bound of 3 x 1536 products)
                continue
            assert _flagged(pc.gemm_ln_x3_expect(c, inp, **mut)[0].astype(F), None, want, bound), (c["name"], mut)
        no_res = dict(inp, res=np.zeros_like(inp["res"]))
        assert _flagged(pc.gemm_ln_x3_expect(c, no_res)[0].astype(F), None, want, bound), c["name"]
        for name, o2 in _out2_mutants(want.astype(F)).items():
            assert _flagged(want.astype(F), o2, want, bound) or (c["T"] == 1 and name == "out2_row_stride_H"), (c["name"], name)


def test_emulated_row_kernels_stay_inside_and_their_defects_land_outside():
    """eps outside the root shows on the near-constant row (every case that has one: T >= 3); unbiased variance, the residual left out
    and both out2 defects on every case."""
    for c in pc.embed_cases():
        inp = pc.embed_inputs(c)
        want, bound = pc.embed_expect(c, inp)
        ids = inp["ids"].copy()
        ids[(ids < 0) | (ids >= pc.VOCAB)] = 0
        posrow = inp["posid"] if inp["posid"] is not None else np.arange(c["T"]) % c["S"]
        r = ((inp["word"][ids] + inp["pos"][posrow]).astype(F) + inp["type"]).astype(F)
        out = kr.layernorm_emulate(r, inp["gamma"], inp["beta"], c["eps"])
        assert not _flagged(out, pr.split_rows(out), want, bound), c["name"]
        assert _flagged(pc.embed_expect(c, inp, ddof=1)[0].astype(F), None, want, bound), c["name"]
        wrong = dict(inp, ids=np.where((inp["ids"] < 0) | (inp["ids"] >= pc.VOCAB), 1, inp["ids"]))       # out-of-range ids to row 1
        assert _flagged(pc.embed_expect(c, wrong)[0].astype(F), None, want, bound), c["name"]
        for name, o2 in _out2_mutants(want.astype(F)).items():
            assert _flagged(want.astype(F), o2, want, bound) or (c["T"] == 1 and name == "out2_row_stride_H"), (c["name"], name)
    for c in pc.add_ln_cases():
        inp = pc.add_ln_inputs(c)
        want, bound = pc.add_ln_expect(c, inp)
        r = inp["y"] if inp["r"] is None else (inp["y"] + inp["r"]).astype(F)
        out = kr.layernorm_emulate(r, inp["gamma"], inp["beta"], c["eps"])
        assert not _flagged(out, pr.split_rows(out), want, bound), c["name"]
        assert _flagged(pc.add_ln_expect(c, inp, ddof=1)[0].astype(F), None, want, bound), c["name"]
        if c["T"] >= 3:
            assert _flagged(pc.add_ln_expect(c, inp, eps_mode="outside")[0].astype(F), None, want, bound), c["name"]
        if inp["r"] is not None:
            assert _flagged(pc.add_ln_expect(c, inp, no_residual=True)[0].astype(F), None, want, bound), c["name"]
        for name, o2 in _out2_mutants(want.astype(F)).items():
            assert _flagged(want.astype(F), o2, want, bound) or (c["T"] == 1 and name == "out2_row_stride_H"), (c["name"], name)


def test_emulated_pooling_stays_inside_and_its_defects_land_outside():
    for c in pc.pool_cases():
        inp = pc.pool_inputs(c)
        for pooling, normalise in pc.POOL_MODES:
            want, bound = pr.pool_expect(inp["x"], inp["mask"], pooling, normalise)
            assert not _flagged(pr.emu_pool(inp["x"], inp["mask"], pooling, normalise), None, want, bound), (c["name"], pooling, normalise)
            assert (want[3] == 0).all() and (bound[3] == 0).all()                              # no visible token / a zero CLS row: exact zeros
            assert (want[pc.pool_zero_rows(pooling)] == 0).all() and (pr.emu_pool(inp["x"], inp["mask"], pooling, normalise)[pc.pool_zero_rows(pooling)] == 0).all()
            mut = dict(count_masked=True) if pooling == 0 else dict(cls_batch0=True)
            assert _flagged(pr.pool_expect(inp["x"], inp["mask"], pooling, normalise, **mut)[0].astype(F), None, want, bound), (c["name"], pooling, normalise)


def test_split_structure_checks_hold_the_split_and_flag_what_is_not_one():
    for c in pc.split_cases():
        x = pc.split_inputs(c).reshape(-1)
        hi, lo = pr.split_bits(x)
        assert pr.split_mismatch(x, hi, lo) == 0 and pr.lo_too_large(hi, lo) == 0, c["name"]
        if x.size < 8:
            continue
        assert pr.split_mismatch(x, hi, hi) > 0 and pr.split_mismatch(x, hi, np.roll(lo, 1)) > 0, c["name"]
        trunc = (np.ascontiguousarray(x, F).view(np.uint32) >> 16).astype(np.uint16)              # truncation instead of round to nearest even
        assert pr.split_mismatch(x, trunc, kr.bf16_bits(x - kr.bf16_value(trunc))) > 0, c["name"]
        assert pr.lo_too_large(hi, hi) > 0, c["name"]
    assert pr.split_mismatch(np.array([1e-40], F), np.array([0], np.uint16), np.array([0], np.uint16)) == 0      # flushed: allowed


# ---- attention ---------------------------------------------------------------------------------------------------------------------------
def _attn_mutant(c, inp, mut):
    """[B * S][H] float64: the reference with one defect (natural units, the float32 launcher's table), or None where it cannot occur."""
    S, hd, B, heads = c["S"], c["hd"], c["B"], c["heads"]
    H = heads * hd
    if (mut in ("last_block_mask", "keys_past_S") and (S % 32 == 0 or S == 1)) or (mut == "block_skipped" and S < 64) or (mut == "bias_flip" and inp["rel"] is None) or \
            (mut == "group8_as_0" and B * heads <= 8):
        return None
    if mut in ("k_lo", "p_lo", "other_scale", "bias_flip", "pv_exchange") and (inp["mask"].sum(axis=1) <= 1).all():
        return None                                      # one visible key: P = 1 whatever the logits are
    out = np.zeros((B * S, H))
    changed = False
    for b in range(B):
        m = inp["mask"][b].copy()
        if mut == "last_block_mask":
            m2 = m.copy(); m2[S // 32 * 32:] = True
            changed |= bool((m2 != m).any()); m = m2
        if mut == "block_skipped":
            m2 = m.copy(); m2[32:64] = False
            changed |= bool((m2 != m).any() and m2.any()); m = m2
        for h in range(heads):
            q, k, v = (a.astype(np.float64) for a in pc.attn_head(c, inp, b, h))
            bias, _ = pc.attn_bias(c, inp, h, "f32", flip=mut == "bias_flip")
            if mut == "k_lo":
                k = kr.bf16_round(k.astype(F)).astype(np.float64)
            if mut == "v_lo":
                v = kr.bf16_round(v.astype(F)).astype(np.float64)
            if mut == "pv_exchange":
                idx = np.arange(S)
                sw = np.where((idx % 16 >= 4) & (idx % 16 < 8), idx + 4, np.where((idx % 16 >= 8) & (idx % 16 < 12), idx - 4, idx))
                v = v[np.minimum(sw, S - 1)]
            scale = 1.0 / math.sqrt(96 - hd if mut == "other_scale" else hd)
            km, kk, vv, bb = m, k, v, bias
            if mut == "keys_past_S":                         # the clamped loads of the last block: key S - 1 once more per slot past S, counted
                extra = 32 - S % 32
                km = np.concatenate([m, np.ones(extra, bool)])
                kk, vv = np.concatenate([k, np.repeat(k[-1:], extra, 0)]), np.concatenate([v, np.repeat(v[-1:], extra, 0)])
                bb = None if bias is None else np.concatenate([bias, np.repeat(bias[:, -1:], extra, 1)], axis=1)
            P = pr.attn_probs(q, kk, np.broadcast_to(km[None, :], (S, km.size)), bb, scale)
            if mut == "p_lo":
                P = kr.bf16_round(P.astype(F)).astype(np.float64)
            out[b * S:(b + 1) * S, h * hd:(h + 1) * hd] = P @ vv
    if mut in ("last_block_mask", "block_skipped") and not changed:
        return None
    if mut == "group8_as_0":
        g = out.reshape(B, S, heads, hd).transpose(0, 2, 1, 3).reshape(B * heads, S, hd).copy()
        g[8:] = g[:B * heads - 8]
        out = g.reshape(B, heads, S, hd).transpose(0, 2, 1, 3).reshape(B * S, H)
    return out


@_cached
def _attn_inp(c):
    return pc.attn_inputs(c)


_ATTN_REF = {}


def _attn_outside(c, vals, launcher):
    inp = _attn_inp(c)
    raw = vals.astype(F) if launcher != "x3_split" else pr.split_rows(vals.astype(F))
    w = kr.Worst()
    bad = pc.attn_check(c, inp, launcher, raw, w, _ATTN_REF)
    return bad > 0 or w.ratio > 1.0


def test_emulated_attention_stays_inside_every_launchers_bound():
    for c in pc.attn_cases():
        inp = _attn_inp(c)
        S, hd, B, heads = c["S"], c["hd"], c["B"], c["heads"]
        for l in pc.ATTN_LAUNCHERS:
            out = np.zeros((B * S, heads * hd), F)
            for b in range(B):
                for h in range(heads):
                    q, k, v = pc.attn_head(c, inp, b, h)
                    out[b * S:(b + 1) * S, h * hd:(h + 1) * hd] = pr.emu_attn(q, k, v, inp["mask"][b], pc.attn_bias(c, inp, h, l)[0], l != "f32")
            assert not _attn_outside(c, out, l), (c["name"], l)
    # a fully masked sequence with anything but zeros in it, and a NaN in a pad row, are violations
    c = [c for c in pc.attn_cases() if c["mask"] == "fullmask"][0]
    inp = _attn_inp(c)
    good = _attn_mutant(c, inp, None)
    assert not _attn_outside(c, good, "f32")
    b = int(np.flatnonzero(~inp["mask"].any(axis=1))[0])
    bad = good.copy(); bad[b * c["S"] + 1, 3] = 1e-30
    assert _attn_outside(c, bad, "f32")
    b2 = int(np.flatnonzero(inp["mask"].any(axis=1) & ~inp["mask"].all(axis=1))[0])
    bad = good.copy(); bad[b2 * c["S"] + int(np.flatnonzero(~inp["mask"][b2])[0]), 0] = np.nan
    assert _attn_outside(c, bad, "f32")


# (defect, the launchers under whose bound it must show): the lo halves exist in the split kernel only
ATTN_MUTANTS = [("block_skipped", pc.ATTN_LAUNCHERS), ("last_block_mask", pc.ATTN_LAUNCHERS), ("keys_past_S", pc.ATTN_LAUNCHERS),
                ("other_scale", pc.ATTN_LAUNCHERS), ("k_lo", ("x3", "x3_split")), ("p_lo", ("x3", "x3_split")), ("v_lo", ("x3", "x3_split")),
                ("pv_exchange", pc.ATTN_LAUNCHERS), ("bias_flip", pc.ATTN_LAUNCHERS), ("group8_as_0", pc.ATTN_LAUNCHERS)]


@pytest.mark.parametrize("mut,launchers", ATTN_MUTANTS)
def test_every_attention_defect_lands_outside_on_every_case_on_which_it_can_occur(mut, launchers):
    rows = []
    for c in pc.attn_cases():
        if mut == "pv_exchange" and c["S"] < 12:
            continue
        vals = _attn_mutant(c, _attn_inp(c), mut)
        if vals is None:
            continue
        rows.append((c["name"], all(_attn_outside(c, vals, l) for l in launchers)))
    assert rows and all(hit for _, hit in rows), (mut, [n for n, hit in rows if not hit])
    print(f"{mut}: caught on all {len(rows)} cases on which it can occur")
