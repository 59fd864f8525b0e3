"""CPU suite for the kernel-level tests' own tools (tests/kernel_refs.py, tests/kernel_cases.py): the float64 references are checked
against independent statements, the emulation of the kernels' rounding scheme must stay inside every derived bound, and every
MUTANT -- a defect of the kind such kernels have, applied to the reference -- must be flagged by the comparator (err / bound > 1
for at least one element) on the very inputs the GPU tests use. That proves inputs and bar can see what they are meant to see.
No GPU, no library call."""
import math

import numpy as np
import pytest

from tests import kernel_cases as kc
from tests import kernel_refs as kr

SMALL = 2048          # the CPU suite works on the GPU cases up to this S (the references are the same code at any S)


def _cases(fn, pred=lambda c: True):
    return [c for c in fn() if c["S"] <= SMALL and pred(c)]


# ---- the tools themselves -----------------------------------------------------------------------------------------------------------
def test_bf16_rounding_is_round_to_nearest_even_and_layout_helpers_invert():
    import torch
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(100000).astype(np.float32) * 10, np.float32([0, -0.0, 1, 1.00390625, 1.01171875, 3.3895314e38])])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(kr.bf16_bits(x), want)
    assert np.array_equal(kr.bf16_round(kr.bf16_round(x)), kr.bf16_round(x))
    pos = kr.vt_pos(np.arange(64))
    assert sorted(pos.tolist()) == list(range(64))
    assert pos[:16].tolist() == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]
    bits = rng.integers(0, 65536, (2, 3, 64, 32)).astype(np.uint16)
    vt = kr.pack_vt(bits)
    assert vt.shape == (2, 96, 64) and vt[1, 2 * 32 + 5, kr.vt_pos(9)] == bits[1, 2, 9, 5]
    assert np.array_equal(kr.unpack_vt(vt), kr.pack_token_major(bits))
    assert kr.pack_token_major(bits)[1, 9, 2 * 32 + 5] == bits[1, 2, 9, 5]


def test_attention_reference_against_an_independent_softmax():
    import torch
    rng = np.random.default_rng(1)
    S, hd = 96, 32
    q, k, v = (rng.standard_normal((S, hd)) for _ in range(3))
    bias = rng.standard_normal((S, S))
    vis = kr.Visibility(kr.mask_right(S, 70), window=9).dense(S)
    out, out_abs = kr.attention_ref(q, k, v, vis, bias, chunk=40)
    s = torch.from_numpy((q @ k.T + bias) * math.log(2.0)).masked_fill(torch.from_numpy(~vis), -math.inf)
    p = torch.softmax(s, dim=1).numpy()
    seen = vis.any(axis=1)                   # (a query without a visible key: zeros here, NaN in torch's softmax)
    assert seen.sum() == 79 and not out[~seen].any()
    p = p[seen]
    assert np.abs(out[seen] - p @ v).max() < 1e-13 and np.abs(out_abs[seen] - p @ np.abs(v)).max() < 1e-13
    # a Visibility object (key range restricted per query chunk) and its dense matrix give the same numbers
    o2, _ = kr.attention_ref(q, k, v, kr.Visibility(kr.mask_right(S, 70), window=9), bias, chunk=40)
    assert np.abs(o2 - out).max() < 1e-13
    oc, _ = kr.attention_ref(q, k, v, kr.Visibility(kr.mask_right(S, 70), causal=True), chunk=40)
    pc = torch.softmax(torch.from_numpy(q @ k.T * math.log(2.0)).masked_fill(torch.from_numpy(~np.tril(np.ones((S, S), bool)) | (np.arange(S) >= 70)[None, :]), -math.inf), dim=1).numpy()
    assert np.abs(oc - pc @ v).max() < 1e-13


def test_the_erf_polynomial_of_the_gemm_epilogue_and_the_slopes_the_bounds_use():
    """gemm.hip's erf polynomial against the exact function, in float64: within 8e-6 on |u| <= 1.9 (most of what a feed-forward
    block produces), 2.7e-5 at worst (|u| >= 3.2, where the clamp holds 0.99997) -- 0.5 |x| times that is the GELU's error, three orders
    below a bf16 rounding of the result. The float32 evaluation stays inside erf_err, the term the bounds carry."""
    u = np.linspace(-6, 6, 2000001)
    err = np.abs(kr.erf_poly(u) - kr.erf64(u))
    assert err.max() <= 2.7e-5 and err[np.abs(u) <= 1.9].max() <= 8.0e-6
    f32 = np.float32
    uc = np.clip(u, -3.2, 3.2).astype(f32)
    t = uc * uc
    p = np.full_like(uc, f32(kr.ERF_POLY[0]))
    for ci in kr.ERF_POLY[1:]:
        p = p * t + f32(ci)
    got = np.clip(p * uc, -1, 1).astype(np.float64)
    assert np.all(np.abs(got - kr.erf64(uc.astype(np.float64))) <= kr.erf_err(uc.astype(np.float64)))
    assert kr.erf_err(u).max() <= 1.3e-3          # (the alternating terms reach 10^3 at the clamp: a worst case, a third of u)
    x = np.linspace(-8, 8, 400001)          # the slopes the bounds use
    g = np.gradient(kr.gelu64(x), x)
    assert np.abs(g).max() <= 1.13
    s = np.gradient(x / (1 + np.exp(-x)), x)
    assert np.abs(s).max() <= 1.1


def test_case_lists_say_what_the_issue_lists():
    w = kc.window_cases()
    assert {c["S"] for c in w} == {32, 64, 96, 128, 160, 512, 544, 2048, 8192} and {c["heads"] for c in w} == {1, 2, 16}
    for S in (544, 2048):
        assert [c["window"] for c in w if c["S"] == S] == [1, 2, 31, 32, 33, 63, 64, 65, 95, 127, 128, 129, 200, S - 1, S, -1]
    assert sorted(c["window"] for c in w if c["S"] == 8192) == [-1, 1, 64, 200]
    assert kc.lengths_for(8192) == [0, 1, 31, 32, 33, 127, 128, 129, 8159, 8191, 8192] and kc.lengths_for(32) == [0, 1, 31, 32]
    assert {c["S"] for c in kc.long_cases()} == {544, 1024, 4128, 8192} and {c["mask"] for c in kc.long_cases()} == {"right", "holes", "left"}
    a = kc.attn_cases()
    assert len(a) == 4 * 3 * 3 * 3 + 3 * 3 * 2 and len({c["name"] for c in a}) == len(a)
    c_ = kc.causal_cases()
    assert len(c_) == 28 and {(c["nq"], c["nkv"]) for c in c_} == {(1, 1), (2, 1), (4, 1), (16, 8), (32, 8), (6, 2)}
    assert sorted(c["S"] for c in c_ if c["nq"] == 6) == [32, 64, 256] and all(sum(d["nq"] == c["nq"] for d in c_) == 5 for c in c_ if c["nq"] != 6)
    g = kc.gemm_cases()
    for c in g:
        assert c["T"] % 256 == 0 and c["N"] % 128 == 0 and c["K"] % 64 == 0
        assert kc.gemm_tile_is_wide(c) == (c["tile"] == "wide"), c["name"]
    assert {(c["mode"], c["tile"]) for c in g} == {(m, t) for m in (0, 1, 2, 4, 7, 8) for t in ("narrow", "wide")}
    assert {c["K"] for c in g} >= {64, 128, 192, 384, 768, 1024, 1152, 2688, 4096}
    assert any(c["mode"] == 8 and c["N"] == 5376 for c in g) and any(c["mode"] == 8 and c["N"] % 256 for c in g)
    assert any(c["mode"] == 0 and c["H"] % 256 for c in g) and all(c["ldo"] < c["T"] for c in g if c["mode"] == 0)


# ---- attention: emulation inside the bound, mutants outside ------------------------------------------------------------------------
def _rows_of_interest(inp):
    """batch rows: the full row, the one that ends 33 short of S (a partial last key block) and a short one."""
    lens = inp["lens"].tolist()
    S = max(lens)
    want = {S, S - 33 if S - 33 > 0 else S - 1, 33 if 33 <= S else 1}
    return [b for b, n in enumerate(lens) if n in want]


def _ref(case, inp, b, h, vis=None, bias="own", scale=1.0, kv_head=None):
    n = int(inp["rowlen"][b])
    qh, kh, vh = kc.head_slices(case, inp, b, h)
    if kv_head is not None:
        kh, vh = kr.bf16_value(inp["k"][b, kv_head]), kr.bf16_value(inp["v"][b, kv_head])
    if isinstance(bias, str):
        bias = kr.rel_bias_dense(inp["rel"][h], case["S"])[:n] if inp["rel"] is not None else None
    vis = kc.visibility(case, inp["mask"][b]) if vis is None else vis
    out, out_abs = kr.attention_ref(qh[:n], kh, vh, vis, bias, scale=scale)
    bmax = float(np.abs(inp["rel"][h]).max()) if inp["rel"] is not None else 0.0
    return out, kr.attention_bound(qh[:n], kh, out, out_abs, bmax), (qh[:n], kh, vh, bias)


ALL_ATTENTION = _cases(kc.window_cases) + _cases(kc.long_cases) + _cases(kc.attn_cases, lambda c: c["S"] in (96, 512) or c["n_rel"] == 512) + \
    _cases(kc.causal_cases)


def test_the_emulated_rounding_scheme_stays_inside_the_derived_bound():
    worst = kr.Worst()
    for case in ALL_ATTENTION:
        inp = kc.attn_inputs(case)
        for b in _rows_of_interest(inp):
            valid = np.flatnonzero(inp["mask"][b])
            n = int(inp["rowlen"][b])
            for h in sorted({0, case["heads"] - 1}):
                out, bound, (qh, kh, vh, bias) = _ref(case, inp, b, h)
                vis = kc.visibility(case, inp["mask"][b]).block(0, n, 0, case["S"])
                emu = kr.attention_emulate(qh, kh, vh, vis, bias)
                worst.add(emu[valid], out[valid], bound[valid], case["name"], b, h, rows=valid)
    print(worst)
    assert worst.ratio <= 1.0, str(worst)
    assert worst.ratio >= 0.1, str(worst)            # ... and the bound is not slack by orders of magnitude


def _flagged(case, inp, b, h, out_mut, out=None, bound=None):
    if out is None:
        out, bound, _ = _ref(case, inp, b, h)
    valid = np.flatnonzero(inp["mask"][b])
    w = kr.Worst()
    return w.add(out_mut[valid], out[valid], bound[valid], case["name"], b, h, rows=valid), w


def _dense(case, inp, b):
    return kc.visibility(case, inp["mask"][b]).block(0, int(inp["rowlen"][b]), 0, case["S"])


def _full_row(inp):
    return int(np.argmax(inp["lens"]))


BANDED = [c for c in _cases(kc.window_cases) if kc.effective_window(c) is not None]


@pytest.mark.parametrize("kind", ["one_too_wide", "one_too_narrow", "one_sided"])
def test_mutant_band_edge(kind):
    n_applied, failed = 0, []
    for case in BANDED:
        inp = kc.attn_inputs(case)
        w = kc.effective_window(case)
        seen = []                                     # per case: the defect must show somewhere in the rows where it can
        for b in _rows_of_interest(inp):
            if inp["lens"][b] < 2:
                continue
            for h in range(case["heads"]):
                vis = _dense(case, inp, b)
                n = vis.shape[0]
                q = np.arange(n)[:, None]
                k = np.arange(case["S"])[None, :]
                if kind == "one_too_wide":
                    mut = inp["mask"][b][None, :] & (np.abs(q - k) <= w + 1)
                elif kind == "one_too_narrow":
                    mut = vis & (np.abs(q - k) <= w - 1)
                else:
                    mut = vis & (k - q != w)
                if np.array_equal(mut[inp["mask"][b][:n]], vis[inp["mask"][b][:n]]):
                    continue                      # the defect cannot show in this row (w + 1 reaches no further key)
                out_mut, _ = kr.attention_ref(*_ref(case, inp, b, h)[2][:3], mut)
                seen.append(_flagged(case, inp, b, h, out_mut)[0])
        if seen:
            if not max(seen) > 1.0:
                failed.append((case["name"], max(seen)))
            n_applied += 1
    assert not failed, (kind, failed)
    assert n_applied >= 0.8 * len(BANDED)          # (one_too_wide cannot show where w + 1 reaches no further key: w = S - 1)


@pytest.mark.parametrize("kind", ["one_block_for_one_wave", "first_walked_block", "last_walked_block", "pad_keys_of_the_last_block"])
def test_mutant_key_block(kind):
    """A 32-key block left out for the 32 queries of a wave (placed on the diagonal: inside any band), the first / the last key block
    a 128-query workgroup walks left out for the whole workgroup, and the mask of the last partial key block ignored."""
    n_applied, failed = 0, []
    for case in _cases(kc.window_cases) + _cases(kc.long_cases) + _cases(kc.attn_cases, lambda c: c["S"] in (96, 512) and c["mask"] == "right"):
        inp = kc.attn_inputs(case)
        w = kc.effective_window(case)
        S = case["S"]
        seen = []
        for b in _rows_of_interest(inp):
            n = int(inp["rowlen"][b])
            if n < 2:
                continue
            vis = _dense(case, inp, b)
            mut = vis.copy()
            wg = (n - 1) // 128 * 128                       # the workgroup of the last valid query
            if kind == "one_block_for_one_wave":
                blk = (n - 1) // 32 // 2
                mut[blk * 32:blk * 32 + 32, blk * 32:blk * 32 + 32] = False
            elif kind == "first_walked_block":
                kb = (max(wg - w, 0) if w is not None else 0) // 32
                mut[wg:wg + 128, kb * 32:kb * 32 + 32] = False
            elif kind == "last_walked_block":
                kb = (n + 31) // 32 - 1 if w is None else min((n + 31) // 32, (wg + 127 + w) // 32 + 1) - 1
                mut[wg:wg + 128, kb * 32:kb * 32 + 32] = False
            else:
                extra = np.zeros(S, bool)
                extra[n:(n + 31) // 32 * 32] = True
                if case["mask"] != "right" or not extra.any():
                    continue
                mut = kr.Visibility(inp["mask"][b] | extra, window=w).block(0, n, 0, S)
            mrow = inp["mask"][b][:n]
            if not (mut[mrow].any(axis=1)).all() or np.array_equal(mut[mrow], vis[mrow]):
                continue                          # (a query left with no key at all is another defect)
            for h in range(case["heads"]):
                out, bound, (qh, kh, vh, bias) = _ref(case, inp, b, h)
                out_mut, _ = kr.attention_ref(qh, kh, vh, mut, bias)
                seen.append(_flagged(case, inp, b, h, out_mut, out, bound)[0])
        if seen:
            if not max(seen) > 1.0:
                failed.append((case["name"], max(seen)))
            n_applied += 1
    assert not failed, (kind, failed)
    assert n_applied >= 20


@pytest.mark.parametrize("kind", ["diagonal_excluded", "one_past_the_diagonal", "gqa_mapping"])
def test_mutant_causal(kind):
    n_applied = 0
    for case in _cases(kc.causal_cases):
        G = case["nq"] // case["nkv"]
        if kind == "gqa_mapping" and (G == 1 or case["nkv"] == 1):
            continue
        inp = kc.attn_inputs(case)
        for b in _rows_of_interest(inp):
            n = int(inp["rowlen"][b])
            if n < 2:
                continue
            for h in range(case["nq"]):
                if kind == "gqa_mapping":
                    if h % case["nkv"] == h // G:
                        continue
                    out_mut = _ref(case, inp, b, h, kv_head=h % case["nkv"])[0]
                else:
                    mut = kr.Visibility(inp["mask"][b], causal=True, diag=-1 if kind == "diagonal_excluded" else 1)
                    out_mut = _ref(case, inp, b, h, vis=mut)[0]
                ratio, wst = _flagged(case, inp, b, h, out_mut)
                assert ratio > 1.0, (kind, str(wst))
                n_applied += 1
    assert n_applied >= 10


@pytest.mark.parametrize("kind", ["bias_at_q_minus_k", "scale_off_by_sqrt2", "sum_not_rescaled_at_one_block_boundary"])
def test_mutant_softmax(kind):
    n_applied = 0
    pick = (lambda c: c["n_rel"] > 0) if kind == "bias_at_q_minus_k" else (lambda c: c["S"] in (96, 512) and c["n_rel"] == 0)
    cases = _cases(kc.attn_cases, pick)
    if kind != "bias_at_q_minus_k":
        cases += _cases(kc.window_cases, lambda c: c["window"] in (64, -1)) + _cases(kc.long_cases) + _cases(kc.causal_cases, lambda c: c["S"] >= 256)
    failed = []
    for case in cases:
        inp = kc.attn_inputs(case)
        seen = []
        for b in _rows_of_interest(inp):
            n = int(inp["rowlen"][b])
            if n < 64:
                continue
            for h in sorted({0, case["heads"] - 1}):
                out, bound, (qh, kh, vh, bias) = _ref(case, inp, b, h)
                if kind == "bias_at_q_minus_k":
                    out_mut = _ref(case, inp, b, h, bias=kr.rel_bias_dense(np.roll(inp["rel"][h][::-1], 1), case["S"])[:n])[0]
                elif kind == "scale_off_by_sqrt2":
                    out_mut = _ref(case, inp, b, h, scale=math.sqrt(2.0))[0]
                else:
                    # l <- l + ps instead of l alpha + ps when the walk enters key block j: the part of the row sum gathered before it
                    # stays 1 / alpha too large, alpha = 2^(max before - max after); the output shrinks by l / l'
                    vis = _dense(case, inp, b)
                    s = np.where(vis, qh.astype(np.float64) @ kh.astype(np.float64).T + (0 if bias is None else bias), -np.inf)
                    run = np.maximum.accumulate(np.where(np.isfinite(s), s, -1e30).reshape(n, -1, 32).max(axis=2), axis=1)
                    j = 32 * (1 + int(np.argmax((run[inp["mask"][b][:n], 1:] > run[inp["mask"][b][:n], :-1] + 1.0).sum(axis=0))))   # the boundary most rows raise their maximum at
                    with np.errstate(invalid="ignore", over="ignore"):
                        m_before, m_after, M = s[:, :j].max(axis=1), s[:, :j + 32].max(axis=1), s.max(axis=1)
                        A = np.exp2(s[:, :j] - M[:, None]).sum(axis=1)
                        l = np.exp2(s - M[:, None]).sum(axis=1)
                        inv_alpha = np.where(np.isfinite(m_before), np.exp2(m_after - m_before), 1.0)
                    out_mut = out * (l / (l + A * (inv_alpha - 1.0)))[:, None]
                seen.append(_flagged(case, inp, b, h, out_mut, out, bound)[0])
        if seen:
            if not max(seen) > 1.0:
                failed.append((case["name"], max(seen)))
            n_applied += 1
    assert not failed, (kind, failed)
    assert n_applied >= 10


# ---- GEMM ------------------------------------------------------------------------------------------------------------------------------
NARROW = [c for c in kc.gemm_cases() if c["tile"] == "narrow"]


def test_emulated_gemm_epilogues_stay_inside_the_derived_bounds():
    """bf16 operands, float32 accumulation (numpy's order), the epilogue in float32, one bf16 rounding where the kernel rounds."""
    worst = kr.Worst()
    for c in NARROW:
        inp = kc.gemm_inputs(c)
        x, w = kr.bf16_value(inp["x"]), kr.bf16_value(inp["w"])
        y, y_abs = kr.gemm_ref(x, w, inp["bias"])
        acc = kr.gemm_emulate(x, w, inp["bias"])
        f32 = np.float32
        if c["mode"] == 0:
            H = c["H"]
            got = {"q": kr.bf16_round(acc[:, :H] * f32(kc.qscale(c))), "k": kr.bf16_round(acc[:, H:2 * H]), "v": kr.bf16_round(acc[:, 2 * H:])}
        elif c["mode"] == 1:
            got = {"out": kr.bf16_round(kr.gelu64(acc).astype(f32))}
        elif c["mode"] == 2:
            got = {"out": acc}
        elif c["mode"] == 4:
            got = {"out": kr.bf16_round(kr.bf16_round(acc) + kr.bf16_value(inp["res"]))}
        elif c["mode"] == 7:
            with np.errstate(over="ignore"):       # exp(+large) = inf: the quotient is the correct 0
                got = {"out": kr.bf16_round(acc[:, 0::2] / (f32(1) + np.exp(-acc[:, 0::2])) * acc[:, 1::2])}
        else:
            got = {"out": kr.bf16_round(kr.gelu64(acc[:, 0::2]).astype(f32) * acc[:, 1::2])}
        for name, (want, bound) in kc.gemm_expect(c, inp, y, y_abs).items():
            worst.add(got[name], want, bound, c["name"] + ":" + name)
    print(worst)
    assert worst.ratio <= 1.0, str(worst)
    assert worst.ratio >= 0.1, str(worst)


@pytest.mark.parametrize("kind", ["k_slice_dropped", "bias_of_the_neighbouring_column", "gate_and_up_swapped", "vt_pos_identity",
                                  "vt_written_past_ldo"])
def test_mutant_gemm(kind):
    n_applied = 0
    for c in NARROW:
        inp = kc.gemm_inputs(c)
        x, w = kr.bf16_value(inp["x"]), kr.bf16_value(inp["w"])
        y, y_abs = kr.gemm_ref(x, w, inp["bias"])
        expect = kc.gemm_expect(c, inp, y, y_abs)
        if kind == "k_slice_dropped":
            ym, _ = kr.gemm_ref(x, w, inp["bias"], drop_k=slice(c["K"] - 32, c["K"]))
            mut = {n: v[0] for n, v in kc.gemm_expect(c, inp, ym, y_abs).items()}
        elif kind == "bias_of_the_neighbouring_column":
            ym = y - inp["bias"].astype(np.float64) + np.roll(inp["bias"].astype(np.float64), 1)
            mut = {n: v[0] for n, v in kc.gemm_expect(c, inp, ym, y_abs).items()}
        elif kind == "gate_and_up_swapped":
            if c["mode"] not in (7, 8):
                continue
            mut = {"out": (kr.epi_swiglu if c["mode"] == 7 else kr.epi_geglu)(y, y_abs, c["K"], swap=True)[0]}
        else:
            if c["mode"] != 0:
                continue
            # the V^T buffer as the test reads it back: [B][H][S] with a sentinel where nothing may be written
            want_vt, bound_vt = kc.vt_expected(c, *expect["v"])
            if kind == "vt_pos_identity":
                mut_vt, _ = kc.vt_expected(c, *expect["v"], pos=np.arange(c["S"]))
            else:
                mut_vt, _ = kc.vt_expected(c, *expect["v"], ldo=c["T"])
            wst = kr.Worst()
            assert wst.add(mut_vt.reshape(-1, c["S"]), want_vt.reshape(-1, c["S"]), bound_vt.reshape(-1, c["S"]), c["name"]) > 1.0, kind
            n_applied += 1
            continue
        wst = kr.Worst()
        for name, (want, bound) in expect.items():
            wst.add(mut[name], want, bound, c["name"] + ":" + name)
        assert wst.ratio > 1.0, (kind, str(wst))
        n_applied += 1
    assert n_applied >= 2


# ---- the LayerNorm-fused kernels -------------------------------------------------------------------------------------------------------
def test_case_lists_of_the_layernorm_kernels_select_what_they_are_meant_to():
    """The launchers' selection rules, restated in tests/kernel_cases.py from launch_gemm_ln, launch_ffn384, launch_qkv384 and
    launch_gemm_lazy: the thresholds the cases sit on are the code's."""
    g = kc.gemm_ln_cases()
    assert {c["K"] for c in g} == {32, 64, 96, 128, 160, 384, 1536} and {c["res"] for c in g} == {"f32", "bf16"}
    assert all(c["T"] % 128 == 0 and c["K"] % 32 == 0 for c in g) and {c["eps"] for c in g} == {1e-12, 1e-5}
    assert kc.gemm_ln_tiles_per_workgroup(dict(T=256 * 128)) == 1 and kc.gemm_ln_tiles_per_workgroup(dict(T=257 * 128)) == 2
    assert sum(kc.gemm_ln_tiles_per_workgroup(c) == 2 for c in g) == 2
    f = kc.ffn384_cases()
    assert {c["kernel"] for c in f} == {"k_ffn384w8<true, 4>", "k_ffn384r", "k_ffn384w8<false, 4>"}
    assert [c["T"] for c in f if c["kernel"] == "k_ffn384r"] == [16512] and 129 * 128 == 16512
    assert kc.ffn384_kernel(dict(T=128 * 128, ctx=True)) == "k_ffn384w8<true, 4>"          # one tile fewer: still half tiles
    assert {c["kernel"] for c in kc.ffn384_cases("nwv8")} == {"k_ffn384r"} and {c["kernel"] for c in kc.ffn384_cases("w4")} == {"k_ffn384"}
    assert all(c["I"] % 32 == 0 and c["I"] // 32 >= 2 and c["I"] <= 1536 and c["T"] % 128 == 0 for c in f)
    q = kc.qkv384_cases()
    assert kc.qkv384_tg(258 * 128) == 2 and kc.qkv384_tg(256 * 128) == 1 and kc.qkv384_tg(257 * 128) == 1 and 258 * 128 == 33024
    assert {c["tg"] for c in q if c["T"] == 33024} == {2} and {c["tg"] for c in q if c["T"] != 33024} == {1}
    assert {c["S"] for c in q} == {32, 128, 512} and {c["head_major"] for c in q} == {0, 1} and any(c["Treal"] < c["T"] for c in q)
    assert all(c["T"] % c["S"] == 0 and c["T"] % 128 == 0 and c["Treal"] % 32 == 0 for c in q + kc.qkv384_cases(True))
    assert all(c["T"] == 256 and c["tg"] == 2 for c in kc.qkv384_cases(True))
    lz = kc.lazy_cases()
    assert all(kc.lazy_tile_selected(c, True) and not kc.lazy_tile_selected(c, False) for c in lz)
    own, = kc.lazy_cases(False)
    assert own["T"] == 11008 and kc.lazy_tile_selected(own, False) and not kc.lazy_tile_selected(dict(own, T=42 * 256), False)
    assert {(c["mode"], c["N"], c["K"]) for c in lz} == {(0, 2304, 768), (0, 768, 256), (1, 3072, 768), (1, 1024, 256), (4, 768, 768), (4, 768, 3072), (4, 256, 192)}
    assert {(c["nslot"], c["T"]) for c in kc.ln_finalize_cases()} == {(n, T) for n in (2, 3, 6, 8) for T in (1, 255, 256, 11008)}
    ln = kc.layernorm_cases()
    assert {(c["H"], c["T"]) for c in ln} == {(H, T) for H in (384, 768, 1024) for T in (1, 5, 127, 512)} and len({c["name"] for c in ln}) == len(ln)
    rows = kc.compare_rows(16512, 128, 1)
    assert {0, 127, 126 * 128, 127 * 128, 128 * 128 - 1, 128 * 128, 16511}.issubset(rows.tolist()) and len(rows) % 128 == 0 and len(rows) < 2500


def test_inputs_of_the_layernorm_kernels_hold_every_row_class():
    c = next(c for c in kc.gemm_ln_cases() if c["K"] == 384 and c["T"] == 384 and c["res"] == "f32")
    inp = kc.gemm_ln_inputs(c)
    parts = kr.gemm_ln_ref(kr.bf16_value(inp["x"]), kr.bf16_value(inp["w"]), inp["bias"], inp["res"], inp["gamma"], inp["beta"], c["eps"])[3]
    cls = kc.ratio_class(parts.ratio)
    assert min(np.bincount(cls)) >= 100 and 3 <= np.median(parts.ratio[cls == 1]) <= 5 and 25 <= np.median(parts.ratio[cls == 2]) <= 40
    assert parts.var[kc.flat_row(c["T"]), 0] < 0.01 * c["eps"]                     # eps-dominated
    g = inp["gamma"]
    assert (g == 0).sum() == 3 and (g < 0).sum() >= 3 and abs(float(g.mean()) - 1.0) < 0.1 and np.abs(inp["beta"]).min() > 0


def _gemm_ln_small():
    return [c for c in kc.gemm_ln_cases() if c["T"] <= 384 and c["K"] in (32, 96, 384, 1536)]


def _gemm_ln_want(c, inp):
    return kr.gemm_ln_ref(kr.bf16_value(inp["x"]), kr.bf16_value(inp["w"]), inp["bias"], inp["res"], inp["gamma"], inp["beta"], c["eps"])


def test_emulated_gemm_ln_stays_inside_the_derived_bound():
    worst = kr.Worst()
    for c in _gemm_ln_small():
        inp = kc.gemm_ln_inputs(c)
        out, b32, b16, _ = _gemm_ln_want(c, inp)
        acc = np.asarray(kr.bf16_value(inp["x"]), np.float32) @ np.asarray(kr.bf16_value(inp["w"]), np.float32).T
        y = kr.layernorm_emulate(acc + (inp["bias"] + inp["res"].astype(np.float32)), inp["gamma"], inp["beta"], c["eps"])
        if c["res"] == "f32":
            worst.add(y, out, b32, c["name"] + ":x32")
        worst.add(kr.bf16_round(y), out, b16, c["name"] + ":x16")
    print(worst)
    assert 0.05 <= worst.ratio <= 1.0, str(worst)


LN_MUTANTS = ["eps_dropped", "eps_outside_the_root", "variance_over_h_minus_1", "slice_missing_from_statistics", "statistics_of_the_neighbour",
              "beta_dropped", "residual_not_added", "residual_added_after_the_layernorm"]


def _ln_mutant(kind, r_of, res, gamma, beta, eps):
    """The mutant's output: r_of(res) is the pre-norm row for a given residual."""
    r = r_of(res)
    if kind == "eps_dropped":
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.nan_to_num(kr.layernorm_ref(r, gamma, beta, eps, eps_mode="dropped")[0], nan=1e30, posinf=1e30, neginf=-1e30)
    if kind == "eps_outside_the_root":
        return kr.layernorm_ref(r, gamma, beta, eps, eps_mode="outside")[0]
    if kind == "variance_over_h_minus_1":
        return kr.layernorm_ref(r, gamma, beta, eps, ddof=1)[0]
    if kind == "slice_missing_from_statistics":
        cols = np.ones(r.shape[1])
        cols[128:256] = 0.0
        return kr.layernorm_ref(r, gamma, beta, eps, stat_cols=cols)[0]
    if kind == "statistics_of_the_neighbour":
        return kr.layernorm_ref(r, gamma, beta, eps, stat_shift=1)[0]
    if kind == "beta_dropped":
        return kr.layernorm_ref(r, gamma, np.zeros_like(beta), eps)[0]
    if kind == "residual_not_added":
        return kr.layernorm_ref(r_of(0.0), gamma, beta, eps)[0]
    return kr.layernorm_ref(r_of(0.0), gamma, beta, eps)[0] + res


@pytest.mark.parametrize("kind", LN_MUTANTS)
def test_mutant_gemm_ln(kind):
    """Every defect lands outside on every case, the two that only a row of near-zero variance can show (eps) on the cases whose
    flat row is eps-dominated: every float32-residual case and the bf16 ones at eps = 1e-5."""
    n_applied = 0
    for c in _gemm_ln_small():
        if kind.startswith("eps") and c["res"] == "bf16" and c["eps"] < 1e-6:
            continue
        inp = kc.gemm_ln_inputs(c)
        out, b32, b16, parts = _gemm_ln_want(c, inp)
        y = kr.gemm_ref(kr.bf16_value(inp["x"]), kr.bf16_value(inp["w"]), inp["bias"])[0]
        mut = _ln_mutant(kind, lambda res: y + res, inp["res"].astype(np.float64), inp["gamma"], inp["beta"], c["eps"])
        bound = b32 if c["res"] == "f32" else b16          # the float32 output where there is one
        wst = kr.Worst()
        wst.add(mut, out, bound, c["name"])
        assert wst.ratio > 1.0, (kind, str(wst))
        if not kind.startswith("eps"):          # ... and on the well-centred rows alone: no mutant hides behind the loose rows
            centred = kc.ratio_class(parts.ratio) == 0
            assert kr.Worst().add(mut[centred], out[centred], bound[centred], c["name"]) > 1.0, (kind, c["name"])
        n_applied += 1
    assert n_applied >= 8


def test_emulated_stand_alone_layernorms_stay_inside_and_their_mutants_fall_outside():
    worst = kr.Worst()
    flagged = {k: 0 for k in LN_MUTANTS[:6]}
    for c in kc.layernorm_cases():
        if c["T"] not in (5, 127):
            continue
        inp = kc.layernorm_inputs(c)
        out, b32, b16, parts = kc.layernorm_expect(c, inp)
        f = np.float32
        if c["xin"] == "lazy":
            st = kr.stats_f32(parts)
            y = st[:, 1:2] * (kr.bf16_value(kr.lazy_rows(inp["x"], inp["gamma"])) - st[:, 0:1] * inp["gamma"]) + inp["beta"]
        else:
            y = kr.layernorm_emulate(inp["x"].astype(f) + (0 if inp["res"] is None else inp["res"].astype(f)), inp["gamma"], inp["beta"], c["eps"])
        worst.add(kr.bf16_round(y), out, b16, c["name"])
        if c["T"] == 127 and c["xin"] != "lazy":
            r = kc.ln_rows(c, inp)[0]
            for kind in flagged:
                mut = _ln_mutant(kind, lambda res: r, 0.0, inp["gamma"], inp["beta"], c["eps"])
                ratio = kr.Worst().add(mut, out, b16, c["name"])
                assert ratio > 1.0, (kind, c["name"], ratio)
                flagged[kind] += 1
    print(worst)
    assert 0.05 <= worst.ratio <= 1.0 and min(flagged.values()) >= 6, (str(worst), flagged)


# ---- the fused layer ---------------------------------------------------------------------------------------------------------------------
def _ffn_small():
    return [c for c in kc.ffn384_cases() + kc.ffn384_cases("nwv8") if c["T"] == 128 or not c["ctx"]]


def test_emulated_fused_layer_stays_inside_the_derived_bound():
    worst = kr.Worst()
    for c in _ffn_small():
        inp = kc.ffn384_inputs(c)
        out, bound, _ = kr.ffn_layer_ref(inp["x"], inp["ctx"], inp["p"], c["eps"], kc.ffn384_table_gelu(c))
        worst.add(kr.ffn_layer_emulate(inp["x"], inp["ctx"], inp["p"], c["eps"], kc.ffn384_table_gelu(c)), out, bound, c["name"])
    print(worst)
    assert 0.02 <= worst.ratio <= 1.0, str(worst)


@pytest.mark.parametrize("kind", ["gamma1_beta1_for_ln2", "bo_missing", "b2_missing", "w2_k_chunks_swapped", "residual1_not_added",
                                  "residual2_not_added", "residual2_added_after_ln"])
def test_mutant_fused_layer(kind):
    """On the rows of |mean| / std < 2 after LayerNorm-2 alone: the bound of the offset rows is looser, and no mutant may need them."""
    n_applied = 0
    for c in _ffn_small():
        if not c["ctx"] and kind in ("bo_missing", "residual1_not_added"):
            continue
        if kind == "w2_k_chunks_swapped" and c["I"] < 96:
            continue
        inp = kc.ffn384_inputs(c)
        out, bound, parts = kr.ffn_layer_ref(inp["x"], inp["ctx"], inp["p"], c["eps"], kc.ffn384_table_gelu(c))
        mut = kr.ffn_layer_ref(inp["x"], inp["ctx"], inp["p"], c["eps"], kc.ffn384_table_gelu(c), mut=kind)[0]
        centred = kc.ratio_class(parts.ratio) == 0
        assert centred.sum() >= 32
        ratio = kr.Worst().add(mut[centred], out[centred], bound[centred], c["name"])
        assert ratio > 1.0, (kind, c["name"], ratio)
        n_applied += 1
    assert n_applied >= 3


def test_tanh_gelu_is_flagged_at_the_gelu_stage_and_is_below_the_resolution_of_the_fused_output():
    """tanh-GELU for erf-GELU moves a value by 5e-4 at most. Behind W2 (1536 terms of either sign) and LayerNorm-2 that is 6e-5 at the
    median of the fused layer's output, against a bf16 step of 3e-3 there: err / bound 0.03 at worst over these cases (0.005 at
    I = 64), and no bound on a bf16 output can make it visible. It is visible where the GELU's own output is: against the bound the
    fused reference carries for gelu(h) (the polynomial term and one bf16 rounding), which is what launch_gemm's MODE 1 is held to on the
    GPU with the same polynomial. Both halves are asserted, so that the statement stays true."""
    c = next(c for c in kc.ffn384_cases() if not c["ctx"])
    inp = kc.ffn384_inputs(c)
    p = inp["p"]
    h, h_abs = kr.gemm_ref(inp["x"], p["w1"], p["b1"])
    want, bound = kr.epi_gelu(h, h_abs, kc.LN_H, table=False)
    assert kr.Worst().add(kr.gelu_tanh64(h), want, bound, c["name"]) > 1.0
    out, bound, _ = kr.ffn_layer_ref(inp["x"], None, p, c["eps"], False)
    mut = kr.ffn_layer_ref(inp["x"], None, p, c["eps"], False, mut="tanh_gelu")[0]
    ratio = kr.Worst().add(mut, out, bound, c["name"])
    print(f"tanh-GELU at the fused output: err / bound {ratio:.3f}, median |err| {np.median(np.abs(mut - out)):.2e}, median bf16 step {np.median(kr.U * np.abs(out)):.2e}")
    assert ratio < 1.0 and np.median(np.abs(mut - out)) < 0.1 * np.median(kr.U * np.abs(out))


# ---- qkv384 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["qscale_applied_to_k", "vt_slot_written_past_the_real_tokens", "head_major_row_written_past_the_real_tokens"])
def test_mutant_qkv384(kind):
    n_applied = 0
    for c in kc.qkv384_cases():
        if c["T"] > 384 or (kind != "qscale_applied_to_k" and c["Treal"] == c["T"]) or (kind.startswith("head") and not c["head_major"]):
            continue
        inp = kc.gemm_inputs(c)
        y, y_abs = kr.gemm_ref(kr.bf16_value(inp["x"]), kr.bf16_value(inp["w"]), inp["bias"])
        q, k, v = kr.qkv_split(y, y_abs, c["K"], c["H"], kc.qscale32())
        want = kc.qkv384_layout(c, q, k, v)
        if kind == "qscale_applied_to_k":
            mut = kc.qkv384_layout(c, q, (k[0] * kc.qscale32(), k[1]), v)
        else:
            mut = kc.qkv384_layout(dict(c, Treal=c["T"]), q, k, v)
        name = {"q": "k", "v": "vt", "h": "q"}[kind[0]]
        assert kr.Worst().add(mut[name][0], *want[name], c["name"]) > 1.0, (kind, c["name"])
        n_applied += 1
    assert n_applied >= 2


# ---- the lazy modes ----------------------------------------------------------------------------------------------------------------------
def _lazy_small():
    return [c for c in kc.lazy_cases() if c["K"] <= 768]


def test_emulated_lazy_modes_stay_inside_the_derived_bounds():
    """bf16 r~, float32 statistics, float32 fold_c / b', rstd (acc - mu c) + b'; MODE 4 with one-pass float32 sums of the row."""
    worst = kr.Worst()
    f = np.float32
    for c in _lazy_small():
        inp = kc.lazy_inputs(c)
        exp, _ = kc.lazy_expect(c, inp)
        if c["mode"] != 4:
            y = kr.lazy_a_emulate(inp["r"], inp["gamma"], inp["beta"], c["eps"], inp["w"], inp["bias"])
            if c["mode"] == 1:
                got = {"out": kr.bf16_round(kr.gelu64(y).astype(f))}
            else:
                H = c["H"]
                got = {"q": kr.bf16_round(y[:, :H] * f(kc.qscale(c))), "k": kr.bf16_round(y[:, H:2 * H]), "v": kr.bf16_round(y[:, 2 * H:])}
        else:
            acc = kr.gemm_emulate(inp["x"], inp["w"], inp["bias"])
            if c["res_stats"]:
                parts = kr.layernorm_ref(inp["r_prev"], inp["gamma"], inp["beta"], c["eps"])[1]
                st = kr.stats_f32(parts)
                res = st[:, 1:2] * (kr.bf16_value(kr.lazy_rows(inp["r_prev"], inp["gamma"])) - st[:, 0:1] * inp["gamma"]) + inp["beta"]
            else:
                res = inp["res_rows"]
            r = (acc + res).astype(f)
            rr = r.reshape(r.shape[0], -1, 128)
            sums = np.stack([rr.sum(axis=2, dtype=f), (rr * rr).sum(axis=2, dtype=f)], axis=2).transpose(1, 0, 2)
            got = {"out": kr.bf16_round(r * inp["out_g"]), "stats": sums.reshape(-1, 2)}
        for name, (want, bound) in exp.items():
            worst.add(got[name], want, bound, c["name"] + ":" + name)
    print(worst)
    assert 0.05 <= worst.ratio <= 1.0, str(worst)


@pytest.mark.parametrize("kind", ["mu_fold_c_dropped", "res_b_dropped", "out_g_of_the_wrong_layernorm"])
def test_mutant_lazy_modes(kind):
    """Flagged on the rows of |mean| / std < 2 alone (mu_fold_c_dropped: on every class -- without an offset mu is small, and so
    is the term; the class-4 rows must show it)."""
    n_applied = 0
    for c in _lazy_small():
        inp = kc.lazy_inputs(c)
        if (kind == "mu_fold_c_dropped") != (c["mode"] != 4) or (kind == "res_b_dropped" and not c["res_stats"]):
            continue
        exp, parts = kc.lazy_expect(c, inp)
        if c["mode"] != 4:
            y, dy = kr.lazy_a_ref(inp["r"], inp["gamma"], inp["beta"], c["eps"], inp["w"], inp["bias"], mut=kind)[:2]
            mut = {n: v[0] for n, v in kc.lazy_epilogue(c, y, dy).items()}
            rows = kc.ratio_class(parts.ratio) == 1
        else:
            prev = (inp["r_prev"], inp["gamma"], inp["beta"], c["eps"]) if c["res_stats"] else None
            og = inp["gamma"] if kind.startswith("out_g") else inp["out_g"]          # (the gamma of the residual's LayerNorm for the output's)
            mut = {"out": kr.lazy_mode4_ref(inp["x"], inp["w"], inp["bias"], og, res_rows=inp["res_rows"], prev=prev, mut=kind)[2]}
            rows = kc.ratio_class(parts.ratio) == 0
        name = "out" if "out" in mut else "k"
        assert rows.sum() >= 16
        assert kr.Worst().add(mut[name][rows], exp[name][0][rows], exp[name][1][rows], c["name"]) > 1.0, (kind, c["name"])
        n_applied += 1
    assert n_applied >= 2


def test_ln_finalize_and_fold_ln_references_and_their_mutants():
    """The one-pass float32 evaluation of k_ln_finalize stays inside its bound on every row class; the mutants (eps dropped or
    outside the root, H - 1, a slice missing) fall outside. fold_ln: float32 sums inside, beta's sum left out of b' outside."""
    f = np.float32
    worst = kr.Worst()
    for c in kc.ln_finalize_cases():
        if c["T"] > 256:
            continue
        part = kc.ln_finalize_inputs(c)
        n = 128 * c["nslot"]
        want, bound = kr.ln_finalize_ref(part, 1.0 / n, c["eps"])
        s = part.sum(axis=0, dtype=f)
        mu = s[:, 0] * f(1.0 / n)
        var = np.maximum(s[:, 1] * f(1.0 / n) - mu * mu, f(0))
        worst.add(np.stack([mu, f(1) / np.sqrt(var + f(c["eps"]))], axis=1), want, bound, c["name"])
        if c["T"] < 255:
            continue
        p8 = part.astype(np.float64)
        s1, s2 = p8[:, :, 0].sum(axis=0), p8[:, :, 1].sum(axis=0)
        v = np.maximum(s2 / n - (s1 / n) ** 2, 0.0)
        with np.errstate(divide="ignore"):
            muts = {"eps_dropped": np.minimum(1.0 / np.sqrt(v), 1e30), "eps_outside": 1.0 / (np.sqrt(v) + c["eps"]), "h_minus_1": 1.0 / np.sqrt(v * n / (n - 1) + c["eps"]),
                    "slice_missing": 1.0 / np.sqrt(np.maximum((s2 - p8[1, :, 1]) / n - ((s1 - p8[1, :, 0]) / n) ** 2, 0.0) + c["eps"])}
        for kind, rstd in muts.items():
            assert kr.Worst().add(np.stack([want[:, 0], rstd], axis=1), want, bound, c["name"]) > 1.0, (kind, c["name"])
    print(worst)
    assert 0.01 <= worst.ratio <= 1.0, str(worst)
    wf = kr.Worst()
    for c in kc.fold_ln_cases():
        inp = kc.fold_ln_inputs(c)
        cc, bf, dc, db = kr.fold_ln_ref(inp["w"], inp["gamma"], inp["beta"], inp["bias"])
        wf.add((inp["w"] @ inp["gamma"])[None, :], cc[None, :], dc[None, :], c["name"] + ":c")
        wf.add((inp["bias"] + inp["w"] @ inp["beta"])[None, :], bf[None, :], db[None, :], c["name"] + ":bf")
        assert kr.Worst().add(inp["bias"].astype(np.float64)[None, :], bf[None, :], db[None, :], c["name"]) > 1.0
        assert kr.Worst().add(cc[None, ::-1], cc[None, :], dc[None, :], c["name"]) > 1.0
    print(wf)
    assert wf.ratio <= 1.0, str(wf)
