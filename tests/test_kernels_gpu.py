"""GPU suite, kernel by kernel: every attention launcher and the GEMM launchers of the encoder side run ONE launch at a time on chosen
inputs (tests/kernel_cases.py) and are compared, element by element, with a float64 statement of the operation at a bar derived from
the number formats (tests/kernel_refs.py: the derivation is its docstring). The model-level suites compare one pooled vector per
row; here every valid query row of every head and every output element of a GEMM is held, and rows past a sequence's length must be
finite.

The launches go through the ak_kt_* wrappers of csrc/kernel_test.hip, which exist in libarchi_hip_dbg.so only and add nothing to
the launchers the forward pass calls; the last test holds that library's forward passes to the product library's bit for bit. The
kernels run in child processes (tests/kernel_worker.py, ARCHI_HIP_DBG=1; at most 3 at a time, each case once, nothing is run again
after a failure); the references are computed here. What tests/test_kernel_refs_cpu.py proves without a GPU: the emulated rounding
scheme stays inside every bound, and every listed defect, applied to the reference, lands outside on these very inputs.

The kernels that carry a LayerNorm -- gemm_ln, the fused hidden-384 layer (ffn384), qkv384, the lazy-LayerNorm modes of launch_gemm_lazy
with ln_finalize and fold_ln, and the stand-alone LayerNorm launches -- run the same way, in three children shared by their tests:
the launchers' own selection at their own thresholds (16 512, 33 024 and 11 008 tokens, 257 tiles) and the forcing switches.

Each test prints the worst err / bound of its kernel and where it occurred; a kernel passes at <= 1."""
import concurrent.futures
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import kernel_cases as kc
from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PAR = 3
_POOL = concurrent.futures.ThreadPoolExecutor(max_workers=PAR)
_DEAD = []                   # a child that ended badly: nothing more is started on the GPU from this file


def _child(tmp_path, group, tag="", extra=None, dbg=True):
    out = str(tmp_path / f"{group}{tag}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AK_") and k != "ARCHI_HIP_DBG"}
    if dbg:
        env["ARCHI_HIP_DBG"] = "1"
    env.update(extra or {})
    t0 = time.time()
    assert not _DEAD, f"not started: child {_DEAD[0]} ended badly before"
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "kernel_worker.py"), group, out], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=900)
    except subprocess.TimeoutExpired:
        _DEAD.append(group + tag)
        raise
    if p.returncode != 0:
        _DEAD.append(group + tag)
    assert p.returncode == 0, f"{group}{tag}: exit {p.returncode}\n" + p.stderr.decode("utf-8", "replace")[-3000:]
    print(f"child {group}{tag}: {time.time() - t0:.0f} s")
    res = np.load(out)
    assert int(res["dbg"]) == int(dbg)
    return res


def _attention(tmp_path, group, cases):
    res = _child(tmp_path, group)
    worst = kr.Worst()
    for case in cases:
        kc.check_attention(case, kc.attn_inputs(case), res[case["name"]], worst)
    print(f"{group}: {worst}")
    assert worst.n > 0 and worst.ratio <= 1.0, str(worst)
    return worst


def test_launch_attn_window(tmp_path):
    """k_attn_long<true> at 16 half-windows around one, two, three and four 32-key blocks, k_attn_long<false> where the launcher drops
    the band (window < 0 or >= S), 32 <= S <= 8192, every length class in every batch."""
    _attention(tmp_path, "window", kc.window_cases())


def test_launch_attn_long(tmp_path):
    """k_attn_long<false> through the encoder's own launcher (512 < S <= 8192): right-padded, holed and left-padded masks."""
    _attention(tmp_path, "long", kc.long_cases())


def test_launch_attn_causal(tmp_path):
    """k_attn_causal at G = 1, 2, 3, 4 and every row length: the decoder reads one row of it, here every row is checked."""
    _attention(tmp_path, "causal", kc.causal_cases())


def test_launch_attn_default_selection_and_alternates(tmp_path):
    """launch_attn (S <= 512): the selection the product makes (k_attn_s at head size 64, k_attn_d at 32), the unstreamed k_attn (no
    prepared mask), and the A/B alternates AK_ATTN_STREAM = 0 / 1 / 2, each in a child of its own (the switch is read once per
    process): same cases, same references, same bar."""
    runs = {"default": _POOL.submit(_child, tmp_path, "attn")}
    for v in ("0", "1", "2"):
        runs["AK_ATTN_STREAM=" + v] = _POOL.submit(_child, tmp_path, "attn", "_stream" + v, {"AK_ATTN_STREAM": v})
    runs = {k: f.result() for k, f in runs.items()}
    worst = {k: kr.Worst() for k in list(runs) + ["unstreamed"]}
    for case in kc.attn_cases():
        inp, ref = kc.attn_inputs(case), {}
        for name, res in runs.items():
            kc.check_attention(case, inp, res[case["name"]], worst[name], ref)
        kc.check_attention(case, inp, runs["default"][case["name"] + "|unstreamed"], worst["unstreamed"], ref)
    for name, w in worst.items():
        print(f"attn {name}: {w}")
    for name, w in worst.items():
        assert w.n > 0 and w.ratio <= 1.0, (name, str(w))


def _check_qkv(c, res, y, y_abs, worst):
    """q, k: every row of the padded T; V^T: vt_pos order, and the sentinel untouched in the slots of tokens past the real ones."""
    e = kc.gemm_expect(dict(c, mode=0), None, y, y_abs)
    (q, qb), (k, kb), (v, vb) = e["q"], e["k"], e["v"]
    worst.add(kr.bf16_value(res[c["name"] + ":q"]), q, qb, c["name"] + ":q")
    worst.add(kr.bf16_value(res[c["name"] + ":k"]), k, kb, c["name"] + ":k")
    c = dict(c, ldo=c.get("ldo", c.get("Treal")))
    want, bound = kc.vt_expected(c, v, vb)
    worst.add(kr.bf16_value(res[c["name"] + ":vt"]).reshape(-1, c["S"]), want.reshape(-1, c["S"]), bound.reshape(-1, c["S"]), c["name"] + ":vt")


def test_launch_gemm_every_epilogue_on_both_tiles(tmp_path):
    """MODE 0 (QKV split, all three outputs), 1 (GELU: polynomial on the narrow tile, table on the wide one), 2 (float32), 4 (bf16
    residual), 7 (SwiGLU), 8 (GeGLU); the tile is the launcher's own choice by shape."""
    res = _child(tmp_path, "gemm")
    worst = {}
    for c in kc.gemm_cases():
        inp = kc.gemm_inputs(c)
        y, y_abs = kr.gemm_ref(kr.bf16_value(inp["x"]), kr.bf16_value(inp["w"]), inp["bias"])
        w = worst.setdefault((c["mode"], c["tile"]), kr.Worst())
        if c["mode"] == 0:
            _check_qkv(c, res, y, y_abs, w)
        else:
            want, bound = kc.gemm_expect(c, inp, y, y_abs)["out"]
            got = res[c["name"] + ":out"]
            w.add(got if got.dtype == np.float32 else kr.bf16_value(got), want, bound, c["name"])
    for key, w in sorted(worst.items()):
        print(f"gemm MODE {key[0]} {key[1]}: {w}")
    for key, w in worst.items():
        assert w.n > 0 and w.ratio <= 1.0, (key, str(w))


def test_gemm_skinny_both_k_branches_and_the_qkv_form(tmp_path):
    res = _child(tmp_path, "skinny")
    worst = kr.Worst()
    for c in kc.skinny_cases():
        inp = kc.gemm_inputs(c)
        y, y_abs = kr.gemm_ref(kr.bf16_value(inp["x"]), kr.bf16_value(inp["w"]), inp["bias"])
        if c["kind"] == "qkv":
            _check_qkv(c, res, y, y_abs, worst)
        elif c["kind"] == "f32":
            worst.add(res[c["name"] + ":out"], *kr.epi_f32(y, y_abs, c["K"]), c["name"])
        else:
            worst.add(kr.bf16_value(res[c["name"] + ":out"]), *kr.epi_gelu_erff(y, y_abs, c["K"]), c["name"])
    print(f"gemm_skinny: {worst}")
    assert worst.n > 0 and worst.ratio <= 1.0, str(worst)


# ---- the kernels that carry a LayerNorm -----------------------------------------------------------------------------------------------
FORCED = {"AK_FFN_NWV": "8", "AK_QKV_TG": "2", "AK_ENC_LAZYLN": "2"}


@pytest.fixture(scope="module")
def ln_children(tmp_path_factory):
    """Three children, each started once: every family by the launchers' own selection, the forcing child (role kernel on small
    batches, 32 tokens per wave in qkv384, the lazy tile at 256 tokens) and the 4-wave generation of the feed-forward kernel."""
    tmp = tmp_path_factory.mktemp("lnfused")
    runs = {"default": _POOL.submit(_child, tmp, "lnfused"), "forced": _POOL.submit(_child, tmp, "lnfused_forced", "", FORCED),
            "w4": _POOL.submit(_child, tmp, "lnfused_w4", "", {"AK_FFN_W8": "0"})}
    return {k: f.result() for k, f in runs.items()}


def _report(worst):
    for key, w in sorted(worst.items()):
        print(f"{key}: {w}")
    for key, w in worst.items():
        assert w.n > 0 and w.ratio <= 1.0, (key, str(w))


def test_launch_gemm_ln(ln_children):
    """k_gemm_ln<RES16> at 1 to 5, 12 and 48 K-steps of its 4-slot ring, one and three tiles and 257 (a second tile per workgroup),
    float32 residual stream (both outputs) and bf16: every row, every element."""
    res = ln_children["default"]
    worst = {}
    for c in kc.gemm_ln_cases():
        inp = kc.gemm_ln_inputs(c)
        out, b32, b16, _ = kr.gemm_ln_ref(kr.bf16_value(inp["x"]), kr.bf16_value(inp["w"]), inp["bias"], inp["res"], inp["gamma"], inp["beta"], c["eps"])
        w = worst.setdefault(f"gemm_ln {c['res']} K/32 {'<= 5' if c['K'] <= 160 else '> 5'}" + (" 257 tiles" if c["T"] > 384 else ""), kr.Worst())
        w.add(kr.bf16_value(res[c["name"] + ":x16"]), out, b16, c["name"] + ":x16")
        if c["res"] == "f32":
            w.add(res[c["name"] + ":x32"], out, b32, c["name"] + ":x32")
    _report(worst)


def test_launch_layernorms_ln_finalize_and_fold_ln(ln_children):
    """k_layernorm in the three combinations the forward pass uses, k_layernorm16, k_ln_apply16 (against LN of the unrounded rows),
    k_ln_finalize and k_fold_ln against float64."""
    res = ln_children["default"]
    worst = {}
    for c in kc.layernorm_cases():
        inp = kc.layernorm_inputs(c)
        out, b32, b16, _ = kc.layernorm_expect(c, inp)
        w = worst.setdefault(f"{c['kernel']} {c['xin']}/{c['res']}", kr.Worst())
        w.add(kr.bf16_value(res[c["name"] + ":y16"]), out, b16, c["name"] + ":y16")
        if c["y32"]:
            w.add(res[c["name"] + ":y32"], out, b32, c["name"] + ":y32")
    for c in kc.ln_finalize_cases():
        want, bound = kr.ln_finalize_ref(kc.ln_finalize_inputs(c), 1.0 / (128 * c["nslot"]), c["eps"])
        worst.setdefault("ln_finalize", kr.Worst()).add(res[c["name"]], want, bound, c["name"])
    for c in kc.fold_ln_cases():
        inp = kc.fold_ln_inputs(c)
        cc, bf, dc, db = kr.fold_ln_ref(inp["w"], inp["gamma"], inp["beta"], inp["bias"])
        w = worst.setdefault("fold_ln", kr.Worst())
        w.add(res[c["name"] + ":c"][None, :], cc[None, :], dc[None, :], c["name"] + ":c")
        w.add(res[c["name"] + ":bf"][None, :], bf[None, :], db[None, :], c["name"] + ":bf")
    _report(worst)


def test_launch_qkv384(ln_children):
    """k_qkv384<1> and, from 33 024 padded tokens on and in the forcing child, <2>: q (scaled), k in both layouts, V^T in vt_pos order;
    rows past the real tokens keep the sentinel in V^T and in head-major q / k. Every element of every buffer."""
    worst = {}
    for forced, res in ((False, ln_children["default"]), (True, ln_children["forced"])):
        for c in kc.qkv384_cases(forced):
            exp = kc.qkv384_expect(c, kc.gemm_inputs(c))
            w = worst.setdefault(f"qkv384<{c['tg']}> {'forced' if forced else 'own choice'} {'head' if c['head_major'] else 'token'}-major", kr.Worst())
            for name in ("q", "k", "vt"):
                want, bound = exp[name]
                w.add(kr.bf16_value(res[c["name"] + ":" + name]).reshape(want.shape), want, bound, c["name"] + ":" + name)
    _report(worst)


def test_launch_ffn384(ln_children):
    """The fused layer kernels: k_ffn384w8<true, 4> (half tiles) and, from 16 512 tokens on and in the forcing child, the role kernel
    k_ffn384r; the ctx-less form and the 4-wave generation. At T <= 1024 every row; at 16 512 the tiles kernel_cases.compare_rows
    lists, every other row finite."""
    worst = {}
    for child in ("default", "nwv8", "w4"):
        res = ln_children["forced" if child == "nwv8" else "w4" if child == "w4" else "default"]
        for c in kc.ffn384_cases(child):
            inp = kc.ffn384_inputs(c)
            got = kr.bf16_value(res[c["name"]])
            rows = kc.compare_rows(c["T"], 128, 7)
            ctx = inp["ctx"][rows] if c["ctx"] else None
            out, bound, _ = kr.ffn_layer_ref(inp["x"][rows], ctx, inp["p"], c["eps"], kc.ffn384_table_gelu(c))
            w = worst.setdefault(f"{c['kernel']} ({child})", kr.Worst())
            w.add(got[rows], out, bound, c["name"], rows=rows)
            assert np.isfinite(got).all(), c["name"]
            print(f"{c['name']}: {len(rows)} of {c['T']} rows compared")
    _report(worst)


def test_launch_gemm_lazy(ln_children):
    """The lazy-LayerNorm modes against the operation on the UNROUNDED rows: MODE 0 / 1 (LN(r) W^T + b, then the split or the GELU),
    MODE 4 (out_g (.) (x W^T + b + LN_prev(r_prev)) and its partial sums), at 256 tokens in the forcing child and at 11 008 by the
    launcher's own rule. Worst err / bound per |mean| / std class of the rows that travel rounded, and what the path loses
    there: the rms error of the rows over the rms error of one bf16 store of the exact result."""
    worst, loss = {}, {}
    for forced, res in ((True, ln_children["forced"]), (False, ln_children["default"])):
        for c in kc.lazy_cases(forced):
            inp = kc.lazy_inputs(c)
            exp, parts = kc.lazy_expect(c, inp)
            if c["mode"] == 4 and c["res_stats"]:
                parts = kr.layernorm_ref(inp["r_prev"], inp["gamma"], inp["beta"], c["eps"])[1]
            cls = kc.ratio_class(parts.ratio)
            if c["mode"] == 0:
                (q, qb), (k, kb), (v, vb) = exp["q"], exp["k"], exp["v"]
                vt, vtb = kc.vt_expected(c, v, vb)
                worst.setdefault("lazy MODE 0 V^T", kr.Worst()).add(kr.bf16_value(res[c["name"] + ":vt"]).reshape(-1, c["S"]), vt.reshape(-1, c["S"]),
                                                                    vtb.reshape(-1, c["S"]), c["name"] + ":vt")
                outs = {"q": (q, qb), "k": (k, kb)}
            else:
                outs = {"out": exp["out"]}
                if "stats" in exp:
                    worst.setdefault("lazy MODE 4 partial sums", kr.Worst()).add(res[c["name"] + ":stats"].reshape(-1, 2), *exp["stats"], c["name"] + ":stats")
            for name, (want, bound) in outs.items():
                got = kr.bf16_value(res[c["name"] + ":" + name])
                for k_ in range(3):
                    rows = np.flatnonzero(cls == k_)
                    tag = f"lazy MODE {c['mode']}{'' if forced else ' (own rule, T = 11008)'} |mean|/std ~ {kc.CLASSES[k_]}"
                    worst.setdefault(tag, kr.Worst()).add(got[rows], want[rows], bound[rows], c["name"] + ":" + name, rows=rows)
                    if c["mode"] == 4 and c["res_stats"]:
                        e2 = loss.setdefault(kc.CLASSES[k_], [0.0, 0.0])
                        fin = np.isfinite(parts.ratio[rows])          # (the flat row: |mean| / std is not a number)
                        e2[0] += float(((got[rows][fin] - want[rows][fin]) ** 2).sum())
                        e2[1] += float(((kr.bf16_round(want[rows][fin].astype(np.float32)) - want[rows][fin]) ** 2).sum())
    for k_, (a, b) in sorted(loss.items()):
        print(f"lazy MODE 4 with res_stats, rows of |mean|/std ~ {k_}: rms error {np.sqrt(a / b):.2f} x that of one bf16 store")
    _report(worst)


def test_dbg_library_forward_passes_equal_the_product_library_bit_for_bit(tmp_path):
    """The kernel-level tests vouch for the product only if the dbg library, with no switch set, runs the same kernels: one fixture
    forward each of the BERT encoder, the decoder and ModernBERT (mix_mean) through both libraries."""
    a = _POOL.submit(_child, tmp_path, "identity", "_dbg")
    b = _POOL.submit(_child, tmp_path, "identity", "_product", None, False)
    a, b = a.result(), b.result()
    for name in ("bert", "decoder", "modernbert_mix_mean"):
        assert a[name].shape == b[name].shape and a[name].size > 0
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name
