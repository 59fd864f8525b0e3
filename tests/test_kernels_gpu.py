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
    """k_attn_causal at G = 1, 2, 4 and every row length: the decoder reads one row of it, here every row is checked."""
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


def test_dbg_library_forward_passes_equal_the_product_library_bit_for_bit(tmp_path):
    """The kernel-level tests vouch for the product only if the dbg library, with no switch set, runs the same kernels: one fixture
    forward each of the BERT encoder, the decoder and ModernBERT (mix_mean) through both libraries."""
    a = _POOL.submit(_child, tmp_path, "identity", "_dbg")
    b = _POOL.submit(_child, tmp_path, "identity", "_product", None, False)
    a, b = a.result(), b.result()
    for name in ("bert", "decoder", "modernbert_mix_mean"):
        assert a[name].shape == b[name].shape and a[name].size > 0
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name
