"""GPU suite, launch by launch, of the kernels behind precision="f32" and precision="bf16x3": the modes that tie the embeddings to the
reference's CPU embedder. Every launcher of encoder_f32.hip, gemm.hip MODE 5 / 6, gemm_ln.hip's split form and the row kernels forward_f32
launches (k32_embed, k32_add_ln, k_pool<false>) runs ONE launch at a time on chosen inputs (tests/parity_kernel_cases.py) and is
compared, element by element, with a float64 statement of the operation at a bound derived from the number formats and the case's own
inputs (tests/parity_kernel_refs.py: the derivation is its docstring; nothing is picked or measured). On top, bit for bit: every
[hi | lo] output is the split of its float32 value, sentinels around every output come back untouched, and k32m_gemm equals the scalar
k32_gemm it replaced.

The launches go through the ak_ktp_* wrappers of csrc/kernel_test.hip (libarchi_hip_dbg.so only), which add nothing to the launchers
forward_f32 calls; tests/test_kernels_gpu.py holds that library's forward passes to the product library's bit for bit. The kernels run in
child processes (tests/parity_kernel_worker.py, ARCHI_HIP_DBG=1; at most 3 at a time, each under its own timeout, each case once; after a
child that ended badly nothing more is started from this file); the references are computed here. What
tests/test_parity_kernel_refs_cpu.py proves without a GPU: the emulated rounding schemes stay inside every bound on these very inputs, and
every listed defect lands outside.

Each test prints the worst err / bound of its kernel and where it occurred; a kernel passes at <= 1 with n > 0."""
import concurrent.futures
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import kernel_refs as kr
from tests import parity_kernel_cases as pc
from tests import parity_kernel_refs as pr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PAR = 3
_POOL = concurrent.futures.ThreadPoolExecutor(max_workers=PAR)
_DEAD = []                   # a child that ended badly: nothing more is started on the GPU from this file
GROUPS = {"gemm": None, "attn": None, "rows": None, "x3w": None, "x3w_wide": {"AK_GEMM_BN": "256"}}


def _child(tmp, group, extra):
    out = str(tmp / f"{group}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AK_") and k != "ARCHI_HIP_DBG"}
    env["ARCHI_HIP_DBG"] = "1"
    env.update(extra or {})
    t0 = time.time()
    assert not _DEAD, f"not started: child {_DEAD[0]} ended badly before"
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "parity_kernel_worker.py"), group, out], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=600)
    except subprocess.TimeoutExpired:
        _DEAD.append(group)
        raise
    if p.returncode != 0:
        _DEAD.append(group)
    assert p.returncode == 0, f"{group}: exit {p.returncode}\n" + p.stderr.decode("utf-8", "replace")[-3000:]
    print(f"child {group}: {time.time() - t0:.0f} s")
    res = np.load(out)
    assert int(res["dbg"]) == 1
    return res


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """The five children, each started once (the wide-tile switch of launch_gemm_x3w is read once per process: a child of its own)."""
    tmp = tmp_path_factory.mktemp("parity")
    runs = {g: _POOL.submit(_child, tmp, g, extra) for g, extra in GROUPS.items()}
    out, err = {}, None
    for g, f in runs.items():
        try:
            out[g] = f.result()
        except BaseException as e:      # noqa: BLE001 -- the other children are still collected; the first failure is the test's
            err = err or e
    if err is not None:
        raise err
    return out


def _report(worst):
    for key, w in sorted(worst.items()):
        print(f"{key}: {w}")
    for key, w in worst.items():
        assert w.n > 0 and w.ratio <= 1.0, (key, str(w))


def test_launch_gemm_f32_and_launch_gemm_x3(children):
    """k32m_gemm and k3_gemm on one case list: T in {1, 31, 128, 129, 1056}, N in {128, 384}, K in {32, 64, 384, 1536}, the three epilogues,
    ldc = N and the q | k | v placement, the four input classes. Sentinels in the other columns and in rows >= T untouched; N % 128 and K % 32
    come back as the error code without a write."""
    res = children["gemm"]
    worst, touched = {}, {}
    for c in pc.gemm_cases():
        inp = pc.gemm_inputs(c)
        rb = pc.gemm_res_block(c, inp)
        for which, expect in (("f32", pr.gemm_f32_expect), ("x3", pr.gemm_x3_expect)):
            want, bound = expect(c["epi"], inp["x"], inp["w"], inp["bias"], rb)
            key = f"launch_gemm_{which} epilogue {c['epi']}"
            n = pc.gemm_check(c, res[f"{c['name']}:{which}"], want, bound, worst.setdefault(key, kr.Worst()))
            touched[key] = touched.get(key, 0) + n
    _report(worst)
    assert not any(touched.values()), f"sentinels overwritten: {touched}"
    for i, _ in enumerate(pc.gemm_refused()):
        assert int(res[f"refused{i}:f32"]) != 0 and int(res[f"refused{i}:x3"]) != 0
        assert (res[f"refused{i}:y"] == np.float32(pc.SENT)).all()


def test_k32m_gemm_equals_the_scalar_k32_gemm_bit_for_bit(children):
    """The claim in encoder_f32.hip: every output of k32m_gemm is one fmaf chain over k ascending, bias added last, `bit-identical to the
    scalar kernel it replaces`. Epilogue 0 and epilogue 1 (erf GELU) on every such case of the GEMM list."""
    res = children["gemm"]
    diff, n = {}, 0
    for c in pc.gemm_cases():
        if c["epi"] == 2:
            continue
        a = res[c["name"] + ":f32"][:c["T"], c["col0"]:c["col0"] + c["N"]]
        b = res[c["name"] + ":scalar"]
        d = int((np.ascontiguousarray(a).view(np.uint32) != b.view(np.uint32)).sum())
        n += a.size
        print(f"{c['name']}: {d} of {a.size} elements differ from the scalar kernel")
        diff.setdefault(c["epi"], []).append((c["name"], d))
    assert n > 0
    for epi, rows in diff.items():
        assert all(d == 0 for _, d in rows), (f"epilogue {epi}", rows)


def test_launch_attn_f32_x3_and_x3_split(children):
    """k32m_attn and k3_attn (both outputs): head size 32 and 64, S in {1, 31, 32, 33, 96, 128, 129, 160, 512}, 1 to 24 (sequence, head)
    groups, right-padded, left-padded, holed masks and a sequence with no visible key (exact zeros), with and without the relative-position
    table. The split launcher reads rows of 3 H + 128 floats and writes [hi | lo] rows. Head size 48: the error code, nothing written."""
    res = children["attn"]
    worst = {f"launch_attn_{l}": kr.Worst() for l in pc.ATTN_LAUNCHERS}
    bad = dict.fromkeys(worst, 0)
    for c in pc.attn_cases():
        inp = pc.attn_inputs(c)
        ref = {}
        for l in pc.ATTN_LAUNCHERS:
            bad[f"launch_attn_{l}"] += pc.attn_check(c, inp, l, res[f"{c['name']}:{l}"], worst[f"launch_attn_{l}"], ref)
    _report(worst)
    assert not any(bad.values()), f"non-zero rows of a fully masked sequence, non-finite pad rows or |lo| above half a step: {bad}"
    for l in pc.ATTN_LAUNCHERS:
        assert int(res[f"hd48:{l}"]) != 0, l
    assert (res["hd48:ctx"] == np.float32(pc.SENT)).all() and (res["hd48:ctx2"] == pc.SENT16).all()


def test_split_hilo_and_split_rows_bit_for_bit(children):
    res = children["rows"]
    n = 0
    for c in pc.split_cases():
        x = pc.split_inputs(c)
        if c["kind"] == "hilo":
            hi, lo = res[c["name"] + ":hi"], res[c["name"] + ":lo"]
            assert pr.split_mismatch(x, hi[:c["n"]], lo[:c["n"]]) == 0, c["name"]
            assert (hi[c["n"]:] == pc.SENT16).all() and (lo[c["n"]:] == pc.SENT16).all(), c["name"]
        else:
            out, K = res[c["name"]], c["K"]
            assert pr.split_mismatch(x, out[:c["rows"], :K], out[:c["rows"], K:]) == 0, c["name"]
            assert (out[c["rows"]:] == pc.SENT16).all(), c["name"]
        n += x.size
    print(f"split_hilo / split_rows: {n} elements, hi and lo bit for bit")


def test_row_kernels_of_both_parity_modes(children):
    """k32_embed, k3_embed, k32_add_ln, k3_add_ln (float32 rows against the LayerNorm bound; the split kernels' [hi | lo] rows against their own
    float32 rows bit for bit) and k_pool<false> (mean / CLS, normalised or not, a single visible token, no visible token, a pooled vector of
    exact zeros)."""
    res = children["rows"]
    worst, mism = {}, {}

    def one(kernel, name, out, want, bound, T, out2=None):
        assert (out[T:] == np.float32(pc.SENT)).all(), name
        w = worst.setdefault(kernel, kr.Worst())
        if out2 is None:
            w.add(out[:T], want, bound, name)
        else:
            assert (out2[T:] == pc.SENT16).all(), name
            mism[kernel] = mism.get(kernel, 0) + pc.split_out_check(name, out[:T], out2[:T], want, bound, w)

    for c in pc.embed_cases():
        want, bound = pc.embed_expect(c, pc.embed_inputs(c))
        one("k32_embed", c["name"], res[c["name"] + ":f32"], want, bound, c["T"])
        one("k3_embed", c["name"], res[c["name"] + ":out"], want, bound, c["T"], res[c["name"] + ":out2"])
    for c in pc.add_ln_cases():
        want, bound = pc.add_ln_expect(c, pc.add_ln_inputs(c))
        one("k32_add_ln", c["name"], res[c["name"] + ":f32"], want, bound, c["T"])
        one("k3_add_ln", c["name"], res[c["name"] + ":out"], want, bound, c["T"], res[c["name"] + ":out2"])
    for c in pc.pool_cases():
        inp = pc.pool_inputs(c)
        for pooling, normalise in pc.POOL_MODES:
            want, bound = pr.pool_expect(inp["x"], inp["mask"], pooling, normalise)
            one("k_pool<false>", f"{c['name']}:{pooling}{normalise}", res[f"{c['name']}:{pooling}{normalise}"], want, bound, c["B"])
            assert (res[f"{c['name']}:{pooling}{normalise}"][pc.pool_zero_rows(pooling)] == 0).all(), (c["name"], pooling, normalise)
    _report(worst)
    assert not any(mism.values()), f"[hi | lo] rows that are not the split of the float32 rows: {mism}"


def test_launch_gemm_x3w_modes_5_and_6_on_both_tiles(children):
    """k_gemm<5> and k_gemm<6> on the narrow tile by the launcher's choice, on the wide tile forced (AK_GEMM_BN=256, a child of its own) and by
    the launcher's own threshold from both sides, and with a second tile per workgroup; nvalid: columns past it keep the sentinel. MODE 6:
    hi + lo against x Phi(x) at the table's bound, |lo| within half a bf16 step of hi."""
    worst, bad = {}, {}
    for child, group in (("default", "x3w"), ("wide", "x3w_wide")):
        for c in pc.x3w_cases(child):
            wide = pc.x3w_selection(c)[0]
            key = f"MODE {c['mode']} {'wide' if wide else 'narrow'} tile ({'forced' if child == 'wide' else 'own choice'})"
            bad[key] = bad.get(key, 0) + pc.x3w_check(c, children[group][c["name"]], pc.x3w_inputs(c), worst.setdefault(key, kr.Worst()))
    _report(worst)
    assert not any(bad.values()), f"columns >= nvalid written (MODE 5) or |lo| above half a step (MODE 6): {bad}"


def test_launch_gemm_ln_x3(children):
    """k_gemm_ln<false, true>: T in {256, 512}, K' in {384, 1536}, rows of |mean| / std ~ 0, 4, 32 and the near-constant row: x32 in place
    against the LayerNorm bound, its [hi | lo] rows bit for bit."""
    res = children["rows"]
    worst, mism = kr.Worst(), 0
    for c in pc.gemm_ln_x3_cases():
        want, bound = pc.gemm_ln_x3_expect(c, pc.gemm_ln_x3_inputs(c))
        mism += pc.split_out_check(c["name"], res[c["name"] + ":x32"], res[c["name"] + ":x16"], want, bound, worst)
    _report({"launch_gemm_ln_x3": worst})
    assert mism == 0, f"{mism} [hi | lo] elements are not the split of x32"
