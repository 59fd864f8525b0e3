"""GPU suite of NomicBERT's row kernels (csrc/nomic.hip), launch by launch, in the manner of tests/test_stack_kernels_gpu.py:
k_nb_embed<NJ>, k_nb_add_ln<NJ> and k_nb_pool_part + k_nb_pool_fin, ONE launch at a time through the ak_ktn_* wrappers, in child
processes on libarchi_hip_dbg.so (tests/nomic_kernel_worker.py; each case once, nothing is run again after a failure). The wrappers
call the launch_nb_* functions the forward pass calls.

Cases, inputs, the float64 references, the derived bounds and what is exact: tests/nomic_kernel_refs.py (err / bound <= 1 through
kernel_refs.Worst; exact outputs bit for bit). tests/test_nomic_cpu.py holds the same expectations to float32 emulations of the
kernels and to the mutants. Each test prints its worst err / bound (-s); DESIGN.md section 1 records them."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import kernel_refs as kr
from tests import nomic_kernel_refs as nk
from tests import stack_kernel_refs as sr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_DEAD = []                   # a child that ended badly: nothing more is started on the GPU from this file
_RES = {}


def _child(tmp_path_factory, group):
    if group in _RES:
        return _RES[group]
    out = str(tmp_path_factory.mktemp("nomic_kernels") / f"{group}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AK_")}
    env["ARCHI_HIP_DBG"] = "1"
    t0 = time.time()
    assert not _DEAD, f"not started: child {_DEAD[0]} ended badly before"
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "nomic_kernel_worker.py"), group, out], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=300)
    except subprocess.TimeoutExpired:
        _DEAD.append(group)
        raise
    if p.returncode != 0:
        _DEAD.append(group)
    assert p.returncode == 0, f"{group}: exit {p.returncode}\n" + p.stderr.decode("utf-8", "replace")[-3000:]
    print(f"child {group}: {time.time() - t0:.0f} s")
    _RES[group] = np.load(out)
    return _RES[group]


def _got(res, prefix):
    return {k[len(prefix) + 1:]: res[k] for k in res.files if k.startswith(prefix + ":") and ":" not in k[len(prefix) + 1:]}


def _hold(res, cases, expect, label):
    worst, bad = kr.Worst(), []
    for c in cases:
        got = _got(res, c["name"])
        bad += [f"{c['name']}:{n}" for n in sr.compare(expect(c), got, worst, c["name"])]
    print(f"{label}: {worst}")
    assert not bad, f"{label}: not bit for bit: {bad[:8]}"
    assert worst.n > 0 and worst.ratio <= 1.0, f"{label}: {worst}"


def test_embed(tmp_path_factory):
    """k_nb_embed<NJ> at every hidden size, S = 32, 96, 192, lengths {-3, 0, 1, 65, S - 1, S, S + 5} clamped to [0, S]: the lengths and
    the key mask bit for bit, stray ids and everything past a length read word row 0, the token-type row is row 0; x32 =
    LayerNorm(word + type; g, b) and h16 at the bound; rows past B * S keep the sentinel."""
    res = _child(tmp_path_factory, "embed")
    assert {c["H"] for c in nk.embed_cases()} == set(nk.HS) and {c["S"] for c in nk.embed_cases()} == {32, 96, 192}
    _hold(res, nk.embed_cases(), lambda c: nk.embed_expect(c, nk.embed_inputs(c)), "embed nb")


def test_add_ln(tmp_path_factory):
    """k_nb_add_ln<NJ> at every hidden size, T in {1, 5, 127, 384}: x32 holds the NORMALISED row (float32) and h16 its bf16, both at
    the bound; y32 is not written; rows past T keep the sentinel."""
    res = _child(tmp_path_factory, "addnorm")
    _hold(res, nk.addnorm_cases(), lambda c: nk.addnorm_expect(c, nk.addnorm_inputs(c)), "add + LayerNorm nb")


def test_pool(tmp_path_factory):
    """k_nb_pool_part + k_nb_pool_fin, mean and cls, normalised and not: lengths around the 64-token chunks (63 / 64 / 65) and
    {S, S - 1, 1, 0} as batch rows at S = 192, 96, 32. Token rows a pool must not read are NaN, the chunk sums are prefilled with NaN:
    every output is finite and at the bound on sum |x_t|; rows of length 0 are zeros. The row of 129 tokens given alone at S = 2048
    comes out bit for bit as in the S = 192 batch (which tokens meet in which sum depends on the length alone)."""
    res = _child(tmp_path_factory, "pool")
    worst, bad = kr.Worst(), []
    for c in nk.pool_cases():
        inp = nk.pool_inputs(c)
        for mode in nk.POOL_MODES:
            got = _got(res, f"{c['name']}:{mode[0]}")
            bad += [c["name"] for n in sr.compare(nk.pool_expect(c, inp, mode), got, worst, f"{c['name']}:{mode[0]}")]
            for b, n in enumerate(c["lens"]):
                if n == 0:
                    assert not got["out"][b].view(np.uint32).any(), f"{c['name']}:{mode[0]}: a row of length 0 is not zeros"
            if "twin" in c:
                assert np.array_equal(got["out"][0].view(np.uint32), res[f"{c['twin']}:{mode[0]}:out"][nk.TWIN_ROW].view(np.uint32)), \
                    f"{c['name']}:{mode[0]}: the same row pooled differently at S = 2048 and in the S = 192 batch"
    print(f"pool nb: {worst}")
    assert not bad, bad
    assert worst.n > 0 and worst.ratio <= 1.0, str(worst)
