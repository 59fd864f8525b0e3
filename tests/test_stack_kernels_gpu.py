"""GPU suite of the small kernels of the stacks, launch by launch, in the manner of tests/test_gemma_kernels_gpu.py: the embedding,
add + norm, RoPE, pooling, dense and L2 kernels of decoder128.hip (Qwen3, `dec`), mbert.hip (ModernBERT, `mb`), gemma.hip (EmbeddingGemma,
`gm`) and nomic.hip (NomicBERT, `nb`), and k_gemm MODE 3, ONE launch at a time through the ak_kts_* wrappers, in child processes on
libarchi_hip_dbg.so (tests/stack_kernel_worker.py; each case once, nothing is run again after a failure). The wrappers call the
launch_* functions the forward passes call.

Cases and inputs: tests/stack_kernel_cases.py. References in float64, the derived bounds and what is exact: tests/stack_kernel_refs.py
(err / bound <= 1 through kernel_refs.Worst; exact outputs bit for bit). tests/test_stack_kernels_cpu.py holds the same expectations
to float32 emulations of the kernels and to the mutants. NomicBERT's cases, inputs, references and bounds: tests/nomic_kernel_refs.py,
held to emulations and mutants by tests/test_nomic_cpu.py. Each test prints its worst err / bound (-s); DESIGN.md section 1 records
NomicBERT's."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import kernel_cases as kc
from tests import kernel_refs as kr
from tests import nomic_kernel_refs as nk
from tests import stack_kernel_cases as sc
from tests import stack_kernel_refs as sr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_DEAD = []                   # a child that ended badly: nothing more is started on the GPU from this file
_RES = {}
FAMS = sc.FAMS + ("nb",)


def _child(tmp_path_factory, group):
    if group in _RES:
        return _RES[group]
    out = str(tmp_path_factory.mktemp("stack_kernels") / f"{group}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AK_")}
    env["ARCHI_HIP_DBG"] = "1"
    t0 = time.time()
    assert not _DEAD, f"not started: child {_DEAD[0]} ended badly before"
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "stack_kernel_worker.py"), group, out], env=env, stdout=subprocess.PIPE,
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
    """Every case's outputs against its expectation; prints and asserts the worst ratio and that nothing exact differs."""
    worst, bad = kr.Worst(), []
    for c in cases:
        got = _got(res, c["name"])
        bad += [f"{c['name']}:{n}" for n in sr.compare(expect(c, got), got, worst, c["name"])]
    print(f"{label}: {worst}")
    assert not bad, f"{label}: not bit for bit: {bad[:8]}"
    assert worst.n > 0 and worst.ratio <= 1.0, f"{label}: {worst}"


@pytest.mark.parametrize("fam", FAMS)
def test_embed(tmp_path_factory, fam):
    """k_dec_embed / k_mb_embed / k_gm_embed<NJ> at every hidden size: lengths clamped to [0, S], stray ids and everything past a
    length read row 0, ModernBERT's mask; Qwen3's and Gemma's x32 bit for bit; h16 (and ModernBERT's LayerNormed x32) at the bound;
    rows past B * S keep the sentinel.
    nb: k_nb_embed<NJ> at every hidden size, S = 32, 96, 192, lengths {-3, 0, 1, 65, S - 1, S, S + 5} clamped to [0, S]: the lengths and
    the key mask bit for bit, stray ids and everything past a length read word row 0, the token-type row is row 0; x32 =
    LayerNorm(word + type; g, b) and h16 at the bound; rows past B * S keep the sentinel."""
    res = _child(tmp_path_factory, "embed")
    if fam == "nb":
        assert {c["H"] for c in nk.embed_cases()} == set(nk.HS) and {c["S"] for c in nk.embed_cases()} == {32, 96, 192}
        _hold(res, nk.embed_cases(), lambda c, got: nk.embed_expect(c, nk.embed_inputs(c)), "embed nb")
        return
    _hold(res, [c for c in sc.embed_cases() if c["fam"] == fam], lambda c, got: sr.embed_expect(c, sc.embed_inputs(c)), f"embed {fam}")


@pytest.mark.parametrize("fam", FAMS)
def test_add_norm(tmp_path_factory, fam):
    """k_dec_add_rmsnorm / k_mb_add_ln<NJ> / k_gm_norm_add_norm<NJ> at T in {1, 5, 127, 512}: the float32 add bit for bit, the norm
    at its bound, the add-only form leaves h16 alone, Gemma to h16 and with out32 aliasing y32; rows past T keep the sentinel.
    nb: k_nb_add_ln<NJ> at every hidden size, T in {1, 5, 127, 384}: x32 holds the NORMALISED row (float32) and h16 its bf16, both at
    the bound; y32 is not written (the child asserts it); rows past T keep the sentinel."""
    res = _child(tmp_path_factory, "addnorm")
    if fam == "nb":
        _hold(res, nk.addnorm_cases(), lambda c, got: nk.addnorm_expect(c, nk.addnorm_inputs(c)), "add + LayerNorm nb")
        return
    _hold(res, [c for c in sc.addnorm_cases() if c["fam"] == fam], lambda c, got: sr.addnorm_expect(c, sc.addnorm_inputs(c)), f"add + norm {fam}")


@pytest.mark.parametrize("fam", ("dec", "mb"))
def test_rope(tmp_path_factory, fam):
    """k_dec_qk_rope (head RMSNorm, rotate_half RoPE, q scaled, v copied bit for bit, head-major) and k_mb_rope (in place) against
    float64 on the float32 tables the launch was handed; the position restarts in every batch row; S = 8192 reaches the last table
    row; nothing behind the outputs is written."""
    res = _child(tmp_path_factory, "rope")
    _hold(res, [c for c in sc.rope_cases() if c["fam"] == fam],
          lambda c, got: sr.rope_expect(c, sc.rope_inputs(c), got["rc"], got["rs"]), f"rope {fam}")


# per family: its cases, their inputs, the launches on one input, the expectation, the S = 192 batch row that the twin case repeats
_POOL = {fam: (sc.pool_cases, sc.pool_inputs, sc.pool_modes, sr.pool_expect, sc.TWIN_ROW) for fam in sc.FAMS}
_POOL["nb"] = (nk.pool_cases, nk.pool_inputs, lambda c: nk.POOL_MODES, nk.pool_expect, nk.TWIN_ROW)


@pytest.mark.parametrize("fam", FAMS)
def test_pool(tmp_path_factory, fam):
    """k_dec_pool; k_mb_pool_part + k_mb_pool_fin (mean and CLS); k_gm_pool_part + k_gm_pool_fin: every length around the 64-token
    chunks as a batch row. Token rows a pool must not read are NaN, the chunk sums are prefilled with NaN: every output is finite and
    at the bound on sum |y_t|; rows of length 0 are zeros. The row of length 129 given alone at S = 2048 comes out bit for bit as
    in the S = 192 batch (stack.h: which tokens meet in which sum depends on n alone). Normalise off: the un-normalised values (the
    same float64 statement without the L2 tail; k_gm_l2's copy is held bit for bit in test_dense_l2_fold).
    nb: k_nb_pool_part + k_nb_pool_fin, mean and cls, normalised and not: lengths around the 64-token chunks (63 / 64 / 65) and
    {S, S - 1, 1, 0} as batch rows at S = 192, 96, 32, the bound on sum |x_t|; rows of length 0 are zeros bit for bit; the row of 129
    tokens alone at S = 2048 as in the S = 192 batch."""
    res = _child(tmp_path_factory, "pool")
    cases, inputs, modes, expect, twin_row = _POOL[fam]
    worst, bad = kr.Worst(), []
    for c in cases():
        if c["fam"] != fam:
            continue
        inp = inputs(c)
        for mode in modes(c):
            got = _got(res, f"{c['name']}:{mode[0]}")
            bad += [c["name"] for n in sr.compare(expect(c, inp, mode), got, worst, f"{c['name']}:{mode[0]}")]
            for b, n in enumerate(c["lens"]):
                if fam == "nb" and n == 0:
                    assert not got["out"][b].view(np.uint32).any(), f"{c['name']}:{mode[0]}: a row of length 0 is not zeros"
            if "twin" in c:
                assert np.array_equal(got["out"][0].view(np.uint32), res[f"{c['twin']}:{mode[0]}:out"][twin_row].view(np.uint32)), \
                    f"{c['name']}:{mode[0]}: the same row pooled differently at S = 2048 and in the S = 192 batch"
    print(f"pool {fam}: {worst}")
    assert not bad, bad
    assert worst.n > 0 and worst.ratio <= 1.0, str(worst)


def test_dense_l2_fold(tmp_path_factory):
    """k_gm_dense (N = 7: the n >= N guard), k_gm_l2 (zero row -> zeros, a row under the 1e-12 floor, normalise off: a bit-exact
    copy), k_gm_fold1p bit for bit."""
    res = _child(tmp_path_factory, "tail")
    _hold(res, sc.dense_cases(), lambda c, got: sr.dense_expect(c, sc.dense_inputs(c)), "dense")
    _hold(res, sc.l2_cases(), lambda c, got: sr.l2_expect(c, sc.l2_inputs(c)), "l2")
    assert not sr.compare(sr.fold_expect(sc.fold_inputs()), _got(res, "fold1p"), kr.Worst(), "fold1p"), "k_gm_fold1p: not 1 + w bit for bit"


def test_gemm_mode3_on_every_tile(tmp_path_factory):
    """k_gemm MODE 3 (plain bf16 rows: the Qwen3 and Gemma QKV projections) through ak_kts_gemm_bf16: the narrow tile, the wide phased
    tile and the wide in-step loop, each picked by the launcher itself; every output element against float64."""
    res = _child(tmp_path_factory, "gemm3")
    assert sorted(c["K"] >= 192 for c in sc.gemm3_cases() if c["tile"] == "wide") == [False, True]      # the in-step loop and the phased one
    for c in sc.gemm3_cases():
        assert kc.gemm_tile_is_wide(c) == (c["tile"] == "wide")
        _hold(res, [c], lambda c, got: sr.gemm3_expect(c, kc.gemm_inputs(c)), f"gemm MODE 3 {c['tile']} K{c['K']}")


def test_decoder_refuses_more_rows_than_a_grid_dimension():
    """ak_decoder_forward_lens at B = 65536, S = 32 (the attention launch indexes the batch row with blockIdx.z): refused under the
    entry point's name before anything is launched (the output keeps its prefill); B = 3 on the same handle works afterwards."""
    import torch
    from archi_amd import _lib, decoder as dm
    shape = dm.QWEN3_SHAPES["qwen3-tiny-g1"]
    dec = dm.HipDecoder(shape, dm.random_qwen3_weights(shape, seed=5))
    B, S = 65536, 32
    stage = torch.ones((B, S + 1), dtype=torch.int32, device="cuda")
    stage[:, S] = torch.arange(B, dtype=torch.int32, device="cuda") % S + 1
    out = torch.full((B, shape[1]), float("nan"), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.HipBackendError, match="ak_decoder_forward_lens: at most 65535 rows per call"):
        dec.forward_lens(stage, B, S, out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "something was launched"
    dec.forward_lens(stage[:3].contiguous(), 3, S, out[:3])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:3]).all()) and bool(torch.isnan(out[3:]).all())
    assert torch.allclose((out[:3] ** 2).sum(-1), torch.ones(3, device="cuda"), atol=1e-4)
    dec.close()
