"""CPU suite behind tests/test_stack_kernels_gpu.py, in the manner of tests/test_kernel_refs_cpu.py: what the float64 references and
their derived bounds (tests/stack_kernel_refs.py) must do before a GPU is asked. On the very inputs the GPU tests use
(tests/stack_kernel_cases.py):
  - a numpy float32 emulation of every kernel in the kernel's summation order stays within the bound, and is bit for bit where the
    expectation is exact: the check that the reference alone passes;
  - every mutant -- a defect applied to the reference -- is flagged: err / bound > 1, a NaN, or a bit mismatch where the expectation
    is exact, in every family the defect can occur in;
  - the ak_kts_* entry points are exactly _lib.KTS_SYMBOLS, in libarchi_hip_dbg.so only."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import kernel_cases as kc
from tests import kernel_refs as kr
from tests import stack_kernel_cases as sc
from tests import stack_kernel_refs as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tables(c, n_pos=None):
    from archi_amd import _lib
    from tests.stack_kernel_worker import rope_tables
    return rope_tables(_lib.load(), c, n_pos)


def _groups():
    """{group: [(case, family, expect(mut), emulate())]} over every GPU case."""
    out = {"embed": [], "addnorm": [], "rope": [], "pool": [], "dense": [], "l2": []}
    for c in sc.embed_cases():
        out["embed"].append((c, c["fam"], lambda mut=None, c=c: sr.embed_expect(c, sc.embed_inputs(c), mut),
                             lambda c=c: sr.embed_emulate(c, sc.embed_inputs(c))))
    for c in sc.addnorm_cases():
        out["addnorm"].append((c, c["fam"], lambda mut=None, c=c: sr.addnorm_expect(c, sc.addnorm_inputs(c), mut),
                               lambda c=c: sr.addnorm_emulate(c, sc.addnorm_inputs(c))))
    for c in sc.rope_cases():
        def exp(mut=None, c=c):
            rc, rs = _tables(c, c["B"] * c["S"] if mut == "pos_t" else None)
            return sr.rope_expect(c, sc.rope_inputs(c), rc, rs, mut)
        out["rope"].append((c, c["fam"], exp, lambda c=c: sr.rope_emulate(c, sc.rope_inputs(c), *_tables(c))))
    for c in sc.pool_cases():
        for mode in sc.pool_modes(c):
            out["pool"].append((dict(c, name=f"{c['name']}:{mode[0]}"), c["fam"],
                                lambda mut=None, c=c, mode=mode: sr.pool_expect(c, sc.pool_inputs(c), mode, mut),
                                lambda c=c, mode=mode: sr.pool_emulate(c, sc.pool_inputs(c), mode)))
    for c in sc.dense_cases():
        out["dense"].append((c, "gm", lambda mut=None, c=c: sr.dense_expect(c, sc.dense_inputs(c), mut), lambda c=c: sr.dense_emulate(c, sc.dense_inputs(c))))
    for c in sc.l2_cases():
        out["l2"].append((c, "gm", lambda mut=None, c=c: sr.l2_expect(c, sc.l2_inputs(c), mut), lambda c=c: sr.l2_emulate(c, sc.l2_inputs(c))))
    return out


GROUPS = _groups()


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_float32_emulation_stays_within_the_bound(group):
    """The kernels' arithmetic restated in numpy float32, in their summation order, against the float64 statement: err / bound <= 1
    on every GPU case, exact outputs bit for bit, per family."""
    worst, bad = {}, []
    for c, fam, expect, emulate in GROUPS[group]:
        w = worst.setdefault(fam, kr.Worst())
        bad += [f"{c['name']}:{n}" for n in sr.compare(expect(), emulate(), w, c["name"], need_all=False)]
    for fam, w in worst.items():
        print(f"{group} {fam}: {w}")
    assert not bad, bad[:8]
    assert all(w.n > 0 and w.ratio <= 1.0 for w in worst.values()), {f: str(w) for f, w in worst.items() if w.ratio > 1.0}


# mutant -> [(group, families in which at least one case must flag it)]
MUTANTS = {
    "eps_outside": [("addnorm", FAMS3 := ("dec", "mb", "gm")), ("pool", ("dec", "mb"))],
    "mean_256nj": [("addnorm", FAMS3), ("embed", FAMS3), ("pool", ("dec", "mb"))],
    "onepass": [("pool", ("mb",)), ("embed", ("mb",))],
    "w_shift": [("addnorm", FAMS3), ("embed", FAMS3), ("pool", ("dec", "mb"))],
    "pos_t": [("rope", ("dec", "mb"))],
    "sign": [("rope", ("dec", "mb"))],
    "partner": [("rope", ("dec", "mb"))],
    "scale_k": [("rope", ("dec",))],
    "n_plus_1": [("pool", ("mb", "gm"))],
    "n_ceil64": [("pool", ("mb", "gm"))],
    "div_S": [("pool", ("mb", "gm"))],
    "cls_1": [("pool", ("mb",))],
    "last_len": [("pool", ("dec",))],
    "no_floor": [("l2", ("gm",)), ("pool", ("dec",))],
    "stride_N": [("dense", ("gm",))],
    "stray_id": [("embed", FAMS3)],
    "len_unclamped": [("embed", FAMS3)],
}


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_mutant_is_flagged(mut):
    """eps outside the root; the mean over 256 NJ features; the one-pass float32 variance; the norm weight one lane off; RoPE at
    position t; the rotate-half sign; the partner at d + hd / 4; the q scale on k; pooling n + 1 / ceil(n / 64) 64 tokens; division
    by S; CLS at token 1; the last token at `len`; no L2 floor; a dense row at stride N; a stray id read as it is; the length not
    clamped -- each, applied to the reference, misses the expectation on the GPU tests' own inputs."""
    for group, fams in MUTANTS[mut]:
        hit = {f: [] for f in fams}
        for c, fam, expect, _ in GROUPS[group]:
            if fam in hit and (not hit[fam] or group != "pool") and sr.flagged(expect(), expect(mut)):
                hit[fam].append(c["name"])
        print(f"{mut} / {group}: " + ", ".join(f"{f}: {len(v)} cases" for f, v in hit.items()))
        assert all(hit.values()), (mut, group, [f for f, v in hit.items() if not v])


def test_mean_over_256nj_is_seen_at_every_partial_hidden_size():
    """H = 128, 384 and 640 are the sizes at which 256 NJ != H: each flags the mutant in each family's add + norm kernel."""
    for c, fam, expect, _ in GROUPS["addnorm"]:
        if c["T"] == 127 and c["form"] != "add":
            assert sr.flagged(expect(), expect("mean_256nj")) == (c["H"] % 256 != 0), c["name"]


def test_gemm_mode3_reference_passes_its_emulation_and_sees_a_dropped_k_slice():
    for c in sc.gemm3_cases()[:2] + sc.gemm3_cases()[3:]:          # (the 4096 x 4096 x 1024 case is the GPU parent's to pay for)
        assert kc.gemm_tile_is_wide(c) == (c["tile"] == "wide")
        inp = kc.gemm_inputs(c)
        exp = sr.gemm3_expect(c, inp)
        w = kr.Worst()
        emu = kr.bf16_bits(kr.gemm_emulate(kr.bf16_value(inp["x"]), kr.bf16_value(inp["w"]), inp["bias"]))
        assert not sr.compare(exp, {"out": emu}, w, c["name"]) and w.ratio <= 1.0, str(w)
        print(f"{c['name']}: {w}")
        assert sr.flagged(exp, sr.gemm3_expect(c, inp, drop_k=slice(32, 64)))


def test_case_lists_say_what_the_issue_asks():
    assert {c["H"] for c in sc.embed_cases() if c["fam"] == "dec"} == set(sc.HS) | {2560} and sc.HS == (128, 256, 384, 640, 768, 1024)
    assert {c["H"] for c in sc.addnorm_cases() if c["fam"] != "dec"} == set(sc.HS)
    assert {c["T"] for c in sc.addnorm_cases()} == {1, 5, 127, 512} and {c["eps"] for c in sc.addnorm_cases()} == {1e-6, 1e-5}
    c = sc.embed_cases()[1]
    inp = sc.embed_inputs(c)
    assert list(inp["lens"][:, 0]) == [-3, 0, 1, c["S"] - 1, c["S"], c["S"] + 5] and c["ld_ids"] > c["S"] and c["vocab"] == 97
    assert {(c["nq"], c["nkv"]) for c in sc.rope_cases() if c["fam"] == "dec"} == {(1, 1), (2, 1), (4, 1), (3, 3)}
    assert any(c["S"] == 8192 for c in sc.rope_cases() if c["fam"] == "dec") and any(c["S"] == 8192 for c in sc.rope_cases() if c["fam"] == "mb")
    assert sc.LENS192 == (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192)
    x = sc.pool_inputs(next(c for c in sc.pool_cases() if c["name"] == "pool_dec_H256_S192"))["x"]
    assert all(np.isfinite(x[b]).all(axis=1).sum() == (1 if n else 0) for b, n in enumerate(sc.LENS192))
    assert {(c["N"], c["K"]) for c in sc.dense_cases()} == {(N, K) for N in (4, 7, 768) for K in (128, 768, 3072)}
    assert {c["D"] for c in sc.l2_cases()} == {128, 256, 768, 1000}
    assert [(c["N"], c["K"], c["T"]) for c in sc.gemm3_cases()] == [(640, 128, 512), (1152, 1024, 512), (4096, 1024, 4096), (1024, 64, 16384)]


def test_stack_wrappers_stay_out_of_the_product_library():
    """ak_kts_* (csrc/kernel_test.hip) exist in libarchi_hip_dbg.so only, are exactly _lib.KTS_SYMBOLS, and none of them is in
    KT_SYMBOLS or KTG_SYMBOLS."""
    from archi_amd import _lib

    def exported(name):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "archi_amd", "lib", name)], stdout=subprocess.PIPE,
                             check=True).stdout.decode()
        return set(re.findall(r"\b(ak_kts_[a-z0-9_]+)\b", out))

    _lib.load()                                                                               # (the libraries are built)
    assert exported("libarchi_hip.so") == set()
    names = {n for n, _, _ in _lib.KTS_SYMBOLS}
    assert exported("libarchi_hip_dbg.so") == names and "ak_kts_gemm_bf16" in names and len(names) == len(_lib.KTS_SYMBOLS)
    assert not names & ({n for n, _, _ in _lib.KT_SYMBOLS} | {n for n, _, _ in _lib.KTG_SYMBOLS})
    assert not any(n.startswith("ak_kt_") or n.startswith("ak_ktg_") for n in names)
