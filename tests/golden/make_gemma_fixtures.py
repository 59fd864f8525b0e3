"""Writes tests/golden/gemma_*.npz from transformers.Gemma3TextModel (float32, eager attention, CPU, use_bidirectional_attention) and
the project's seeded weights: python tests/golden/make_gemma_fixtures.py. Each file holds shape name, seed, std, ids, lens, the expected
embeddings (mean pooled, through the shape's Dense head, normalised), the sensitivities of the reference per row to four ablations
(1 - cos against the causal stack, the stack without a window, with both thetas equal, with head_dim ** -0.5 as the score scale), the
error of the all-bf16 Gemma3TextModel against its float32 self, and the bar of the GPU test: per figure the larger of the project's
bf16 bar and that error (tests/gemma_ref.py).

std 0.1, not the project's usual 0.02, for the reason make_modernbert_fixtures.py gives: with 0.02 the window and the second theta
move the embeddings by less than any bf16 tolerance. The lengths sit on both sides of the half-window (32) and of the 32-key block."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

ALL_LENS = [2048, 1024, 513, 300, 130, 97, 66, 65, 34, 33, 32, 1]
# name -> (shape, seed, std, lens)
CASES = {
    "tiny": ("gm-tiny", 21, 0.1, ALL_LENS),
    "g2": ("gm-g2", 22, 0.1, [513, 300, 130, 97, 66, 65, 33, 1]),
    "global": ("gm-global", 23, 0.1, [300, 130, 66, 34, 1]),
    "local": ("gm-local", 24, 0.1, [1024, 300, 130, 97, 66, 33, 32]),
}
SENS_KEYS = ("sens_causal", "sens_no_window", "sens_same_theta", "sens_wrong_scale")
SENS_MIN_ROW, SENS_MAX_ROW = 66, 1024      # rows the sensitivity assertion covers: past the window, and as far as it was measured


def path(name: str) -> str:
    return os.path.join(HERE, f"gemma_{name}.npz")


def build(name: str, with_bf16: bool = True, ablations=None):
    from tests.gemma_ref import ABLATIONS, make_case
    shape, seed, std, lens = CASES[name]
    return make_case(shape, seed, std, lens, with_bf16=with_bf16, ablations=ABLATIONS if ablations is None else ablations)


def save(name: str, case: dict) -> None:
    np.savez_compressed(path(name), shape_name=np.array(case["shape_name"]), seed=np.int64(case["seed"]), std=np.float64(case["std"]),
                        ids=case["ids"].astype(np.int16), lens=case["lens"], expected=case["expected"].astype(np.float32),
                        bf16_cos=np.float64(case["bf16_cos"]), bf16_abs=np.float64(case["bf16_abs"]),
                        bar_cos=np.float64(case["bar_cos"]), bar_abs=np.float64(case["bar_abs"]), **{k: case[k] for k in SENS_KEYS})


def load(name: str) -> dict:
    z = np.load(path(name))
    d = {k: z[k] for k in z.files}
    d["shape_name"] = str(d["shape_name"])
    d["ids"] = d["ids"].astype(np.int32)
    d["seed"] = int(d["seed"])
    for k in ("std", "bf16_cos", "bf16_abs", "bar_cos", "bar_abs"):
        d[k] = float(d[k])
    return d


def sensitivity(case: dict):
    """-> {key: (worst 1 - cos over the rows of SENS_MIN_ROW .. SENS_MAX_ROW tokens, value of the 2048-token row or None)} for the
    ablations the fixture holds."""
    lens = np.asarray(case["lens"])
    rows = (lens >= SENS_MIN_ROW) & (lens <= SENS_MAX_ROW)
    out = {}
    for key in SENS_KEYS:
        s = np.asarray(case[key])
        if s.size:
            out[key] = (float(s[rows].min()), float(s[lens == 2048][0]) if (lens == 2048).any() else None)
    return out


if __name__ == "__main__":
    for name in (sys.argv[1:] or CASES):
        case = build(name)
        need = 10.0 * case["bar_cos"]
        text = ", ".join(f"{k} min {v[0]:.3g}" + (f" (2048: {v[1]:.3g})" if v[1] is not None else "") for k, v in sensitivity(case).items())
        print(f"{name}: bf16 self-error 1 - cos {case['bf16_cos']:.3g} max |d| {case['bf16_abs']:.3g}; bar {case['bar_cos']:.3g} / "
              f"{case['bar_abs']:.3g}; need {need:.3g}: {text}", flush=True)
        save(name, case)
