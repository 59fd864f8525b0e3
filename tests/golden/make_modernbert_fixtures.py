"""Writes tests/golden/modernbert_*.npz from transformers.ModernBertModel (float32, eager attention, CPU) and the project's seeded
weights: python tests/golden/make_modernbert_fixtures.py. Each file holds shape name, seed, std, ids, lens, pooling, the expected
embeddings, the sensitivities of the reference to the window and to the two thetas (1 - cos per row against the reference with the
window removed / both thetas equal), the error of the all-bf16 ModernBertModel against its float32 self, and the bar of the GPU
test: per figure the larger of the project's bf16 bar and that error (tests/modernbert_ref.py).

std 0.1, not the project's usual 0.02: with 0.02 the window and the second theta move the embeddings by less than any bf16
tolerance, so a forward pass without them would pass. Every fixture that covers the window or the thetas must show a sensitivity of
at least 10x its own bar on every row of at least 130 tokens (tests/test_modernbert_cpu.py asserts it)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

# name -> (shape, seed, std, lens, pooling)
CASES = {
    "mix_mean": ("modernbert-tiny-mix", 11, 0.1, [320, 200, 140, 130, 129, 65, 64, 1], "mean"),
    "mix_cls": ("modernbert-tiny-cls", 12, 0.1, [513, 512, 130, 65, 1], "cls"),
    "global_mean": ("modernbert-tiny-global", 13, 0.1, [513, 200, 64], "mean"),
    "local_mean": ("modernbert-tiny-local", 14, 0.1, [512, 140, 129, 1], "mean"),
    "h256_mean": ("modernbert-tiny-256", 15, 0.1, [320, 200, 140], "mean"),
    "long_cls": ("modernbert-tiny-cls", 16, 0.1, [8192, 300, 65], "cls"),
}
MIN_SENS_ROW = 130          # shorter rows sit inside one window: they are there for the edges


def path(name: str) -> str:
    return os.path.join(HERE, f"modernbert_{name}.npz")


def build(name: str, with_bf16: bool = True):
    from tests.modernbert_ref import make_case
    shape, seed, std, lens, pooling = CASES[name]
    return make_case(shape, seed, std, lens, pooling, with_bf16=with_bf16)


def save(name: str, case: dict) -> None:
    np.savez_compressed(path(name), shape_name=np.array(case["shape_name"]), seed=np.int64(case["seed"]), std=np.float64(case["std"]),
                        ids=case["ids"].astype(np.int16), lens=case["lens"], pooling=np.array(case["pooling"]),
                        expected=case["expected"].astype(np.float32), sens_window=case["sens_window"], sens_theta=case["sens_theta"],
                        bf16_cos=np.float64(case["bf16_cos"]), bf16_abs=np.float64(case["bf16_abs"]),
                        bar_cos=np.float64(case["bar_cos"]), bar_abs=np.float64(case["bar_abs"]))


def load(name: str) -> dict:
    z = np.load(path(name))
    d = {k: z[k] for k in z.files}
    d["shape_name"], d["pooling"] = str(d["shape_name"]), str(d["pooling"])
    d["ids"] = d["ids"].astype(np.int32)
    for k in ("seed",):
        d[k] = int(d[k])
    for k in ("std", "bf16_cos", "bf16_abs", "bar_cos", "bar_abs"):
        d[k] = float(d[k])
    return d


def sensitivity_ok(case: dict):
    """-> (ok, text): every row of at least MIN_SENS_ROW tokens moves by >= 10x the fixture's 1 - cos bar when the window is removed
    and when the thetas are made equal (whichever the fixture's layer types can show)."""
    long_rows = np.asarray(case["lens"]) >= MIN_SENS_ROW
    need = 10.0 * case["bar_cos"]
    ok, text = True, []
    for key in ("sens_window", "sens_theta"):
        s = np.asarray(case[key])
        if s.size == 0:
            continue
        worst = float(s[long_rows].min())
        text.append(f"{key} min {worst:.3g} (need {need:.3g})")
        ok = ok and worst >= need
    return ok, ", ".join(text)


if __name__ == "__main__":
    for name in (sys.argv[1:] or CASES):
        case = build(name)
        ok, text = sensitivity_ok(case)
        print(f"{name}: bf16 self-error 1 - cos {case['bf16_cos']:.3g} max |d| {case['bf16_abs']:.3g}; bar {case['bar_cos']:.3g} / "
              f"{case['bar_abs']:.3g}; {text}; {'ok' if ok else 'NOT SENSITIVE ENOUGH'}", flush=True)
        save(name, case)
