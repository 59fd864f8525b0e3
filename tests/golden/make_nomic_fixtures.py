"""Writes tests/golden/nomic_*.npz from transformers.NomicBertModel (float32, eager attention, CPU) and the project's seeded weights:
python tests/golden/make_nomic_fixtures.py. Each file holds shape name, seed, std, ids, lens, pooling, the expected embeddings, the
error of the all-bf16 NomicBertModel against its float32 self on those rows, and the bar of the GPU test: per figure the larger of the
project's bf16 bar and that error (tests/nomic_ref.py). The weights come from the seed and are not stored.

std 0.1 and more, not the project's usual 0.02: measured on a 3-layer hidden-256 model at 0.02, replacing theta 1000 by 10000 moves the
embeddings by 1 - cos 1.2e-7 and removing RoPE altogether by 4.8e-7 -- a forward pass without RoPE would pass. Every mean-pooled fixture
must show, on every row of at least 5 tokens, a sensitivity of at least 10x its own 1 - cos bar to each of tests/nomic_ref.ABLATIONS
(tests/test_nomic_cpu.py asserts it from NomicBertModel alone). Where std 0.1 did not give that the std was changed, not the factor:
the hidden-128 mean fixtures at 0.1 moved by 8e-4 to 1.9e-3 under theta 10000 and by 1.3e-3 to 1.7e-3 under the attention scale times
sqrt(2) (three seeds), so they are drawn at 0.15; the hidden-768 cut at 0.1 has an all-bf16 error of 1.3e-3 (ten times that is more
than the scale moves it), at 0.05 the scale moves it by 9e-4, so it is drawn at 0.065."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))


def _base_lens():
    """64 rows of up to 512 tokens: a batch large enough that every GEMM of the layer runs on the wide tile."""
    return [512, 511, 257, 256, 130, 65, 33, 5] + [int(n) for n in np.random.RandomState(5).randint(6, 513, size=56)]


# name -> (shape, seed, std, lens, pooling)
CASES = {
    "tiny_mean": ("nomic-tiny-mean", 31, 0.15, [320, 130, 64, 33, 32, 17, 5, 1], "mean"),
    "tiny_cls": ("nomic-tiny-cls", 42, 0.1, [513, 512, 100, 1], "cls"),
    "tiny_256": ("nomic-tiny-256", 31, 0.1, [160, 129, 2], "mean"),
    "tiny_long": ("nomic-tiny-long", 41, 0.15, [8192, 300, 65], "mean"),
    "base_cut2": ("nomic-base-cut2", 43, 0.065, _base_lens(), "mean"),
}
MIN_SENS_ROW = 5            # shorter rows are there for the edges
SENS_FACTOR = 10.0


def path(name: str) -> str:
    return os.path.join(HERE, f"nomic_{name}.npz")


def build(name: str, with_bf16: bool = True):
    from tests.nomic_ref import make_case
    shape, seed, std, lens, pooling = CASES[name]
    return make_case(shape, seed, std, lens, pooling, with_bf16=with_bf16)


def save(name: str, case: dict) -> None:
    np.savez_compressed(path(name), shape_name=np.array(case["shape_name"]), seed=np.int64(case["seed"]), std=np.float64(case["std"]),
                        ids=case["ids"].astype(np.int16), lens=case["lens"], pooling=np.array(case["pooling"]),
                        expected=case["expected"].astype(np.float32), bf16_cos=np.float64(case["bf16_cos"]),
                        bf16_abs=np.float64(case["bf16_abs"]), bar_cos=np.float64(case["bar_cos"]), bar_abs=np.float64(case["bar_abs"]))


def load(name: str) -> dict:
    z = np.load(path(name))
    d = {k: z[k] for k in z.files}
    d["shape_name"], d["pooling"] = str(d["shape_name"]), str(d["pooling"])
    d["ids"] = d["ids"].astype(np.int32)
    d["seed"] = int(d["seed"])
    for k in ("std", "bf16_cos", "bf16_abs", "bar_cos", "bar_abs"):
        d[k] = float(d[k])
    return d


def sensitivity_ok(case: dict, sens: dict):
    """-> (ok, text): every row of at least MIN_SENS_ROW tokens moves by >= 10x the fixture's 1 - cos bar under every ablation."""
    rows = np.asarray(case["lens"]) >= MIN_SENS_ROW
    need = SENS_FACTOR * case["bar_cos"]
    worst = {k: float(np.asarray(v)[rows].min()) for k, v in sens.items()}
    return all(v >= need for v in worst.values()), f"need {need:.3g}: " + ", ".join(f"{k} min {v:.3g}" for k, v in worst.items())


if __name__ == "__main__":
    from tests.nomic_ref import sensitivities
    for name in (sys.argv[1:] or CASES):
        case = build(name)
        text = ""
        if case["pooling"] == "mean":
            ok, text = sensitivity_ok(case, sensitivities(case["shape_name"], case["seed"], case["std"], case["ids"], case["lens"],
                                                          case["pooling"], case["expected"]))
            text = "; " + text + ("; ok" if ok else "; NOT SENSITIVE ENOUGH")
        print(f"{name}: bf16 self-error 1 - cos {case['bf16_cos']:.3g} max |d| {case['bf16_abs']:.3g}; bar {case['bar_cos']:.3g} / "
              f"{case['bar_abs']:.3g}{text}", flush=True)
        save(name, case)
