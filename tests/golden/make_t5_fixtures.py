"""Writes tests/golden/t5_*.npz from transformers.T5EncoderModel (float32, eager attention, CPU) and the project's seeded weights:
python tests/golden/make_t5_fixtures.py. Each file holds shape name, seed, std, bias std, ids, lens, pooling, the expected embeddings,
the error of the all-bf16 T5EncoderModel against its float32 self on those rows, and the bar of the GPU test: per figure the larger of
the project's bf16 bar and that error (tests/t5_ref.py). The weights come from the seed and are not stored.

Every fixture must show, on every mean-pooled row of at least 5 tokens, a sensitivity of at least 10x its own 1 - cos bar to each of
tests/t5_ref.MUTANTS (clamp_half: on every row longer than D + 64; tests/test_t5_cpu.py asserts it from T5EncoderModel alone). Where a
std did not give that the std was changed, not the factor; the figures measured while choosing them are in docs/EXPERIMENTS.md.
With 8 buckets and D = 16 (tiny_d16) the last bucket of a side starts at distance 6: clamping at D / 2 = 8 changes no table entry,
that mutant IS the model and t5_ref.sensitivities leaves it out there."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

EDGE_LENS = [320, 200, 129, 64, 33, 5, 1]


def _base_lens():
    """24 rows of up to 512 tokens: as one tile the QKV and feed-forward GEMMs of the layer run on the wide phased tile."""
    return [512, 511, 257, 130, 65, 33, 5] + [int(n) for n in np.random.RandomState(5).randint(200, 513, size=17)]


# name -> (shape, seed, std, bias std, lens, pooling)
CASES = {
    "tiny_relu": ("t5-tiny-relu", 31, 0.1, 4.0, EDGE_LENS, "mean"),
    "tiny_gated": ("t5-tiny-gated", 32, 0.05, 2.0, EDGE_LENS, "mean"),
    "tiny_long": ("t5-tiny-gated", 41, 0.05, 4.0, [1100, 300, 65], "mean"),
    "tiny_d16": ("t5-tiny-d16", 33, 0.05, 4.0, [160, 129, 97, 33, 5], "mean"),
    "base_cut2": ("t5-base-cut2", 43, 0.035, 8.0, _base_lens(), "mean"),
}
MIN_SENS_ROW = 5            # shorter rows are there for the edges
SENS_FACTOR = 10.0


def path(name: str) -> str:
    return os.path.join(HERE, f"t5_{name}.npz")


def build(name: str):
    from tests.t5_ref import make_case
    shape, seed, std, bias_std, lens, pooling = CASES[name]
    return make_case(shape, seed, std, bias_std, lens, pooling)


def save(name: str, case: dict) -> None:
    np.savez_compressed(path(name), shape_name=np.array(case["shape_name"]), seed=np.int64(case["seed"]), std=np.float64(case["std"]),
                        bias_std=np.float64(case["bias_std"]), ids=case["ids"].astype(np.int16), lens=case["lens"],
                        pooling=np.array(case["pooling"]), expected=case["expected"].astype(np.float32), bf16_cos=np.float64(case["bf16_cos"]),
                        bf16_abs=np.float64(case["bf16_abs"]), bar_cos=np.float64(case["bar_cos"]), bar_abs=np.float64(case["bar_abs"]))


def load(name: str) -> dict:
    z = np.load(path(name))
    d = {k: z[k] for k in z.files}
    d["shape_name"], d["pooling"] = str(d["shape_name"]), str(d["pooling"])
    d["ids"] = d["ids"].astype(np.int32)
    d["seed"] = int(d["seed"])
    for k in ("std", "bias_std", "bf16_cos", "bf16_abs", "bar_cos", "bar_abs"):
        d[k] = float(d[k])
    return d


def sensitivity_ok(case: dict, sens: dict):
    """-> (ok, text): every row of at least MIN_SENS_ROW tokens moves by >= 10x the fixture's 1 - cos bar under every mutant;
    clamp_half is asked of the rows longer than D + 64 only (shorter rows hold few or no pairs beyond D / 2)."""
    from archi_amd.t5 import T5_SHAPES
    lens = np.asarray(case["lens"])
    D = T5_SHAPES[case["shape_name"]][8]
    need = SENS_FACTOR * case["bar_cos"]
    worst = {}
    for k, v in sens.items():
        rows = (lens > D + 64) if k == "clamp_half" else (lens >= MIN_SENS_ROW)
        rows &= ~np.isnan(np.asarray(v))
        if rows.any():
            worst[k] = float(np.asarray(v)[rows].min())
    return all(v >= need for v in worst.values()), f"need {need:.3g}: " + ", ".join(f"{k} min {v:.3g}" for k, v in worst.items())


if __name__ == "__main__":
    from tests.t5_ref import sensitivities
    for name in (sys.argv[1:] or CASES):
        case = build(name)
        ok, text = sensitivity_ok(case, sensitivities(case))
        print(f"{name}: bf16 self-error 1 - cos {case['bf16_cos']:.3g} max |d| {case['bf16_abs']:.3g}; bar {case['bar_cos']:.3g} / "
              f"{case['bar_abs']:.3g}; {text}{'; ok' if ok else '; NOT SENSITIVE ENOUGH'}", flush=True)
        save(name, case)
