"""Regenerates tests/golden/qwen2_*.npz: transformers.Qwen2Model in float32 on the CPU with eager attention and the seeded weights of
tests.qwen2_ref.fixture_weights (archi_amd.qwen2.random_qwen2_weights at the std and bias_std of tests.qwen2_ref.FIXTURES), each row
alone, last-token or mean pooling + L2 normalisation (bidirectional fixtures: an explicit all-visible 4D mask). No weights are stored: a
fixture holds the ids, the lengths, the expected embeddings, the shape name, the seed, the two stds and its bar.

The bar of a fixture, per figure (1 - cos, max |d|): the larger of the bf16 encoder bar (3e-4 / 3e-3) and the error of the SAME HF model
run entirely in bf16 on the CPU against its float32 self. No margin. Both measured errors are stored beside the bar.

    python tests/golden/make_qwen2_fixtures.py [name ...]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.qwen2_ref import ABS_BAR, COS_BAR, FIXTURES, MODES, fixture_inputs, fixture_weights, hf_model, reference  # noqa: E402


def main():
    import torch
    for name in sys.argv[1:] or FIXTURES:
        shape, seed, ids, lens, std, bias_std = fixture_inputs(name)
        w = fixture_weights(name)
        attention, pooling = MODES.get(name, ("causal", "last"))
        want = reference(hf_model(shape, w), ids, lens, attention=attention, pooling=pooling)
        low = reference(hf_model(shape, w, dtype=torch.bfloat16), ids, lens, attention=attention, pooling=pooling)
        cos = (want * low).sum(1) / (np.linalg.norm(want, axis=1) * np.linalg.norm(low, axis=1))
        bf16_cos, bf16_abs = float((1 - cos).max()), float(np.abs(want - low).max())
        path = os.path.join(HERE, f"qwen2_{name}.npz")
        np.savez_compressed(path, ids=ids, lens=lens, expected=want, shape=np.array(shape), seed=np.array(seed), std=np.array(std),
                            bias_std=np.array(bias_std), attention=np.array(attention), pooling=np.array(pooling), bf16_cos=np.array(bf16_cos),
                            bf16_abs=np.array(bf16_abs), cos_bar=np.array(max(COS_BAR, bf16_cos)), abs_bar=np.array(max(ABS_BAR, bf16_abs)))
        print(f"{path} {want.shape}: HF bf16 against float32 1 - cos {bf16_cos:.2e}, max |d| {bf16_abs:.2e}", flush=True)


if __name__ == "__main__":
    main()
