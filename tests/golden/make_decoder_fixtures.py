"""Regenerates tests/golden/decoder_*.npz: transformers.Qwen3Model in float32 on the CPU with the seeded weights of
archi_amd.decoder.random_qwen3_weights, each row alone, last-token pooling + L2 normalisation. No weights are stored: a fixture
holds the ids, the lengths, the expected embeddings, the shape name and the seed.

    python tests/golden/make_decoder_fixtures.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from archi_amd.decoder import QWEN3_SHAPES, random_qwen3_weights  # noqa: E402
from tests.decoder_ref import hf_model, reference  # noqa: E402

# (file tag, shape, seed, S, lengths): GQA ratios 1, 2 and 4; ragged lengths inside one tile including 1 and S; one 2048-token row
FIXTURES = [
    ("g1_B6_S64", "qwen3-tiny-g1", 11, 64, [1, 64, 17, 33, 32, 5]),
    ("g2_B5_S96", "qwen3-tiny-g2", 12, 96, [96, 1, 50, 95, 31]),
    ("g4_B4_S128", "qwen3-tiny-g4", 13, 128, [128, 64, 1, 77]),
    ("g2_B2_S2048", "qwen3-tiny-g2", 14, 2048, [2048, 300]),
]


def main():
    for tag, shape, seed, S, lens in FIXTURES:
        w = random_qwen3_weights(shape, seed=seed)
        vocab = QWEN3_SHAPES[shape][0]
        rng = np.random.default_rng(seed)
        lens = np.asarray(lens, np.int32)
        ids = np.zeros((len(lens), S), np.int32)
        for i, n in enumerate(lens):
            ids[i, :n] = rng.integers(1, vocab, n)
        want = reference(hf_model(shape, w), ids, lens)
        path = os.path.join(HERE, f"decoder_{tag}.npz")
        np.savez_compressed(path, ids=ids, lens=lens, expected=want, shape=np.array(shape), seed=np.array(seed))
        print(path, want.shape)


if __name__ == "__main__":
    main()
