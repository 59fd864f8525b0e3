"""Regenerates tests/golden/mpnet_*.npz: transformers.MPNetModel in float32 on the CPU with the seeded weights of
archi_amd.encoder.random_mpnet_weights (relative-position bias weights of magnitude ~1), mean pooling + L2 normalisation. No
weights are stored: a fixture holds the ids (MPNet's pad id past each length), the lengths, the expected embeddings, the shape
name and the seed.

    python tests/golden/make_mpnet_fixtures.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from archi_amd.encoder import MPNET_SHAPES  # noqa: E402
from tests.mpnet_ref import PAD_ID, hf_embed, hf_model, pad_rows  # noqa: E402

# (file tag, shape, seed, S, lengths): head size 64 (a 2-layer cut of the 768 shape: the all-mpnet-base-v2 layer) and 32; ragged
# lengths inside one tile including 1 and S; one 512-token row (distances up to 511, every bucket)
FIXTURES = [
    ("hd64_B5_S96", "mpnet-cut2", 21, 96, [96, 1, 40, 95, 33]),
    ("hd64_B2_S512", "mpnet-cut2", 22, 512, [512, 200]),
    ("hd32_B6_S64", "mpnet-tiny-hd32", 23, 64, [1, 64, 17, 33, 32, 5]),
    ("hd32_B3_S256", "mpnet-tiny-hd32", 24, 256, [256, 129, 7]),
]


def main():
    for tag, shape, seed, S, lens in FIXTURES:
        model, _ = hf_model(shape, seed)
        vocab = MPNET_SHAPES[shape][0]
        rng = np.random.default_rng(seed)
        toks = [rng.integers(PAD_ID + 4, vocab, n).tolist() for n in lens]   # no pad id inside a row
        ids, mask = pad_rows(toks, S)
        want = hf_embed(model, ids, mask, pooling="mean")
        path = os.path.join(HERE, f"mpnet_{tag}.npz")
        np.savez_compressed(path, ids=ids, lens=np.asarray(lens, np.int32), expected=want, shape=np.array(shape),
                            seed=np.array(seed))
        print(path, want.shape, os.path.getsize(path))


if __name__ == "__main__":
    main()
