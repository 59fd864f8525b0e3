"""Regenerates tests/golden/xlmr_tokenizer.json (a small Unigram tokenizer trained with `tokenizers`, XLM-R's special-token layout)
and tests/golden/xlmr_*.npz: transformers.XLMRobertaModel in float32 on the CPU with the seeded bf16-exact weights of
archi_amd.encoder.random_xlmr_weights, pooling + L2 normalisation. No weights are stored: a fixture holds the ids (XLM-R's pad id past
each length; some rows hold the pad id inside them, as a text with a literal <pad> is tokenised), the lengths, the pooling, the
expected embeddings, the shape name and the seed.

    python tests/golden/make_xlmr_fixtures.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from archi_amd.encoder import XLMR_SHAPES  # noqa: E402
from tests.xlmr_ref import PAD_ID, TOKENIZER_JSON, hf_embed, hf_model, make_tokenizer_json, pad_rows  # noqa: E402

# (file tag, shape, seed, S, lengths, pooling, pad ids inside rows): head size 64 and 32, ragged lengths including 1 and S, one
# 512-token row, rows with the pad id inside them
FIXTURES = [
    ("hd64_B5_S96", "xlmr-tiny-hd64", 51, 96, [96, 1, 40, 95, 33], "cls", True),
    ("hd64_B2_S512", "xlmr-tiny-hd64", 52, 512, [512, 200], "mean", True),
    ("hd32_B6_S64", "xlmr-tiny-hd32", 53, 64, [1, 64, 17, 33, 32, 5], "mean", True),
    ("hd32_B3_S256", "xlmr-tiny-hd32", 54, 256, [256, 129, 7], "cls", False),
]


def main():
    make_tokenizer_json(TOKENIZER_JSON)
    print(TOKENIZER_JSON, os.path.getsize(TOKENIZER_JSON))
    for tag, shape, seed, S, lens, pooling, inner_pad in FIXTURES:
        model, _ = hf_model(shape, seed)
        vocab = XLMR_SHAPES[shape][0]
        rng = np.random.default_rng(seed)
        toks = [rng.integers(4, vocab, n).tolist() for n in lens]
        if inner_pad:                                        # a literal <pad> inside the longer rows (never the first token)
            for t in toks:
                if len(t) > 8:
                    for j in rng.choice(np.arange(1, len(t)), 2, replace=False):
                        t[j] = PAD_ID
        ids, mask = pad_rows(toks, S)
        want = hf_embed(model, ids, mask, pooling=pooling)
        path = os.path.join(HERE, f"xlmr_{tag}.npz")
        np.savez_compressed(path, ids=ids, lens=np.asarray(lens, np.int32), expected=want, shape=np.array(shape),
                            seed=np.array(seed), pooling=np.array(pooling))
        print(path, want.shape, os.path.getsize(path))


if __name__ == "__main__":
    main()
