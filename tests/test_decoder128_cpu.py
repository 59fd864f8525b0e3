"""CPU tests of what the three head-128 decoder families share on the Python side (archi_amd/_decoder128.py behind decoder.py,
llama.py and qwen2.py): the seeded generators draw what they drew when the committed fixtures were computed, and each family's
weight order is the header's."""
import hashlib
import json
import os

import numpy as np
import pytest

from archi_amd import decoder, llama, qwen2

DIGESTS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "decoder_family_weight_digests.json")))
FAMILIES = {"qwen3-tiny-g2": (decoder, decoder.random_qwen3_weights, decoder.QWEN3_SHAPES),
            "ll-tiny-g2": (llama, llama.random_llama_weights, llama.LLAMA_SHAPES),
            "q2-tiny-g5": (qwen2, qwen2.random_qwen2_weights, qwen2.QWEN2_SHAPES)}


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_seeded_weights_are_the_recorded_draws(name):
    """SHA-256 over the float32 bytes of the weights in weight_order, recorded before the generators were merged: one torch generator
    per call, embed_tokens, norm, then per layer the keys in LAYER_KEYS order. A reordered draw changes every fixture's weights."""
    mod, gen, shapes = FAMILIES[name]
    assert set(DIGESTS) == set(FAMILIES)
    w = gen(name, seed=DIGESTS[name]["seed"])
    order = mod.weight_order(shapes[name][2])
    assert list(w) == order
    h = hashlib.sha256()
    for n in order:
        assert w[n].dtype == np.float32
        h.update(np.ascontiguousarray(w[n]).tobytes())
    assert h.hexdigest() == DIGESTS[name]["sha256"]


@pytest.mark.parametrize("mod,per_layer,optional", [(decoder, 11, ("q_norm", "k_norm")), (llama, 9, ()), (qwen2, 12, ("bq", "bk", "bv"))],
                         ids=["qwen3", "llama", "qwen2"])
def test_pointer_counts_and_optional_keys(mod, per_layer, optional):
    """2 + per_layer * L names, and a family's optional pointers directly after wv (csrc/decoder128.h LlFeatures' order)."""
    plain = ("wq", "wk", "wv", "wo", "ln_in", "ln_post", "w_gate", "w_up", "w_down")
    assert tuple(mod.LAYER_KEYS) == plain[:3] + optional + plain[3:]
    assert tuple(mod.HF_LAYER_NAMES) == tuple(mod.LAYER_KEYS)
    for L in (1, 3):
        order = mod.weight_order(L)
        assert len(order) == 2 + per_layer * L and len(set(order)) == len(order)
        assert order[:2] == ["embed_tokens", "norm"]
        for l in range(L):
            assert order[2 + per_layer * l: 2 + per_layer * (l + 1)] == [f"l{l}.{k}" for k in mod.LAYER_KEYS]
