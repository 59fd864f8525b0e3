"""GPU tests of what the four stacks share (csrc/stack.h, archi_amd/_stack.py), on the tiny shapes: the workspace that
regrows between calls, and the zero padding of an intermediate size off the wide GEMM tile. Both compare bit for bit, so there is no
tolerance to choose."""
import numpy as np
import pytest

from archi_amd.decoder import QWEN3_SHAPES, HipDecoder, random_qwen3_weights
from archi_amd.gemma import GEMMA_SHAPES, HipGemma, random_gemma_weights
from archi_amd.modernbert import MODERNBERT_SHAPES, HipModernBert, random_modernbert_weights
from archi_amd.nomic import NOMIC_SHAPES, HipNomicBert, random_nomic_weights

pytestmark = pytest.mark.gpu

FAMILIES = {
    "qwen3-tiny-g2": (HipDecoder, QWEN3_SHAPES, lambda s: random_qwen3_weights(s, seed=11)),
    "modernbert-tiny-mix": (HipModernBert, MODERNBERT_SHAPES, lambda s: random_modernbert_weights(s, seed=12, std=0.1)),
    "gm-tiny": (HipGemma, GEMMA_SHAPES, lambda s: random_gemma_weights(s, seed=13, std=0.1)),
    "nomic-tiny-mean": (HipNomicBert, NOMIC_SHAPES, lambda s: random_nomic_weights(s, seed=14, std=0.1)),
}


def _ids(vocab, seed, lens, width):
    rng = np.random.RandomState(seed)
    ids = np.zeros((len(lens), width), np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.randint(3, vocab, size=n)
    return ids, np.asarray(lens, np.int32)


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_workspace_regrows(hip, name):
    """(B 2, S 32), then (B 5, S 96), then the first call again on one handle: with 256-row tiles 256 token rows, then 512 (and more
    rows), then 256 inside the grown workspace. The repeat equals the first call, and the larger call equals a fresh handle's."""
    cls, shapes, weights = FAMILIES[name]
    shape = shapes[name]
    w = weights(shape)
    small = _ids(shape[0], 1, [32, 7], 32)
    large = _ids(shape[0], 2, [96, 1, 33, 64, 50], 96)
    m = cls(shape, w, device=0)
    first = m.forward(*small).cpu().numpy()
    second = m.forward(*large).cpu().numpy()
    third = m.forward(*small).cpu().numpy()
    m.close()
    fresh = cls(shape, w, device=0)
    want = fresh.forward(*large).cpu().numpy()
    fresh.close()
    assert first.shape == (2, m.out_dim) and second.shape == (5, m.out_dim)
    assert np.isfinite(first).all() and np.isfinite(second).all() and np.abs(second).max() > 0
    assert np.array_equal(first, third)
    assert np.array_equal(second, want)


def _zero_rows(a, n):
    return np.concatenate([a, np.zeros((n, a.shape[1]), a.dtype)], axis=0)


def _zero_cols(a, n):
    return np.concatenate([a, np.zeros((a.shape[0], n), a.dtype)], axis=1)


def _padded_modernbert():
    """modernbert-tiny-mix (I = 192: 2 I = 384 is off the 256-wide tile, the library pads to 256) and the same model given as I = 256:
    64 zero rows behind each half of every Wi, 64 zero columns behind every mlp_wo."""
    shape = MODERNBERT_SHAPES["modernbert-tiny-mix"]
    I, pad = shape[4], 256 - shape[4]
    assert I == 192
    w = random_modernbert_weights(shape, seed=21, std=0.1)
    wp = dict(w)
    for l in range(shape[2]):
        wi = w[f"l{l}.wi"]
        wp[f"l{l}.wi"] = np.concatenate([_zero_rows(wi[:I], pad), _zero_rows(wi[I:], pad)], axis=0)
        wp[f"l{l}.mlp_wo"] = _zero_cols(w[f"l{l}.mlp_wo"], pad)
    return HipModernBert, shape, w, shape[:4] + (256,) + shape[5:], wp


def _padded_gemma():
    """gm-tiny at intermediate 320 (2 I = 640: the library pads to 384) and the same model given as intermediate 384: zero gate / up
    rows, zero w_down columns."""
    tiny = GEMMA_SHAPES["gm-tiny"]
    shape, wide, pad = tiny[:6] + (320,) + tiny[7:], tiny[:6] + (384,) + tiny[7:], 64
    w = random_gemma_weights(shape, seed=22, std=0.1)
    wp = dict(w)
    for l in range(shape[2]):
        wp[f"l{l}.w_gate"], wp[f"l{l}.w_up"] = _zero_rows(w[f"l{l}.w_gate"], pad), _zero_rows(w[f"l{l}.w_up"], pad)
        wp[f"l{l}.w_down"] = _zero_cols(w[f"l{l}.w_down"], pad)
    return HipGemma, shape, w, wide, wp


def _padded_nomic():
    """nomic-tiny-mean (I = 192: the library pads 2 I = 384 to 512) and the same model given as I = 256: 64 zero rows behind every
    w_gate and w_up, 64 zero columns behind every w_down."""
    shape = NOMIC_SHAPES["nomic-tiny-mean"]
    I, pad = shape[4], 256 - shape[4]
    assert I == 192
    w = random_nomic_weights(shape, seed=23, std=0.1)
    wp = dict(w)
    for l in range(shape[2]):
        wp[f"l{l}.w_gate"], wp[f"l{l}.w_up"] = _zero_rows(w[f"l{l}.w_gate"], pad), _zero_rows(w[f"l{l}.w_up"], pad)
        wp[f"l{l}.w_down"] = _zero_cols(w[f"l{l}.w_down"], pad)
    return HipNomicBert, shape, w, shape[:4] + (256,) + shape[5:], wp


@pytest.mark.parametrize("family", [_padded_modernbert, _padded_gemma, _padded_nomic], ids=["modernbert", "gemma", "nomic"])
def test_library_padding_equals_explicit_zero_padding(hip, family):
    """The library must build the very matrices the test builds by hand: results are equal bit for bit."""
    cls, shape, w, shape_padded, w_padded = family()
    ids, lens = _ids(shape[0], 3, [1, 33, 96], 96)
    m = cls(shape, w, device=0)
    got = m.forward(ids, lens).cpu().numpy()
    m.close()
    m = cls(shape_padded, w_padded, device=0)
    want = m.forward(ids, lens).cpu().numpy()
    m.close()
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    assert np.array_equal(got, want)
