"""GPU tests of the head-128 decoder stack as one implementation behind three ABIs (csrc/decoder128.hip; ak_decoder_*, ak_llama_*,
ak_qwen2_*): the same weights give the same bits through ak_llama_* and ak_qwen2_*, and ak_decoder_create refuses what the shared
config check refuses."""
import ctypes

import numpy as np
import pytest

from archi_amd.llama import LLAMA_SHAPES, random_llama_weights
from archi_amd.qwen2 import Qwen2Shape

pytestmark = pytest.mark.gpu


def test_llama_and_qwen2_abis_run_one_loop(hip):
    """ll-tiny-g2 with seeded Llama weights through HipLlama, and the same weights plus all-zero q / k / v biases through HipQwen2:
    B = 3, S = 96, lens (96, 1, 37), causal + last, causal + mean, bidirectional + mean. The same kernels on the same operands in the
    same order (a zero bias vector in place of the stack's zero_bias): equal bits."""
    from archi_amd.llama import HipLlama
    from archi_amd.qwen2 import HipQwen2
    ls = LLAMA_SHAPES["ll-tiny-g2"]
    assert ls.window == 0 and ls.scaling is None and (ls.hidden, ls.layers, ls.q_heads, ls.kv_heads) == (256, 3, 4, 2)
    w = random_llama_weights("ll-tiny-g2", seed=21, std=0.05)
    wb = dict(w)
    for l in range(ls.layers):
        for k, n in (("bq", ls.q_heads), ("bk", ls.kv_heads), ("bv", ls.kv_heads)):
            wb[f"l{l}.{k}"] = np.zeros(n * 128, np.float32)
    S, lens = 96, np.array([96, 1, 37], np.int32)
    ids = np.random.default_rng(5).integers(0, ls.vocab, (3, S)).astype(np.int32)
    for attention, pooling in (("causal", "last"), ("causal", "mean"), ("bidirectional", "mean")):
        a = HipLlama(ls._replace(attention=attention), w, device=0)
        b = HipQwen2(Qwen2Shape(*ls[:9], attention=attention), wb, device=0)
        got_a = a.forward(ids, lens, pooling=pooling, S=S).cpu().numpy()
        got_b = b.forward(ids, lens, pooling=pooling, S=S).cpu().numpy()
        a.close()
        b.close()
        assert np.isfinite(got_a).all() and np.abs(got_a).max() > 0
        assert np.array_equal(got_a, got_b), (attention, pooling)


@pytest.mark.parametrize("field", ["hidden", "intermediate"])
def test_decoder_create_refuses_a_zero_size(hip, field):
    """hidden = 0 and intermediate = 0 pass `% 128` and `% 64`: the shared check's positive-size rule refuses them under ak_decoder_create's
    name, before any weight is read and without a forward. Largest matrix of the shape: embed_tokens, 1000 x 256 bf16 = 500 KiB."""
    from archi_amd import _lib
    from archi_amd._lib import AkDecoderConfig
    sizes = dict(vocab_size=1000, hidden=256, layers=1, q_heads=2, kv_heads=2, head_dim=128, intermediate=512, max_position=8192)
    sizes[field] = 0
    cfg = AkDecoderConfig(sizes["vocab_size"], sizes["hidden"], sizes["layers"], sizes["q_heads"], sizes["kv_heads"], sizes["head_dim"],
                          sizes["intermediate"], sizes["max_position"], 1e-6, 1e6)
    import torch
    n = 2 + 11 * sizes["layers"]
    room = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")       # every pointer: room for the largest matrix of the shape
    ptrs = (ctypes.c_void_p * n)(*([room.data_ptr()] * n))
    h = ctypes.c_void_p()
    rc = hip.ak_decoder_create(ctypes.byref(cfg), ptrs, n, ctypes.byref(h))
    assert rc != 0 and not h.value
    assert _lib.last_error() == "ak_decoder_create: sizes must be positive"
