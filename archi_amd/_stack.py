"""What the Python handles of the stacks share (HipDecoder, HipModernBert, HipGemma, HipNomicBert; csrc/stack.h is the library's side):
weight upload, the pointer array, create / close, the pooling rule, the tile layout of forward_lens and its validation, forward. Also
the safetensors directory reader and the seeded weight generators of the families' loaders.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Iterable, Optional

import numpy as np

from . import _lib
from ._lib import POOLING, HipBackendError, check


def read_safetensors_dir(model_dir: str) -> Dict[str, "object"]:
    """model.safetensors or sharded model-*.safetensors of a local checkpoint directory -> {tensor name: torch tensor}. A "model."
    prefix on the tensor names is stripped. No network."""
    from safetensors.torch import load_file     # torch loader: bf16 checkpoints load too
    files = sorted(f for f in os.listdir(model_dir) if f.endswith(".safetensors"))
    if not files:
        raise FileNotFoundError(f"{model_dir}: no *.safetensors file")
    sd = {}
    for f in files:
        sd.update(load_file(os.path.join(model_dir, f)))
    return {(k[6:] if k.startswith("model.") else k): v for k, v in sd.items()}


def seeded_mat_vec(seed: int, std: float = 0.02, vec_mean: float = 1.0):
    """(mat, vec) drawing from one torch generator seeded with `seed`: mat(r, c, s=std) a matrix of std s ROUNDED TO bf16 (kept as
    float32 values: the released checkpoints are bf16, and a float32 reference on the same values measures the kernels' activation
    rounding alone); vec(n) a norm weight drawn around vec_mean with std 0.1, not set to it."""
    import torch
    g = torch.Generator().manual_seed(seed)

    def mat(r, c, s=std):
        return (torch.randn(r, c, generator=g) * s).to(torch.bfloat16).float().numpy()

    def vec(n):
        v = 0.1 * torch.randn(n, generator=g)
        return (vec_mean + v if vec_mean else v).numpy().astype(np.float32)

    return mat, vec


class HipStack:
    """Base of the four handles. PyTorch-ROCm only HOLDS the weights in HBM (bf16 matrices, fp32 vectors) and hands raw device
    pointers to the C ABI. A subclass states what differs:"""
    family = ""                 # as the "weight missing" message names the model family
    prefix = ""                 # the library symbols: ak_<prefix>_create / _destroy / _forward_lens
    embed_key = ""              # the embedding matrix: bf16 like every name whose last part is in matrix_keys
    matrix_keys = frozenset()
    abi_pooling = True          # ak_<prefix>_forward_lens takes a pooling argument
    out_name = "hidden"         # how forward_lens' message names the output width (self.out_dim)
    poolings = ("mean", "cls")  # what _pooling accepts; None stands for self.pooling, the model's own
    pooling_noun = ""           # as _pooling's message names the family: "<noun> pool 'mean' or 'cls'"

    def _upload(self, weights, names: Iterable[str], device: Optional[int]) -> None:
        """Binds the library and the device; the weights `names` (numpy arrays or torch tensors) -> self._tensors on the device."""
        import torch
        self._lib = _lib.init(device)
        self._dev = torch.device("cuda", _lib.bound_device())
        self._tensors = {}
        for name in names:
            if name not in weights:
                raise HipBackendError(f"{self.family} weight {name!r} missing")
            arr = weights[name]
            t = arr if isinstance(arr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(arr))
            is_matrix = name == self.embed_key or name.split(".")[-1] in self.matrix_keys
            self._tensors[name] = t.to(device=self._dev, dtype=torch.bfloat16 if is_matrix else torch.float32).contiguous()

    def _create(self, cfg, ptr_names: Iterable[str]) -> None:
        """ak_<prefix>_create on the config struct and the device pointers of `ptr_names`, in the header's order."""
        import torch
        self._ptrs = [self._tensors[n].data_ptr() for n in ptr_names]
        self._cfg = cfg
        h = ctypes.c_void_p()
        torch.cuda.synchronize(self._dev)
        fn = f"ak_{self.prefix}_create"
        check(getattr(self._lib, fn)(ctypes.byref(cfg), (ctypes.c_void_p * len(self._ptrs))(*self._ptrs), len(self._ptrs), ctypes.byref(h)), fn)
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            getattr(self._lib, f"ak_{self.prefix}_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _pooling(self, pooling: Optional[str]) -> str:
        """The pooling a call runs with; a ValueError for one the family does not implement."""
        pooling = pooling or self.pooling
        if pooling not in self.poolings:
            raise ValueError(f"pooling {pooling!r}: {self.pooling_noun} pool " + " or ".join(repr(p) for p in self.poolings))
        return pooling

    def forward_lens(self, stage, n_rows: int, S: int, out, pooling: Optional[str] = None, normalise: bool = True) -> None:
        """The provider's tile layout, as HipEncoder.forward_lens: `stage` an int32 CUDA tensor [n_rows, S + 1] (S ids per row,
        the length in column S), `out` a float32 CUDA tensor view [n_rows, out_dim]."""
        import torch
        pooling = self._pooling(pooling)
        if stage.dtype != torch.int32 or not stage.is_cuda or not stage.is_contiguous() or tuple(stage.shape) != (n_rows, S + 1):
            raise ValueError("forward_lens: stage must be a contiguous int32 CUDA tensor [n_rows, S + 1]")
        if out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (n_rows, self.out_dim):
            raise ValueError(f"forward_lens: out must be a contiguous float32 CUDA tensor [n_rows, {self.out_name}]")
        if S % 32 or S > self.max_seq:
            raise ValueError(f"sequence length {S} must be a multiple of 32, <= {self.max_seq}")
        base = stage.data_ptr()
        fn = f"ak_{self.prefix}_forward_lens"
        args = [self._h, ctypes.c_void_p(base), S + 1, ctypes.c_void_p(base + 4 * S), S + 1, n_rows, S]
        if self.abi_pooling:
            args.append(POOLING[pooling])
        check(getattr(self._lib, fn)(*args, int(normalise), ctypes.c_void_p(out.data_ptr()),
                                     ctypes.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream)), fn)

    def forward(self, ids, lens, pooling: Optional[str] = None, normalise: bool = True, S: Optional[int] = None):
        """ids [B, W] (row i holds lens[i] ids), lens [B] -> [B, out_dim] float32 CUDA tensor (one tile, S = W rounded up to 32
        unless given)."""
        import torch
        ids = np.asarray(ids, np.int32)
        B, W = ids.shape
        if S is None:
            S = max(32, (W + 31) // 32 * 32)
        stage = np.zeros((B, S + 1), np.int32)
        stage[:, :min(W, S)] = ids[:, :S]
        stage[:, S] = np.asarray(lens, np.int32)
        st = torch.from_numpy(stage).to(self._dev)
        out = torch.empty((B, self.out_dim), dtype=torch.float32, device=self._dev)
        self.forward_lens(st, B, S, out, pooling=pooling, normalise=normalise)
        return out
