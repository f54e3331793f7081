"""Torch-facing wrapper for the HBM-streaming kernel (csrc/kernels/hbm_stream.hip).

Calls straight into libdlnb.so on torch's current HIP stream; as for
ops.gemm there is no fallback to a PyTorch path.
"""
from __future__ import annotations

from .. import _native


def chunk_bytes() -> int:
    """Bytes per array of the kernel's work unit (kernels::kHbmChunkBytes)."""
    return int(_native.lib().dlnb_hbm_chunk_bytes())


def stream_add(a, b, out, us: float = 0.0, grid: int = 0, totals=None, per_block=None, start=None):
    """out = a + b (bf16, fp32 math, one rounding) by a persistent grid of one block per CU.

    a, b, out: contiguous bf16 CUDA tensors of the same number of elements, a
    multiple of 8, 16-byte aligned. us = 0 sweeps the arrays once; us > 0 keeps
    sweeping (wrapping round) for `us` microseconds of the device clock. grid:
    blocks (0 = every CU, at most the CUs); block i takes chunks i, i + grid, ...
    of chunk_bytes() per array. totals (optional): int64 CUDA tensor of >= 2
    words the kernel ADDS {chunks processed, ticks requested} to. per_block
    (optional): int64 CUDA tensor of >= grid words, word i = block i's chunk
    count. start (optional): (int64 CUDA tensor, index) that receives the
    kernel's start (s_memrealtime ticks)."""
    import torch
    for t in (a, b, out):
        if t.dtype != torch.bfloat16:
            raise TypeError(f"unsupported dtype {t.dtype}")
        if not t.is_contiguous():
            raise ValueError("a, b and out must be contiguous")
    n = a.numel()
    if b.numel() != n or out.numel() != n:
        raise ValueError("a, b and out must have the same number of elements")
    for name, w, least in (("totals", totals, 2), ("per_block", per_block, max(grid, 1))):
        if w is not None and (w.dtype != torch.int64 or w.numel() < least):
            raise ValueError(f"{name} must be an int64 tensor of >= {least} elements")
    if per_block is not None and grid <= 0:
        raise ValueError("per_block needs an explicit grid")
    sp = start[0].data_ptr() + 8 * start[1] if start is not None else None
    _native.check(_native.lib().dlnb_hbm_stream(
        a.data_ptr(), b.data_ptr(), out.data_ptr(), n, float(us), a.device.index or 0, grid,
        torch.cuda.current_stream(a.device).cuda_stream, sp,
        totals.data_ptr() if totals is not None else None,
        per_block.data_ptr() if per_block is not None else None))
    return out
