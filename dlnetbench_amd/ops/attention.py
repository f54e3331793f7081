"""Torch-facing wrapper for the fused attention forward kernels (csrc/kernels/attention.hip, attention_fp8.hip).

Calls straight into libdlnb.so on torch's current HIP stream; as for
ops.gemm and ops.stream there is no fallback to a PyTorch path.
"""
from __future__ import annotations

import math

from .. import _native

HEAD_DIM = 128


def kv_tile() -> int:
    """Keys per KV-tile step, the kernel's unit of work (kernels::kAttnKvTile)."""
    return int(_native.lib().dlnb_attn_kv_tile())


def step_flops() -> float:
    """FLOPs of one KV-tile step: both products of a 128-row Q tile with kv_tile() keys."""
    return 4.0 * 128 * kv_tile() * HEAD_DIM


def attention_fwd(q, k, v, out=None, lse=None, causal: bool = False, scale: float | None = None, us: float = 0.0,
                  grid: int = 0, totals=None, per_block=None, start=None, v_scale: float = 1.0):
    """out = v_scale softmax(scale q k^T (+ causal mask)) v, with fp32 scores, softmax and accumulation.

    q: [B, H, Sq, 128], k and v: [B, Hkv, Skv, 128], contiguous CUDA tensors
    of one dtype: bf16 (attention.hip), or float8_e4m3fn (attention_fp8.hip:
    both products on the fp8 MFMA, P quantized to e4m3 in registers; fold the
    Q and K descales into scale and pass V's as v_scale, which bf16 inputs do
    not take). H % Hkv == 0 (query head h reads KV head h // (H // Hkv)); Sq and
    Skv multiples of 128; causal needs Sq == Skv. scale defaults to
    1 / sqrt(128). out (bf16, q's shape) and lse (fp32 [B, H, Sq], the natural
    log of each row's sum of exp(scaled scores)) are written when given; out
    is allocated otherwise. us = 0 computes every 128-row Q tile once; us > 0
    keeps recomputing them (wrapping round) for `us` microseconds of the device
    clock. grid: blocks, one per CU (0 = every CU, at most the CUs); block i
    takes Q tiles i, i + grid, ... totals (optional): int64 CUDA tensor of >= 2
    words the kernel ADDS {KV-tile steps, ticks requested} to. per_block
    (optional): int64 CUDA tensor of >= grid words, word i = block i's steps.
    start (optional): (int64 CUDA tensor, index) that receives the kernel's
    start (s_memrealtime ticks). Shapes the kernel does not serve raise
    NativeError."""
    import torch
    fp8 = q.dtype == getattr(torch, "float8_e4m3fn", None)
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dtype != q.dtype or not (fp8 or t.dtype == torch.bfloat16):
            raise TypeError(f"unsupported dtype {t.dtype} of {name}")
        if t.dim() != 4 or t.shape[-1] != HEAD_DIM:
            raise ValueError(f"{name} must be [B, heads, S, {HEAD_DIM}]")
        if not t.is_contiguous():
            raise ValueError("q, k and v must be contiguous")
    B, H, Sq, _ = q.shape
    if k.shape != v.shape or k.shape[0] != B:
        raise ValueError("k and v must have the same shape and q's batch size")
    Hkv, Skv = k.shape[1], k.shape[2]
    if not fp8 and v_scale != 1.0:
        raise ValueError("v_scale belongs to float8_e4m3fn inputs")
    if out is None:
        out = torch.empty(q.shape, device=q.device, dtype=torch.bfloat16)
    if out.dtype != torch.bfloat16 or out.shape != q.shape or not out.is_contiguous():
        raise ValueError("out must be a contiguous bf16 tensor of q's shape")
    if lse is not None and (lse.dtype != torch.float32 or tuple(lse.shape) != (B, H, Sq) or not lse.is_contiguous()):
        raise ValueError("lse must be a contiguous float32 tensor of shape [B, H, Sq]")
    for name, w, least in (("totals", totals, 2), ("per_block", per_block, max(grid, 1))):
        if w is not None and (w.dtype != torch.int64 or w.numel() < least):
            raise ValueError(f"{name} must be an int64 tensor of >= {least} elements")
    if per_block is not None and grid <= 0:
        raise ValueError("per_block needs an explicit grid")
    sp = start[0].data_ptr() + 8 * start[1] if start is not None else None
    head = (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr() if lse is not None else None,
            B, H, Hkv, Sq, Skv, float(scale if scale is not None else 1.0 / math.sqrt(HEAD_DIM)))
    tail = (int(bool(causal)), float(us), q.device.index or 0, grid, torch.cuda.current_stream(q.device).cuda_stream, sp,
            totals.data_ptr() if totals is not None else None, per_block.data_ptr() if per_block is not None else None)
    if fp8:
        _native.check(_native.lib().dlnb_attention_fwd_fp8(*head, float(v_scale), *tail))
    else:
        _native.check(_native.lib().dlnb_attention_fwd(*head, *tail))
    return out
