"""Torch-facing wrappers for the MXFP8 wire kernels (csrc/kernels/wire_quant.hip).

Calls straight into libdlnb.so on torch's current HIP stream; as for
ops.gemm and ops.stream there is no fallback to a PyTorch path.

Wire format (OCP MX v1.0, MXFP8 E4M3; csrc/include/dlnb/wire_quant.hpp): a
message of n bf16 elements is padded with zeros to np = round_up(n, 32) and
travels as np e4m3 bytes, np / 32 e8m0 scale bytes and zero padding up to a
multiple of 16 bytes. ``mx_reference`` is the same format written in plain
torch from that definition: the tests' yardstick, not a code path.
"""
from __future__ import annotations

from .. import _native

BLOCK = 32


def padded(n: int) -> int:
    return (n + BLOCK - 1) // BLOCK * BLOCK


def wire_bytes(n: int) -> int:
    """Bytes of the wire block of a message of n bf16 elements."""
    return int(_native.lib().dlnb_mx_wire_bytes(int(n)))


def _stream(t):
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def _check(t, dtype, name):
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def mx_quantize(src, wire, block_elems: int = 0, nblocks: int = 1, n_total: int = -1):
    """Quantize `nblocks` message blocks of `block_elems` bf16 elements of src into wire (uint8).

    Message block j covers src[j * block_elems ...]; elements at index >=
    n_total (default: all of src) and anything beyond block_elems inside the
    padded block read as zero. Block j is written to
    wire[j * wire_bytes(block_elems) ...], padding bytes included.
    block_elems = 0: one block of src.numel() elements."""
    import torch
    _check(src, torch.bfloat16, "src")
    _check(wire, torch.uint8, "wire")
    n_total = src.numel() if n_total < 0 else n_total
    block_elems = block_elems or n_total
    if n_total > src.numel():
        raise ValueError("n_total exceeds src")
    if wire.numel() < nblocks * wire_bytes(block_elems):
        raise ValueError(f"wire holds {wire.numel()} bytes, {nblocks * wire_bytes(block_elems)} needed")
    _native.check(_native.lib().dlnb_mx_quantize(src.data_ptr(), n_total, block_elems, nblocks, wire.data_ptr(),
                                                 _stream(src)))
    return wire


def mx_dequantize(wire, dst, block_elems: int = 0, nblocks: int = 1, n_total: int = -1):
    """The inverse of mx_quantize: writes dst[i] (bf16) for i < n_total (default: all of dst) only."""
    import torch
    _check(wire, torch.uint8, "wire")
    _check(dst, torch.bfloat16, "dst")
    n_total = dst.numel() if n_total < 0 else n_total
    block_elems = block_elems or n_total
    if n_total > dst.numel():
        raise ValueError("n_total exceeds dst")
    if wire.numel() < nblocks * wire_bytes(block_elems):
        raise ValueError(f"wire holds {wire.numel()} bytes, {nblocks * wire_bytes(block_elems)} needed")
    _native.check(_native.lib().dlnb_mx_dequantize(wire.data_ptr(), block_elems, nblocks, dst.data_ptr(), n_total,
                                                   _stream(dst)))
    return dst


def mx_dequant_reduce(wire, dst, block_elems: int, nblocks: int, n: int = -1):
    """dst[i] = bf16(sum over the nblocks wire blocks, in block order, fp32) for i < n (default block_elems)."""
    import torch
    _check(wire, torch.uint8, "wire")
    _check(dst, torch.bfloat16, "dst")
    n = block_elems if n < 0 else n
    if n > dst.numel() or n > block_elems:
        raise ValueError("n exceeds dst or the block")
    if wire.numel() < nblocks * wire_bytes(block_elems):
        raise ValueError(f"wire holds {wire.numel()} bytes, {nblocks * wire_bytes(block_elems)} needed")
    _native.check(_native.lib().dlnb_mx_dequant_reduce(wire.data_ptr(), block_elems, nblocks, dst.data_ptr(), n,
                                                       _stream(dst)))
    return dst


# ---- the format in plain torch (CPU or GPU tensors): the tests' yardstick


def mx_reference(x):
    """(payload uint8 [np], scale uint8 [np / 32]) of one message block x (bf16, 1-D).

    Per 32 elements: e = clamp(floor(log2(amax)) - 8, -127, 127) (amax == 0:
    -127), scale byte e + 127; payload rne_e4m3fn(clamp(x * 2^-e, -448, 448)).
    A block holding an Inf or a NaN gets scale 0xFF (its payload is
    unspecified; zeros here)."""
    import torch
    n = x.numel()
    np_ = padded(n)
    xf = torch.zeros(np_, dtype=torch.float32, device=x.device)
    xf[:n] = x.reshape(-1).float()
    b = xf.view(-1, BLOCK)
    finite = torch.isfinite(b).all(dim=1)
    amax = torch.where(torch.isfinite(b), b.abs(), torch.zeros_like(b)).amax(dim=1).double()
    # floor(log2(amax)) from frexp: amax = m * 2^ex, m in [0.5, 1)
    _, ex = torch.frexp(amax)
    e = torch.where(amax > 0, ex.to(torch.int64) - 1 - 8, torch.full_like(ex, -127, dtype=torch.int64))
    e = e.clamp(-127, 127)
    scaled = (b.double() * torch.pow(torch.tensor(2.0, dtype=torch.float64, device=x.device), -e.double()).unsqueeze(1))
    scaled = torch.where(finite.unsqueeze(1), scaled, torch.zeros_like(scaled)).clamp(-448.0, 448.0).float()
    payload = scaled.to(torch.float8_e4m3fn).view(torch.uint8).reshape(-1)
    scale = torch.where(finite, e + 127, torch.full_like(e, 0xFF)).to(torch.uint8)
    return payload, scale


def mx_reference_wire(x, block_elems: int = 0, nblocks: int = 1):
    """The whole wire (uint8) of nblocks message blocks of x, as mx_quantize lays it out."""
    import torch
    block_elems = block_elems or x.numel()
    wb = wire_bytes(block_elems)
    np_ = padded(block_elems)
    out = torch.zeros(nblocks * wb, dtype=torch.uint8, device=x.device)
    flat = x.reshape(-1)
    for j in range(nblocks):
        blk = flat[j * block_elems:min((j + 1) * block_elems, flat.numel())]
        full = torch.zeros(block_elems, dtype=torch.bfloat16, device=x.device)
        full[:blk.numel()] = blk
        p, s = mx_reference(full)
        out[j * wb:j * wb + np_] = p
        out[j * wb + np_:j * wb + np_ + np_ // BLOCK] = s
    return out


def mx_reference_products(wire, block_elems: int, nblocks: int = 1):
    """float32 [nblocks, block_elems]: float(e4m3) * 2^e of every element of the wire blocks (NaN for scale 0xFF)."""
    import torch
    wb = wire_bytes(block_elems)
    np_ = padded(block_elems)
    rows = []
    for j in range(nblocks):
        w = wire[j * wb:(j + 1) * wb]
        q = w[:np_].view(torch.float8_e4m3fn).float().view(-1, BLOCK)
        sb = w[np_:np_ + np_ // BLOCK].to(torch.int64)
        mult = torch.pow(torch.tensor(2.0, dtype=torch.float64, device=wire.device), (sb - 127).double()).float()
        mult = torch.where(sb == 0xFF, torch.full_like(mult, float("nan")), mult)
        rows.append((q * mult.unsqueeze(1)).reshape(-1)[:block_elems])
    return torch.stack(rows)


def mx_reference_dequant(wire, block_elems: int, nblocks: int = 1):
    """bf16 [nblocks * block_elems]: bf16(float(e4m3) * 2^e)."""
    import torch
    return mx_reference_products(wire, block_elems, nblocks).to(torch.bfloat16).reshape(-1)


def mx_reference_dequant_reduce(wire, block_elems: int, nblocks: int):
    """bf16 [block_elems]: the products of blocks 0, 1, ... added in that order in fp32, rounded once."""
    import torch
    p = mx_reference_products(wire, block_elems, nblocks)
    acc = p[0].clone()
    for r in range(1, nblocks):
        acc = acc + p[r]
    return acc.to(torch.bfloat16)
