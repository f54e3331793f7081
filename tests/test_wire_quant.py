"""--wire-quant mxfp8 without a GPU: the host implementation of the MXFP8 wire format against the torch
reference written from the format (ops.quant.mx_reference), bit for bit; commtest on the CPU backends; dp, fsdp
and the MoE hybrid with the quantizing communicator; the option's checks and the report block."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

from dlnetbench_amd import _native  # noqa: E402
from dlnetbench_amd.ops import quant  # noqa: E402
from dlnetbench_amd.utils import launch, report  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")
DLNB = os.path.join(BIN, "dlnb")
SIZES = [1, 31, 32, 33, 64, 1000, 4096 + 32]


def bits(t):
    return t.view(torch.int16)


def random_bf16(n, seed):
    """Uniform [-1, 1) times 2^k, k in [-12, 12]; a share of the blocks has its scaled amax in (448, 512)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, generator=g) * 2 - 1) * torch.pow(torch.tensor(2.0), torch.randint(-12, 13, (n,), generator=g).float())
    x[::97] = 0.0
    return x.to(torch.bfloat16)


def host_quantize(x, block=0, nblocks=1, n_total=-1):
    block = block or x.numel()
    n_total = x.numel() if n_total < 0 else n_total
    wire = torch.full((nblocks * quant.wire_bytes(block),), 0xAA, dtype=torch.uint8)
    _native.check(_native.lib().dlnb_mx_quantize_host(x.data_ptr(), n_total, block, nblocks, wire.data_ptr()))
    return wire


def host_dequantize(wire, block, nblocks=1, n_total=-1):
    n_total = block * nblocks if n_total < 0 else n_total
    dst = torch.full((block * nblocks,), float("nan"), dtype=torch.bfloat16)
    _native.check(_native.lib().dlnb_mx_dequantize_host(wire.data_ptr(), block, nblocks, dst.data_ptr(), n_total))
    return dst


def host_dequant_reduce(wire, block, nblocks, n=-1):
    n = block if n < 0 else n
    dst = torch.full((block,), float("nan"), dtype=torch.bfloat16)
    _native.check(_native.lib().dlnb_mx_dequant_reduce_host(wire.data_ptr(), block, nblocks, dst.data_ptr(), n))
    return dst


@pytest.mark.parametrize("n", SIZES + [100000, (1 << 21) + 5])
def test_wire_bytes_formula(n):
    np_ = (n + 31) // 32 * 32
    assert quant.wire_bytes(n) == (np_ + np_ // 32 + 15) // 16 * 16


@pytest.mark.parametrize("n", SIZES)
def test_host_quantize_and_dequantize_match_the_reference(n):
    x = random_bf16(n, 10 + n)
    ref = quant.mx_reference_wire(x)
    p, s = quant.mx_reference(x)
    np_ = quant.padded(n)
    assert torch.equal(ref[:np_], p) and torch.equal(ref[np_:np_ + np_ // 32], s) and not bool(ref[np_ + np_ // 32:].any())
    wire = host_quantize(x)
    assert torch.equal(wire, ref)  # payload, scales and the zero padding
    got = host_dequantize(wire, n)
    assert torch.equal(bits(got), bits(quant.mx_reference_dequant(ref, n)))


@pytest.mark.parametrize("block,nblocks,n_total", [(1000, 3, 3000), (1001, 3, 2500), (4096, 4, 33), (33, 5, 165)])
def test_host_message_blocks(block, nblocks, n_total):
    """Several message blocks; elements at index >= n_total read as zero and are not written back."""
    x = random_bf16(n_total, 3 + block)
    full = torch.zeros(block * nblocks, dtype=torch.bfloat16)
    full[:n_total] = x
    ref = quant.mx_reference_wire(full, block, nblocks)
    assert torch.equal(host_quantize(x, block, nblocks, n_total), ref)
    got = host_dequantize(ref, block, nblocks, n_total)
    want = quant.mx_reference_dequant(ref, block, nblocks)
    assert torch.equal(bits(got[:n_total]), bits(want[:n_total]))
    assert bool(torch.isnan(got[n_total:]).all())


@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("n", SIZES)
def test_host_dequant_reduce_matches_the_rank_ordered_sum(W, n):
    x = random_bf16(W * n, 50 + W + n)
    ref = quant.mx_reference_wire(x, n, W)
    assert torch.equal(bits(host_dequant_reduce(ref, n, W)), bits(quant.mx_reference_dequant_reduce(ref, n, W)))


def test_large_size_takes_the_threaded_path():
    n = (1 << 21) + 40  # more than one piece of the host loops
    x = random_bf16(n, 9)
    ref = quant.mx_reference_wire(x)
    wire = host_quantize(x)
    assert torch.equal(wire, ref)
    assert torch.equal(bits(host_dequantize(wire, n)), bits(quant.mx_reference_dequant(ref, n)))
    assert torch.equal(bits(host_dequant_reduce(wire, n, 1)), bits(quant.mx_reference_dequant_reduce(ref, n, 1)))


def special_blocks():
    """Eight 32-element blocks: zeros, one element at 2^-100, amax mantissa 1.75 and 1.9375 (scaled amax 448
    and 496: the saturation zone), an Inf, a NaN, negative zeros, a tiny block below 2^-118."""
    x = torch.zeros(8, 32, dtype=torch.float32)
    x[1, 5] = 2.0 ** -100
    x[2] = torch.linspace(-1.0, 1.0, 32)
    x[2, 7] = 1.75
    x[3] = torch.linspace(-1.0, 1.0, 32) * 1.9
    x[3, 9] = -1.9375
    x[3, 10] = 1.875
    x[4] = 0.5
    x[4, 3] = float("inf")
    x[5] = -0.25
    x[5, 31] = float("nan")
    x[6] = -0.0
    x[7] = 2.0 ** -125
    return x.to(torch.bfloat16).reshape(-1)


def test_special_blocks():
    x = special_blocks()
    n = x.numel()
    ref = quant.mx_reference_wire(x)
    got = host_quantize(x)
    scales = got[n:n + n // 32]
    assert torch.equal(scales, ref[n:n + n // 32])
    assert scales.tolist() == [0, 127 - 100 - 8, 127 - 8, 127 - 8, 0xFF, 0xFF, 0, 0]
    for b in (0, 1, 2, 3, 6, 7):  # (the payload of a non-finite block is unspecified)
        assert torch.equal(got[b * 32:(b + 1) * 32], ref[b * 32:(b + 1) * 32]), b
    # the saturation zone: 1.9375 * 2^8 = 496 and 1.875 * 2^8 = 480 clamp to 448 (0x7E), never NaN (0x7F)
    assert got[3 * 32 + 9] == 0xFE and got[3 * 32 + 10] == 0x7E and got[2 * 32 + 7] == 0x7E
    assert got[1 * 32 + 5] == 0x78  # 2^-100 * 2^108 = 256
    d = host_dequantize(got, n)
    want = quant.mx_reference_dequant(ref, n)
    for b in (0, 1, 2, 3, 6):  # amax == 0 or >= 2^-118: bit for bit
        assert torch.equal(bits(d[b * 32:(b + 1) * 32]), bits(want[b * 32:(b + 1) * 32])), b
    assert float(d[1 * 32 + 5]) == 2.0 ** -100 and bool((bits(d[6 * 32:7 * 32]) == -0x8000).all())
    assert bool(torch.isnan(d[4 * 32:6 * 32]).all())
    tiny = d[7 * 32:8 * 32].float()  # below 2^-118: finite, no larger than amax
    assert bool(torch.isfinite(tiny).all()) and bool((tiny.abs() <= 2.0 ** -125).all())
    # a block with a NaN poisons its part of a sum, and only that
    s = host_dequant_reduce(torch.cat([got, got]), n, 2)
    assert bool(torch.isnan(s[4 * 32:6 * 32]).all()) and float(s[1 * 32 + 5]) == 2.0 ** -99


def test_saturation_zone_is_common():
    """About one block in nine of uniform data scales its amax into (448, 512): without the clamp those
    elements would convert to NaN."""
    x = (torch.rand(32 * 4096, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(torch.bfloat16)
    wire = host_quantize(x)
    n = x.numel()
    assert not bool(((wire[:n] & 0x7F) == 0x7F).any())
    assert int(((wire[:n] & 0x7F) == 0x7E).sum()) > 100
    assert torch.equal(wire, quant.mx_reference_wire(x))


# ---- commtest


def run_commtest(n, *extra):
    code, outs = launch.launch(n, [DLNB, "commtest", *extra], timeout=120, capture=True)
    text = "".join(o or "" for o in outs)
    lines = [json.loads(ln) for ln in (outs[0] or "").splitlines() if ln.startswith("{")]
    assert code == 0 and lines, text[-3000:]
    return lines[0]


def test_commtest_loopback_cpu_exact():
    p = subprocess.run([DLNB, "commtest", "--backend", "loopback-cpu", "--ranks", "4", "--wire-quant", "mxfp8", "--sizes",
                        "1,33,4096,100000"], capture_output=True, text=True, timeout=120)
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, p.stdout[-2000:] + p.stderr[-3000:]
    assert lines[0]["ok"] and lines[0]["wire_quant"] == "mxfp8" and lines[0]["world_size"] == 4


def test_commtest_cpu_backend_exact():
    out = run_commtest(2, "--backend", "cpu", "--wire-quant", "mxfp8", "--sizes", "1,33,4096,100000")
    assert out["ok"] and out["wire_quant"] == "mxfp8" and out["world_size"] == 2 and out["backend"] == "CPU-SHM"


def test_commtest_catches_a_misrouted_quantized_block():
    """The fault injector sits above the quantizing communicator: a swapped output fails the bit-exact check."""
    env = dict(os.environ, DLNB_COMM_FAULT="mode=swap,op=all_gather")
    p = subprocess.run([DLNB, "commtest", "--backend", "loopback-cpu", "--ranks", "2", "--wire-quant", "mxfp8", "--sizes",
                        "4096"], capture_output=True, text=True, timeout=120, env=env)
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode != 0 and lines and not lines[0]["ok"], p.stdout + p.stderr[-2000:]


def test_commtest_rejects_other_dtypes():
    p = subprocess.run([DLNB, "commtest", "--backend", "loopback-cpu", "--ranks", "2", "--wire-quant", "mxfp8", "--dtype",
                        "fp32", "--sizes", "64"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--wire-quant" in p.stderr and "--dtype" in p.stderr


# ---- strategies


def run_strategy(prog, *args, ranks=0):
    """ranks > 0: loopback-cpu threads of one process; else 2 processes on the shm backend."""
    if ranks:
        p = subprocess.run([os.path.join(BIN, prog), *map(str, args), "--backend", "loopback-cpu", "--ranks", str(ranks),
                            "--quiet"], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
        docs = report.parse_output(p.stdout)
    else:
        code, outs = launch.launch(2, [os.path.join(BIN, prog), *map(str, args), "--backend", "cpu", "--quiet"],
                                   timeout=120, capture=True)
        assert code == 0, "".join(o or "" for o in outs)[-3000:]
        docs = report.parse_output(outs[0])
    assert len(docs) == 1
    return next(iter(docs.values()))


def check_block(doc, kinds):
    wq = doc["global"]["dlnb"]["wire_quant"]
    assert wq["format"] == "mxfp8_e4m3" and wq["block"] == 32
    assert set(wq["ops"]) == {"all_reduce", "all_gather", "reduce_scatter", "all_to_all"}
    for k, o in wq["ops"].items():
        assert o["calls"] > 0 or k not in kinds, (k, o)
        if not o["calls"]:
            continue
        ratio = o["wire_bytes"] / o["payload_bytes"]
        assert ratio >= 33 / 64, (k, o)
        if o["payload_bytes"] / o["calls"] >= 1 << 20:
            assert ratio <= 33 / 64 + 1e-3, (k, o)
    return wq


def test_dp_all_reduce(data_dir):
    d = run_strategy("dp", "tiny_dense_8_bfloat16", 4, data_dir, "-w", 1, "-r", 2, "--wire-quant", "mxfp8")
    assert d["global"]["world_size"] == 2
    check_block(d, {"all_reduce"})


def test_fsdp_all_gather_and_reduce_scatter(data_dir):
    d = run_strategy("fsdp", "tiny_dense_8_bfloat16", 4, 2, data_dir, "-w", 1, "-r", 2, "--wire-quant", "mxfp8", ranks=2)
    check_block(d, {"all_gather", "reduce_scatter"})


def test_moe_all_to_all(data_dir):
    d = run_strategy("hybrid_3d_moe", "tiny_moe_8_bfloat16", 1, 2, 2, data_dir, "-w", 1, "-r", 2, "--wire-quant", "mxfp8",
                     ranks=2)
    check_block(d, {"all_to_all"})


def test_large_messages_reach_the_ratio(root):
    """A real model's buckets (>= 1 MiB of payload per call): wire bytes are 33/64 of the bf16 bytes."""
    d = run_strategy("dp", "vit_b_16_bfloat16", 4, root, "-w", 0, "-r", 1, "--wire-quant", "mxfp8", "--time-scale", 0.01,
                     ranks=2)
    o = check_block(d, {"all_reduce"})["ops"]["all_reduce"]
    assert o["payload_bytes"] / o["calls"] >= 1 << 20 and o["wire_bytes"] / o["payload_bytes"] <= 33 / 64 + 1e-3


def test_block_absent_without_the_option(data_dir):
    d = run_strategy("dp", "tiny_dense_8_bfloat16", 4, data_dir, "-w", 1, "-r", 1, ranks=2)
    assert "wire_quant" not in d["global"]["dlnb"]
    d = run_strategy("dp", "tiny_dense_8_bfloat16", 4, data_dir, "-w", 1, "-r", 1, "--wire-quant", "none", ranks=2)
    assert "wire_quant" not in d["global"]["dlnb"]


@pytest.mark.parametrize("dtype", ["fp8", "fp32", "fp16"])
def test_option_rejected_with_another_wire_dtype(dtype, data_dir):
    p = subprocess.run([os.path.join(BIN, "dp"), "tiny_dense_8_bfloat16", "4", data_dir, "--wire-quant", "mxfp8",
                        "--wire-dtype", dtype], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "--wire-quant" in p.stderr and "--wire-dtype" in p.stderr


def test_option_rejects_unknown_modes(data_dir):
    p = subprocess.run([os.path.join(BIN, "dp"), "tiny_dense_8_bfloat16", "4", data_dir, "--wire-quant", "fp4"],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "--wire-quant must be none or mxfp8" in p.stderr


def test_engine_keyword():
    from dlnetbench_amd import engine
    args = engine.build_args("dp", "m", 4, wire_quant="mxfp8")
    assert args[args.index("--wire-quant") + 1] == "mxfp8"
    assert "--wire-quant" in subprocess.run([os.path.join(BIN, "dp"), "--help"], capture_output=True, text=True).stdout


def test_c_abi_symbols():
    L = _native.lib()
    for name in ("dlnb_mx_quantize", "dlnb_mx_dequantize", "dlnb_mx_dequant_reduce", "dlnb_mx_wire_bytes",
                 "dlnb_mx_quantize_host", "dlnb_mx_dequantize_host", "dlnb_mx_dequant_reduce_host"):
        assert isinstance(getattr(L, name), ctypes._CFuncPtr), name
