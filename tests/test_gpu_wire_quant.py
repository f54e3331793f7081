"""--wire-quant mxfp8 on one MI355X: the three wire kernels against the torch reference of the format
(ops.quant.mx_reference), bit for bit; commtest over loopback and xgmi; fsdp and dp end to end; bandwidth.

RCCL cannot put two ranks on one GPU, so RCCL at W > 1 stays unexercised here (the quantizing communicator
passes 1-rank groups through untouched). `--graph` is refused for --backend loopback (its ranks rendezvous on
the host, replay.cpp), so the captured fsdp / dp runs use two xgmi processes on GPU 0 instead."""
import json
import os
import statistics
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


from dlnetbench_amd import engine  # noqa: E402
from dlnetbench_amd.ops import quant, stream  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DLNB = os.path.join(ROOT, "build", "bin", "dlnb")
GUARD = 128


def bits(t):
    return t.view(torch.int16)


def random_bf16(n, seed):
    """Uniform [-1, 1) times 2^k, k in [-12, 12]: every exponent's blocks, a share of them with the scaled
    amax in (448, 512) (the saturation zone)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, generator=g) * 2 - 1
    k = torch.randint(-12, 13, (n,), generator=g).float()
    x = x * torch.pow(torch.tensor(2.0), k)
    x[::97] = 0.0
    return x.to(torch.bfloat16)


def guarded(nbytes, offset=0):
    """(whole, view): nbytes of a 0xFF-filled (NaN) buffer with GUARD bytes on each side; offset shifts the
    view (an unaligned base pointer)."""
    whole = torch.full((GUARD + offset + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD + offset:GUARD + offset + nbytes]


def guards_intact(whole, nbytes, offset=0):
    lo = whole[:GUARD + offset]
    hi = whole[GUARD + offset + nbytes:]
    return bool((lo == 0xFF).all()) and bool((hi == 0xFF).all())


# (block_elems or 0 = n, nblocks, source offset in bytes)
LAYOUTS = [(0, 1, 0), (1000, 3, 0), (4096, 4, 0), (1001, 3, 0), (0, 1, 2)]


@pytest.mark.parametrize("n", [32, 33, 8 * 32 + 8, 65536 + 40])
@pytest.mark.parametrize("block,nblocks,offset", LAYOUTS)
def test_quantize_and_dequantize_match_the_reference(n, block, nblocks, offset):
    block = block or n
    m = min(n, block * nblocks)  # elements that exist
    x = random_bf16(m, 1000 + n + block)
    full = torch.zeros(block * nblocks, dtype=torch.bfloat16)
    full[:m] = x
    ref = quant.mx_reference_wire(full, block, nblocks)
    wb = quant.wire_bytes(block)
    assert wb == (quant.padded(block) * 33 // 32 + 15) // 16 * 16

    src_whole, src = guarded(m * 2, offset)
    src.copy_(x.view(torch.uint8).cuda())
    wire_whole, wire = guarded(nblocks * wb)
    quant.mx_quantize(src.view(torch.bfloat16), wire, block, nblocks, n_total=m)
    torch.cuda.synchronize()
    assert torch.equal(wire.cpu(), ref), (n, block, nblocks)
    assert guards_intact(wire_whole, nblocks * wb) and guards_intact(src_whole, m * 2, offset)

    dst_whole, dst = guarded(block * nblocks * 2, offset)
    quant.mx_dequantize(ref.cuda(), dst.view(torch.bfloat16), block, nblocks, n_total=m)
    torch.cuda.synchronize()
    want = quant.mx_reference_dequant(ref, block, nblocks)
    got = dst.view(torch.bfloat16).cpu()
    assert torch.equal(bits(got[:m]), bits(want[:m]))
    assert bool((dst[m * 2:] == 0xFF).all())  # nothing at or beyond n_total was written
    assert guards_intact(dst_whole, block * nblocks * 2, offset)


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
    wire = torch.zeros(quant.wire_bytes(n), dtype=torch.uint8, device="cuda")
    quant.mx_quantize(x.cuda(), wire)
    got = wire.cpu()
    scales = got[n:n + n // 32]
    assert torch.equal(scales, ref[n:n + n // 32])
    assert scales[4] == 0xFF and scales[5] == 0xFF and scales[0] == 0 and scales[6] == 0 and scales[7] == 0
    finite = [0, 1, 2, 3, 6, 7]
    for b in finite:
        assert torch.equal(got[b * 32:(b + 1) * 32], ref[b * 32:(b + 1) * 32]), b
    assert torch.equal(got[n + n // 32:], ref[n + n // 32:])  # padding
    # the saturation zone really is in play: 1.9375 * 2^8 = 496 clamps to 448 (0x7E), never NaN (0x7F)
    assert got[3 * 32 + 9] == 0xFE and got[3 * 32 + 10] == 0x7E and got[2 * 32 + 7] == 0x7E
    dst = torch.full((n,), float("nan"), dtype=torch.bfloat16, device="cuda")
    quant.mx_dequantize(wire, dst)
    d = dst.cpu()
    want = quant.mx_reference_dequant(ref, n)
    for b in (0, 1, 2, 3, 6):  # amax == 0 or >= 2^-118: bit for bit
        assert torch.equal(bits(d[b * 32:(b + 1) * 32]), bits(want[b * 32:(b + 1) * 32])), b
    assert bool(torch.isnan(d[4 * 32:6 * 32]).all())
    tiny = d[7 * 32:8 * 32].float()  # below 2^-118: finite, no larger than amax
    assert bool(torch.isfinite(tiny).all()) and bool((tiny.abs() <= 2.0 ** -125).all())


@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("n", [33, 8 * 32 + 8, 65536 + 40])
def test_dequant_reduce_matches_the_rank_ordered_sum(W, n):
    x = random_bf16(W * n, 77 + W + n)
    x[5::n] = -0.0
    ref = quant.mx_reference_wire(x, n, W)
    want = quant.mx_reference_dequant_reduce(ref, n, W)
    whole, dst = guarded(n * 2)
    quant.mx_dequant_reduce(ref.cuda(), dst.view(torch.bfloat16), n, W)
    torch.cuda.synchronize()
    assert torch.equal(bits(dst.view(torch.bfloat16).cpu()), bits(want))
    assert guards_intact(whole, n * 2)
    # fewer elements than the block holds: the rest stays
    whole, dst = guarded(n * 2)
    quant.mx_dequant_reduce(ref.cuda(), dst.view(torch.bfloat16), n, W, n=n - 17)
    torch.cuda.synchronize()
    assert torch.equal(bits(dst.view(torch.bfloat16).cpu()[:n - 17]), bits(want[:n - 17]))
    assert bool((dst[(n - 17) * 2:] == 0xFF).all()) and guards_intact(whole, n * 2)


def test_nan_block_poisons_the_sum():
    x = torch.ones(4 * 64, dtype=torch.bfloat16)
    x[2 * 64 + 40] = float("nan")
    wire = torch.zeros(4 * quant.wire_bytes(64), dtype=torch.uint8, device="cuda")
    quant.mx_quantize(x.cuda(), wire, 64, 4)
    dst = torch.zeros(64, dtype=torch.bfloat16, device="cuda")
    quant.mx_dequant_reduce(wire, dst, 64, 4)
    d = dst.cpu().float()
    assert bool((d[:32] == 4.0).all()) and bool(torch.isnan(d[32:]).all())


def test_captured_launch_replays_the_same_bits():
    n = 65536 + 40
    x = random_bf16(n, 5).cuda()
    wire = torch.zeros(quant.wire_bytes(n), dtype=torch.uint8, device="cuda")
    back = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    quant.mx_quantize(x, wire)
    quant.mx_dequantize(wire, back)
    torch.cuda.synchronize()
    eager_wire, eager_back = wire.clone(), back.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        quant.mx_quantize(x, wire)
        quant.mx_dequantize(wire, back)
    for _ in range(2):
        wire.fill_(0xFF)
        back.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(wire, eager_wire) and torch.equal(bits(back), bits(eager_back))


# ---- the communicator


def launch(n, args, env_extra=None, timeout=140):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.update(env_extra or {})
    cmd = [sys.executable, "-m", "dlnetbench_amd.utils.launch", "-n", str(n), "--timeout", str(timeout)] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout + 30, env=env, cwd=ROOT)


SIZES = "1,33,4096,100000"


def test_commtest_loopback_exact():
    p = subprocess.run([DLNB, "commtest", "--backend", "loopback", "--ranks", "4", "--wire-quant", "mxfp8", "--sizes",
                        SIZES], capture_output=True, text=True, timeout=170, env=dict(os.environ, DLNB_NO_TORCH="1"))
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, p.stdout[-2000:] + p.stderr[-3000:]
    assert lines[0]["ok"] and lines[0]["wire_quant"] == "mxfp8" and lines[0]["world_size"] == 4


@pytest.mark.parametrize("extra", [[], ["--registered"], ["--graph"]], ids=["plain", "registered", "graph"])
def test_commtest_xgmi_exact(extra):
    p = launch(2, [DLNB, "commtest", "--backend", "xgmi", "-d", "0,0", "--wire-quant", "mxfp8", "--sizes", SIZES, *extra],
               {"DLNB_XGMI_TIMEOUT_S": "60"})
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, p.stdout[-2000:] + p.stderr[-3000:]
    assert lines[0]["ok"] and lines[0]["wire_quant"] == "mxfp8" and lines[0]["backend"] == "XGMI"
    assert lines[0]["graph"] == ("--graph" in extra) and lines[0]["registered"] == ("--registered" in extra)


def check_run(doc, kinds):
    d = doc["global"]["dlnb"]
    wq = d["wire_quant"]
    assert wq["format"] == "mxfp8_e4m3" and wq["block"] == 32
    for k in kinds:
        o = wq["ops"][k]
        assert o["calls"] > 0 and o["wire_bytes"] * 64 >= o["payload_bytes"] * 33, (k, o)
    for r in doc["ranks"]:
        assert "timer_negative_intervals" not in r, r["timer_negative_intervals"]
    it = d["iteration"]
    print(doc["section"], it["median_ms"], it["compute_floor_ms"], wq)
    assert it["median_ms"] >= 0.9 * it["compute_floor_ms"]


RUNS = [("fsdp", (4, 2), ("all_gather", "reduce_scatter")), ("dp", (4,), ("all_reduce",))]


@pytest.mark.parametrize("strategy,params,kinds", RUNS)
def test_strategies_on_loopback(strategy, params, kinds, data_dir):
    doc = engine.run_native(strategy, "tiny_dense_8_bfloat16", *params, base_path=data_dir, warmup=1, runs=2,
                            backend="loopback", ranks=2, wire_quant="mxfp8", quiet=True)
    assert doc["global"]["world_size"] == 2
    check_run(doc, kinds)


@pytest.mark.parametrize("strategy,params,kinds", RUNS)
def test_strategies_captured_on_xgmi(strategy, params, kinds, data_dir, tmp_path):
    out = tmp_path / "r.json"
    args = [os.path.join(ROOT, "build", "bin", strategy), "tiny_dense_8_bfloat16", *[str(p) for p in params], data_dir,
            "-w", "1", "-r", "3", "--backend", "xgmi", "-d", "0,0", "--compute", "spin", "--graph", "--wire-quant",
            "mxfp8", "--quiet", "--json", str(out)]
    p = launch(2, args, {"DLNB_XGMI_TIMEOUT_S": "60"})
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    doc = json.loads(out.read_text())
    assert doc["global"]["backend"] == "XGMI" and doc["global"]["dlnb"]["graph"] > 0
    check_run(doc, kinds)


# ---- bandwidth: against the one-shot streaming add (three bf16 arrays) moving the same total bytes in this
# process. The bounds are the lowest of five measured ratios x 0.9, rounded down to one decimal
# (profiles/wire_quant.md): the margin is for clocks and neighbours on a shared machine.
QUANTIZE_MIN_RATIO = 0.8  # measured 0.956 .. 0.988
DEQUANT_REDUCE_MIN_RATIO = 1.0  # measured 1.164 .. 1.239


def median_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def stream_add_gbps(total_bytes):
    """GB/s of stream.stream_add one-shot over three arrays that together hold total_bytes."""
    n = total_bytes // 3 // 2 // 8 * 8
    a = torch.randn(n, device="cuda").to(torch.bfloat16)
    b = torch.randn(n, device="cuda").to(torch.bfloat16)
    c = torch.empty_like(a)
    ms = median_ms(lambda: stream.stream_add(a, b, c))
    return 3 * n * 2 / ms / 1e6


def quantize_ratio():
    n = (256 << 20) // 2
    x = torch.randn(n, device="cuda").to(torch.bfloat16)
    wire = torch.empty(quant.wire_bytes(n), dtype=torch.uint8, device="cuda")
    ms = median_ms(lambda: quant.mx_quantize(x, wire))
    moved = n * 2 + wire.numel()
    return (moved / ms / 1e6) / stream_add_gbps(moved), moved / ms / 1e6


def dequant_reduce_ratio():
    W, n = 8, (256 << 20) // 2 // 8
    x = torch.randn(W * n, device="cuda").to(torch.bfloat16)
    wire = torch.empty(W * quant.wire_bytes(n), dtype=torch.uint8, device="cuda")
    quant.mx_quantize(x, wire, n, W)
    dst = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    ms = median_ms(lambda: quant.mx_dequant_reduce(wire, dst, n, W))
    moved = wire.numel() + n * 2
    return (moved / ms / 1e6) / stream_add_gbps(moved), moved / ms / 1e6


def test_quantize_bandwidth():
    ratio, gbps = quantize_ratio()
    print(f"mx_quantize 256 MiB: {gbps:.0f} GB/s, {ratio:.3f} x stream_add")
    assert ratio >= QUANTIZE_MIN_RATIO


def test_dequant_reduce_bandwidth():
    ratio, gbps = dequant_reduce_ratio()
    print(f"mx_dequant_reduce W=8: {gbps:.0f} GB/s, {ratio:.3f} x stream_add")
    assert ratio >= DEQUANT_REDUCE_MIN_RATIO
