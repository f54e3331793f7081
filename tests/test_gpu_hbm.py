"""The HBM-streaming kernel (ops.stream.stream_add): exact results, honest accounting, deadline, bandwidth."""
import statistics

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


from dlnetbench_amd import _native  # noqa: E402
from dlnetbench_amd.ops import gemm, stream  # noqa: E402

CHUNK = 32768  # elements per chunk and array (64 KiB of bf16)
NAN = float("nan")


def test_chunk_size():
    assert stream.chunk_bytes() == 2 * CHUNK


@pytest.fixture(scope="module")
def big():
    """Three arrays of 512 MiB (each twice the Infinity Cache), a and b random, and a + b by torch."""
    n = (512 << 20) // 2
    a = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    b = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    gemm.fill_random_(a, 11)
    gemm.fill_random_(b, 12)
    c = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    ref = a + b
    torch.cuda.synchronize()
    return a, b, c, ref


def guarded(n):
    """n elements inside a NaN-filled tensor with 64 guard elements (128 bytes) on each side."""
    buf = torch.full((n + 128,), NAN, device="cuda", dtype=torch.bfloat16)
    return buf, buf[64:64 + n]


@pytest.mark.parametrize("grid", [1, 3, 0])
@pytest.mark.parametrize("n", [8, 32760, 32768, 32776, 3 * 32768 + 24, 2 ** 20 + 8])
def test_one_shot_is_exact(big, n, grid):
    a, b, _, ref = big
    buf, c = guarded(n)
    assert c.data_ptr() % 16 == 0
    stream.stream_add(a[:n], b[:n], c, grid=grid)
    torch.cuda.synchronize()
    # torch's bf16 add is fp32 math with one rounding, as the kernel's: bit for bit
    assert torch.equal(c, ref[:n])
    assert torch.isnan(buf[:64]).all() and torch.isnan(buf[64 + n:]).all()


def test_rejects_bad_arguments(big):
    a, b, _, _ = big
    buf, c = guarded(64)
    with pytest.raises(_native.NativeError):  # n % 8 != 0
        stream.stream_add(a[:12], b[:12], c[:12])
    for args in ((a[1:9], b[:8], c[:8]), (a[:8], b[1:9], c[:8]), (a[:8], b[:8], c[1:9])):  # 2 bytes off
        with pytest.raises(_native.NativeError):
            stream.stream_add(*args)
    with pytest.raises(_native.NativeError):  # one block per CU: no grid beyond the CUs
        stream.stream_add(a[:8], b[:8], c[:8], grid=100000)
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()  # nothing was launched


def test_deadline_full_coverage(big):
    a, b, _, ref = big
    n = 64 * CHUNK
    c = torch.full((n,), NAN, device="cuda", dtype=torch.bfloat16)
    totals = torch.zeros(2, device="cuda", dtype=torch.int64)
    per_block = torch.zeros(3, device="cuda", dtype=torch.int64)
    stream.stream_add(a[:n], b[:n], c, us=2000.0, grid=3, totals=totals, per_block=per_block)
    torch.cuda.synchronize()
    print("chunks", totals[0].item(), "per block", per_block.tolist())
    assert totals[0].item() >= 64
    assert per_block.sum().item() == totals[0].item()
    assert torch.equal(c, ref[:n])


def test_deadline_partial_coverage_accounting_is_true(big):
    a, b, _, ref = big
    chunks = 1024
    n = chunks * CHUNK
    c = torch.full((n,), NAN, device="cuda", dtype=torch.bfloat16)
    totals = torch.zeros(2, device="cuda", dtype=torch.int64)
    per_block = torch.zeros(2, device="cuda", dtype=torch.int64)
    stream.stream_add(a[:n], b[:n], c, us=50.0, grid=2, totals=totals, per_block=per_block)
    torch.cuda.synchronize()
    counts = per_block.tolist()
    print("chunks", totals[0].item(), "per block", counts)
    assert 0 < totals[0].item() < chunks
    assert sum(counts) == totals[0].item()
    written = torch.zeros(chunks, dtype=torch.bool, device="cuda")
    for blk, cnt in enumerate(counts):
        written[[blk + 2 * j for j in range(cnt)]] = True
    c2, r2 = c.view(chunks, CHUNK), ref[:n].view(chunks, CHUNK)
    assert torch.equal(c2[written], r2[written])
    assert torch.isnan(c2[~written]).all()


def test_deadline_hits_duration(big):
    a, b, c, _ = big
    n = (256 << 20) // 2  # 3 x 256 MiB, default grid
    a, b, c = a[:n], b[:n], c[:n]
    s = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream.stream_add(a, b, c, us=50.0)  # first launch of the kernel (code object load) outside the timing
    torch.cuda.synchronize()
    for us in (200.0, 5000.0):
        times = []
        for _ in range(3):
            e0.record(s)
            stream.stream_add(a, b, c, us=us)
            e1.record(s)
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        print(us, times)
        ms = sorted(times)[1]
        assert us / 1e3 * 0.97 <= ms <= us / 1e3 * 1.10 + 0.05, (us, times)


def test_start_stamp_and_ticks(big):
    a, b, c, _ = big
    n = 64 * CHUNK
    slots = torch.zeros(3, device="cuda", dtype=torch.int64)
    totals = torch.zeros(2, device="cuda", dtype=torch.int64)
    us = 300.0
    gemm.stamp_(slots, 0)
    stream.stream_add(a[:n], b[:n], c[:n], us=us, totals=totals, start=(slots, 1))
    gemm.stamp_(slots, 2)
    torch.cuda.synchronize()
    before, start, after = slots.tolist()
    hz = _native.lib().dlnb_wallclock_hz(0)
    ticks = int(us * 1e-6 * hz + 0.5)
    assert before <= start <= after, (before, start, after)
    assert after - start >= ticks  # the stamp is the kernel's own entry: the whole deadline follows it
    assert totals[1].item() == ticks
    swept = totals[0].item()
    stream.stream_add(a[:n], b[:n], c[:n], totals=totals)  # one shot: every chunk once, no ticks
    torch.cuda.synchronize()
    assert totals[1].item() == ticks and totals[0].item() == swept + 64


def test_bandwidth_against_torch(big):
    """One shot over 3 x 512 MiB on every CU against torch.add on the same tensors, interleaved, median of 5."""
    a, b, c, _ = big
    fns = {"kernel": lambda: stream.stream_add(a, b, c), "torch": lambda: torch.add(a, b, out=c)}
    times = {k: [] for k in fns}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(5):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e-3)
    gbps = {k: 3 * a.numel() * 2 / statistics.median(v) / 1e9 for k, v in times.items()}
    print("GB/s", gbps, "ratio", gbps["kernel"] / gbps["torch"])
    assert gbps["kernel"] >= 0.8 * gbps["torch"], gbps
