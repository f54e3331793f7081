"""Bandwidth of the HBM-streaming kernel (ops.stream.stream_add) vs torch.add on MI355X.

    python -m dlnetbench_amd hbm-bench [--mb 16,64,256,1024,1536] [--grid N]

One-shot c = a + b over three bf16 arrays whose total size is each --mb value
(MiB): a working set inside the 32 MiB of L2, inside the 256 MiB Infinity
Cache, and beyond it (HBM). Per size one JSON line: GB/s (bytes read and
written / time; median, best) of the kernel and of ``torch.add(a, b, out=c)``
on the same tensors, interleaved round by round in one process.
"""
from __future__ import annotations

import argparse
import json
import statistics


def measure(fns, rounds: int, iters: int):
    """{name: [seconds per call]} over `rounds` interleaved rounds of `iters` calls each."""
    import torch
    res = {name: [] for name, _ in fns}
    for _, fn in fns:  # warm
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) * 1e-3 / iters)
    return res


def main(argv=None) -> int:
    import torch
    from dlnetbench_amd.ops import gemm, stream

    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", default="16,64,256,1024,1536", help="working-set sizes (MiB, all three arrays together)")
    ap.add_argument("--grid", type=int, default=0, help="blocks, one per CU (0 = every CU)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args(argv)
    chunk = stream.chunk_bytes()
    for mb in (float(x) for x in a.mb.split(",")):
        per = max(chunk, int(mb * (1 << 20) / 3) // chunk * chunk)  # bytes per array: whole chunks
        n = per // 2
        A = torch.empty(n, device="cuda", dtype=torch.bfloat16)
        B = torch.empty(n, device="cuda", dtype=torch.bfloat16)
        C = torch.empty(n, device="cuda", dtype=torch.bfloat16)
        gemm.fill_random_(A, 1)
        gemm.fill_random_(B, 2)
        fns = [("kernel", lambda: stream.stream_add(A, B, C, grid=a.grid)), ("torch", lambda: torch.add(A, B, out=C))]
        res = measure(fns, a.rounds, a.iters)
        out = {"working_set_mib": round(3 * per / (1 << 20), 2), "grid": a.grid}
        for k, v in res.items():
            out[f"{k}_GBps_median"] = round(3 * per / statistics.median(v) / 1e9, 1)
            out[f"{k}_GBps_best"] = round(3 * per / min(v) / 1e9, 1)
        out["ratio_median"] = round(out["kernel_GBps_median"] / out["torch_GBps_median"], 3)
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
