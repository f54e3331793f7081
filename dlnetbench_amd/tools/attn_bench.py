"""Rate of the fused attention kernel (ops.attention.attention_fwd) vs torch SDPA on MI355X.

    python -m dlnetbench_amd attn-bench [--seq 1024,2048,4096,8192] [--heads 32] [--grid N] [--dtype bf16|fp8]

One-shot forward attention, B = 1, head dimension 128, for every sequence
length with the causal mask on and off, as MHA (Hkv = H) and as GQA 4:1. Per
shape one JSON line: TF/s (the FLOPs of the visible score blocks only: half
the square plus the diagonal under the causal mask; median, best) of the
kernel and of ``torch.nn.functional.scaled_dot_product_attention`` on the
same tensors, interleaved round by round in one process, and their ratio.
--dtype fp8 times the e4m3 kernel (kernel_*), the bf16 kernel (bf16_*) on bf16
tensors of the same shape and SDPA in bf16 in the same interleaved rounds, and
adds fp8_vs_bf16_median.
"""
from __future__ import annotations

import argparse
import json
import statistics

from .hbm_bench import measure


def main(argv=None) -> int:
    import torch
    import torch.nn.functional as F
    from dlnetbench_amd.ops import attention, gemm

    ap = argparse.ArgumentParser()
    ap.add_argument("--seq", default="1024,2048,4096,8192", help="sequence lengths (multiples of 128)")
    ap.add_argument("--heads", type=int, default=32, help="query heads (a multiple of 4)")
    ap.add_argument("--grid", type=int, default=0, help="blocks, one per CU (0 = every CU)")
    ap.add_argument("--dtype", choices=("bf16", "fp8"), default="bf16", help="the kernel's Q, K, V type")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args(argv)
    H, D = a.heads, attention.HEAD_DIM
    for S in (int(x) for x in a.seq.split(",")):
        for Hkv in (H, H // 4):
            q = torch.empty(1, H, S, D, device="cuda", dtype=torch.bfloat16)
            k = torch.empty(1, Hkv, S, D, device="cuda", dtype=torch.bfloat16)
            v = torch.empty_like(k)
            o = torch.empty_like(q)
            for i, t in enumerate((q, k, v)):
                gemm.fill_random_(t, i + 1)
            # SDPA takes MHA shapes: the expanded view reads the same K / V heads as the kernel's index mapping
            ke = k[:, :, None].expand(1, Hkv, H // Hkv, S, D).reshape(1, H, S, D) if Hkv != H else k
            ve = v[:, :, None].expand(1, Hkv, H // Hkv, S, D).reshape(1, H, S, D) if Hkv != H else v
            if a.dtype == "fp8":
                q8, k8, v8 = (torch.empty_like(t, dtype=torch.float8_e4m3fn) for t in (q, k, v))
                for i, t in enumerate((q8, k8, v8)):
                    gemm.fill_random_(t, i + 1)
            for causal in (False, True):
                fns = [("kernel", lambda: attention.attention_fwd(q, k, v, out=o, causal=causal, grid=a.grid)),
                       ("torch", lambda: F.scaled_dot_product_attention(q, ke, ve, is_causal=causal))]
                if a.dtype == "fp8":
                    fns = [("kernel", lambda: attention.attention_fwd(q8, k8, v8, out=o, causal=causal, grid=a.grid)),
                           ("bf16", fns[0][1]), fns[1]]
                res = measure(fns, a.rounds, a.iters)
                tiles = S // 128
                blocks = tiles * (tiles + 1) // 2 if causal else tiles * tiles  # visible 128 x 128 score blocks per head
                flops = 4.0 * 128 * 128 * D * blocks * H
                out = {"seq": S, "heads": H, "kv_heads": Hkv, "causal": causal, "grid": a.grid}
                for name, t in res.items():
                    out[f"{name}_TFs_median"] = round(flops / statistics.median(t) / 1e12, 1)
                    out[f"{name}_TFs_best"] = round(flops / min(t) / 1e12, 1)
                out["ratio_median"] = round(out["kernel_TFs_median"] / out["torch_TFs_median"], 3)
                if a.dtype == "fp8":
                    out["fp8_vs_bf16_median"] = round(out["kernel_TFs_median"] / out["bf16_TFs_median"], 3)
                print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
