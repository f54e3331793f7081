"""The fused attention kernel (ops.attention.attention_fwd) against a float64 reference; its deadline form, refusals and mode."""
import math

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


from dlnetbench_amd import _native, engine  # noqa: E402
from dlnetbench_amd.ops import attention  # noqa: E402

SCALE = 1.0 / math.sqrt(128)
# (B, H, Hkv, Sq, Skv, causal, hot): hot multiplies Q by 8 and K's second 128 keys by 4 (scores near +-100, the
# row max moving upward at the second tile)
CASES = [
    (1, 1, 1, 128, 128, False, False),
    (1, 1, 1, 128, 128, True, False),
    (1, 2, 2, 384, 384, True, False),
    (1, 2, 1, 256, 256, False, False),
    (2, 4, 2, 128, 384, False, False),
    (1, 1, 1, 256, 256, False, True),
]
_cache = {}


def problem(case):
    """bf16 q, k, v of the case and, in float64 from those same values, (O_ref, P_ref |V|, lse_ref)."""
    if case not in _cache:
        B, H, Hkv, Sq, Skv, causal, hot = case
        g = torch.Generator(device="cuda").manual_seed(1234)
        q = torch.randn(B, H, Sq, 128, device="cuda", generator=g).to(torch.bfloat16)
        k = torch.randn(B, Hkv, Skv, 128, device="cuda", generator=g).to(torch.bfloat16)
        v = torch.randn(B, Hkv, Skv, 128, device="cuda", generator=g).to(torch.bfloat16)
        if hot:
            q = q * 8
            k[:, :, 128:] *= 4
        kd = k.double().repeat_interleave(H // Hkv, dim=1)
        vd = v.double().repeat_interleave(H // Hkv, dim=1)
        s = SCALE * q.double() @ kd.transpose(-1, -2)
        if causal:
            s = s.masked_fill(torch.ones(Sq, Skv, device="cuda").triu(1).bool(), float("-inf"))
        lse = torch.logsumexp(s, dim=-1)
        p = torch.exp(s - lse[..., None])
        _cache[case] = (q, k, v, p @ vd, p @ vd.abs(), lse)
    return _cache[case]


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(x)) for x in c))
def test_matches_the_float64_reference(case, grid):
    q, k, v, o_ref, pv_abs, lse_ref = problem(case)
    o = torch.full_like(q, float("nan"))
    lse = torch.full(q.shape[:3], float("nan"), device="cuda")
    attention.attention_fwd(q, k, v, out=o, lse=lse, causal=case[5], scale=SCALE, grid=grid)
    torch.cuda.synchronize()
    # the kernel's two bf16 roundings: P (relative 2^-9 each, bounded by 2^-8 of P |V|) and O (2^-9 of |O|)
    bound = 2.0 ** -8 * pv_abs + 2.0 ** -9 * o_ref.abs() + 1e-4 * v.double().abs().max()
    err = (o.double() - o_ref).abs()
    print("max err / bound", (err / bound).max().item(), "lse err", (lse.double() - lse_ref).abs().max().item())
    assert bool((err <= bound).all())  # (NaN fails)
    assert bool(((lse.double() - lse_ref).abs() <= 1e-4 * lse_ref.abs().clamp(min=1.0)).all())


def test_deadline_form_repeats_the_one_shot_result():
    case = CASES[2]
    q, k, v, _, _, _ = problem(case)
    grid, us = 6, 2000.0  # one block per item: the one-shot run lasts as long as its longest item
    _native.lib().dlnb_wallclock_hz(0)  # (the clock calibration's wait, outside the timings)
    o1, o2 = torch.full_like(q, float("nan")), torch.full_like(q, float("nan"))
    l1, l2 = (torch.full(q.shape[:3], float("nan"), device="cuda") for _ in range(2))
    attention.attention_fwd(q, k, v, out=o2, causal=True, us=10.0, grid=grid)  # both kernels' first launches
    attention.attention_fwd(q, k, v, out=o1, causal=True, grid=grid)
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    e[0].record()
    attention.attention_fwd(q, k, v, out=o1, lse=l1, causal=True, scale=SCALE, grid=grid)
    e[1].record()
    torch.cuda.synchronize()
    totals = torch.zeros(2, device="cuda", dtype=torch.int64)
    per_block = torch.zeros(grid, device="cuda", dtype=torch.int64)
    slots = torch.zeros(1, device="cuda", dtype=torch.int64)
    e[2].record()
    attention.attention_fwd(q, k, v, out=o2, lse=l2, causal=True, scale=SCALE, us=us, grid=grid, totals=totals,
                            per_block=per_block, start=(slots, 0))
    e[3].record()
    torch.cuda.synchronize()
    item_us, task_us = e[0].elapsed_time(e[1]) * 1e3, e[2].elapsed_time(e[3]) * 1e3
    print("longest item", item_us, "us; task", task_us, "us; steps", totals.tolist(), per_block.tolist())
    assert torch.equal(o1, o2) and torch.equal(l1, l2)  # every recomputation is identical
    assert totals[0].item() > 2 * (1 + 2 + 3)  # more than one sweep of the 2 heads' 3 Q tiles
    assert per_block.sum().item() == totals[0].item()
    assert totals[1].item() == round(us * 1e-6 * _native.lib().dlnb_wallclock_hz(0))
    assert slots[0].item() > 0
    assert us <= task_us <= us + 3 * item_us


@pytest.mark.parametrize("shape,causal,word", [((1, 2, 2, 192, 128), False, "Sq"), ((1, 2, 2, 128, 256), True, "causal"),
                                               ((1, 3, 2, 128, 128), False, "Hkv")])
def test_launcher_refuses(shape, causal, word):
    B, H, Hkv, Sq, Skv = shape
    q = torch.zeros(B, H, Sq, 128, device="cuda", dtype=torch.bfloat16)
    k = torch.zeros(B, Hkv, Skv, 128, device="cuda", dtype=torch.bfloat16)
    o = torch.full_like(q, float("nan"))
    with pytest.raises(_native.NativeError, match=word):
        attention.attention_fwd(q, k, k, out=o, causal=causal)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all())  # nothing was launched


def test_strategy_runs_with_attn_compute(data_dir):
    doc = engine.run_native("dp", "tiny_dense_8_bfloat16", 4, base_path=data_dir, warmup=1, runs=2, compute="attn",
                            quiet=True)
    c = doc["global"]["dlnb"]["compute"]
    it = doc["global"]["dlnb"]["iteration"]
    print(it["median_ms"], it["compute_floor_ms"], c["attn"])
    assert c["mode"] == "attn" and c["attn"]["kv_tile"] == attention.kv_tile() == 128
    assert c["attn"]["TFLOPs"] > 0 and c["attn"]["kv_tile_steps"] > 0
    assert it["median_ms"] >= 0.9 * it["compute_floor_ms"]
