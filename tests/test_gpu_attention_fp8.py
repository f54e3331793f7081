"""The fp8 fused attention kernel (ops.attention.attention_fwd on float8_e4m3fn) against a float64 reference; its deadline form, refusals and mode."""
import math

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not hasattr(torch, "float8_e4m3fn"):
    pytest.skip("no torch.float8_e4m3fn", allow_module_level=True)
FP8 = torch.float8_e4m3fn


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


from dlnetbench_amd import _native, engine  # noqa: E402
from dlnetbench_amd.ops import attention  # noqa: E402

SCALE = 1.0 / math.sqrt(128)
# (B, H, Hkv, Sq, Skv, causal, kind). 640 keys are 5 steps: the 3-stage ring wraps, under the mask with the diagonal
# tile at a wrapped stage. hot: Q x 8, K's second 128 keys x 4 (scores near +-100, the row max moving upward at the
# second tile) and v_scale = 0.5. eyeV: V[k][d] = (d == k % 128), exact in e4m3, so O shows P key by key: a wrong key
# map or V^T order moves whole entries of O, which random V could hide under the P bound.
CASES = [
    (1, 1, 1, 128, 128, False, "rand"),
    (1, 1, 1, 128, 128, True, "rand"),
    (1, 2, 2, 640, 640, True, "rand"),
    (1, 2, 1, 256, 256, False, "rand"),
    (2, 4, 2, 128, 640, False, "rand"),
    (1, 1, 1, 256, 256, False, "hot"),
    (1, 1, 1, 128, 128, True, "eyeV"),
    (1, 1, 1, 256, 256, False, "eyeV"),
]
_cache = {}


def problem(case):
    """e4m3 q, k, v of the case, v_scale and, in float64 from those same values, (O_ref, P_ref |V|, lse_ref)."""
    if case not in _cache:
        B, H, Hkv, Sq, Skv, causal, kind = case
        g = torch.Generator(device="cuda").manual_seed(1234)
        q = torch.randn(B, H, Sq, 128, device="cuda", generator=g).to(FP8).float()
        k = torch.randn(B, Hkv, Skv, 128, device="cuda", generator=g).to(FP8).float()
        v = torch.randn(B, Hkv, Skv, 128, device="cuda", generator=g).to(FP8).float()
        v_scale = 1.0
        if kind == "hot":  # (powers of two: still e4m3 values)
            q = q * 8
            k[:, :, 128:] *= 4
            v_scale = 0.5
        if kind == "eyeV":
            v = torch.eye(128, device="cuda").repeat(Skv // 128, 1).expand(B, Hkv, Skv, 128).contiguous()
        kd = k.double().repeat_interleave(H // Hkv, dim=1)
        vd = v.double().repeat_interleave(H // Hkv, dim=1)
        s = SCALE * q.double() @ kd.transpose(-1, -2)
        if causal:
            s = s.masked_fill(torch.ones(Sq, Skv, device="cuda").triu(1).bool(), float("-inf"))
        lse = torch.logsumexp(s, dim=-1)
        p = torch.exp(s - lse[..., None])
        # the keys a row sees, |V| summed over them (the flush term of the bound)
        seen = (s > float("-inf")).double() @ vd.abs()
        _cache[case] = (q.to(FP8), k.to(FP8), v.to(FP8), v_scale, v_scale * (p @ vd), p @ vd.abs(), seen, lse)
    return _cache[case]


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(x)) if not isinstance(x, str) else x for x in c))
def test_matches_the_float64_reference(case, grid):
    q, k, v, v_scale, o_ref, pv_abs, seen, lse_ref = problem(case)
    o = torch.full(q.shape, float("nan"), device="cuda", dtype=torch.bfloat16)
    lse = torch.full(q.shape[:3], float("nan"), device="cuda")
    attention.attention_fwd(q, k, v, out=o, lse=lse, causal=case[5], scale=SCALE, grid=grid, v_scale=v_scale)
    torch.cuda.synchronize()
    # The kernel's own roundings, nothing else:
    #  * P to e4m3 (3 mantissa bits): half an ulp of a normal is 2^-4 of it, so 2^-4 P |V| summed over the keys;
    #  * P below e4m3's normals: the kernel rounds 2^8 p, p <= 1 relative to the row maximum; e4m3's subnormal step
    #    is 2^-9, half of it 2^-10, which is 2^-18 of the row maximum per key. O divides by l >= 1 (in units of the
    #    row maximum's term), so 2^-18 |V| summed over the keys the row sees;
    #  * O to bf16 (8 bits): half an ulp is 2^-9 |O|;
    #  * fp32 sums and v_exp_f32: 1e-4 max |V|, the bf16 kernel's test's term.
    # v_scale multiplies the result, so all of it (O_ref carries it already).
    bound = (v_scale * (2.0 ** -4 * pv_abs + 2.0 ** -18 * seen + 1e-4 * v.double().abs().max())
             + 2.0 ** -9 * o_ref.abs())
    err = (o.double() - o_ref).abs()
    print("max err / bound", (err / bound).max().item(), "lse err", (lse.double() - lse_ref).abs().max().item())
    assert bool((err <= bound).all())  # (NaN fails)
    # l is summed in fp32 before P is rounded: the bf16 kernel's tolerance
    assert bool(((lse.double() - lse_ref).abs() <= 1e-4 * lse_ref.abs().clamp(min=1.0)).all())


def test_deadline_form_repeats_the_one_shot_result():
    case = CASES[2]
    q, k, v = problem(case)[:3]
    grid, us = 10, 2000.0  # one block per item: the one-shot run lasts as long as its longest item
    _native.lib().dlnb_wallclock_hz(0)  # (the clock calibration's wait, outside the timings)
    o1, o2 = (torch.full(q.shape, float("nan"), device="cuda", dtype=torch.bfloat16) for _ in range(2))
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
    assert totals[0].item() > 2 * (1 + 2 + 3 + 4 + 5)  # more than one sweep of the 2 heads' 5 Q tiles
    assert per_block.sum().item() == totals[0].item()
    assert totals[1].item() == round(us * 1e-6 * _native.lib().dlnb_wallclock_hz(0))
    assert slots[0].item() > 0
    assert us <= task_us <= us + 3 * item_us


@pytest.mark.parametrize("shape,causal,word", [((1, 2, 2, 192, 128), False, "Sq"), ((1, 2, 2, 128, 256), True, "causal"),
                                               ((1, 3, 2, 128, 128), False, "Hkv")])
def test_launcher_refuses(shape, causal, word):
    B, H, Hkv, Sq, Skv = shape
    q = torch.zeros(B, H, Sq, 128, device="cuda").to(FP8)
    k = torch.zeros(B, Hkv, Skv, 128, device="cuda").to(FP8)
    o = torch.full(q.shape, float("nan"), device="cuda", dtype=torch.bfloat16)
    with pytest.raises(_native.NativeError, match=word):
        attention.attention_fwd(q, k, k, out=o, causal=causal)
    with pytest.raises(TypeError):
        attention.attention_fwd(q, k.to(torch.bfloat16), k, out=o, causal=causal)
    with pytest.raises(ValueError, match="v_scale"):
        attention.attention_fwd(q.to(torch.bfloat16), k.to(torch.bfloat16), k.to(torch.bfloat16), out=o, v_scale=0.5)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all())  # nothing was launched


def test_strategy_runs_with_fp8_attn_compute(data_dir):
    doc = engine.run_native("dp", "tiny_dense_8_bfloat16", 4, base_path=data_dir, warmup=1, runs=2, compute="attn",
                            compute_dtype="fp8", quiet=True)
    c = doc["global"]["dlnb"]["compute"]
    it = doc["global"]["dlnb"]["iteration"]
    print(it["median_ms"], it["compute_floor_ms"], c["attn"])
    assert c["mode"] == "attn" and c["attn"]["dtype"] == "fp8_e4m3"
    assert c["attn"]["TFLOPs"] > 0 and c["attn"]["kv_tile_steps"] > 0
    assert it["median_ms"] >= 0.9 * it["compute_floor_ms"]
