"""--compute hbm end to end on one MI355X: every strategy family, graph replay, ranks sharing the GPU.

Each run is a child process of the native binary (engine.run_native), as in test_gpu_strategies.py."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


from dlnetbench_amd import engine  # noqa: E402

CASES = [
    ("fsdp", "tiny_dense_8_bfloat16", (4, 1)),
    ("dp", "tiny_dense_8_bfloat16", (4,)),
    ("hybrid_2d", "tiny_dense_8_bfloat16", (1, 4)),
]


def check_hbm_block(c):
    assert c["mode"] == "hbm"
    h = c["hbm"]
    assert h["grid"] == c["num_cus"] - 32
    assert h["bytes_moved"] > 0 and h["busy_s"] > 0 and h["GBps"] > 0
    assert h["working_set_bytes"] <= 3 * (512 << 20) and h["chunk_bytes"] == 65536
    assert h["working_set_bytes"] % (3 * h["chunk_bytes"]) == 0
    return h


@pytest.mark.parametrize("strategy,model,params", CASES)
def test_strategy_runs_with_hbm_compute(strategy, model, params, data_dir):
    doc = engine.run_native(strategy, model, *params, base_path=data_dir, warmup=1, runs=2, compute="hbm",
                            backend="rccl", quiet=True)
    g = doc["global"]
    assert g["backend"] == "RCCL" and g["device"] == "GPU"
    it = g["dlnb"]["iteration"]
    floor = it["compute_floor_ms"]
    print(strategy, it["median_ms"], floor, g["dlnb"]["compute"]["hbm"])
    assert it["median_ms"] >= 0.9 * floor
    assert it["median_ms"] < 3.0 * floor + 5.0
    check_hbm_block(g["dlnb"]["compute"])
    assert "chain_capped" not in doc["ranks"][0]  # no gates, no programs: spin's paths


def test_graph_replay_keeps_the_device_totals(data_dir):
    warmup, runs = 1, 3
    doc = engine.run_native("fsdp", "tiny_dense_8_bfloat16", 4, 1, base_path=data_dir, warmup=warmup, runs=runs,
                            compute="hbm", backend="rccl", quiet=True, graph=True)
    d = doc["global"]["dlnb"]
    assert d["graph"] > 0
    it = d["iteration"]
    floor = it["compute_floor_ms"]
    assert it["median_ms"] >= 0.9 * floor
    assert it["median_ms"] < 1.5 * floor + 5.0
    h = check_hbm_block(d["compute"])
    # every replay's tasks added their ticks: the warm-up's (one more where the lane graphs fell back to a
    # single graph and warmed that once) and the timed runs', each the table's compute time
    iters = warmup + runs + (1 if "fallback" in d.get("lane_graphs", {}) else 0)
    print(h, iters, floor)
    assert abs(h["busy_s"] - iters * floor * 1e-3) <= 0.01 * iters * floor * 1e-3


def test_two_ranks_share_the_gpu(data_dir):
    runs = 2
    doc = engine.run_native("fsdp", "tiny_dense_8_bfloat16", 4, 2, base_path=data_dir, warmup=1, runs=runs,
                            compute="hbm", backend="loopback", ranks=2, quiet=True)
    g = doc["global"]
    assert g["backend"] == "LOOPBACK" and g["world_size"] == 2 and len(doc["ranks"]) == 2
    c = g["dlnb"]["compute"]
    assert c["mode"] == "hbm" and c["hbm"]["grid"] == (c["num_cus"] - 32) // 2  # the ranks split the free CUs
    assert c["hbm"]["bytes_moved"] > 0
    for r in doc["ranks"]:
        assert len(r["runtime"]) == runs  # (the FSDP proxy's iteration timer)
        # the waits for the all-gathers are timed from the streaming tasks' own start stamps
        for k in ("allgather_wait_fwd", "allgather_wait_bwd"):
            assert len(r[k]) >= runs, (k, r[k])
        assert "timer_negative_intervals" not in r, r["timer_negative_intervals"]
