"""--compute hbm on hosts without a GPU: the CPU device's fallback, the mode list, the profile classifier."""
import pytest

from dlnetbench_amd import _native, engine
from dlnetbench_amd.tools import prof_merge


def test_hbm_falls_back_to_sleep_on_the_cpu_device(data_dir):
    doc = engine.run("dp", "tiny_dense_8_bfloat16", 4, base_path=data_dir, backend="cpu", compute="hbm", warmup=1,
                     runs=2, quiet=True)
    c = doc["global"]["dlnb"]["compute"]
    assert c["mode"] == "hbm" and c["effective_mode"] == "sleep"
    assert "hbm" not in c  # nothing streamed: no bandwidth block
    it = doc["global"]["dlnb"]["iteration"]
    assert it["median_ms"] >= 0.9 * it["compute_floor_ms"]


def test_unknown_mode_error_lists_every_mode(data_dir):
    with pytest.raises(_native.NativeError) as e:
        engine.run("dp", "tiny_dense_8_bfloat16", 4, base_path=data_dir, backend="cpu", compute="nope", warmup=0,
                   runs=1, quiet=True)
    msg = str(e.value)
    assert "unknown compute mode 'nope'" in msg
    for mode in ("auto", "sleep", "spin", "gemm", "gemm-work", "flops", "hbm"):
        assert mode in msg.split("(", 1)[1], (mode, msg)


def test_prof_merge_gives_the_streaming_kernel_its_own_class(tmp_path):
    name = ("void dlnb::kernels::(anonymous namespace)::hbm_stream_kernel<true>(__bf16 const*, __bf16 const*, "
            "__bf16*, unsigned long, unsigned long, unsigned long*, unsigned long*, unsigned long*, unsigned long*)")
    assert prof_merge.classify(name) == "compute_hbm"
    assert prof_merge.classify("busy_spin_kernel(unsigned long, float*)") == "compute_wait"
    p = tmp_path / "x_kernel_trace.csv"
    p.write_text('"Kernel_Name","Start_Timestamp","End_Timestamp"\n'
                 f'"{name}",1000000,3000000\n'
                 '"dlnb::kernels::busy_spin_kernel(unsigned long, float*)",3000000,4000000\n'
                 f'"{name}",4000000,5000000\n')
    cls = prof_merge.collect([str(tmp_path)])
    assert cls["compute_hbm"]["calls"] == 2 and abs(cls["compute_hbm"]["time_ms"] - 3.0) < 1e-9
    assert cls["compute_wait"]["calls"] == 1
    assert list(cls["compute_hbm"]["kernels"]) == ["void dlnb::kernels::hbm_stream_kernel<true>"]
