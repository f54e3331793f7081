"""--compute attn on hosts without a GPU: the CPU device's fallback, the mode list, the profile classifier."""
import pytest

from dlnetbench_amd import _native, engine
from dlnetbench_amd.tools import prof_merge


def test_attn_falls_back_to_sleep_on_the_cpu_device(data_dir):
    doc = engine.run("dp", "tiny_dense_8_bfloat16", 4, base_path=data_dir, backend="cpu", compute="attn", warmup=1,
                     runs=2, quiet=True)
    c = doc["global"]["dlnb"]["compute"]
    assert c["mode"] == "attn" and c["effective_mode"] == "sleep"
    assert "attn" not in c  # nothing computed: no rate block


def test_unknown_mode_error_lists_attn(data_dir):
    with pytest.raises(_native.NativeError) as e:
        engine.run("dp", "tiny_dense_8_bfloat16", 4, base_path=data_dir, backend="cpu", compute="nope", warmup=0,
                   runs=1, quiet=True)
    assert "attn" in str(e.value).split("(", 1)[1]


def test_prof_merge_gives_the_attention_kernel_its_own_class():
    name = ("void dlnb::kernels::(anonymous namespace)::attention_fwd_kernel<true>(__bf16 const*, __bf16 const*, "
            "__bf16 const*, __bf16*, float*, int, int, int, int, int, float, int, unsigned long, unsigned long*, "
            "unsigned long*, unsigned long*, unsigned long*)")
    assert prof_merge.classify(name) == "compute_attn"
