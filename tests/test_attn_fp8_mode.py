"""--compute attn --compute-dtype fp8 on hosts without a GPU: the CPU device's fallback and the profile classifier."""
from dlnetbench_amd import engine
from dlnetbench_amd.tools import prof_merge


def test_fp8_attn_falls_back_to_sleep_on_the_cpu_device(data_dir):
    doc = engine.run("dp", "tiny_dense_8_bfloat16", 4, base_path=data_dir, backend="cpu", compute="attn",
                     compute_dtype="fp8", warmup=1, runs=2, quiet=True)
    c = doc["global"]["dlnb"]["compute"]
    assert c["mode"] == "attn" and c["effective_mode"] == "sleep"
    assert "attn" not in c  # nothing computed: no rate block


def test_prof_merge_files_the_fp8_kernel_under_compute_attn():
    name = ("void dlnb::kernels::(anonymous namespace)::attention_fwd_fp8_kernel<true>(char const*, char const*, "
            "char const*, __bf16*, float*, int, int, int, int, int, float, float, int, unsigned long, unsigned long*, "
            "unsigned long*, unsigned long*, unsigned long*)")
    assert prof_merge.classify(name) == "compute_attn"
