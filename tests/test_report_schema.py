"""The report document's schema, pinned: the tree of key paths of three
CPU-backend runs against tests/golden/report_schema.json (recorded before the
runner was split into setup / replay / report). Key paths only, no values;
the elements of an array collapse into one entry (`[]`).
"""
import json
import os

import pytest

from dlnetbench_amd.utils import launch, report

# The only subtrees left out: their keys are this machine's (the DLNB_* / NCCL_* /
# HSA_* variables of the environment, the runtime libraries found).
MACHINE_KEYED = ("global.dlnb.env", "global.dlnb.runtime")

MODEL = "vit_b_16_bfloat16"  # the smallest model of models/
CASES = {
    "dp_w1": (1, "dp", (MODEL, 4)),
    "fsdp_w2": (2, "fsdp", (MODEL, 4, 2)),
    "hybrid_2d_w2_s2": (2, "hybrid_2d", (MODEL, 2, 4)),
}


def key_paths(node, prefix=""):
    """Sorted key paths of a JSON value; array elements share the path `prefix[]`."""
    out = set()
    if isinstance(node, dict):
        for k, v in node.items():
            p = f"{prefix}.{k}" if prefix else k
            out.add(p)
            if p not in MACHINE_KEYED:
                out |= key_paths(v, p)
    elif isinstance(node, list):
        for v in node:
            if isinstance(v, (dict, list)):
                out.add(prefix + "[]")
                out |= key_paths(v, prefix + "[]")
    return out


def run_case(bindir, root, name):
    n, prog, params = CASES[name]
    cmd = [os.path.join(bindir, prog), *map(str, params), root, "-w", "1", "-r", "2", "--backend", "cpu", "--quiet"]
    code, outs = launch.launch(n, cmd, timeout=120, capture=True)
    assert code == 0, "".join(o or "" for o in outs)[-3000:]
    docs = report.parse_output(outs[0])
    assert len(docs) == 1, outs[0][-2000:]
    return sorted(key_paths(next(iter(docs.values()))))


@pytest.mark.parametrize("name", sorted(CASES))
def test_report_schema_is_unchanged(name, root):
    bindir = os.path.join(root, "build", "bin")
    with open(os.path.join(root, "tests", "golden", "report_schema.json")) as f:
        golden = json.load(f)[name]
    got = run_case(bindir, root, name)
    assert got == golden, {"missing": sorted(set(golden) - set(got)), "new": sorted(set(got) - set(golden))}
