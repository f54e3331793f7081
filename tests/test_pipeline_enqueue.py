"""What every rank enqueues on every stream, against a recording.

Each case runs a strategy binary as loopback-cpu rank threads with --timeline
(one warm-up, one timed iteration, every iteration kept) and reduces the trace
and the report to what does not depend on the clock:

  * per rank and lane (the trace's track name), the ordered list of
    (cat, name, args) of its spans - ts and dur removed; no span argument is
    measured (table_us is the table time, unscaled);
  * per rank, the length of every array in its report section and the
    (nranks, bytes_per_op, ops) of its comm summary;
  * the report's `global` section without the measured or host-dependent
    fields named in DROPPED.

tests/golden/pipeline_enqueue.json holds that for every case, recorded before
the pipeline strategy's steps, link exchanges and set-up were folded; a host
refactor of the strategies must reproduce it exactly. Loopback-cpu runs the
TP / EP collectives on the compute stream (eager), so the inner lane and the
compute program are not covered here.

    python tests/test_pipeline_enqueue.py --record

regenerates the recording (twice, and refuses to write it if the two differ).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "data")
BIN = os.path.join(ROOT, "build", "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden", "pipeline_enqueue.json")

DENSE, DEEP, MOE = "tiny_dense_8_bfloat16", "tiny_deep_8_bfloat16", "tiny_moe_8_bfloat16"
ILV = ["--pp-schedule", "interleaved", "--pp-virtual"]

# id: (ranks, program, positional arguments, options) - the tiny models and tuples of tests/test_cpu_strategies.py
CASES = {
    "gpipe-s1": (1, "hybrid_2d", [DENSE, 1, 2], []),
    "gpipe-s2-mb4": (2, "hybrid_2d", [DENSE, 2, 4], []),
    "gpipe-s2-mb4-buckets2": (2, "hybrid_2d", [DENSE, 2, 4], ["--dp-buckets", 2]),
    "gpipe-s2-mb4-reference": (2, "hybrid_2d", [DENSE, 2, 4], ["--schedule", "reference"]),
    "1f1b-s4-mb2": (4, "hybrid_2d", [DENSE, 4, 2], ["--pp-schedule", "1f1b"]),  # warm-up clipped by mb
    "1f1b-s2-mb8-buckets2": (2, "hybrid_2d", [DENSE, 2, 8], ["--pp-schedule", "1f1b", "--dp-buckets", 2]),
    "interleaved-w2-s2-mb2-v2": (2, "hybrid_2d", [DEEP, 2, 2], ILV + [2]),  # mb == S: all forwards first
    "interleaved-w4-s4-mb4-v3": (4, "hybrid_2d", [DEEP, 4, 4], ILV + [3]),
    "interleaved-w4-s2-mb4-v2-buckets2": (4, "hybrid_2d", [DEEP, 2, 4], ILV + [2, "--dp-buckets", 2]),
    "dualpipe-w2": (2, "hybrid_2d", [DEEP, 2, 4], ["--pp-schedule", "dualpipe"]),
    "dualpipe-w4": (4, "hybrid_2d", [DEEP, 4, 8], ["--pp-schedule", "dualpipe"]),
    "dualpipe-moe": (4, "hybrid_3d_moe", [MOE, 2, 4, 2], ["--pp-schedule", "dualpipe"]),  # whole-gradient mirror
    "3d-microbatch": (4, "hybrid_3d", [DENSE, 2, 2, 2], ["--tp-granularity", "microbatch"]),
    "3d-layer": (4, "hybrid_3d", [DENSE, 2, 2, 2], ["--tp-granularity", "layer"]),
    "3d-sequence-parallel": (4, "hybrid_3d", [DENSE, 2, 2, 2], ["--sequence-parallel"]),
    "moe": (4, "hybrid_3d_moe", [MOE, 2, 2, 2], []),
    "moe-ep-overlap-gpipe": (4, "hybrid_3d_moe", [MOE, 2, 4, 2], ["--pp-schedule", "gpipe", "--ep-overlap"]),
    "moe-ep-overlap-1f1b": (4, "hybrid_3d_moe", [MOE, 2, 4, 2], ["--pp-schedule", "1f1b", "--ep-overlap"]),
    "moe-ep-imbalance": (4, "hybrid_3d_moe", [MOE, 1, 2, 4], ["--ep-imbalance", 1.0]),
    "4d": (8, "hybrid_4d", [MOE, 2, 2, 2, 2], []),
    # buffer allocation / registration order of the other strategies
    "dp": (2, "dp", [DENSE, 5], []),
    "dp-zero2": (2, "dp", [DENSE, 5], ["--zero", 2]),
    "cp-ring": (2, "hybrid_cp", [DENSE, 2], ["--cp-algo", "ring"]),
    "cp-ulysses": (2, "hybrid_cp", [DENSE, 2], ["--cp-algo", "ulysses"]),
}

# Fields of `global` left out, by name at any depth: measured times, and what names the host or the checkout.
DROPPED = {"warmup_times", "timed_region_s", "per_run_max_s", "median_ms", "mean_ms", "p95_ms", "min_ms",
           "timed_ms_per_iter",  # measured
           "stats_file", "path", "env"}  # host / checkout


def _strip(x):
    if isinstance(x, dict):
        return {k: _strip(v) for k, v in x.items() if k not in DROPPED}
    if isinstance(x, list):
        return [_strip(v) for v in x]
    return x


def fingerprint(case):
    ranks, prog, pos, opts = CASES[case]
    with tempfile.TemporaryDirectory() as tmp:
        tl, rep = os.path.join(tmp, "tl.json"), os.path.join(tmp, "r.json")
        cmd = [os.path.join(BIN, prog), *map(str, pos), DATA, *map(str, opts), "--backend", "loopback-cpu", "--ranks",
               str(ranks), "--compute", "sleep", "-w", "1", "-r", "1", "--time-scale", "0.1", "--quiet",
               "--timeline", tl, "--timeline-iters", "0", "--json", rep]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-2000:]
        with open(tl) as f:
            trace = json.load(f)["traceEvents"]
        with open(rep) as f:
            doc = json.load(f)
    lane_name = {(m["pid"], m["tid"]): m["args"]["name"] for m in trace if m["ph"] == "M" and m["name"] == "thread_name"}
    out = {"global": _strip(doc["global"]), "ranks": [{"lanes": {}, "arrays": {}, "comm": {}} for _ in range(ranks)]}
    for e in trace:
        if e["ph"] == "X":
            out["ranks"][e["pid"]]["lanes"].setdefault(lane_name[(e["pid"], e["tid"])], []).append(
                [e["cat"], e["name"], e["args"]])
    for r in doc["ranks"]:
        mine = out["ranks"][r["rank"]]
        mine["arrays"] = {k: len(v) for k, v in r.items() if isinstance(v, list)}
        mine["comm"] = {k: [v["nranks"], v["bytes_per_op"], v["ops"]] for k, v in r["comm"].items()}
    return out


# The recording stores every distinct span once ("spans") and the lanes as indices into that table.
def pack(fp):
    table, index = [], {}
    for r in fp["ranks"]:
        for lane, spans in r["lanes"].items():
            for i, s in enumerate(spans):
                key = json.dumps(s, sort_keys=True)
                if key not in index:
                    index[key] = len(table)
                    table.append(s)
                spans[i] = index[key]
    return dict(fp, spans=table)


def unpack(packed):
    fp = json.loads(json.dumps({k: v for k, v in packed.items() if k != "spans"}))
    for r in fp["ranks"]:
        for lane, idx in r["lanes"].items():
            r["lanes"][lane] = [packed["spans"][i] for i in idx]
    return fp


def first_difference(want, got, where="$"):
    """Path and values of the first entry in which two JSON values differ, or None."""
    if type(want) is not type(got):
        return f"{where}: recorded {want!r}, now {got!r}"
    if isinstance(want, dict):
        for k in list(want) + [k for k in got if k not in want]:
            if k not in want or k not in got:
                return f"{where}.{k}: " + ("not in the recording" if k not in want else "missing now")
            d = first_difference(want[k], got[k], f"{where}.{k}")
            if d:
                return d
        return None
    if isinstance(want, list):
        for i, (a, b) in enumerate(zip(want, got)):
            d = first_difference(a, b, f"{where}[{i}]")
            if d:
                return d
        if len(want) != len(got):
            return f"{where}: recorded {len(want)} entries, now {len(got)}"
        return None
    return None if want == got else f"{where}: recorded {want!r}, now {got!r}"


@pytest.fixture(scope="module")
def golden():
    if not os.path.exists(os.path.join(BIN, "hybrid_2d")):
        pytest.skip("native binaries not built (run make)")
    with open(GOLDEN) as f:
        return json.load(f)


def test_recording_covers_every_case(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("case", list(CASES))
def test_enqueue_fingerprint(case, golden):
    want, got = unpack(golden[case]), fingerprint(case)
    diff = first_difference(want, got)
    if diff:
        print(diff)
    assert want == got, diff


def record():
    first = {c: fingerprint(c) for c in CASES}
    second = {c: fingerprint(c) for c in CASES}
    diff = first_difference(first, second)
    if diff:
        sys.exit("two recordings differ, nothing written: " + diff)
    with open(GOLDEN, "w") as f:
        json.dump({c: pack(fp) for c, fp in first.items()}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes,", len(first), "cases")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    record()
