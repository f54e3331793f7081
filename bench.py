#!/usr/bin/env python3
"""Headline benchmark: Llama-3-8B FSDP proxy iteration on N MI355X GPUs.

Metric (BASELINE.json): proxy iteration time (ms) + effective GB/s for the
Llama-3-8B FSDP proxy (model_stats/llama3_8b_16_bfloat16.txt: local batch
16, seq 8192, 8.03 B parameters, B200-roofline fwd/bwd times of the
reference's tables), 32 FSDP units, sharding factor = N (fully sharded over
the GPUs of the job), bf16 on the wire, compute = hand-written MFMA GEMMs
bounded to the table's times. One process per GPU; under torchrun every
rank runs this file. Weak scaling: each GPU keeps its local batch of 16.

A plain run does only what the headline needs: it sets up, warms up, times
the K steps (one child process of the native binary per rank), writes the
step's outputs when ``--dump-outputs DIR`` is given, and prints the line.
Read off the headline's own report, at no extra cost:

* ``slow_iterations``: per timed iteration of the headline, the slowest
  rank's last collective (its duration), its GPU's sclk at the iteration's
  end and the lowest 5-ms sample inside it, and the power at the end (hwmon);
  ``slow`` lists the iterations over median + 0.1 ms.

``--dump-outputs DIR``: after the timed steps rank 0 writes what the last
step left in the FSDP step's result buffers to ``DIR/<name>.npy`` (float32):
every unit's reduced gradient shard (``grad_shard_NNN``), the two gather
buffers (``gathered_params_0/1``: the parameters of units 0 and 1, gathered
last) and the stand-in GEMM's product (``gemm_product``, C = A.B^T of the
compute tasks). At most 48 MB in all: a larger buffer is written as a fixed
sample (blocks of 1024 elements, one per equal stretch of the buffer, at
offsets hashed from the buffer's name). All buffers are filled from fixed
seeds, so two runs with the same arguments write the same files.

The headline is compute-bound by construction (2.8 s of compute against
~40 ms of all-link collectives at N = 8), so with ``--full`` secondary
measurements, each a run of its own, ride along as extra keys of the same
JSON line, and at N > 1 the exactness pass of
the collectives runs before anything is timed:

* ``comm_bound``: the ViT-H/32 fp8 data-parallel proxy (BASELINE config 5,
  model_stats/vit_h_32_float8.txt: 7.13 ms of compute, a 1.26 GB bf16
  gradient all-reduce in 8 buckets) - the one baseline config where
  communication dominates; iteration time, exposed communication
  (barrier_time) and all-reduce bus bandwidth.
* ``comm_bound.rccl_default_ctas``: the same step with RCCL choosing its own
  CTA count instead of the ``maxCTAs`` cap that fits every comm lane into
  the 32 CUs the deadline compute leaves free (what the budget costs the
  all-reduce over the links).
* ``comm_bound.gemm_work``: the same with fixed-work compute (the GEMM count
  calibrated to the table time with nothing else running), so collective
  interference shows up as a longer iteration and ``compute_stretch`` > 1.
* ``compute_stretch``: the headline FSDP configuration with fixed-work
  compute for a few iterations (task time under the concurrent
  all-gathers / reduce-scatters over the uncontended time).
* ``comm_bound_xgmi`` (N > 1): the comm-bound ViT-H DP run again over our
  own xGMI collective kernels (``--backend xgmi``, HIP graph) instead of
  RCCL, with the RCCL/xgmi time ratio. It runs last, in a child process per
  rank with a short device-wait timeout, so a failure there can only cost
  this block, never the headline.
* ``headline_xgmi`` (N > 1): the headline FSDP step itself over the xgmi
  kernels (zero-copy all-gather / reduce-scatter into registered buffers),
  with its effective bus bandwidth as a ratio of the headline's (RCCL).
  Also a child process per rank, after ``comm_bound_xgmi``.

* ``model_fit`` (N > 1): the cost model's eta and alpha fitted to the
  link_bench times, and every block's prediction redone with them.
* ``timeline`` (N > 1): the headline configuration for 2 more iterations
  with ``--timeline`` (device-clock spans on every rank), summarised: the
  largest exposed communication of any rank, the fraction of communication
  that ran under compute, and each collective's mean duration and bus
  bandwidth on the device clock while the compute ran beside it.
* ``link_bench`` (N > 1): every collective's bus bandwidth at 16 MB and 128 MB
  per rank on the job's GPUs with nothing else running, over RCCL, the xgmi
  kernels (staged) and the xgmi zero-copy path (``dlnb commtest --bench``,
  HIP-graph replayed): the links' side of the numbers above.

At N = 1 a "collective" is a local device copy: bus bandwidth is reported
as null (nccl-tests convention: nothing crosses a link).

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
       (N > 1: torchrun --nproc-per-node N ... bench.py --gpus N ...)
Prints one JSON line on rank 0.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
from typing import Any, Dict, Optional

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "proxy iter time (ms) + effective GB/s, Llama-3-8B DP/FSDP at 1/2/4/8 MI355X"
# the reference publishes no numbers; the derived C2 compute
# floor (fwd + bwd of llama3_8b_16_bfloat16 = 2814.7 ms) is the number an
# ideal overlap would hit on any hardware.
BASELINE_MS = 2814.74976
DEFAULT_MODEL = "llama3_8b_16_bfloat16"
C5_MODEL = "vit_h_32_float8"
# BASELINE configs C3 / C4 (8 GPUs): llama3_70b hybrid_3d S=2 mb=4 T=4 and
# mixtral hybrid_3d_moe S=2 mb=16 EP=4; GPipe floors 3.81 s and 13.56 s.
C3_MODEL, C3_PARAMS = "llama3_70b_16_bfloat16", "2,4,4"
C4_MODEL, C4_PARAMS = "mixtral_8x7b_16_bfloat16", "2,16,4"


def _store_env(world: int, rank: int, attempt: str = "") -> None:
    """Point the native runtime's TCP rendezvous store at this torchrun job.

    Single node (the bench's case): rank 0's store binds an ephemeral port
    and publishes host:port in a file named after torchrun's MASTER_PORT, the
    launcher's pid and the phase (`attempt`: every benchmark run of this
    process rendezvouses on a fresh store, so a file from an earlier phase or
    job is never read); the other ranks poll that file (DLNB_STORE_FILE).
    Multi-node: MASTER_PORT + 1 + phase index."""
    os.environ.pop("DLNB_STORE_ADDR", None)
    os.environ.pop("DLNB_STORE_FILE", None)
    if world == 1:
        return
    host = os.environ.get("MASTER_ADDR", "127.0.0.1")
    port = int(os.environ.get("MASTER_PORT", "29500"))
    if int(os.environ.get("LOCAL_WORLD_SIZE", world)) != world:
        phase = sum(ord(c) for c in attempt) % 97 if attempt else 0
        os.environ["DLNB_STORE_ADDR"] = f"{host}:{port + 1 + phase}"
        return
    path = f"/tmp/dlnb_bench_store_{port}_{os.getppid()}{attempt}"
    os.environ["DLNB_STORE_FILE"] = path
    if rank == 0:
        import atexit
        atexit.register(lambda: os.path.exists(path) and os.remove(path))


def _busbw(doc: dict, kind: str, world: int) -> Optional[float]:
    """Mean over ranks of one collective's bus bandwidth; None at 1 rank."""
    if world <= 1:
        return None
    vals = [r["comm"][kind]["busbw_GBps"] for r in doc["ranks"] if "busbw_GBps" in r["comm"].get(kind, {})]
    return float(f"{sum(vals) / len(vals):.4g}") if vals else None


def _algbw(doc: dict, kind: str) -> Optional[float]:
    vals = [r["comm"][kind]["algbw_GBps"] for r in doc["ranks"] if "algbw_GBps" in r["comm"].get(kind, {})]
    return round(sum(vals) / len(vals), 2) if vals else None


def _energy(doc: dict) -> Optional[Dict[str, float]]:
    per_rank = [sum(r["energy_consumed"]) / len(r["energy_consumed"]) for r in doc["ranks"]
                if r.get("energy_consumed")]
    if not per_rank or not any(per_rank):
        return None
    return {"all_gpus": round(sum(per_rank), 2), "per_gpu": round(sum(per_rank) / len(per_rank), 2)}


def _mean_of(doc: dict, key: str) -> Optional[float]:
    """Mean over ranks and runs of a per-rank timer (seconds) -> ms."""
    vals = [v for r in doc["ranks"] for v in r.get(key, [])]
    return round(sum(vals) / len(vals) * 1e3, 4) if vals else None


def _run_bounded(cmd: list, env: dict, timeout: float, stdout: Any = subprocess.PIPE) -> subprocess.CompletedProcess:
    """subprocess.run with the child killed at `timeout` and reported as an
    error (never an exception that skips the rest of the bench)."""
    try:
        return subprocess.run(cmd, env=env, timeout=timeout, stdout=stdout, stderr=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired as e:
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        raise RuntimeError(f"timeout after {timeout:.0f} s (wall budget): " + err[-200:]) from None


class _Budget:
    """The bench's wall-clock budget (the N > 1 run must print
    its line within a bounded time, whatever hangs). Every phase after the
    headline asks plan(name, want_s, need_s) for its child's time limit: the
    smaller of what it wants and what is left (minus a reserve for the final
    line); None = skip the phase (less than need_s left). All ranks must take
    the same decisions (a rank that skips a phase its peers run leaves them
    waiting at a rendezvous), so on one node rank 0 decides and publishes
    each decision in a file the other ranks wait for; across nodes every rank
    decides from its own clock (the phases are lockstep, so the clocks agree
    to the rendezvous skew)."""

    def __init__(self, total_s: float, reserve_s: float, world: int, rank: int) -> None:
        import time
        self._t = time.monotonic
        self.start = self._t()
        self.total, self.reserve, self.world, self.rank = total_s, reserve_s, world, rank
        # one node (torchrun's LOCAL_WORLD_SIZE == WORLD_SIZE): rank 0's plan files;
        # otherwise (several nodes, or a launcher that does not say) own clocks
        self.shared = world > 1 and int(os.environ.get("LOCAL_WORLD_SIZE", "0")) == world
        self.dir = f"/tmp/dlnb_bench_plan_{os.environ.get('MASTER_PORT', '0')}_{os.getppid()}"
        self.plans: Dict[str, Any] = {}
        self.seen_dir = False
        if self.shared and rank == 0:
            import atexit
            import shutil
            os.makedirs(self.dir, exist_ok=True)
            atexit.register(lambda: shutil.rmtree(self.dir, ignore_errors=True))

    def left(self) -> float:
        return self.total - (self._t() - self.start) - self.reserve

    def plan(self, name: str, want_s: float, need_s: float) -> Optional[float]:
        import time
        if not self.shared or self.rank == 0:
            left = self.left()
            t = round(min(want_s, left), 1)
            dec = t if t >= need_s and t > 0 else None
            if self.shared:
                tmp = os.path.join(self.dir, name + ".tmp")
                with open(tmp, "w") as f:
                    json.dump({"timeout": dec}, f)
                os.replace(tmp, os.path.join(self.dir, name + ".json"))
        else:
            path = os.path.join(self.dir, name + ".json")
            deadline = self._t() + max(30.0, self.left() + self.reserve)
            dec = None
            while self._t() < deadline:
                if os.path.exists(path):
                    try:
                        with open(path) as f:
                            dec = json.load(f)["timeout"]
                    except FileNotFoundError:
                        # rank 0 finished between the check and the read (its exit removes the plans):
                        # nothing more runs with it - skip, as when the directory is already gone
                        dec = None
                    break
                if os.path.isdir(self.dir):
                    self.seen_dir = True
                elif self.seen_dir:
                    break  # rank 0 has finished (and removed the plans): nothing more runs
                time.sleep(0.02)
        self.plans[name] = dec
        return dec

    def report(self) -> Dict[str, Any]:
        return {"wall_budget_s": self.total, "reserve_s": self.reserve,
                "timeouts_s": {k: v for k, v in self.plans.items() if v is not None},
                "skipped": [k for k, v in self.plans.items() if v is None]}


def _skipped(budget: _Budget) -> Dict[str, Any]:
    return {"skipped": f"wall budget ({budget.total:.0f} s) left too little time for this block"}


def _child_run(a: argparse.Namespace, world: int, rank: int, tag: str, strategy: str, model: str,
               params: tuple, timeout: float, backend: str = "xgmi", graph: bool = True,
               **kw: Any) -> Dict[str, Any]:
    """One benchmark run by the native binary as a child of every rank (its
    own rendezvous, a bounded wall time); rank 0 returns the child's report."""
    from dlnetbench_amd import engine
    _store_env(world, rank, tag)
    out = f"/tmp/dlnb_bench{tag}_{os.environ.get('MASTER_PORT', '0')}_{os.getppid()}.json"
    args = engine.build_args(strategy, model, *params, base_path=a.base_path, backend=backend,
                             graph=graph or None, devices=a.devices, time_scale=a.time_scale, silent=True,
                             json=out if rank == 0 else None, **kw)
    env = dict(os.environ, DLNB_XGMI_TIMEOUT_S=os.environ.get("DLNB_XGMI_TIMEOUT_S", "20"),
               DLNB_BLOCK=tag.lstrip("."), DLNB_STORE_TIMEOUT=str(max(10, int(timeout))))
    # bounded by the wall budget (_Budget), so a first-time cross-device
    # failure costs this block and the line still prints
    p = _run_bounded([os.path.join(ROOT, "build", "bin", strategy), *args], env, timeout, stdout=sys.stderr)
    if p.returncode != 0:
        raise RuntimeError(f"exit {p.returncode}: " + (p.stderr or "")[-300:])
    if rank != 0:
        return {}
    with open(out) as f:
        d = json.load(f)
    os.remove(out)
    return d


def _xgmi_child(a: argparse.Namespace, world: int, rank: int, tag: str, strategy: str, model: str,
                params: tuple, timeout: float, **kw: Any) -> Dict[str, Any]:
    """One benchmark run over the xgmi backend (HIP graph) as a child of every rank."""
    return _child_run(a, world, rank, tag, strategy, model, params, timeout, backend="xgmi", graph=True,
                      compute=a.compute, **kw)


def _exact_backends(a: argparse.Namespace) -> str:
    """Backends the exactness pass checks: the CPU backend on CPU runs; on the
    GPU RCCL and the xgmi kernels, or xgmi alone when ranks share a GPU (RCCL
    refuses that)."""
    if a.backend == "cpu":
        return "cpu"
    devs = [d for d in (a.devices or "").split(",") if d.strip()]
    shared = len(devs) != len(set(devs))
    if a.backend == "xgmi" or shared:
        return "xgmi"
    return "rccl,xgmi"


def _exactness(a: argparse.Namespace, world: int, rank: int, timeout: float) -> Dict[str, Any]:
    """Before any timed phase of a multi-rank job: every collective (all-reduce
    in and out of place, all-gather, reduce-scatter, all-to-all, ring
    send/recv) of every backend the bench times, eager and graph-replayed
    (xgmi also zero-copy registered), bf16 and fp8, at 3 sizes, checked
    exactly across the real ranks (`dlnb commtest --suite`, a child of every
    rank). xgmi runs with the vmcnt release first and the system-scope one if
    that fails. Returns the suite report (identical on every rank: its
    verdicts are all-reduced)."""
    _store_env(world, rank, ".exact")
    out = f"/tmp/dlnb_bench.exact_{os.environ.get('MASTER_PORT', '0')}_{os.getppid()}_{rank}.json"
    cmd = [os.path.join(ROOT, "build", "bin", "dlnb"), "commtest", "--suite", "--backends", _exact_backends(a),
           "--dtypes", a.exact_dtypes, "--sizes", a.exact_sizes, "--release-fallback", "--json", out]
    if a.devices:
        cmd += ["-d", a.devices]
    env = dict(os.environ, DLNB_XGMI_TIMEOUT_S=os.environ.get("DLNB_EXACT_XGMI_TIMEOUT_S", "10"),
               DLNB_STORE_TIMEOUT=str(max(10, int(timeout))), DLNB_BLOCK="exact")
    p = _run_bounded(cmd, env, timeout)
    if not os.path.exists(out):
        raise RuntimeError(f"exit {p.returncode}: " + (p.stderr or "")[-300:])
    with open(out) as f:
        d = json.load(f)
    os.remove(out)
    return d


def _link_bench(a: argparse.Namespace, world: int, rank: int, backend: str, registered: bool,
                timeout: float) -> Dict[str, Any]:
    """Collective bandwidth on the job's own GPUs, nothing else running
    (`dlnb commtest --bench --graph`: 10 graph-replayed ops per size after 3
    warm-ups, nccl-tests algbw / busbw, max time over ranks): what the links
    give each collective of the backend, next to what the strategies got.
    Returns {op: {elements: {"busbw_GBps", "time_us"}}} on rank 0."""
    tag = ".lb" + backend + ("r" if registered else "")
    _store_env(world, rank, tag)
    cmd = [os.path.join(ROOT, "build", "bin", "dlnb"), "commtest", "--bench", "--backend", backend,
           "--dtype", "bf16", "--sizes", a.link_sizes, "--iters", "10", "--warmup", "3"]
    if backend != "cpu":
        cmd.append("--graph")
    if registered:
        cmd.append("--registered")
    if a.devices:
        cmd += ["-d", a.devices]
    env = dict(os.environ, DLNB_XGMI_TIMEOUT_S=os.environ.get("DLNB_XGMI_TIMEOUT_S", "20"),
               DLNB_STORE_TIMEOUT=str(max(10, int(timeout))), DLNB_BLOCK="link_" + backend)
    p = _run_bounded(cmd, env, timeout)
    if p.returncode != 0:
        raise RuntimeError(f"exit {p.returncode}: " + (p.stderr or "")[-300:])
    if rank != 0:
        return {}
    out: Dict[str, Any] = {}
    for ln in p.stdout.splitlines():
        if not ln.startswith("{"):
            continue
        j = json.loads(ln)
        if j.get("commtest") != "bench" or j["op"] == "copy":
            continue
        out.setdefault(j["op"], {})[str(int(j["count"]))] = {"busbw_GBps": round(j["busbw_GBps"], 2),
                                                             "time_us": round(j["time_us"], 1)}
    return out


def _link_block(a: argparse.Namespace, world: int, rank: int, xgmi_ok: bool, budget: "_Budget",
                est: "_Estimator") -> Dict[str, Any]:
    """RCCL, xgmi staged and xgmi zero-copy collective bandwidth at N > 1."""
    res: Dict[str, Any] = {"dtype": "bf16", "elements_per_rank": [int(x) for x in a.link_sizes.split(",")],
                           "hip_graph": a.backend != "cpu"}
    checked = _exact_backends(a)  # the backends these ranks can run (ranks sharing a GPU: no RCCL)
    runs = [("cpu", "cpu", False)] if checked == "cpu" else [("rccl", "rccl", False)] if "rccl" in checked else []
    if checked != "cpu":
        if xgmi_ok:
            runs += [("xgmi", "xgmi", False), ("xgmi_registered", "xgmi", True)]
        else:
            res["xgmi"] = {"error": "skipped: the xgmi exactness check failed on these ranks"}
    for key, backend, reg in runs:
        t = budget.plan("link_bench_" + key, min(a.link_timeout, 2 * est.setup + 40), est.setup + 5)
        if t is None:
            res[key] = _skipped(budget)
            continue
        try:
            res[key] = _link_bench(a, world, rank, backend, reg, t)
        except Exception as e:  # noqa: BLE001
            res[key] = {"error": str(e)[:300]}
    return res


def _exact_block(a: argparse.Namespace, world: int, rank: int, timeout: float) -> Dict[str, Any]:
    res: Dict[str, Any] = {}
    try:
        d = _exactness(a, world, rank, timeout)
        res = {"exact": d["exact"], "exact_detail": {
            "ok": d["ok"], "seconds": round(d["seconds"], 2), "sizes": d["sizes"], "xgmi_release": d["xgmi_release"],
            "rccl_nranks": d["rccl_nranks"], "world_size": d["world_size"],
            "failed": [f"{r['backend']}/{r['mode']}/{r['dtype']}" + (f"/{r['release']}" if r.get("release") else "")
                       for r in d["results"] if not r["ok"]]}}
    except Exception as e:  # noqa: BLE001
        res = {"exact": {}, "exact_detail": {"error": str(e)[:300]}}
    return res


class _Phases:
    """Wall seconds of every bench phase on this rank (the line's
    ``phase_seconds``: where the driver's run time went)."""

    def __init__(self) -> None:
        import time
        self._t = time.monotonic
        self.start = self._t()
        self.s: Dict[str, float] = {}

    def add(self, name: str, t0: float) -> None:
        self.s[name] = round(self._t() - t0, 2)

    def now(self) -> float:
        return self._t()

    def report(self) -> Dict[str, float]:
        return dict(self.s, total=round(self._t() - self.start, 2))


class _Estimator:
    """Expected wall seconds of a child run, for its time limit: setup (the
    headline's own: process start, RCCL / xgmi communicators, buffers, graph
    capture; scaled for the hybrids' larger working sets) + its iterations at
    the xGMI cost model's iteration time (x --time-scale), or the headline's
    measured one. A block's limit is 2x that + 20 s, capped by its flag and by
    the wall budget (_Budget.plan)."""

    def __init__(self, a: argparse.Namespace, world: int, headline_s: float, headline_iters: int,
                 headline_ms: float) -> None:
        self.a, self.world = a, world
        self.head_ms = headline_ms
        self.setup = max(5.0, 1.5 * (headline_s - headline_iters * headline_ms / 1e3))

    def iter_s(self, strategy: str, model: str, params: tuple, **kw: Any) -> float:
        a = self.a
        try:
            from dlnetbench_amd.parallel.plan import predict
            ms = predict(strategy, model, list(params), self.world, base=a.base_path, **kw)["iter_ms"]
        except Exception:  # noqa: BLE001
            ms = self.head_ms
        return ms * (a.time_scale if a.time_scale is not None else 1.0) / 1e3

    def want(self, nominal_s: float, cap_s: float) -> float:
        return min(cap_s, 2.0 * nominal_s + 20.0)


def _predicted_ms(a: argparse.Namespace, world: int, strategy: str, model: str, params: tuple,
                  **kw: Any) -> Optional[float]:
    """The xGMI cost model's iteration time for this run (parallel/plan.py
    predict: direct all-link collectives at 75 % of 153 GB/s per link, 15 us
    each): what the measured value should land near on an 8 x MI355X node.
    None when compute is time-scaled or the model has no prediction."""
    if a.time_scale is not None:
        return None
    try:
        from dlnetbench_amd.parallel.plan import predict
        return round(predict(strategy, model, list(params), world, base=a.base_path, **kw)["iter_ms"], 3)
    except Exception:  # noqa: BLE001
        return None


def _model_fit(a: argparse.Namespace, world: int, extra: Dict[str, Any]) -> Optional[Dict[str, Any]]:
    """The cost model refitted to this node: eta and alpha from the measured
    link_bench times (xgmi_model.fit_link_model), then every block's
    prediction again with them - what the links measured here say the
    strategies should take."""
    try:
        from dlnetbench_amd.parallel.xgmi_model import fit_link_model
        lb = extra["link_bench"]
        key = next((k for k in ("rccl", "xgmi_registered", "xgmi", "cpu") if isinstance(lb.get(k), dict)
                    and "error" not in lb[k] and lb[k]), None)
        if key is None:
            return None
        f = fit_link_model(lb[key], world)
        if not f.get("eta"):
            # (noisy link timings - a loaded host's CPU backend - can leave no positive fit)
            return {"backend": key, "error": "no fit: the link timings gave eta " + str(f.get("eta"))}
        kw = {"eta": f["eta"], "alpha_us": f["alpha_us"]}
        pred: Dict[str, Any] = {"headline": _predicted_ms(a, world, "fsdp", a.model, (a.units, world), **kw)}
        if "comm_bound" in extra:
            pred["comm_bound"] = _predicted_ms(a, world, "dp", a.c5_model, (a.c5_buckets,), wire=a.c5_wire, **kw)
        for name, model, params, ov in (("hybrid_3d", a.c3_model, a.c3, False),
                                        ("hybrid_3d_moe", a.c4_model, a.c4, False),
                                        ("hybrid_3d_moe_ep_overlap", a.c4_model, a.c4, True)):
            if name.split("_ep_")[0] in extra:
                strat = "hybrid_3d" if name == "hybrid_3d" else "hybrid_3d_moe"
                pred[name] = _predicted_ms(a, world, strat, model, tuple(int(x) for x in params.split(",")),
                                           ep_overlap=ov, **kw)
        return {"backend": key, "eta": f["eta"], "alpha_us": f["alpha_us"], "per_op": f["per_op"],
                "predicted_ms": pred}
    except Exception as e:  # noqa: BLE001
        return {"error": str(e)[:300]}


def _rank_ms(d: dict) -> Optional[Dict[str, Any]]:
    """Mean iteration time of each rank (its own host timer, ms): min / max and the slowest rank."""
    means = {}
    for r in d.get("ranks", []):
        v = r.get("runtime") or r.get("runtimes")
        if v:
            means[int(r.get("rank", len(means)))] = sum(v) / len(v) * 1e3
    if not means:
        return None
    slow = max(means, key=means.get)
    return {"min": round(min(means.values()), 3), "max": round(means[slow], 3), "slowest_rank": slow}


def _per_run_ms(d: dict) -> list:
    """Every timed iteration's time (ms): the slowest rank's per run."""
    return [round(x * 1e3, 3) for x in d["global"]["dlnb"]["iteration"].get("per_run_max_s", [])]


def _slow_iterations(d: dict, margin_ms: float = 0.1) -> Optional[Dict[str, Any]]:
    """Attribution of the iterations slower than median + margin: per timed iteration the
    slowest rank's time, that rank's last collective's duration and its GPU's sclk (at the iteration's end,
    and the lowest 5-ms sample inside it) and power at the end (hwmon)."""
    per = _per_run_ms(d)
    if not per:
        return None
    ranks = d.get("ranks") or []
    slow_rank = (_rank_ms(d) or {}).get("slowest_rank", 0)
    r = next((x for x in ranks if x.get("rank", 0) == slow_rank), ranks[0] if ranks else {})

    def col(key, scale=1.0, nd=3):
        v = r.get(key)
        return [round(x * scale, nd) for x in v] if isinstance(v, list) and len(v) == len(per) else None

    med = sorted(per)[len(per) // 2]

    def per_iter_sum(keys):  # the timers' entries of each iteration, summed (ms)
        tot = [0.0] * len(per)
        found = False
        for k in keys:
            v = r.get(k)
            if not isinstance(v, list) or not v or len(v) % len(per):
                continue
            n = len(v) // len(per)
            found = True
            for i in range(len(per)):
                tot[i] += sum(v[i * n:(i + 1) * n]) * 1e3
        return [round(x, 3) for x in tot] if found else None

    out = {"rank": slow_rank, "median_ms": med, "max_minus_median_ms": round(max(per) - med, 3),
           "last_collective": r.get("iteration_last_collective"),
           "last_collective_ms": col("iteration_last_collective_ms"),
           # the exposed-communication waits of each iteration (device clock): a slow iteration whose waits did
           # not grow lost its time elsewhere (launch, host)
           "exposed_ms": per_iter_sum(("barrier_time", "allgather", "allgather_wait_fwd", "allgather_wait_bwd",
                                       "barrier", "pp_comm_time", "tp_comm_time", "ep_comm_time",
                                       "dp_exposed_time", "cp_exposed_time", "param_allgather_exposed")),
           "sclk_mhz": col("iteration_sclk_mhz", nd=0), "sclk_min_mhz": col("iteration_sclk_min_mhz", nd=0),
           "power_w": col("iteration_power_w", nd=1)}
    pl = r.get("prearm_launch_ms")  # host time of each pre-armed launch (issued during the iteration before)
    if isinstance(pl, list) and pl:
        out["prearm_launch_ms"] = [round(x, 3) for x in pl]
    out["slow"] = [i for i, x in enumerate(per) if x > med + margin_ms]
    return out


def _hybrid_block(a: argparse.Namespace, world: int, rank: int, tag: str, strategy: str, model: str,
                  params: tuple, floor_note: str, budget: "_Budget", est: "_Estimator", runs: int,
                  ep_overlap: bool = False) -> Dict[str, Any]:
    """One BASELINE hybrid config (C3 hybrid_3d / C4 hybrid_3d_moe) on the job's
    GPUs over RCCL: 1 warm-up + `runs` timed iterations in a child process
    (every run's time in per_run_ms; the reference's hybrid_3d default is 3
    runs, cpp/hybrid_parallel/hybrid_3d.cpp:62 - as many as the wall budget
    affords), its time against the GPipe compute floor and the xGMI model's
    prediction, and its per-group communication. ep_overlap: the same config
    with --ep-overlap (each half-microbatch's all-to-all under the other
    half's compute instead of on the compute stream)."""
    res: Dict[str, Any] = {"model": model, "strategy": strategy, "params": list(params), "backend": "RCCL"}
    if ep_overlap:
        res["ep_overlap"] = True
    nominal = 2 * est.setup + 10 + (1 + runs) * est.iter_s(strategy, model, params, ep_overlap=ep_overlap)
    t = budget.plan(tag.lstrip("."), est.want(nominal, a.hybrid_timeout), nominal)
    if t is None:
        res.update(_skipped(budget))
        return res
    try:
        d = _child_run(a, world, rank, tag, strategy, model, params, t, backend=a.hybrid_backend,
                       graph=False, compute=a.compute, warmup=1, runs=runs, ep_overlap=ep_overlap or None)
        if rank != 0:
            return res
        g, it = d["global"], d["global"]["dlnb"]["iteration"]
        res["per_run_ms"] = _per_run_ms(d)
        pred = _predicted_ms(a, world, strategy, model, params, ep_overlap=ep_overlap)
        res.update({"ms_per_step": round(it["timed_ms_per_iter"], 3), "median_ms": round(it["median_ms"], 3),
                    "floor_ms": round(it["compute_floor_ms"], 3), "floor_note": floor_note,
                    "vs_floor": round(it["timed_ms_per_iter"] / it["compute_floor_ms"], 4)
                    if it["compute_floor_ms"] else None,
                    "predicted_ms": pred,
                    "vs_predicted": round(it["timed_ms_per_iter"] / pred, 4) if pred else None,
                    "backend": g["backend"], "rccl_nranks": g["dlnb"].get("rccl_nranks")})
        for k in ("pp_comm_time", "dp_comm_time", "tp_comm_time", "ep_comm_time", "dp_ep_comm_time"):
            v = _mean_of(d, k)
            if v is not None:
                res[k + "_ms"] = v
        bw = {}
        for k in ("tp_allreduce", "ep_alltoall", "dp_allreduce", "sendrecv"):
            b = _busbw(d, k, world)
            if b is not None:
                bw[k] = b
        res["busbw_GBps"] = bw
    except Exception as e:  # noqa: BLE001
        res["error"] = str(e)[:300]
    return res


def _xgmi_ab(a: argparse.Namespace, world: int, rank: int, c5: dict, budget: "_Budget",
             est: "_Estimator") -> Dict[str, Any]:
    """The comm-bound DP secondary over the xgmi backend (HIP graph)."""
    res: Dict[str, Any] = {"backend": "XGMI", "hip_graph": True}
    nominal = est.setup + (5 + a.c5_steps) * est.iter_s("dp", a.c5_model, (a.c5_buckets,), wire=a.c5_wire)
    t = budget.plan("comm_bound_xgmi", est.want(nominal, 90), nominal)
    if t is None:
        return _skipped(budget)
    try:
        d = _xgmi_child(a, world, rank, ".xgmi", "dp", a.c5_model, (a.c5_buckets,), t, warmup=5,
                        runs=a.c5_steps, wire_dtype=a.c5_wire)
        if rank != 0:
            return res
        it = d["global"]["dlnb"]["iteration"]
        res.update({"ms_per_step": round(it["timed_ms_per_iter"], 4), "median_ms": round(it["median_ms"], 4),
                    "exposed_comm_ms": _mean_of(d, "barrier_time"),
                    "allreduce_busbw_GBps": _busbw(d, "allreduce", world),
                    "allreduce_algbw_GBps": _algbw(d, "allreduce")})
        if c5.get("ms_per_step"):
            # > 1: the xgmi kernels finish the comm-bound step faster than the comm_bound block's backend
            res["speedup_vs_comm_bound"] = round(c5["ms_per_step"] / res["ms_per_step"], 4)
            res["comm_bound_backend"] = c5.get("backend")
    except Exception as e:  # noqa: BLE001
        res = {"error": str(e)[:300]}
    return res


def _timeline_block(a: argparse.Namespace, world: int, rank: int, budget: "_Budget",
                    est: "_Estimator") -> Dict[str, Any]:
    """The headline configuration again for 1 + 2 iterations with --timeline
    (device-clock spans of every collective and compute task on every rank,
    csrc/src/timeline.cpp), summarised: per rank how much communication ran
    under compute and how much was exposed, and every collective's duration
    and bus bandwidth on the device clock while the compute ran beside it."""
    from dlnetbench_amd.tools import timeline as tlt
    res: Dict[str, Any] = {"iterations": 2}
    path = f"/tmp/dlnb_bench.trace_{os.environ.get('MASTER_PORT', '0')}_{os.getppid()}.json"
    nominal = est.setup + 3 * est.head_ms / 1e3
    t = budget.plan("timeline", est.want(nominal, a.timeline_timeout), nominal)
    if t is None:
        return _skipped(budget)
    try:
        d = _child_run(a, world, rank, ".tl", "fsdp", a.model, (a.units, world), t,
                       backend=a.hybrid_backend, graph=a.graph and a.backend in ("auto", "rccl", "xgmi"),
                       compute=a.compute, warmup=1, runs=2,
                       schedule=a.schedule, wire_dtype="bf16", timeline=path, timeline_iters=2)
        if rank != 0:
            return res
        # launch hops / drains the chained compute tasks absorbed (not in the spans' idle time)
        res["chain_absorbed_ms_per_iter"] = ((d["global"]["dlnb"].get("chain_capped") or {})
                                             .get("absorbed_ms_per_iter_max"))
        ev = tlt.load(path)
        bad = tlt.check(ev)
        s = tlt.summarize(ev)
        last = str(max(int(i) for r in s.values() for i in r))
        per = {pid: its[last] for pid, its in s.items() if last in its}
        res["ranks"] = len(per)
        res["well_formed"] = not bad
        res["span_ms_max"] = round(max(r["span_ms"] for r in per.values()), 3)
        res["comm_exposed_ms_max"] = round(max(r["comm_exposed_ms"] for r in per.values()), 3)
        if all("host_ms" in r for r in per.values()):
            # what the host's timing adds to the device span (launch + completion detection)
            res["host_boundary_ms_max"] = round(max(r["host_ms"] - r["span_ms"] for r in per.values()), 3)
        busy = sum(r["comm_busy_ms"] for r in per.values())
        res["comm_hidden_frac"] = round(sum(r["comm_hidden_ms"] for r in per.values()) / busy, 4) if busy else None
        ops: Dict[str, Any] = {}
        for e in ev:
            if e["cat"] == "compute" or str(e["args"].get("iter")) != last:
                continue
            op = e["name"].split(" ")[0]
            o = ops.setdefault(op, {"count": 0, "us": 0.0, "bytes": 0.0, "ranks": e["args"].get("ranks", 1)})
            o["count"] += 1
            o["us"] += e["dur"]
            o["bytes"] += float(e["args"].get("bytes", 0.0))
        from dlnetbench_amd.parallel.plan import busbw_factor
        for op, o in ops.items():
            n = int(o["ranks"])
            kind = {"all_reduce": "allreduce", "all_gather": "allgather", "reduce_scatter": "reduce_scatter",
                    "all_to_all": "alltoall"}.get(op, "sendrecv")
            gbps = o["bytes"] / (o["us"] * 1e3) if o["us"] else None
            ops[op] = {"count": o["count"], "mean_us": round(o["us"] / o["count"], 1),
                       "busbw_GBps": round(gbps * busbw_factor(kind, n), 2) if gbps and n > 1 else None}
        res["ops"] = ops
    except Exception as e:  # noqa: BLE001
        res = {"error": str(e)[:300]}
    finally:
        if rank == 0 and os.path.exists(path):
            os.remove(path)
    return res


def _headline_xgmi(a: argparse.Namespace, world: int, rank: int, doc: dict, budget: "_Budget",
                   est: "_Estimator") -> Dict[str, Any]:
    """The headline FSDP step itself over the xgmi kernels (zero-copy
    all-gather / reduce-scatter into registered buffers): its effective bus
    bandwidth next to the headline's, under the same deadline compute."""
    res: Dict[str, Any] = {"backend": "XGMI", "hip_graph": True}
    nominal = est.setup + (1 + a.xgmi_headline_steps) * est.head_ms / 1e3
    t = budget.plan("headline_xgmi", est.want(nominal, 150), nominal)
    if t is None:
        return _skipped(budget)
    try:
        d = _xgmi_child(a, world, rank, ".xgmih", "fsdp", a.model, (a.units, world), t, warmup=1,
                        runs=a.xgmi_headline_steps, schedule=a.schedule, wire_dtype="bf16")
        if rank != 0:
            return res
        it = d["global"]["dlnb"]["iteration"]
        res.update({"ms_per_step": round(it["timed_ms_per_iter"], 3), "median_ms": round(it["median_ms"], 3),
                    "exposed_comm_ms": round(it["timed_ms_per_iter"] - it["compute_floor_ms"], 3),
                    "effective_busbw_GBps": {k: _busbw(d, k, world) for k in ("allgather", "reduce_scatter")}})
        base = {k: _busbw(doc, k, world) for k in ("allgather", "reduce_scatter")}
        res["busbw_ratio_vs_headline"] = {k: round(res["effective_busbw_GBps"][k] / v, 4)
                                          for k, v in base.items() if v and res["effective_busbw_GBps"][k]}
        res["headline_backend"] = doc["global"]["backend"]
    except Exception as e:  # noqa: BLE001
        res = {"error": str(e)[:300]}
    return res


def _dp_block(a: argparse.Namespace, world: int, rank: int, budget: _Budget, est: _Estimator, tag: str,
              graph: bool, compute: str, **kw: Any) -> Dict[str, Any]:
    """The comm-bound ViT-H DP step (BASELINE C5) as a child run of every rank,
    bounded by the budget; returns the child's report (rank 0) or raises."""
    nominal = est.setup + (5 + a.c5_steps) * est.iter_s("dp", a.c5_model, (a.c5_buckets,), wire=a.c5_wire)
    if compute in ("gemm-work", "flops"):
        nominal += 5.0  # the fixed-work calibration
    t = budget.plan(tag.lstrip("."), est.want(nominal, 90), nominal)
    if t is None:
        raise _Skip()
    return _child_run(a, world, rank, tag, "dp", a.c5_model, (a.c5_buckets,), t, backend=a.backend, graph=graph,
                      compute=compute, warmup=5, runs=a.c5_steps, wire_dtype=a.c5_wire, **kw)


class _Skip(Exception):
    pass


def _c5_blocks(a: argparse.Namespace, world: int, rank: int, budget: _Budget, est: _Estimator, graph: bool,
               on_gpu: bool) -> Dict[str, Any]:
    """BASELINE C5 (ViT-H/32 fp8 DP, 8 buckets) and its variants: RCCL's own
    CTA count, geometric buckets, fixed-work compute (compute_stretch)."""
    c5: Dict[str, Any] = {}

    def common(d: dict) -> Dict[str, Any]:
        dl = d["global"]["dlnb"]
        it = dl["iteration"]
        cc = dl.get("chain_capped") or {}
        return {"ms_per_step": round(it["timed_ms_per_iter"], 4), "median_ms": round(it["median_ms"], 4),
                # the device-timed exposed all-reduce tail (barrier_time: last all-reduce's end stamp minus
                # the last backward's deadline) next to what the host sees over the floor
                "exposed_comm_ms": _mean_of(d, "barrier_time"),
                "step_minus_floor_ms": round(it["median_ms"] - it["compute_floor_ms"], 4),
                "allreduce_busbw_GBps": _busbw(d, "allreduce", world),
                "chain_capped": cc or None,
                "chain_absorbed_ms_per_iter": cc.get("absorbed_ms_per_iter_max"),
                "lane_graphs": (dl.get("lane_graphs") or {}).get("enabled")}

    try:
        d = _dp_block(a, world, rank, budget, est, ".c5", graph, a.compute)
        if rank == 0:
            it = d["global"]["dlnb"]["iteration"]
            c5.update({
                "model": a.c5_model, "strategy": f"dp{world}", "num_buckets": a.c5_buckets,
                "wire_dtype": a.c5_wire, "compute": a.compute,
                "compute_dtype": d["global"]["dlnb"]["compute"].get("gemm_dtype", "auto"),
                **common(d),
                "floor_ms": round(it["compute_floor_ms"], 4),
                "allreduce_bytes": d["global"]["msg_size_avg_bytes"] * a.c5_buckets,
                "allreduce_algbw_GBps": _algbw(d, "allreduce"),
                "transport": "link" if world > 1 else "local-copy",
                "backend": d["global"]["backend"],
            })
        else:
            c5["backend"] = "?"
    except _Skip:
        return _skipped(budget)
    except Exception as e:  # noqa: BLE001
        # the variants still run: whether a block runs must not depend on an
        # outcome that can differ between ranks (only on rank 0's plan)
        c5["error"] = str(e)[:300]
    variants = []
    if on_gpu and a.c5_ctas_ab and a.hybrid_backend == "rccl":
        # the same step with RCCL's own CTA count (no maxCTAs cap from the
        # comm-CU budget): one comm lane cannot deadlock against another, so
        # this shows what the 32-CU budget costs the all-reduce over the links
        variants.append(("rccl_default_ctas", ".c5c", a.compute, {"rccl_max_ctas": 0}))
    if 0 < a.c5_bucket_ratio < 1:
        # opt-in policy: shrink the exposed tail (the last bucket's all-reduce
        # runs after the backward ends)
        variants.append(("geometric_buckets", ".c5g", a.compute, {"dp_bucket_ratio": a.c5_bucket_ratio}))
    if a.stretch_steps > 0 and on_gpu:
        variants.append(("gemm_work", ".c5w", "gemm-work", {}))
    for key, tag, compute, kw in variants:
        try:
            d = _dp_block(a, world, rank, budget, est, tag, graph, compute, **kw)
            if rank == 0:
                v = common(d)
                if key == "rccl_default_ctas":
                    v["allreduce_algbw_GBps"] = _algbw(d, "allreduce")
                if key == "geometric_buckets":
                    v = {"bucket_ratio": a.c5_bucket_ratio, **v}
                if key == "gemm_work":
                    v.pop("allreduce_busbw_GBps")
                    v["compute_stretch"] = st = d["global"]["dlnb"].get("compute_stretch")
                    it = d["global"]["dlnb"]["iteration"]
                    if st:
                        # the step's excess over the compute it actually ran (the floor stretched by the
                        # collectives beside it): what exposed_comm_ms (the device-timed tail) must explain
                        v["step_minus_stretched_floor_ms"] = round(it["median_ms"] - it["compute_floor_ms"] * st, 4)
                c5[key] = v
        except _Skip:
            c5[key] = _skipped(budget)
        except Exception as e:  # noqa: BLE001
            c5[key] = {"error": str(e)[:300]}
    return c5


def _backend_key(name: Optional[str]) -> str:
    return {"RCCL": "rccl", "XGMI": "xgmi", "CPU-SHM": "cpu", "MIXED": "mixed"}.get(name or "", (name or "").lower())


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline: the exactness pass (N > 1) and the secondary "
                         "blocks (comm_bound, compute_stretch, link_bench, timeline, xgmi, hybrids)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last step computed to DIR/<name>.npy (float32)")
    ap.add_argument("--model", default=DEFAULT_MODEL)
    ap.add_argument("--units", type=int, default=32)
    ap.add_argument("--compute", default="gemm")
    ap.add_argument("--no-graph", dest="graph", action="store_false",
                    help="enqueue every iteration instead of replaying one captured HIP graph")
    ap.add_argument("--schedule", default="overlap")
    ap.add_argument("--backend", default="auto")
    ap.add_argument("--devices", default=None,
                    help="device list by local rank, e.g. 0,0 to put 2 ranks on one GPU (xgmi backend tests)")
    ap.add_argument("--base-path", default=ROOT, help="directory holding model_stats/ and models/")
    ap.add_argument("--time-scale", type=float, default=None, help="scale every compute duration (tests)")
    ap.add_argument("--wall-budget-s", type=float, default=float(os.environ.get("DLNB_BENCH_WALL_S", "420")),
                    help="wall seconds for the whole bench: every phase after the headline gets at most what is "
                         "left and is skipped when too little is (env DLNB_BENCH_WALL_S)")
    ap.add_argument("--budget-reserve-s", type=float, default=10.0,
                    help="seconds of the wall budget kept for writing the line")
    ap.add_argument("--c5-model", default=C5_MODEL, help="comm-bound DP secondary ('none' skips it)")
    ap.add_argument("--c5-buckets", type=int, default=8)
    ap.add_argument("--c5-steps", type=int, default=50)
    ap.add_argument("--c5-wire", default="bf16", help="wire dtype of the comm-bound all-reduce")
    ap.add_argument("--c5-bucket-ratio", type=float, default=0.7,
                    help="comm_bound.geometric_buckets: the same step with geometric bucket sizes (share r^i per "
                         "bucket, a small last all-reduce); 0 skips it")
    ap.add_argument("--no-c5-ctas-ab", dest="c5_ctas_ab", action="store_false",
                    help="skip the comm-bound rerun with RCCL's default CTA count")
    ap.add_argument("--stretch-steps", type=int, default=2,
                    help="fixed-work FSDP iterations for compute_stretch (0 skips)")
    ap.add_argument("--xgmi-ab", choices=["auto", "on", "off"], default="auto",
                    help="comm_bound_xgmi / headline_xgmi secondaries (auto: when N > 1 on the GPU)")
    ap.add_argument("--xgmi-headline-steps", type=int, default=2,
                    help="timed steps of the headline_xgmi secondary (0 skips it)")
    ap.add_argument("--exact", choices=["auto", "on", "off"], default="auto",
                    help="exactness pass of every timed backend across the ranks before timing (auto: N > 1)")
    ap.add_argument("--exact-dtypes", default="bf16,fp8_e4m3")
    ap.add_argument("--exact-sizes", default="4097,300000,2097157",
                    help="elements per rank: one-shot with a ragged tail, two-shot / zero-copy, multi-piece")
    ap.add_argument("--exact-timeout", type=float, default=120.0)
    ap.add_argument("--hybrids", choices=["auto", "on", "off"], default="auto",
                    help="BASELINE C3 hybrid_3d / C4 hybrid_3d_moe blocks (auto: N == 8 on the GPU)")
    ap.add_argument("--c3-model", default=C3_MODEL)
    ap.add_argument("--c3", default=C3_PARAMS, help="hybrid_3d num_stages,num_microbatches,num_tensor_shards")
    ap.add_argument("--c3-runs", type=int, default=2, help="timed iterations of the C3 block")
    ap.add_argument("--c4-model", default=C4_MODEL)
    ap.add_argument("--c4", default=C4_PARAMS, help="hybrid_3d_moe num_stages,num_microbatches,num_expert_shards")
    ap.add_argument("--c4-runs", type=int, default=2, help="timed iterations of the C4 blocks")
    ap.add_argument("--hybrid-timeout", type=float, default=150.0)
    ap.add_argument("--c4-ep-overlap", choices=["on", "off"], default="on",
                    help="also run C4 with --ep-overlap (the all-to-alls off the compute stream)")
    ap.add_argument("--timeline-block", choices=["auto", "on", "off"], default="auto",
                    help="headline config with --timeline for 2 iterations, summarised (auto: N > 1 on GPU)")
    ap.add_argument("--timeline-timeout", type=float, default=120.0)
    ap.add_argument("--link-bench", choices=["auto", "on", "off"], default="auto",
                    help="collective bandwidth of RCCL and the xgmi kernels on the job's GPUs (auto: N > 1 on GPU)")
    ap.add_argument("--link-sizes", default="8388608,67108864", help="--link-bench elements per rank (bf16)")
    ap.add_argument("--link-timeout", type=float, default=90.0)
    ap.add_argument("--fallback-backend", default="auto",
                    help="when the headline fails on its backend (N > 1), time it again on this one in a bounded "
                         "child run and run the blocks after it there too, the failure kept in the line "
                         "(auto: xgmi, on the GPU, when the exactness pass proved it exact; none: off)")
    ap.add_argument("--json", default=None, help="also write the full headline report here (rank 0)")
    a = ap.parse_args()
    a.hybrid_backend = "rccl" if a.backend == "auto" else a.backend
    checked_backends = _exact_backends(a)  # before a fallback changes a.backend

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world != a.gpus:
        print(f"[bench] warning: --gpus {a.gpus} but WORLD_SIZE={world}; using WORLD_SIZE", file=sys.stderr)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # An iteration takes ~3 s: a collective that has not completed within a
    # minute is hung - abort it and fall back (graph retry / error key)
    # instead of waiting out the runtime's 15-minute default. Both headline
    # attempts hanging then cost 2 minutes of the wall budget, not 6.
    os.environ.setdefault("DLNB_TIMEOUT", "60")
    # Rendezvous / host-barrier waits: ranks run the phases in lockstep (the
    # worst legitimate skew is a communicator setup, seconds), so a rank that
    # waits 2 minutes for a peer means the peer failed - stop there rather than
    # after the store's 15-minute default.
    os.environ.setdefault("DLNB_STORE_TIMEOUT", "120")
    # Everything below is native (HIP + RCCL from /opt/rocm); torch is not needed.
    os.environ.setdefault("DLNB_NO_TORCH", "1")
    # The native build this bench runs (dlnetbench_amd/_lib/libdlnb.so, loaded here; the child binaries link
    # the same build): a tree that was not built stops here, before anything is timed.
    from dlnetbench_amd import _native
    native_build = _native.version()
    budget = _Budget(a.wall_budget_s, a.budget_reserve_s, world, rank)
    ph = _Phases()
    on_gpu = a.backend in ("auto", "rccl", "xgmi")
    # Multi-rank: prove the collectives exact on these ranks before timing them.
    # (every rank gets the same all-reduced verdict, so all ranks take the
    # same decisions below)
    exact: Dict[str, Any] = {}
    if a.full and (a.exact == "on" or (a.exact == "auto" and world > 1)):
        t0 = ph.now()
        t = budget.plan("exact", a.exact_timeout, 5.0)
        exact = _exact_block(a, world, rank, t) if t else {"exact": {}, "exact_detail": _skipped(budget)}
        ph.add("exact", t0)
        if rank == 0:
            print(f"[bench] exactness: {json.dumps(exact)}", file=sys.stderr)
    xgmi_exact_ok = not exact or bool(exact.get("exact", {}).get("xgmi", False))
    # The xgmi blocks run with the release mode the pass proved exact on these
    # ranks (the system-scope one when the default vmcnt hand-off failed).
    rel = (exact.get("exact_detail") or {}).get("xgmi_release")
    if xgmi_exact_ok and rel:
        os.environ["DLNB_XGMI_RELEASE"] = rel

    from dlnetbench_amd.utils.stats import load_stats
    st = load_stats(os.path.join(a.base_path, "model_stats", a.model + ".txt"))
    use_graph = a.graph and on_gpu and a.schedule == "overlap"

    # The result line must be the only stdout line: route whatever the native
    # libraries print (e.g. RCCL's banner) to stderr while the benchmark runs.
    sys.stdout.flush()
    saved = os.dup(1)
    os.dup2(2, 1)
    extra: Dict[str, Any] = {}
    doc: Optional[dict] = None
    headline_error: Optional[str] = None
    headline_graph_error: Optional[str] = None
    try:
        # The headline runs as a bounded child process of every rank (the
        # native binary), like every block after it: a device
        # failure ends that process - its queues, and any kernel still
        # spinning on them, go with it - and never this one, which still
        # prints the line.
        fsdp_kw = dict(schedule=a.schedule, wire_dtype="bf16")
        # the headline's outputs (rank 0 of the child writes them after its timed steps)
        dump_kw = dict(dump_outputs=os.path.abspath(a.dump_outputs)) if a.dump_outputs else {}
        t0 = ph.now()
        est0 = _Estimator(a, world, 20.0, 0, 3000.0)
        nominal = est0.setup + (a.warmup + a.steps) * est0.iter_s("fsdp", a.model, (a.units, world))

        def head(tag: str, graph: bool) -> dict:
            # (the headline always runs: at least 60 s, more when the budget has it)
            t = budget.plan(tag.lstrip("."), max(60.0, est0.want(nominal, 300)), 1.0) or 60.0
            d = _child_run(a, world, rank, tag, "fsdp", a.model, (a.units, world), t, backend=a.backend,
                           graph=graph, compute=a.compute, warmup=a.warmup, runs=a.steps, **fsdp_kw, **dump_kw)
            return d if rank == 0 else {}

        try:
            try:
                doc = head(".headline", use_graph)
            except RuntimeError as e:
                if not use_graph:
                    raise
                # Graph capture is symmetric across ranks, so every rank takes
                # this path; the retry is a fresh child on a fresh store.
                headline_graph_error = str(e)[:300]
                print(f"[bench] HIP graph run failed ({e}); retrying with per-iteration enqueue in a new process",
                      file=sys.stderr)
                use_graph = False
                doc = head(".headline.retry", False)
            if rank == 0 and a.json and doc:
                with open(a.json, "w") as f:
                    json.dump(doc, f)
        except Exception as e:  # noqa: BLE001
            # still print a line (value null, the error): the driver reads
            # what failed instead of nothing
            headline_error = str(e)[:500]
        ph.add("headline", t0)
    finally:
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(saved)
    fallback: Optional[Dict[str, Any]] = None
    fb = a.fallback_backend
    if fb == "auto":
        fb = "xgmi" if on_gpu and world > 1 and a.backend == "auto" and exact.get("exact", {}).get("xgmi") else "none"
    if doc is None and world > 1 and fb != "none" and (fb != a.backend or a.fallback_backend != "auto"):
        # The headline's backend failed on these ranks (e.g. a first cross-device
        # RCCL run): time the same step on the fallback backend, a bounded child
        # run of every rank, and run every block after it there too - a value
        # with its backend named and the failure kept, instead of a null line.
        t0 = ph.now()
        # ~30 s of setup (communicators, buffers, graph capture of the 8B model) + the iterations
        est0 = _Estimator(a, world, 20.0, 0, 3000.0)
        nominal = est0.setup + (a.warmup + a.steps) * est0.iter_s("fsdp", a.model, (a.units, world))
        t = budget.plan("headline_fallback", est0.want(nominal, 300), nominal)
        fallback = {"backend": fb, "primary_backend": a.backend, "primary_error": headline_error}
        if t is None:
            fallback["skipped"] = _skipped(budget)["skipped"]
        else:
            try:
                d = _child_run(a, world, rank, ".hfb", "fsdp", a.model, (a.units, world), t, backend=fb,
                               graph=use_graph, compute=a.compute, warmup=a.warmup, runs=a.steps,
                               **dict(schedule=a.schedule, wire_dtype="bf16"),
                               **(dict(dump_outputs=os.path.abspath(a.dump_outputs)) if a.dump_outputs else {}))
                doc = d if rank == 0 else {}
                a.backend = a.hybrid_backend = fb
            except Exception as e:  # noqa: BLE001
                fallback["error"] = str(e)[:300]
        ph.add("headline_fallback", t0)
    head_ms = doc["global"]["dlnb"]["iteration"]["timed_ms_per_iter"] if doc else 3000.0
    est = _Estimator(a, world, ph.s.get("headline", 30.0), a.warmup + a.steps, head_ms)
    if doc is not None and a.full:
        # Secondary measurements, in order of value, each a bounded child run
        # of every rank: failures and overruns are reported, never fatal.
        if a.c5_model != "none":
            t0 = ph.now()
            extra["comm_bound"] = _c5_blocks(a, world, rank, budget, est, use_graph, on_gpu)
            ph.add("comm_bound", t0)
        # The cross-GPU link evidence right after C5, before the hybrids (VERDICT
        # r4 #4: a slow first cross-device hybrid must not skip it): collective
        # bandwidth with nothing else running, RCCL and xgmi, then the
        # comm-bound step over the xgmi kernels.
        if a.link_bench == "on" or (a.link_bench == "auto" and world > 1 and on_gpu):
            t0 = ph.now()
            extra["link_bench"] = _link_block(a, world, rank, xgmi_exact_ok, budget, est)
            ph.add("link_bench", t0)
        # xgmi A/B in child processes (see the module docstring); skipped when
        # the exactness pass found the xgmi kernels wrong on these ranks.
        xgmi_on = on_gpu and (a.xgmi_ab == "on" or (a.xgmi_ab == "auto" and world > 1))
        skip = {"error": "skipped: the xgmi exactness check failed on these ranks (see exact_detail)"}
        if a.c5_model != "none" and xgmi_on:
            t0 = ph.now()
            extra["comm_bound_xgmi"] = (_xgmi_ab(a, world, rank, extra.get("comm_bound", {}), budget, est)
                                        if xgmi_exact_ok else skip)
            ph.add("comm_bound_xgmi", t0)
        # BASELINE C3 / C4 hybrids (8 GPUs), each a child process per rank.
        if a.hybrids == "on" or (a.hybrids == "auto" and world == 8 and on_gpu):
            c3 = tuple(int(x) for x in a.c3.split(","))
            c4 = tuple(int(x) for x in a.c4.split(","))
            note = "GPipe (mb + S - 1)(f_mb + b_mb), BASELINE.md "
            t0 = ph.now()
            extra["hybrid_3d"] = _hybrid_block(a, world, rank, ".c3", "hybrid_3d", a.c3_model, c3, note + "C3",
                                               budget, est, a.c3_runs)
            ph.add("hybrid_3d", t0)
            t0 = ph.now()
            extra["hybrid_3d_moe"] = _hybrid_block(a, world, rank, ".c4", "hybrid_3d_moe", a.c4_model, c4,
                                                   note + "C4", budget, est, a.c4_runs)
            ph.add("hybrid_3d_moe", t0)
            if a.c4_ep_overlap == "on":
                t0 = ph.now()
                # the MI355X-side schedule for the same config: the 1,024
                # all-to-alls per iteration leave the compute stream
                extra["hybrid_3d_moe"]["ep_overlap"] = _hybrid_block(
                    a, world, rank, ".c4o", "hybrid_3d_moe", a.c4_model, c4, note + "C4", budget, est, a.c4_runs,
                    ep_overlap=True)
                ph.add("hybrid_3d_moe_ep_overlap", t0)
        if a.stretch_steps > 0 and on_gpu:
            t0 = ph.now()
            nominal = est.setup + 5.0 + (1 + a.stretch_steps) * head_ms / 1e3
            t = budget.plan("compute_stretch", est.want(nominal, 150), nominal)
            if t is None:
                extra["compute_stretch_error"] = _skipped(budget)["skipped"]
            else:
                try:
                    d = _child_run(a, world, rank, ".work", "fsdp", a.model, (a.units, world), t, backend=a.backend,
                                   graph=use_graph, compute="gemm-work", warmup=1, runs=a.stretch_steps, **fsdp_kw)
                    if rank == 0:
                        extra["compute_stretch"] = d["global"]["dlnb"].get("compute_stretch")
                        extra["gemm_work_ms_per_step"] = round(d["global"]["dlnb"]["iteration"]["timed_ms_per_iter"],
                                                               3)
                except Exception as e:  # noqa: BLE001
                    extra["compute_stretch_error"] = str(e)[:300]
            ph.add("compute_stretch", t0)
        # Device timeline of the headline configuration (every rank's spans).
        if a.timeline_block == "on" or (a.timeline_block == "auto" and world > 1 and on_gpu):
            t0 = ph.now()
            extra["timeline"] = _timeline_block(a, world, rank, budget, est)
            ph.add("timeline", t0)
        # the headline over the xgmi kernels last
        if xgmi_on and a.xgmi_headline_steps > 0 and not (fallback and fallback["backend"] == "xgmi"):
            t0 = ph.now()
            extra["headline_xgmi"] = _headline_xgmi(a, world, rank, doc, budget, est) if xgmi_exact_ok else skip
            ph.add("headline_xgmi", t0)
    if rank != 0:
        return 0
    out: Dict[str, Any] = {"metric": METRIC, "value": None, "unit": "ms", "n_gpus": world, "steps": a.steps,
                           "warmup": a.warmup, "ms_per_step": None, "higher_is_better": False, "scaling": "weak",
                           "vs_baseline": None, "dtype": "bf16", "full": bool(a.full),
                           "native_build": native_build}
    if doc is not None:
        g = doc["global"]
        it = g["dlnb"]["iteration"]
        ms = it["timed_ms_per_iter"]
        exposed = ms - it["compute_floor_ms"]
        out.update({
            "value": round(ms, 3),
            "ms_per_step": round(ms, 3),
            "vs_baseline": round(ms / BASELINE_MS, 4) if a.model == DEFAULT_MODEL and a.time_scale is None else None,
            "data": ("synthetic (random-init buffers; compute = MFMA GEMM stand-in bounded to the table durations)"
                     if a.compute == "gemm" else f"synthetic (random-init buffers; compute mode {a.compute})"),
            "config": {
                "model": a.model,
                "global_batch": int(g["local_batch_size"]) * world,
                "seq_len": st.seq_len,
                "parallelism": f"fsdp{world}",
                "num_units": g["num_units"],
                "sharding_factor": g["sharding_factor"],
                "compute": a.compute,
                "schedule": a.schedule,
                "backend": g["backend"],
                "hip_graph": bool(use_graph),
                "device_gates": g.get("device_gates"),
            },
            # null at N = 1: a 1-rank all-gather / reduce-scatter is a local copy
            "effective_busbw_GBps": {k: _busbw(doc, k, world) for k in ("allgather", "reduce_scatter")},
            "exposed_comm_ms": round(exposed, 3),
            # compute tasks per iteration that waited longer than a launch hop (the chained
            # deadline's 30-us absorb cap) and that wait in ms - kept in the time, not hidden
            "chain_capped": g["dlnb"].get("chain_capped"),
            # launch hops / drains the chained deadline tasks took out of their own compute
            # (<= 30 us each): not in the iteration time, reported so nothing is hidden
            "chain_absorbed_ms_per_iter": (g["dlnb"].get("chain_capped") or {}).get("absorbed_ms_per_iter_max"),
            # one linear HIP graph per stream joined by device gates (or why not), and whether each
            # iteration's launch was pre-armed during the previous one
            "lane_graphs": g["dlnb"].get("lane_graphs"),
            "prearm": g["dlnb"].get("prearm"),
            "median_ms": round(it["median_ms"], 3),
            "per_run_ms": _per_run_ms(doc),
            "slow_iterations": _slow_iterations(doc),
            # every rank's mean iteration (ms): at N > 1 the straggler and the spread behind the max
            "rank_ms": _rank_ms(doc),
            "baseline_ms": BASELINE_MS,
            "baseline_note": "derived reference floor (BASELINE.md C2: fwd+bwd of llama3_8b_16_bfloat16); lower is better",
            "rccl_cta_budget": g["dlnb"].get("rccl_cta_budget"),
            # energy per step (J): hwmon / amd-smi power sampled every 5 ms on every GPU
            # (the reference's energy_consumed, plots_pareto_energy.py); sum over GPUs and mean per GPU
            "energy_J_per_step": _energy(doc),
            "energy_source": g["dlnb"].get("energy_source"),
            # ncclCommCount of every RCCL communicator of the headline run: proof
            # that RCCL formed an N-rank group
            "rccl_nranks": g["dlnb"].get("rccl_nranks"),
            "runtime": g["dlnb"].get("runtime"),
            # the xGMI cost model's iteration at this N (BASELINE.md "Link-model
            # expectations"): the headline and the comm-bound block should land
            # near these on an 8 x MI355X node (plus ~1-2 ms of fixed overhead)
            "predicted_ms": _predicted_ms(a, world, "fsdp", a.model, (a.units, world)),
        })
    else:
        out["error"] = "headline failed: " + (headline_error or "?")
        out["data"] = "synthetic"
        out["config"] = {"model": a.model, "parallelism": f"fsdp{world}", "compute": a.compute}
    cb = extra.get("comm_bound")
    if cb and "error" not in cb and "skipped" not in cb:
        cb["predicted_ms"] = _predicted_ms(a, world, "dp", a.c5_model, (a.c5_buckets,), wire=a.c5_wire)
    if "link_bench" in extra:
        fit = _model_fit(a, world, extra)
        if fit:
            out["model_fit"] = fit
    if fallback is not None:
        out["headline_fallback"] = fallback
    if headline_graph_error:
        # the HIP-graph headline failed and the value (if any) is the per-iteration retry's
        out["headline_graph_error"] = headline_graph_error
    out.update(exact)
    # Every timed number is qualified by the exactness verdict of its backend
    # (VERDICT r3 #4): "verified" per checked backend; a block timed on a
    # backend whose collectives were not exact on these ranks keeps its
    # numbers and carries "error".
    if exact.get("exact"):
        ver = {b: bool(exact["exact"].get(b)) for b in checked_backends.split(",")}
        out["verified"] = ver
        for key, blk in [("headline", out), ("comm_bound", extra.get("comm_bound")),
                         ("hybrid_3d", extra.get("hybrid_3d")), ("hybrid_3d_moe", extra.get("hybrid_3d_moe")),
                         ("hybrid_3d_moe_ep_overlap", (extra.get("hybrid_3d_moe") or {}).get("ep_overlap"))]:
            if not isinstance(blk, dict):
                continue
            b = _backend_key(blk.get("backend") if key != "headline" else (blk.get("config") or {}).get("backend"))
            if b in ver and not ver[b] and "error" not in blk:
                blk["error"] = f"{b} exactness failed (see exact_detail); timed anyway"
    elif exact:
        # the pass ran but did not complete (timeout, crash, budget): nothing is verified
        out["verified"] = {b: None for b in checked_backends.split(",")}
        out["verified_note"] = "exactness pass did not complete: " + json.dumps(exact.get("exact_detail"))[:200]
    else:
        out["verified"] = None  # no exactness pass (N = 1: collectives are local copies)
    out.update(extra)
    out["budget"] = budget.report()
    # rank 0's wall seconds per phase (the headline's includes setup, warm-up and the timed steps)
    out["phase_seconds"] = ph.report()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
