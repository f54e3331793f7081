// Report assembly (dlnb/report.hpp): this rank's entry, then the document
// from every rank's entry.
#include <algorithm>
#include <cmath>

#include "dlnb/report.hpp"
#include "dlnb/xgmi.hpp"

extern char** environ;

namespace dlnb {

namespace {

double percentile(std::vector<double> v, double q) {
  if (v.empty()) return 0;
  std::sort(v.begin(), v.end());
  double pos = q * (v.size() - 1);
  size_t lo = static_cast<size_t>(std::floor(pos)), hi = static_cast<size_t>(std::ceil(pos));
  return v[lo] + (v[hi] - v[lo]) * (pos - lo);
}

// Iteration time = max over ranks per run (the slowest rank bounds a step).
Json iteration_block(Context& ctx, Strategy& strat, const char* rkey, const TimedRuns& tr,
                     const std::vector<Json>& ranks) {
  std::vector<double> per_run(static_cast<size_t>(tr.runs), 0.0);
  for (const auto& rj : ranks) {
    const Json& v = rj.at(rkey);
    for (size_t i = 0; i < v.size() && i < per_run.size(); ++i) per_run[i] = std::max(per_run[i], v.at(i).as_double());
  }
  Json it = Json::object();
  it["per_run_max_s"] = Json(per_run);
  it["median_ms"] = percentile(per_run, 0.5) * 1e3;
  double mean = 0;
  for (double x : per_run) mean += x;
  it["mean_ms"] = per_run.empty() ? 0.0 : mean / per_run.size() * 1e3;
  it["p95_ms"] = percentile(per_run, 0.95) * 1e3;
  it["min_ms"] = per_run.empty() ? 0.0 : *std::min_element(per_run.begin(), per_run.end()) * 1e3;
  it["timed_ms_per_iter"] = tr.runs > 0 ? tr.timed_region_s / tr.runs * 1e3 : 0.0;
  double floor_us = strat.compute_floor_us(ctx);
  it["compute_floor_ms"] = floor_us / 1e3 * ctx.opt.time_scale;
  return it;
}

// `compute_stretch` and `chain_capped`: maxima over the ranks' entries.
void rank_maxima(const std::vector<Json>& ranks, Json& ext) {
  double worst = 0;
  for (const auto& rj : ranks)
    if (rj.contains("compute_stretch")) worst = std::max(worst, rj.at("compute_stretch").as_double());
  if (worst > 0) ext["compute_stretch"] = worst;  // max over ranks
  // Compute tasks that waited beyond the chain's absorb cap per iteration
  // (the wait stays in the iteration time; max over ranks)
  // absorbed_*: lateness the chained tasks took out of their own compute
  // (launch hops, drains): invisible in the iteration time, shown here
  static const char* const keys[] = {"tasks_per_iter",        "ms_per_iter",          "gate_wait_timeouts",
                                     "compute_gate_timeouts", "absorbed_ms_per_iter", "absorbed_tasks_per_iter"};
  double mx[6] = {0, 0, 0, 0, 0, 0};
  bool any = false;
  for (const auto& rj : ranks)
    if (rj.contains("chain_capped")) {
      any = true;
      for (int k = 0; k < 6; ++k) mx[k] = std::max(mx[k], rj.at("chain_capped").at(keys[k]).as_double());
    }
  if (!any) return;
  Json c = Json::object();
  for (int k = 0; k < 6; ++k) c[std::string(keys[k]) + "_max"] = mx[k];
  ext["chain_capped"] = c;
}

// `wire_quant`: what rank 0's communicators quantized (comm.hpp WireQuantCounts).
Json wire_quant_json(const WireQuantCounts& c) {
  static const char* const names[4] = {"all_reduce", "all_gather", "reduce_scatter", "all_to_all"};
  Json ops = Json::object();
  for (int k = 0; k < 4; ++k) {
    Json o = Json::object();
    o["calls"] = static_cast<long long>(c.ops[k].calls);
    o["payload_bytes"] = static_cast<long long>(c.ops[k].payload_bytes);
    o["wire_bytes"] = static_cast<long long>(c.ops[k].wire_bytes);
    ops[names[k]] = o;
  }
  Json j = Json::object();
  j["format"] = "mxfp8_e4m3";
  j["block"] = 32;
  j["ops"] = ops;
  return j;
}

}  // namespace

Json rank_report(Context& ctx, Strategy& strat, const TimedRuns& tr, const Replay& replay) {
  const RankInfo& ri = ctx.boot->info;
  const TimerSet& T = *strat.timers();
  const int runs = tr.runs;
  Json rank = strat.rank_json();
  if (replay.prearmed()) {
    rank["prearm_go_timeouts"] = replay.go_timeouts();
    Json a = Json::array();
    for (double x : tr.arm_s) a.push_back(x * 1e3);
    rank["prearm_launch_ms"] = a;
  }
  rank["energy_consumed"] = T.values_json("energy_consumed");
  if (!tr.sensors.empty()) {
    Json c = Json::array(), lo = Json::array(), hi = Json::array(), w = Json::array();
    for (const auto& x : tr.sensors) {
      c.push_back(x.sclk_mhz);
      lo.push_back(x.sclk_min_mhz);
      hi.push_back(x.sclk_max_mhz);
      w.push_back(x.power_w);
    }
    rank["iteration_sclk_mhz"] = c;
    rank["iteration_sclk_min_mhz"] = lo;
    rank["iteration_sclk_max_mhz"] = hi;
    rank["iteration_power_w"] = w;
  }
  {
    // the duration of each timed iteration's last collective (ms)
    const std::string tk = strat.tail_collective_timer();
    const auto& v = tk.empty() ? std::vector<double>() : T.get(tk);
    if (runs > 0 && !v.empty() && v.size() % static_cast<size_t>(runs) == 0) {
      const size_t per = v.size() / static_cast<size_t>(runs);
      Json a = Json::array();
      for (int r = 0; r < runs; ++r) a.push_back(v[(static_cast<size_t>(r) + 1) * per - 1] * 1e3);
      rank["iteration_last_collective_ms"] = a;
      rank["iteration_last_collective"] = tk;
    }
  }
  {
    // chained deadline tasks: lateness absorbed (<= the cap each) and beyond
    // the cap (deadline_sync.hpp), gate waits that timed out
    ComputeEngine::ChainCounters cc;
    if (runs > 0 && ctx.compute->chain_counters(cc)) {
      Json c = Json::object();
      c["tasks_per_iter"] = cc.capped_tasks / runs;
      c["ms_per_iter"] = cc.capped_s / runs * 1e3;
      c["absorbed_tasks_per_iter"] = cc.absorbed_tasks / runs;
      c["absorbed_ms_per_iter"] = cc.absorbed_s / runs * 1e3;
      // device gate waits that gave up at their bound (never expected): a comm
      // lane's gate_wait, a deadline task's gate, a gate event's wait
      c["gate_wait_timeouts"] = cc.wait_timeouts + static_cast<double>(ctx.dev->gate_event_timeouts());
      c["compute_gate_timeouts"] = cc.gate_timeouts;
      // waits that left on the host's abort word, program blocks that came late for a task
      c["aborted_waits"] = cc.aborted;
      c["late_blocks"] = cc.late_blocks;
      rank["chain_capped"] = c;
    }
  }
  // intervals whose stamps came out of order (recorded as 0; never expected)
  if (T.has_negatives()) rank["timer_negative_intervals"] = T.negatives_json();
  rank["hostname"] = ri.hostname;
  rank["rank"] = ri.rank;
  rank["local_rank"] = ri.local_rank;
  rank["device_name"] = ctx.dev->name();
  rank["device_index"] = ctx.dev->index();
  rank["comm"] = strat.comm_summary();
  // Fixed-work compute: measured task time / uncontended (table) time over
  // the timed runs. > 1 means the collectives running beside the compute
  // (HBM traffic, CUs, power) slowed it down.
  const double task_s = T.sum("compute_task_time"), table_s = T.sum("compute_task_table");
  if (!T.get("compute_task_time").empty() && table_s > 0) {
    rank["compute_stretch"] = task_s / table_s;
    rank["compute_task_s"] = task_s;
    rank["compute_table_s"] = table_s;
  }
  return rank;
}

Json global_report(Context& ctx, Strategy& strat, const RunSetup& setup, const TimedRuns& tr, const Replay& replay,
                   const std::vector<std::string>& rank_docs, const Json& timeline_info) {
  const Options& opt = ctx.opt;
  const std::string& backend = setup.backend;
  Json g = strat.global_json();
  Json ext = Json::object();
  ext["strategy"] = strategy_name(opt.strategy);
  ext["schedule"] = opt.schedule;
  ext["graph"] = static_cast<double>(replay.nodes());
  if (opt.graph) ext["lane_graphs"] = replay.describe();
  // pre-armed replay loop (each iteration's launch submitted during the one
  // before, released by a host store; DLNB_PREARM=0 launches in the loop)
  ext["prearm"] = replay.prearmed();
  ext["wire_dtype"] = dtype_name(ctx.wire);
  if (opt.wire_quant != "none") ext["wire_quant"] = wire_quant_json(ctx.wire_quant);
  ext["compute"] = ctx.compute->describe();
  ext["stats_file"] = setup.stats_path;
  ext["stats_dtype"] = ctx.stats.dtype;
  ext["stats_device"] = ctx.stats.device;
  ext["warmup"] = opt.warmup;
  ext["runs"] = tr.runs;
  ext["warmup_times"] = Json(tr.warm);
  ext["timed_region_s"] = tr.timed_region_s;
  ext["energy_source"] = setup.meter->source();
  // ranks of this job on this rank's device (> 1: loopback threads or -d 0,0;
  // the deadline compute then runs in 500-us slices, compute.cpp)
  ext["ranks_on_device"] = ctx.ranks_on_device;
  if (ctx.timeline) ext["timeline"] = timeline_info;
  {
    const int lanes = setup.lanes;
    Json b = Json::object();
    b["lanes"] = lanes;
    b["comm_cus"] = opt.comm_cus;
    b["max_ctas_per_lane"] = ctx.lane_ctas;  // 0 = RCCL default
    b["applies"] = setup.rccl;
    b["fits"] = !setup.rccl || !setup.gemm_compute || ctx.lane_ctas == 0 ? true : lanes * ctx.lane_ctas <= opt.comm_cus;
    if (backend == "xgmi" || backend == "mixed") {
      // xgmi kernels: blocks per lane = blocks_per_cu x max_ctas, so a lane
      // occupies max_ctas CUs at the measured occupancy
      const int bpc = xgmi::min_blocks_per_cu();
      b["xgmi_blocks_per_cu"] = bpc;
      b["xgmi_blocks_per_lane"] = ctx.lane_ctas > 0 ? bpc * ctx.lane_ctas : 0;
    }
    ext["rccl_cta_budget"] = b;
  }
  {
    Json cl = comm_log_json(ctx.comm_log);
    ext["communicators"] = cl.at("communicators");
    ext["rccl_nranks"] = cl.at("rccl_nranks");
    if (ctx.dev->kind() == DeviceKind::GPU) ext["runtime"] = runtime_info();
  }
  {
    // Collective-library knobs of this run (the reference recorded them as
    // SbatchMan job variables, plots/parser.py:151-154).
    Json env = Json::object();
    for (char** e = environ; e && *e; ++e) {
      std::string kv = *e;
      if (starts_with(kv, "NCCL_") || starts_with(kv, "RCCL_") || starts_with(kv, "HSA_") || starts_with(kv, "DLNB_")) {
        size_t eq = kv.find('=');
        if (eq != std::string::npos) env[kv.substr(0, eq)] = kv.substr(eq + 1);
      }
    }
    ext["env"] = env;
  }
  std::vector<Json> ranks;
  for (const auto& s : rank_docs) ranks.push_back(Json::parse(s));
  ext["iteration"] = iteration_block(ctx, strat, setup.rkey, tr, ranks);
  rank_maxima(ranks, ext);
  g["dlnb"] = ext;

  Json doc = Json::object();
  doc["section"] = strat.section_id();
  doc["title"] = strat.section_title();
  doc["global"] = g;
  Json rarr = Json::array();
  for (auto& r : ranks) rarr.push_back(r);
  doc["ranks"] = rarr;
  return doc;
}

}  // namespace dlnb
