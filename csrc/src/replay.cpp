// HIP graph replay of one iteration (dlnb/replay.hpp).
//
// Lane graphs (the default): every stream of the strategy is captured into
// its own linear graph, launched on that stream, and the streams' ordering
// is carried by device gates (Device::set_gate_events: an event record
// raises a gate, a wait spins on it) instead of graph edges. The graph
// executor then has no fork to spread over its hardware queues: compute
// stays on the compute stream's queue and every collective on its lane's,
// so no compute task queues behind a collective (profiles/absorb_r4.md), and
// every stamp pair on one stream times exactly that stream's work. It needs
// every stream on a hardware queue of its own (a gate wait would otherwise
// hold the queue its signal sits behind): probed first, and a single graph
// with event edges when they share one (lane_graphs.reason says why).
#include <algorithm>
#include <cstdlib>
#include <exception>
#include <iostream>

#include "dlnb/aux.hpp"
#include "dlnb/replay.hpp"

namespace dlnb {

namespace {
Json graph_shape(const GraphExec& g) {
  Json e = Json::object();
  e["nodes"] = static_cast<double>(g.nodes());
  e["edges"] = static_cast<double>(g.edges());
  return e;
}
}  // namespace

Replay::Replay(Context& ctx, Strategy& strat, const std::string& backend)
    : ctx_(ctx), strat_(strat), backend_(backend), T_(*strat.timers()), TL_(ctx.timeline.get()) {}

Replay::~Replay() {
  if (std::uncaught_exceptions() != 0) {
    // (before the timed loop: nothing is aborted here, the words are kept)
    if (!timed_) return;
    // The run failed inside the timed loop: abort the device waits before
    // anything is torn down - an armed replay is NOT released (its go
    // wait sees the abort and lets it run through poisoned: no compute,
    // no waits); a CLI process ends here (device_failure). The words are
    // not freed (hipHostFree waits for the device, which may be hung).
    // a loopback hub's GPU ranks have no abort word to raise here
    // (t_fail->dev is unset for them), so their armed replay spins on.
    device_failure("exception in the timed loop: " + last_error_message());
    return;
  }
  // (after the words and the owned streams the members go: lane graphs, the graph)
  if (hs_) ctx_.dev->free_stamps(hs_, nhs_);
  alt_owned_.clear();
  free_lane_done();
}

void Replay::free_lane_done() {
  if (lane_done_) ctx_.dev->free_stamps(lane_done_, lane_done_n_);
  lane_done_ = nullptr;
  lane_done_n_ = 0;
}

// Back to no lanes: before the single graph is captured in their place.
void Replay::drop_lanes() {
  lane_graphs_.clear();
  free_lane_done();  // the single graph signals after its launch
  joined_ = false;
  alt_ss_.clear();
  alt_owned_.clear();
  ctx_.dev->set_gate_events(false);
}

void Replay::build() {
  DLNB_REQUIRE(ctx_.dev->kind() == DeviceKind::GPU, "--graph needs a GPU");
  // xgmi kernels take their epochs from device-side counters, so a replayed
  // graph issues fresh ones; the loopback backends synchronise on the host.
  DLNB_REQUIRE(backend_ == "rccl" || backend_ == "xgmi" || backend_ == "mixed",
               "--graph needs --backend rccl, xgmi or mixed");
  DLNB_REQUIRE(strat_.capturable(), "--graph cannot capture --schedule reference (it blocks the host)");
  ss_ = strat_.streams();
  others_.assign(ss_.begin() + 1, ss_.end());
  std::string why;
  if (env_int("DLNB_LANE_GRAPHS", 1) == 0) {
    why = "DLNB_LANE_GRAPHS=0";
  } else if (ss_.size() < 2) {
    why = "one stream";
  } else if (ctx_.ranks_on_device > 1 && env_int("DLNB_LANE_SHARED", 0) == 0) {
    // a task spinning on its gate holds its CUs, which another rank's
    // compute on the same device - the one the collective waits for - needs
    // (DLNB_LANE_SHARED=1, with grids that fit side by side - --comm-cus -
    // and no slicing: the multi-rank lane path rehearsed on one GPU)
    why = "ranks share the device";
  } else {
    std::string detail;
    if (!ctx_.dev->queues_independent(ss_, 0.05, &detail)) why = "streams share a hardware queue (" + detail + ")";
  }
  // every rank takes the same decision, and every rank takes part in it
  const bool lanes = ctx_.hg().allreduce_max(why.empty() ? 0.0 : 1.0) < 0.5;
  if (!lanes && why.empty()) why = "another rank cannot use lane graphs";
  // Gate waits bounded by 4x the compute floor (at least 15 s) unless
  // DLNB_GATE_TIMEOUT_S is set: a gate that never comes costs the warm-up
  // that much before the safety valve (warmup_trouble), not 60 s per wait.
  if (!std::getenv("DLNB_GATE_TIMEOUT_S")) {
    const double t = std::max(15.0, 4.0 * strat_.compute_floor_us(ctx_) * 1e-6 * ctx_.opt.time_scale);
    ctx_.dev->set_gate_timeout(t);
    ctx_.compute->set_gate_timeout(t);
    lane_info_["gate_timeout_s"] = t;
  }
  capture(lanes, why);
  replay_ = true;
  origin_ = ss_[0];
}

// Capture one iteration: lane graphs when `lanes` (the capture may still
// fall back to the single graph: not linear, no program), else the single
// graph; `why` is the reason reported when there are no lanes.
void Replay::capture(bool lanes, std::string why) {
  TraceRange tr("dlnb:graph_capture");
  T_.begin_capture();
  if (TL_) TL_->begin_capture();
  if (lanes && !capture_lanes(&why)) {
    lanes = false;
    T_.end_capture();
    if (TL_) TL_->end_capture();
    T_.begin_capture();
    if (TL_) TL_->begin_capture();
  }
  if (!lanes) {
    // the engine's slot reset heads the graph, before every stream's first node
    graph_ = ctx_.dev->capture(
        *ss_[0], others_, [this] {
          strat_.enqueue_iteration();
          T_.finish_stalls();
        }, [this] {
          ctx_.compute->reset_clocks(*ss_[0]);
          T_.iteration_start(*ss_[0]);
        });
    ctx_.compute->after_capture();  // task lists of the launches captured (fixed-work tasks)
    lanes_ss_ = {ss_[0]};
  }
  T_.end_capture();
  if (TL_) TL_->end_capture();
  lane_info_["enabled"] = lanes;
  if (lanes) {
    lane_info_["program_join"] = joined_;
    lane_info_["alternating_streams"] = !alt_ss_.empty();
  }
  if (!lanes) lane_info_["reason"] = why;
  Json per = Json::array();
  size_t total = 0;
  bool all_linear = true;
  for (size_t i = 0; i < (lanes ? lane_graphs_.size() : 1); ++i) {
    const GraphExec& g = lanes ? *lane_graphs_[i] : *graph_;
    Json e = graph_shape(g);
    e["linear"] = g.linear();
    e["node_types"] = g.node_types();
    total += g.nodes();
    all_linear = all_linear && g.linear();
    per.push_back(e);
  }
  lane_info_["graphs"] = per;
  lane_info_["linear"] = all_linear;
  if (ctx_.rank() == 0 && !ctx_.opt.quiet) {
    if (lanes)
      std::cout << "[dlnb] captured one iteration into " << lane_graphs_.size() << " lane graphs of " << total
                << " nodes (" << (all_linear ? "all linear" : "NOT all linear") << ")" << std::endl;
    else
      std::cout << "[dlnb] captured one iteration into a HIP graph of " << total << " nodes"
                << (why.empty() ? "" : " (no lane graphs: " + why + ")") << std::endl;
  }
}

// One graph per stream. False (with `why`, the lanes dropped) when every
// rank's verdict is the single graph instead.
bool Replay::capture_lanes(std::string* why) {
  ctx_.dev->set_gate_events(true);
  // each lane ends by clearing its own deadline slot for the next replay
  lane_done_n_ = ss_.size();
  lane_done_ = ctx_.dev->alloc_stamps(lane_done_n_);
  // A compute program on the compute lane ends with a join on the other
  // lanes' end gates and signals the whole iteration from inside the
  // kernel (ComputeEngine::set_lane_join); otherwise every lane ends with
  // its own done word (and clears its deadline slot).
  std::vector<uint64_t*> end_gates;
  for (size_t i = 1; i < ss_.size(); ++i) end_gates.push_back(ctx_.dev->alloc_gate());
  ctx_.compute->set_lane_join(*ss_[0], end_gates, 1u, lane_done_);
  const long progs0 = ctx_.compute->programs_on(*ss_[0]);
  lane_graphs_ = ctx_.dev->capture_lanes(
      ss_, [this] {
        T_.iteration_start(*ss_[0]);
        strat_.enqueue_iteration();
        T_.finish_stalls();
      },
      [this, &end_gates](size_t i) {
        if (ctx_.compute->program_joined(*ss_[0])) {
          if (i > 0) ctx_.dev->signal_gate(*ss_[i], end_gates[i - 1], 1u);
        } else {
          ctx_.compute->reset_slot(*ss_[i]);
          ctx_.dev->lane_done(*ss_[i], lane_done_ + i);
        }
        // The graph's last kernel carries its system-scope release (an L2
        // write-back: ~50 us after a collective's copy, round 5 traces):
        // a trailing no-op takes it, after the lane's signal is out.
        ctx_.dev->pad(*ss_[i]);
      });
  ctx_.compute->after_capture();  // the compute programs' task lists
  joined_ = ctx_.compute->program_joined(*ss_[0]);
  // A lane whose graph is not a chain (a library adding its own stream
  // to the capture, e.g. a collective's side work joined back) would be
  // spread over executor streams that may share the compute lane's
  // hardware queue - where a gate wait could hold the node that raises
  // its gate. Then the whole iteration is captured as one graph instead.
  // Lanes pay only when the compute lane is one compute program: a lane
  // of one launch per task puts every kernel boundary (28-60 us: drain,
  // dispatch) on one queue, which the single graph spreads over four
  // (C5 7.40-7.65 ms against 7.27, gemm-work C5 14.5 ms against 7.8:
  // profiles/lanes_r5.md). DLNB_LANE_GRAPHS=2 keeps such lanes anyway.
  bool linear = true;
  for (const auto& g : lane_graphs_) linear = linear && g->linear();
  // ... or when its tasks are long single kernels (the pipeline hybrids:
  // one task per micro-batch; their boundaries cost little, while the
  // single graph's executor queues them behind collectives - hybrid_3d
  // S=2 mb=4 on 2 ranks: 100.0 ms with lanes against 104.9-106.7,
  // profiles/lanes_n2_r5.md). DLNB_LANE_MIN_TASK_US (1000).
  const double task_us = ctx_.compute->lane_task_us(*ss_[0]);
  const bool long_tasks = task_us >= static_cast<double>(env_int("DLNB_LANE_MIN_TASK_US", 1000)) &&
                          strat_.lanes_without_program();
  // a compute program per iteration qualifies joined or not (not joined:
  // work follows it on the compute lane, which then ends with its own
  // done word - ADVICE r5)
  // - ONE program launch in the iteration: a task too short for a program
  // (< 20 us) splits it into several launches with kernels between, whose
  // boundaries all land on the compute lane's one queue
  const long progs = ctx_.compute->programs_on(*ss_[0]) - progs0;
  const bool program_ok = joined_ || (progs == 1 && !ctx_.compute->program_split(*ss_[0])) || long_tasks ||
                          env_int("DLNB_LANE_GRAPHS", 1) >= 2;
  lane_info_["compute_programs"] = static_cast<double>(progs);
  lane_info_["compute_task_us"] = task_us;
  const double verdict = ctx_.hg().allreduce_max(!linear ? 2.0 : (!program_ok ? 1.0 : 0.0));
  if (verdict < 0.5) {
    pick_replay_streams();
    return true;
  }
  // the rejected lanes' shapes (which library added what to a capture)
  Json rej = Json::array();
  for (const auto& g : lane_graphs_) {
    Json e = graph_shape(*g);
    e["node_types"] = g->node_types();
    rej.push_back(e);
  }
  lane_info_["rejected_lane_graphs"] = rej;
  drop_lanes();
  *why = verdict > 1.5 ? "a lane graph is not linear"
                       : "the compute lane is not one compute program (and the strategy's launch-per-task "
                         "lanes do not pay: Strategy::lanes_without_program)";
  return false;
}

// The streams the lane graphs are launched on.
void Replay::pick_replay_streams() {
  lanes_ss_ = ss_;
  // the first replay starts from cleared slots too
  ctx_.compute->reset_clocks(*ss_[0]);
  ss_[0]->synchronize();
  // Every other replay goes to a second set of streams (same
  // priorities: the compute lane normal, the comm lanes high): a
  // launched graph's completion holds its queue for ~70-100 us after
  // its last node (round 5 traces), and the pre-armed next replay would
  // wait behind it. A graph runs on any stream; its nodes do not depend
  // on the one it was captured on.
  // Both sets are streams made here, after setup: replays on the
  // strategy's own streams (made before the communicators) ran their
  // collectives slower - every other iteration 0.13 ms (C5) / 0.3 ms
  // (headline) longer in round 5's A/B - so neither set is the capture's.
  // (not with ranks sharing the device, DLNB_LANE_SHARED: two processes'
  // extra stream sets oversubscribe the hardware queues - 2 ranks on one
  // GPU ran 143.4 ms without and 149.5-164.7 with, profiles/lanes_n2_r5.md)
  bool alt = ctx_.ranks_on_device == 1;
  const size_t n = ss_.size();
  if (alt) {
    std::vector<Stream*> all;
    for (size_t i = 0; i < 2 * n; ++i) {
      alt_owned_.push_back(ctx_.dev->create_stream(i % n > 0));
      all.push_back(alt_owned_.back().get());
    }
    std::string detail;
    alt = ctx_.dev->queues_independent(all, 0.05, &detail);
  }
  alt = ctx_.hg().allreduce_max(alt ? 0.0 : 1.0) < 0.5;
  if (alt) {
    for (size_t i = 0; i < n; ++i) {
      lanes_ss_[i] = alt_owned_[i].get();
      alt_ss_.push_back(alt_owned_[n + i].get());
    }
  } else {
    alt_owned_.clear();
  }
}

std::string Replay::warmup_trouble(double last_warm_s) {
  ComputeEngine::ChainCounters cc;
  double timeouts = static_cast<double>(ctx_.dev->gate_event_timeouts());
  if (ctx_.compute->chain_counters(cc)) timeouts += cc.wait_timeouts + cc.gate_timeouts;
  const double floor_s = strat_.compute_floor_us(ctx_) * 1e-6 * ctx_.opt.time_scale;
  const bool slow = last_warm_s > 2.0 * floor_s + static_cast<double>(env_int("DLNB_LANE_WARM_SLACK_S", 5));
  if (ctx_.hg().allreduce_max((timeouts > 0 || slow) ? 1.0 : 0.0) <= 0.5) return "";
  return timeouts > 0 ? "gate waits timed out in the warm-up" : "a warm-up replay ran over twice the compute floor";
}

void Replay::fall_back_to_single_graph(const std::string& reason) {
  if (ctx_.rank() == 0 && !ctx_.opt.quiet) std::cerr << "[dlnb] lane graphs: " << reason << "; the single graph instead\n";
  ctx_.dev->synchronize();
  drop_lanes();
  lane_info_ = Json::object();
  capture(false, "lanes fell back after the warm-up");
  lane_info_["fallback"] = reason;
}

void Replay::enqueue() {
  if (replay_) {
    const uint64_t it = ++dev_iter_;
    const auto& L = lanes_for(it);
    for (Stream* l : L) ctx_.dev->set_iteration(*l, it);
    if (lane_graphs_.empty())
      graph_->launch(*origin_);
    else
      for (size_t i = 0; i < lane_graphs_.size(); ++i) lane_graphs_[i]->launch(*L[i]);
  } else {
    T_.iteration_start(*strat_.streams()[0]);
    strat_.enqueue_iteration();
    T_.finish_stalls();
  }
}

void Replay::enqueue_timed() {
  if (TL_ && replay_ && tl_edges_) TL_->edge(*origin_, 0);
  enqueue();
  if (TL_ && replay_ && tl_edges_) TL_->edge(*origin_, 1);
}

void Replay::wait_iteration() {
  if (lane_done_) {
    CompletionFlag cf(lane_done_, joined_ ? 1 : lane_done_n_, dev_iter_);
    strat_.synchronize();
  } else {
    strat_.synchronize();
  }
}

// Graph replays on a GPU (DLNB_PREARM=1, the default): the host runs one
// launch ahead. Iteration r+1's graph is enqueued while r runs, behind a
// one-wave kernel that holds the launch stream until the host stores r+2 in
// a host-coherent "go" word; a kernel after each graph stores r+1 in a
// "done" word the host polls (CompletionFlag). Each iteration is still
// timed alone, from the go store to the host seeing its done word, but its
// start no longer waits for hipGraphLaunch's submission after an idle
// device (~70 us) and its end not for hipStreamQuery (~20 us)
// (profiles/host_boundary_r4.md). Iteration 0 is armed before the timed
// region starts (as the last warm-up iteration would in a longer loop); all
// of its device work runs inside it, as does the loop's closing device
// synchronize. DLNB_PREARM=0: launch, then poll the streams (A/B).
// Lane graphs: every lane has its own go wait and done word; the host
// waits for all of them (the iteration ends when every stream has).
void Replay::begin_timed() {
  // DLNB_TIMELINE_EDGES=1 (with --timeline --graph): a stamp kernel on the
  // launch stream before and after each timed graph launch (Timeline::edge;
  // two more kernels per iteration, so off by default)
  tl_edges_ = env_int("DLNB_TIMELINE_EDGES", 0) != 0;
  nlanes_ = lanes_ss_.size();
  nhs_ = 2 + nlanes_;
  if (replay_ && ctx_.dev->kind() == DeviceKind::GPU && env_int("DLNB_PREARM", 1) != 0) hs_ = ctx_.dev->alloc_stamps(nhs_);
  timed_ = true;
  // An armed replay waits for its go through the whole iteration before it:
  // its wait's bound (after which it runs anyway, counted in
  // prearm_go_timeouts) is 4x the compute floor + 60 s.
  go_timeout_s_ = std::max(60.0, 4.0 * strat_.compute_floor_us(ctx_) * 1e-6 * ctx_.opt.time_scale + 60.0);
}

void Replay::arm(int r) {
  const uint64_t it = ++dev_iter_;
  armed_iter_.push_back(it);
  const auto& L = lanes_for(it);
  for (size_t i = 0; i < nlanes_; ++i) {
    Stream& l = *L[i];
    ctx_.dev->host_wait(l, hs_, static_cast<uint64_t>(r) + 1, go_timeout_s_, hs_ + 1, it);
    if (TL_ && tl_edges_ && i == 0) TL_->edge(l, 0);
    if (lane_graphs_.empty())
      graph_->launch(l);
    else
      lane_graphs_[i]->launch(l);
    if (TL_ && tl_edges_ && i == 0) TL_->edge(l, 1);
    // (lane graphs signal from inside: their last node, lane_done)
    if (!lane_done_) ctx_.dev->host_signal(l, hs_ + 2 + i, static_cast<uint64_t>(r) + 1);
  }
}

size_t Replay::nodes() const {
  size_t nodes = graph_ ? graph_->nodes() : 0;
  for (const auto& g : lane_graphs_) nodes += g->nodes();
  return nodes;
}

}  // namespace dlnb
