// The run's report document (the reference's ccutils JSON section plus the
// `dlnb` block), assembled from plain inputs after the timed loop.
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "dlnb/aux.hpp"
#include "dlnb/replay.hpp"

namespace dlnb {

// What the runner's setup leaves for the loops and the report.
struct RunSetup {
  explicit RunSetup(int rank) : fault(rank) {}
  std::string backend;     // resolved (select_backend)
  std::string stats_path;
  int lanes = 1;           // collective_lanes(): the CTA budget's divisor
  bool rccl = false;       // the CTA budget applies (rccl, mixed, xgmi)
  bool gemm_compute = false;
  std::unique_ptr<EnergyMeter> meter;
  FaultInjector fault;
  long long iter_no = 0;   // iterations started (warm-up and timed): the fault injector's count
  const char* rkey = "";   // Strategy::runtime_key()
};

// What the warm-up and the timed loop measured on the host.
struct TimedRuns {
  std::vector<double> warm;    // s per warm-up iteration
  int runs = 0;
  double timed_region_s = 0;   // max over ranks
  // host time of each arm() (the launches of the next replay): a launch that
  // blocks on the runtime shows up here (profiles/stall_r5.md)
  std::vector<double> arm_s;
  // clock / power at each iteration's end (the sampler thread's latest
  // readings, and sclk's range over the iteration: VERDICT r5 #7)
  std::vector<EnergyMeter::Sensors> sensors;
};

// This rank's entry of the document's `ranks`.
Json rank_report(Context& ctx, Strategy& strat, const TimedRuns& runs, const Replay& replay);
// The document, from every rank's rank_report() (dumped, in rank order);
// `timeline_info`: the `timeline` block (--timeline), else null.
Json global_report(Context& ctx, Strategy& strat, const RunSetup& setup, const TimedRuns& runs, const Replay& replay,
                   const std::vector<std::string>& rank_docs, const Json& timeline_info);

}  // namespace dlnb
