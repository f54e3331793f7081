// One rank's iteration replay: the captured graph(s) of one iteration, the
// streams they are launched on, the host's completion words and the pre-armed
// handshake (runner.cpp drives it: build -> warm-up -> loop mode | timed loop).
// Without --graph it enqueues the strategy's iteration eagerly.
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "dlnb/strategy.hpp"

namespace dlnb {

class Replay {
 public:
  Replay(Context& ctx, Strategy& strat, const std::string& backend);
  // The destruction rules (replay.cpp): on an exception leaving the timed
  // loop the device waits are aborted before anything is released, and the
  // host words are kept; otherwise words, owned streams, graphs, in that order.
  ~Replay();
  Replay(const Replay&) = delete;
  Replay& operator=(const Replay&) = delete;

  // --graph: decides lane graphs or the single graph (every rank takes part in
  // every verdict, in the same order) and captures one iteration.
  void build();
  bool lanes() const { return !lane_graphs_.empty(); }
  // After the warm-up, lane graphs only (every rank takes part): what went
  // wrong with the lane replays, or "" when they stay.
  std::string warmup_trouble(double last_warm_s);
  // Re-captures the iteration as the single graph (`lane_graphs.fallback`);
  // the caller warms it once.
  void fall_back_to_single_graph(const std::string& reason);

  void enqueue();
  // enqueue() between the --timeline edge stamps (DLNB_TIMELINE_EDGES=1)
  void enqueue_timed();
  // Host wait for the iteration just enqueued: lane graphs by their done words
  // (the graphs' own completion comes later: each ends with a marker), else
  // the streams.
  void wait_iteration();

  // Start of the timed loop: allocates the handshake words of the pre-armed
  // loop (graph replays on a GPU, DLNB_PREARM=1), and from here on an
  // exception is a failure of the timed loop (~Replay).
  void begin_timed();
  bool prearmed() const { return hs_ != nullptr; }
  // Submits timed replay r behind its go wait.
  void arm(int r);
  void go(int r) { __atomic_store_n(hs_, static_cast<uint64_t>(r) + 1, __ATOMIC_RELEASE); }
  void wait_armed(int r) {
    if (lane_done_) {
      CompletionFlag cf(lane_done_, joined_ ? 1 : lane_done_n_, armed_iter_.at(static_cast<size_t>(r)));
      strat_.synchronize();
    } else {
      CompletionFlag cf(hs_ + 2, nlanes_, static_cast<uint64_t>(r) + 1);
      strat_.synchronize();
    }
  }
  double go_timeouts() const { return static_cast<double>(__atomic_load_n(hs_ + 1, __ATOMIC_ACQUIRE)); }

  // The report's `lane_graphs` block and `graph` (nodes captured, 0: eager).
  const Json& describe() const { return lane_info_; }
  size_t nodes() const;

 private:
  void capture(bool lanes, std::string why);
  bool capture_lanes(std::string* why);
  void pick_replay_streams();
  void drop_lanes();
  void free_lane_done();
  // the streams replay `it` runs on (lane graphs alternate between two sets)
  const std::vector<Stream*>& lanes_for(uint64_t it) const { return !alt_ss_.empty() && (it & 1) ? alt_ss_ : lanes_ss_; }

  Context& ctx_;
  Strategy& strat_;
  const std::string backend_;
  TimerSet& T_;
  Timeline* TL_;
  // (graphs first, owned streams last: members go in reverse order)
  std::unique_ptr<GraphExec> graph_;
  std::vector<std::unique_ptr<GraphExec>> lane_graphs_;
  // lane graphs: each lane's last node stores the iteration number here (the
  // host's completion words; Device::lane_done)
  uint64_t* lane_done_ = nullptr;
  size_t lane_done_n_ = 0;
  bool joined_ = false;  // the compute program's join signals the iteration (lane_done[0] alone)
  Json lane_info_ = Json::object();
  std::vector<Stream*> lanes_ss_;  // streams the replay is launched on (lane graphs: each; else the compute stream)
  std::vector<Stream*> alt_ss_;    // lane graphs: the second set, odd replays
  std::vector<Stream*> ss_, others_;  // --graph: the strategy's streams (compute first)
  std::vector<std::unique_ptr<Stream>> alt_owned_;
  bool replay_ = false;
  Stream* origin_ = nullptr;
  // Device iteration word (gates' sequence numbers): one value per replay,
  // stored at the head of every lane before its graph runs.
  uint64_t dev_iter_ = 0;
  // the pre-armed loop
  bool timed_ = false;
  bool tl_edges_ = false;
  size_t nlanes_ = 0, nhs_ = 0;
  uint64_t* hs_ = nullptr;  // [0] go, [1] go-wait timeouts, [2 + i] lane i done
  double go_timeout_s_ = 0;
  std::vector<uint64_t> armed_iter_;  // device iteration number of each armed replay
};

}  // namespace dlnb
