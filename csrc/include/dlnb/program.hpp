// The task list of one stream's compute program (ComputeEngine::begin_program
// .. end_program, kernels::gemm_tn_deadline_program), built on the host with
// no device in sight.
//
// Between the compute tasks the stream's gate-event waits and records arrive
// (Device::StreamFold) and are folded into the list: a wait becomes a gate of
// the next task, a record the done gate of the task before it, and where
// neither fits (a task has two gate slots and one done gate) a gate-only task
// (kernels::kTaskGateOnly) carries them. The program may be launched in
// pieces (take()); end() appends the lane join. Every task gets its index
// among the iteration's program tasks on the stream (DlTask::epoch), which
// runs on across the pieces.
#pragma once

#include <cstdint>
#include <functional>
#include <utility>
#include <vector>

#include "dlnb/kernels.hpp"

namespace dlnb {

// A lane join (ComputeEngine::set_lane_join): the program's last task(s) wait
// for `gates`, raised with `tag`, and the last one stores the iteration
// number into *host_done.
struct ProgramJoin {
  std::vector<uint64_t*> gates;
  uint32_t tag = 0;
  uint64_t* host_done = nullptr;
};

class ProgramBuilder {
 public:
  // Program tasks of one iteration on one stream (the kernels derive a task's
  // epoch, 1..32767, from its index and the iteration word).
  static constexpr uint32_t kMaxTasks = 4096;

  // base(): the sync words every task carries (iter, counters, gate_timeout,
  // abort), asked for whenever the builder makes a task of its own.
  // fixed_work: gate-only tasks of a fixed-work program have ticks 0; in a
  // deadline program 1 (the stream's chain goes on from when its gates opened).
  ProgramBuilder(std::function<kernels::DlSync()> base, bool fixed_work)
      : base_(std::move(base)), fixed_(fixed_work) {}

  bool open() const { return open_; }
  // A short task was launched on its own while the program was open.
  bool split() const { return split_; }
  void mark_split() { split_ = true; }
  const std::vector<kernels::DlTask>& tasks() const { return tasks_; }

  // An empty program whose task index starts at 0.
  void begin();
  // A gate-event wait: the next task waits for (gate, tag). The same gate
  // again replaces its tag (its latest record).
  void fold_wait(const uint64_t* gate, uint32_t tag);
  // A gate-event record: (gate, tag) is raised once everything before it is
  // done - by the task right before it, else by a gate-only task.
  void fold_record(uint64_t* gate, uint32_t tag);
  // A compute task: it takes the pending waits as its gates (those beyond its
  // free gate slots go to gate-only tasks before it) and the next index.
  void append(kernels::DlTask t);
  // The tasks so far, for a launch (pending waits leave with them, as
  // gate-only tasks); the program stays as open as it was.
  std::vector<kernels::DlTask> take();
  // Closes the program. With a join and tasks left to launch, the join
  // task(s) follow them - two gates each, the last one stores the done word;
  // they advance no index - and true is returned. take() has the rest.
  bool end(const ProgramJoin* join);

 private:
  kernels::DlTask gate_task() const;
  void push_task(kernels::DlTask t);
  // The pending waits as gate-only tasks (two gates each); the last one
  // raises done_gate when given.
  void emit_pending(uint64_t* done_gate, uint32_t done_tag);
  void take_pending(kernels::DlSync& sync);

  std::function<kernels::DlSync()> base_;
  bool fixed_;
  bool open_ = false;
  uint32_t index_ = 0;  // program tasks of the iteration so far (DlTask::epoch)
  std::vector<kernels::DlTask> tasks_;
  // folded waits (gate, tag) the next task takes as its gates
  std::vector<std::pair<const uint64_t*, uint32_t>> pending_;
  bool done_free_ = false;  // tasks_.back() has no done gate: a record right after it takes that one
  bool split_ = false;
};

}  // namespace dlnb
