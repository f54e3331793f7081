#include "dlnb/program.hpp"

namespace dlnb {

void ProgramBuilder::begin() {
  DLNB_REQUIRE(!open_, "begin_program: a program is already open on this stream");
  open_ = true;
  index_ = 0;
  tasks_.clear();
  pending_.clear();
  done_free_ = false;
  split_ = false;
}

void ProgramBuilder::fold_wait(const uint64_t* gate, uint32_t tag) {
  for (auto& w : pending_)
    if (w.first == gate) {  // the same gate again: its latest record
      w.second = tag;
      return;
    }
  pending_.emplace_back(gate, tag);
}

void ProgramBuilder::fold_record(uint64_t* gate, uint32_t tag) {
  if (pending_.empty() && done_free_ && !tasks_.empty()) {
    // recorded right after a task: that task's done gate
    tasks_.back().sync.done_gate = gate;
    tasks_.back().sync.done_tag = tag;
    done_free_ = false;
    return;
  }
  emit_pending(gate, tag);
  if (tasks_.empty() || tasks_.back().sync.done_gate != gate) {
    // nothing pending and no task to carry it: a gate-only task raises it
    kernels::DlTask t = gate_task();
    t.sync.done_gate = gate;
    t.sync.done_tag = tag;
    push_task(t);
  }
  done_free_ = false;
}

void ProgramBuilder::append(kernels::DlTask t) {
  take_pending(t.sync);
  push_task(t);
  done_free_ = t.sync.done_gate == nullptr;
}

std::vector<kernels::DlTask> ProgramBuilder::take() {
  // folded waits not taken by a task yet: the launch ends with them (a
  // kernel of its own follows it on the stream)
  emit_pending(nullptr, 0);
  done_free_ = false;
  std::vector<kernels::DlTask> ts;
  ts.swap(tasks_);
  return ts;
}

bool ProgramBuilder::end(const ProgramJoin* join) {
  emit_pending(nullptr, 0);  // waits after the last task: before the join
  open_ = false;
  if (!join || tasks_.empty()) return false;
  size_t g = 0;
  do {
    kernels::DlTask t;
    t.sync = base_();
    for (int i = 0; i < 2 && g < join->gates.size(); ++i, ++g) {
      t.sync.gate[i] = join->gates[g];
      t.sync.tag[i] = join->tag;
    }
    if (g >= join->gates.size()) t.sync.tstart[0] = join->host_done;
    tasks_.push_back(t);
  } while (g < join->gates.size());
  return true;
}

kernels::DlTask ProgramBuilder::gate_task() const {
  kernels::DlTask t;
  t.sync = base_();
  t.ticks = fixed_ ? 0 : 1;
  t.flags = kernels::kTaskGateOnly;
  return t;
}

void ProgramBuilder::push_task(kernels::DlTask t) {
  DLNB_REQUIRE(index_ < kMaxTasks, "more than 4096 program tasks per iteration on one stream");
  t.epoch = index_++;  // the kernel derives the epoch from it and the iteration word
  tasks_.push_back(t);
}

void ProgramBuilder::emit_pending(uint64_t* done_gate, uint32_t done_tag) {
  while (!pending_.empty()) {
    kernels::DlTask t = gate_task();
    for (int i = 0; i < 2 && !pending_.empty(); ++i) {
      t.sync.gate[i] = pending_.front().first;
      t.sync.tag[i] = pending_.front().second;
      pending_.erase(pending_.begin());
    }
    if (pending_.empty() && done_gate) {
      t.sync.done_gate = done_gate;
      t.sync.done_tag = done_tag;
    }
    push_task(t);
    done_free_ = false;
  }
}

void ProgramBuilder::take_pending(kernels::DlSync& sync) {
  if (pending_.empty()) return;
  const size_t free_slots = (sync.gate[0] ? 0u : 1u) + (sync.gate[1] ? 0u : 1u);
  if (pending_.size() > free_slots) {
    // keep the last free_slots for the task, the rest before it
    std::vector<std::pair<const uint64_t*, uint32_t>> keep(pending_.end() - static_cast<long>(free_slots),
                                                           pending_.end());
    pending_.resize(pending_.size() - free_slots);
    emit_pending(nullptr, 0);
    pending_ = keep;
  }
  for (int i = 0; i < 2 && !pending_.empty(); ++i) {
    if (sync.gate[i]) continue;
    sync.gate[i] = pending_.front().first;
    sync.tag[i] = pending_.front().second;
    pending_.erase(pending_.begin());
  }
}

}  // namespace dlnb
