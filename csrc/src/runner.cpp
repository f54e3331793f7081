// Benchmark runner shared by all strategies: bootstrap, device/backend
// selection, warm-up, run-count estimation, timed runs, loop mode. The
// iteration's graph replay is replay.cpp, the report document report.cpp.
//
// Reference flow: main() of each driver (e.g. cpp/data_parallel/dp.cpp:127-303):
// parse args -> read stats -> MPI_Init -> topology print -> set device ->
// CCL init -> buffers -> barrier -> warm-up (MPI_Wtime) -> optional
// estimate_runs -> PROXY_LOOP or timed runs -> ccutils JSON section.
// Deviations: estimate_runs averages warm-ups over warm-ups (the reference
// divides a world-sum by the warm-up count, cpp/utils.hpp:127-128) and takes
// the max over ranks; loop mode is a run-time flag (or a *_loop argv[0]).
#include <algorithm>
#include <exception>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <mutex>
#include <sstream>
#include <thread>

#include <sys/prctl.h>

#include "dlnb/kernels.hpp"
#include "dlnb/report.hpp"

namespace dlnb {

namespace {
thread_local const uint64_t* t_done_flag = nullptr;
thread_local size_t t_done_n = 0;
thread_local uint64_t t_done_value = 0;

// The run on this thread, for device_failure (set by run_rank).
struct FailGuard {
  Device* dev = nullptr;
  std::vector<Communicator*>* comms = nullptr;
  bool cli_exit = false;  // CLI process owning its ranks: end the process at the first failure
  int rank = 0;
  bool fired = false;
};
thread_local FailGuard* t_fail = nullptr;
std::atomic<bool> g_poisoned{false};
}  // namespace

void device_failure(const std::string& why) {
  FailGuard* f = t_fail;
  if (!f || f->fired) return;
  f->fired = true;
  if (f->dev) f->dev->raise_abort();
  if (f->cli_exit && f->dev) {  // (GPU runs only: a CPU run's failure path is its own, unchanged)
    std::fprintf(stderr,
                 "[dlnb] rank %d error: %s\n[dlnb] rank %d: device waits aborted; exiting without teardown (the "
                 "driver reclaims the GPU queues)\n",
                 f->rank, why.c_str(), f->rank);
    std::fflush(stdout);
    std::fflush(stderr);
    std::_Exit(3);
  }
  if (f->comms)
    for (Communicator* c : *f->comms)
      if (c) c->abort();
}

bool process_poisoned() { return g_poisoned.load(); }

CompletionFlag::CompletionFlag(const uint64_t* flags, size_t n, uint64_t value)
    : prev_(t_done_flag), prev_n_(t_done_n), prev_value_(t_done_value) {
  t_done_flag = flags;
  t_done_n = n;
  t_done_value = value;
}
CompletionFlag::~CompletionFlag() {
  t_done_flag = prev_;
  t_done_n = prev_n_;
  t_done_value = prev_value_;
}

void sync_streams(const std::vector<Stream*>& streams, const std::vector<Communicator*>& comms, Device& dev) {
  (void)dev;
  // Poll period: with the default 50-us timer slack a 20-us sleep woke ~70 us
  // late, and every timed iteration ends inside this loop (the reference times
  // each iteration from the host); slack 1 us + 5-us sleeps bound the wake-up
  // latency to a few us for a fraction of one core.
  thread_local const bool slack_set = [] {  // (timer slack is per thread)
    prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0);
    return true;
  }();
  (void)slack_set;
  const double timeout = static_cast<double>(env_int("DLNB_TIMEOUT", 900));
  const double t0 = now_s();
  int polls = 0;
  const uint64_t* flag = t_done_flag;
  const size_t nflags = t_done_n;
  const uint64_t want = t_done_value;
  auto done = [&](Stream* s) {
    if (!flag) return s->query();
    for (size_t i = 0; i < nflags; ++i)
      if (__atomic_load_n(flag + i, __ATOMIC_ACQUIRE) < want) return false;
    return true;
  };
  for (Stream* s : streams) {
    while (!done(s)) {
      if (++polls % 64 == 0) {
        for (Communicator* c : comms) {
          if (!c) continue;
          std::string err = c->async_error();
          if (!err.empty()) {
            device_failure("communication failure: " + err);
            for (Communicator* a : comms)
              if (a) a->abort();
            DLNB_THROW("communication failure: " << err);
          }
        }
        if (now_s() - t0 > timeout) {
          std::ostringstream m;
          m << "iteration did not complete within DLNB_TIMEOUT=" << timeout << " s (hung collective or dead peer)";
          if (flag) {
            // lane graphs: which lanes' done words (host-mapped) are behind
            m << "; lane done words (want " << want << "):";
            for (size_t i = 0; i < nflags; ++i) m << " " << __atomic_load_n(flag + i, __ATOMIC_ACQUIRE);
          }
          device_failure(m.str());
          for (Communicator* a : comms)
            if (a) a->abort();
          DLNB_THROW(m.str());
        }
      }
      std::this_thread::sleep_for(std::chrono::microseconds(5));
    }
  }
}

Json comm_stats_json(const std::vector<CommStat>& stats, const TimerSet& t) {
  Json out = Json::object();
  for (const auto& s : stats) {
    const auto& v = t.get(s.timer);
    Json e = Json::object();
    e["kind"] = s.name;
    e["nranks"] = s.nranks;
    e["bytes_per_op"] = s.bytes_per_op;
    e["ops"] = static_cast<long long>(v.size());
    double tot = 0;
    for (double x : v) tot += x;
    e["total_s"] = tot;
    // A 1-rank group moves nothing over a link: its "collective" is a local
    // device copy (or nothing), so it reports busbw 0 and says so.
    e["transport"] = s.nranks > 1 ? "link" : "local-copy";
    if (!v.empty() && tot > 0) {
      double algbw = s.bytes_per_op * v.size() / tot / 1e9;
      e["algbw_GBps"] = algbw;
      e["busbw_GBps"] = algbw * busbw_factor(s.kind, s.nranks);
    }
    out[s.name] = e;
  }
  return out;
}

Buffer comm_buffer(Device& dev, Communicator& c, size_t bytes) {
  if (!c.wants_peer_buffers()) return dev.alloc(bytes);
  Buffer b = dev.alloc_peer(bytes);
  c.register_buffer(b.data(), bytes);
  return b;
}

void Strategy::join_or_stall_tail(Context& ctx, Stream& compute, bool prog, Stream& dp_lane, Event& dp_done,
                                  const uint64_t* dp_end) {
  const bool join = prog && !ctx.opt.optimizer && dp_end && timers_->task_stamps();
  if (prog) ctx.compute->end_program(compute, join);
  if (join) {
    timers_->stall_until(compute, dp_end, "dp_exposed_time");
  } else {
    dp_lane.record(dp_done);
    timers_->stall_after_task(compute, dp_done, "dp_exposed_time");
  }
}

void optimizer_step(Context& ctx, Stream& s, void* param, void* mom, const void* grad, size_t n, uint64_t* end_stamp,
                    uint32_t* done) {
  if (ctx.dev->kind() == DeviceKind::GPU) {
    kernels::sgd_momentum_bf16(param, mom, grad, n, 1e-4f, 0.9f, s.native(), end_stamp, done);
    return;
  }
  ctx.dev->host_task(s, [param, mom, grad, n] {
    auto* p = static_cast<uint16_t*>(param);
    auto* m = static_cast<uint16_t*>(mom);
    auto* g = static_cast<const uint16_t*>(grad);
    for (size_t i = 0; i < n; ++i) {
      float mv = 0.9f * bf16_to_float(m[i]) + bf16_to_float(g[i]);
      m[i] = float_to_bf16(mv);
      p[i] = float_to_bf16(bf16_to_float(p[i]) - 1e-4f * mv);
    }
  });
  // (the CPU device's stamp: when the stream reaches it, i.e. after the task above)
  if (end_stamp) ctx.dev->stamp(s, end_stamp);
}

// ------------------------------------------------------------- topology

void print_topology(Context& ctx) {
  // Reference: cpp/netcommunicators.hpp:142-290 builds a switch/node tree
  // from SLURM_TOPOLOGY_ADDR (fake address when SLURM is absent, :154-157).
  // Here each rank also reports its GPU, and rank 0 prints the node's
  // xGMI link matrix.
  std::string addr = env_or("SLURM_TOPOLOGY_ADDR", "");
  if (addr.empty()) addr = "root." + ctx.boot->info.hostname;
  std::ostringstream me;
  me << addr << "|" << ctx.boot->info.hostname << "|" << ctx.dev->name() << "|" << ctx.dev->index();
  auto all = ctx.hg().allgather(me.str());
  if (ctx.rank() != 0) return;
  // path -> ranks
  std::map<std::string, std::vector<int>> leaves;
  std::map<std::string, std::string> dev_of;
  for (size_t r = 0; r < all.size(); ++r) {
    auto f = split(all[r], '|');
    leaves[f[0]].push_back(static_cast<int>(r));
    dev_of[f[0]] = f.size() > 2 ? f[2] : "?";
  }
  std::ostringstream os;
  os << "=== topology: " << all.size() << " ranks on " << leaves.size() << " node(s) ===\n";
  std::vector<std::string> prev;
  for (const auto& kv : leaves) {
    auto parts = split(kv.first, '.');
    size_t common = 0;
    while (common < prev.size() && common < parts.size() - 1 && prev[common] == parts[common]) ++common;
    for (size_t d = common; d < parts.size(); ++d) {
      os << std::string(2 * d, ' ') << (d ? "└─ " : "") << parts[d];
      if (d + 1 == parts.size()) {
        os << "  ranks [";
        for (size_t i = 0; i < kv.second.size(); ++i) os << (i ? "," : "") << kv.second[i];
        os << "]  " << dev_of[kv.first];
      }
      os << "\n";
    }
    prev = parts;
  }
  if (ctx.dev->kind() == DeviceKind::GPU) os << describe_gpu_links();
  std::cout << os.str() << std::flush;
}

namespace {

std::vector<int> parse_device_list(const std::string& s) {
  std::vector<int> v;
  if (s.empty()) return v;
  for (auto& p : split(s, ',')) {
    std::string t = trim(p);
    if (!t.empty()) v.push_back(std::stoi(t));
  }
  return v;
}

std::unique_ptr<Strategy> make_strategy(StrategyKind k) {
  switch (k) {
    case StrategyKind::DP: return make_dp();
    case StrategyKind::FSDP: return make_fsdp();
    case StrategyKind::HybridCP: return make_cp();
    default: return make_pipeline(k);
  }
}

bool file_exists(const std::string& p) {
  std::ifstream f(p);
  return static_cast<bool>(f);
}

}  // namespace

namespace {

// Wraps the backend's factory and logs every communicator it creates (name,
// members, the library's own rank count) into ctx.comm_log for the report.
class RecordingFactory : public CommFactory {
 public:
  RecordingFactory(std::unique_ptr<CommFactory> inner, std::vector<CommRecord>* log, std::vector<Communicator*>* live)
      : inner_(std::move(inner)), log_(log), live_(live) {}
  std::string backend_name() const override { return inner_->backend_name(); }
  std::unique_ptr<Communicator> create(const std::string& name, const std::vector<int>& members,
                                       size_t capacity_bytes, bool need_p2p, int max_ctas) override {
    auto c = inner_->create(name, members, capacity_bytes, need_p2p, max_ctas);
    log_->push_back({name, c->backend_name(), c->size(), c->library_nranks()});
    return c;
  }
  void add_live(Communicator* c) { live_->push_back(c); }

 private:
  std::unique_ptr<CommFactory> inner_;
  std::vector<CommRecord>* log_;
  std::vector<Communicator*>* live_;
};

// The outermost communicator wrapper (tracing, when --timeline wraps the
// factory afterwards) is what the strategy holds; it reports itself here.
class LiveFactory : public CommFactory {
 public:
  LiveFactory(std::unique_ptr<CommFactory> inner, std::vector<Communicator*>* live)
      : inner_(std::move(inner)), live_(live) {}
  std::string backend_name() const override { return inner_->backend_name(); }
  std::unique_ptr<Communicator> create(const std::string& name, const std::vector<int>& members,
                                       size_t capacity_bytes, bool need_p2p, int max_ctas) override {
    auto c = inner_->create(name, members, capacity_bytes, need_p2p, max_ctas);
    live_->push_back(c.get());
    return c;
  }

 private:
  std::unique_ptr<CommFactory> inner_;
  std::vector<Communicator*>* live_;
};

}  // namespace

Json comm_log_json(const std::vector<CommRecord>& log) {
  Json out = Json::object();
  Json all = Json::array();
  Json rccl = Json::object();
  for (const auto& r : log) {
    Json e = Json::object();
    e["name"] = r.name;
    e["backend"] = r.backend;
    e["nranks"] = r.nranks;
    e["library_nranks"] = r.library_nranks;
    all.push_back(e);
    if (r.library_nranks >= 0) rccl[r.name] = r.library_nranks;
  }
  out["communicators"] = all;
  out["rccl_nranks"] = rccl;
  return out;
}

int collective_lanes(const Options& o, int world) {
  switch (o.strategy) {
    case StrategyKind::DP: return 1;
    case StrategyKind::FSDP: {
      const int F = std::max(1, o.sharding_factor);
      const bool replicas = world / F > 1;
      return o.comm_lanes == "split" ? 2 + (replicas ? 1 : 0) : 1;
    }
    case StrategyKind::HybridCP: return 2;
    default: return o.num_stages > 1 ? 3 : 1;
  }
}

std::string select_backend(Context& ctx, const std::string& requested, const std::string& devices) {
  const RankInfo& ri = ctx.boot->info;
  std::string backend = requested;
  const bool in_process = backend == "loopback" || backend == "loopback-cpu";
  const int ngpu = in_process ? 0 : gpu_device_count();
  if (backend == "auto") backend = ngpu > 0 ? "rccl" : "cpu";
  if (backend == "rccl" || backend == "xgmi" || backend == "mixed") {
    DLNB_REQUIRE(ngpu > 0, "--backend " << backend << " requested but no GPU is visible");
    std::vector<int> list = parse_device_list(devices);
    if (list.empty())
      for (int i = 0; i < ngpu; ++i) list.push_back(i);
    DLNB_REQUIRE(ri.local_rank < static_cast<int>(list.size()),
                 "local rank " << ri.local_rank << " has no device (device list has " << list.size() << ")");
    int dev_index = list[static_cast<size_t>(ri.local_rank)];
    DLNB_REQUIRE(dev_index >= 0 && dev_index < ngpu, "device id " << dev_index << " out of range");
    ctx.ranks_on_device = 0;
    for (int r = 0; r < ri.local_size && r < static_cast<int>(list.size()); ++r)
      ctx.ranks_on_device += list[static_cast<size_t>(r)] == dev_index;
    ctx.dev = make_gpu_device(dev_index);
    ctx.comms = backend == "rccl"    ? make_rccl_factory(ctx.hg(), *ctx.dev)
                : backend == "xgmi" ? make_xgmi_factory(ctx.hg(), *ctx.dev)
                                    : make_mixed_factory(ctx.hg(), *ctx.dev);
  } else if (backend == "cpu") {
    ctx.dev = make_cpu_device();
    ctx.comms = make_shm_factory(ctx.hg(), *ctx.dev);
  } else if (backend == "loopback" || backend == "loopback-cpu") {
    DLNB_REQUIRE(ctx.boot->hub, "--backend " << backend << " runs inside one process (run_benchmark starts the rank threads)");
    if (backend == "loopback-cpu") {
      // CPU device only: no HIP call at all (GPU-less hosts and CPU tests)
      ctx.dev = make_cpu_device(loopback_cpu_abort_flag(*ctx.boot->hub));
      ctx.ranks_on_device = ri.world_size;
    } else {
      // Every rank on the same GPU: the one given by -d (default 0).
      const int ngpu = gpu_device_count();
      DLNB_REQUIRE(ngpu > 0, "--backend loopback needs a GPU (loopback-cpu runs the ranks on the CPU device)");
      std::vector<int> list = parse_device_list(devices);
      const int dev_index = list.empty() ? 0 : list[0];
      for (int d : list)
        DLNB_REQUIRE(d == dev_index, "--backend loopback puts every rank on one device (-d " << devices << ")");
      DLNB_REQUIRE(dev_index >= 0 && dev_index < ngpu, "device id " << dev_index << " out of range");
      ctx.dev = make_gpu_device(dev_index);
      ctx.ranks_on_device = ri.world_size;
    }
    ctx.comms = make_loopback_factory(ctx.hg(), *ctx.dev, ctx.boot->hub);
  } else {
    DLNB_THROW("unknown backend '" << backend << "' (auto, rccl, xgmi, mixed, cpu, loopback, loopback-cpu)");
  }
  ctx.comms = wrap_comm_quant(std::move(ctx.comms), *ctx.dev, ctx.opt.wire_quant, &ctx.wire_quant);
  ctx.comms = wrap_comm_faults(std::move(ctx.comms), *ctx.dev, ri.rank);
  ctx.comms.reset(new RecordingFactory(std::move(ctx.comms), &ctx.comm_log, &ctx.live_comms));
  return backend;
}

namespace {

Json run_rank(const Options& opt, std::unique_ptr<Bootstrap> boot);

// Set by main_for: this process is a CLI binary, not a library host (Python).
std::atomic<bool> g_cli_process{false};

// State of one loopback job, shared by its rank threads (heap-held so a rank
// thread that outlives run_loopback - detached after a failure - never
// touches a dead stack frame).
struct LoopbackJob {
  Options opt;
  std::shared_ptr<LocalStore> store;
  std::shared_ptr<LoopbackHub> hub;
  std::vector<Json> docs;
  std::mutex mu;
  std::condition_variable done_cv;
  int done = 0;
  std::string first_error;
};

// --backend loopback / loopback-cpu: the job's ranks are threads of this process sharing one
// LocalStore (host barriers / gathers) and one LoopbackHub (collectives). A
// failing rank aborts both (and the job's CPU abort switch), so the others
// leave their waits instead of hanging; the first failure is rethrown.
// Rank threads of loopback jobs still running. A job whose rank threads did
// not drain after a failure detaches them (below); they keep GPU streams and
// buffers until they finally leave their waits, so this process refuses new
// loopback jobs until then (they would share the GPU with the
// next job and may still run at interpreter exit).
std::atomic<int> g_loopback_threads{0};

Json run_loopback(const Options& opt) {
  const int n = opt.ranks;
  DLNB_REQUIRE(n >= 1, "--ranks must be >= 1");
  const int live = g_loopback_threads.load();
  DLNB_REQUIRE(live == 0, "a previous loopback job of this process still has " << live
                              << " rank threads blocked (detached after its failure); run the next job in a new process");
  DLNB_REQUIRE(env_int("WORLD_SIZE", 1) == 1 && env_int("DLNB_WORLD_SIZE", 1) == 1,
               "--backend loopback runs all ranks inside one process: launch it once, not under a multi-rank launcher");
  auto job = std::make_shared<LoopbackJob>();
  job->opt = opt;
  job->store = std::make_shared<LocalStore>();
  job->hub = make_loopback_hub(n, static_cast<double>(env_int("DLNB_STORE_TIMEOUT", 900)));
  job->docs.resize(static_cast<size_t>(n));
  std::vector<std::thread> threads;
  for (int r = 0; r < n; ++r) {
    g_loopback_threads.fetch_add(1);
    threads.emplace_back([job, r, n] {
      try {
        Json d = run_rank(job->opt, bootstrap_loopback(r, n, job->store, job->hub));
        loopback_drained(*job->hub, false, 0);
        std::lock_guard<std::mutex> g(job->mu);
        job->docs[static_cast<size_t>(r)] = std::move(d);
      } catch (const std::exception& e) {
        const std::string msg = "rank " + std::to_string(r) + ": " + e.what();
        {
          std::lock_guard<std::mutex> g(job->mu);
          if (job->first_error.empty()) job->first_error = msg;
        }
        loopback_abort(*job->hub, msg);
        job->store->abort(msg);
      }
      g_loopback_threads.fetch_sub(1);
      std::lock_guard<std::mutex> g(job->mu);
      ++job->done;
      job->done_cv.notify_all();
    });
  }
  // After the first failure the other rank threads get a bounded grace
  // period to leave their waits and tear down. A thread still blocked then
  // must not hold the job forever: the CLI process ends with the rank's
  // error (as a multi-process job would); a library host (Python) gets the
  // error as an exception, with the stuck threads detached (they only hold
  // the job's heap state).
  const double grace_s = static_cast<double>(env_int("DLNB_LOOPBACK_ABORT_GRACE_S", 10));
  std::unique_lock<std::mutex> g(job->mu);
  job->done_cv.wait(g, [&] { return job->done == n || !job->first_error.empty(); });
  if (job->done < n &&
      !job->done_cv.wait_for(g, std::chrono::duration<double>(grace_s), [&] { return job->done == n; })) {
    const int stuck = n - job->done;
    const std::string err = job->first_error;
    g.unlock();
    std::fprintf(stderr, "[dlnb] error: %s\n[dlnb] %d of %d rank threads still blocked %.0f s after the failure\n",
                 err.c_str(), stuck, n, grace_s);
    std::fflush(stderr);
    if (g_cli_process.load()) std::_Exit(2);
    for (auto& t : threads) t.detach();
    throw Error(err + " (" + std::to_string(stuck) +
                " rank threads still blocked were detached; this process runs no further loopback job until they "
                "exit)");
  }
  g.unlock();
  for (auto& t : threads) t.join();
  if (!job->first_error.empty()) throw Error(job->first_error);
  return job->docs[0];
}

}  // namespace

bool cli_process() { return g_cli_process.load(); }

Json run_benchmark(const Options& opt) {
  DLNB_REQUIRE(!process_poisoned(),
               "an earlier run of this process failed and left device work that did not drain: start a new process");
  if (opt.backend == "loopback" || opt.backend == "loopback-cpu") return run_loopback(opt);
  return run_rank(opt, bootstrap_from_env(opt.store_addr));
}

namespace {

Json run_rank_impl(const Options& opt, Context& ctx, std::unique_ptr<Strategy>& strat);

Json run_rank(const Options& opt, std::unique_ptr<Bootstrap> boot) {
  // ctx and the strategy outlive the try block: a failing loopback rank
  // aborts the hub (waking its peers' waits) BEFORE its streams are torn
  // down - their destructors drain queued work that may wait on those peers.
  Context ctx;
  ctx.opt = opt;
  ctx.boot = std::move(boot);
  std::unique_ptr<Strategy> strat;
  FailGuard guard;
  guard.comms = &ctx.live_comms;
  guard.rank = ctx.boot->info.rank;
  guard.cli_exit = g_cli_process.load() && !ctx.boot->hub && env_int("DLNB_FAIL_EXIT", 1) != 0;
  struct GuardScope {
    FailGuard* prev;
    explicit GuardScope(FailGuard* g) : prev(t_fail) { t_fail = g; }
    ~GuardScope() { t_fail = prev; }
  } scope(&guard);
  try {
    Json r = run_rank_impl(opt, ctx, strat);
    t_fail = scope.prev;  // the run is over: strategy teardown is not a failure of it
    return r;
  } catch (const std::exception& e) {
    // The strategy is destroyed before the device (ctx outlives strat): its
    // events, buffers and communicators must not go while a stream task still
    // uses them (a CPU stream waiting on a freed event never returned - seen
    // after a peer died mid-iteration, library host).
    if (ctx.dev && ctx.dev->kind() == DeviceKind::GPU && !ctx.boot->hub) {
      // GPU: abort the device waits (CLI: the process ends here), abort the
      // communicators, then wait - bounded - for the device to drain; work
      // that does not drain keeps everything it may use (nothing is freed) and
      // this process runs nothing more.
      guard.dev = ctx.dev.get();
      device_failure(e.what());
      if (!ctx.dev->abort_and_drain()) {
        g_poisoned.store(true);
        const std::string msg = std::string(e.what()) +
                                " (device work did not drain within DLNB_ABORT_DRAIN_S after the abort: this process "
                                "runs no further benchmark)";
        (void)strat.release();
        (void)ctx.timeline.release();
        (void)ctx.compute.release();
        (void)ctx.comms.release();
        (void)ctx.dev.release();
        throw Error(msg);
      }
    } else if (ctx.dev && !ctx.boot->hub) {
      ctx.dev->abort_and_drain();
    }
    if (ctx.boot->hub) {
      const std::string msg = "rank " + std::to_string(ctx.boot->info.rank) + ": " + e.what();
      loopback_abort(*ctx.boot->hub, msg);
      if (auto* ls = dynamic_cast<LocalStore*>(ctx.boot->store.get())) ls->abort(msg);
      // The other ranks' streams may still hold copies into this rank's
      // buffers or waits on its events: drain this rank's work, then free
      // nothing (ctx / strat destructors) until every rank has drained too.
      try {
        if (ctx.dev) ctx.dev->synchronize();
      } catch (const std::exception&) {
      }
      loopback_drained(*ctx.boot->hub, true, static_cast<double>(env_int("DLNB_LOOPBACK_ABORT_GRACE_S", 10)));
    }
    throw;
  }
}

// Backend / device, workload, compute engine, the CTA budget, strategy setup
// and timers: everything before the first iteration.
RunSetup setup_rank(const Options& opt, Context& ctx, std::unique_ptr<Strategy>& strat) {
  const RankInfo& ri = ctx.boot->info;

  // ---- backend / device (cpp/utils.hpp:62-117 set_local_device)
  const std::string backend = select_backend(ctx, opt.backend, opt.devices);
  if (t_fail && ctx.dev->kind() == DeviceKind::GPU && !ctx.boot->hub) t_fail->dev = ctx.dev.get();

  // ---- workload
  std::string stats_path = opt.stats_file.empty() ? stats_path_for(opt.base_path, opt.model) : opt.stats_file;
  ctx.stats = parse_model_stats(stats_path);
  if (!opt.base_path.empty()) {
    std::string ap;
    try {
      ap = arch_path_for(opt.base_path, opt.model);
    } catch (const Error&) {
    }
    if (!ap.empty() && file_exists(ap)) {
      ctx.arch = parse_model_arch(ap);
      ctx.have_arch = true;
    }
  }
  ctx.wire = parse_dtype(opt.wire_dtype);
  ComputeShape shape;
  shape.hidden = static_cast<int>(ctx.stats.embedded_dim);
  uint64_t ffn = ctx.stats.ffn_dim ? ctx.stats.ffn_dim : (ctx.have_arch && ctx.arch.ff_dim ? ctx.arch.ff_dim : 4 * ctx.stats.embedded_dim);
  shape.ffn = static_cast<int>(ffn);
  std::string cdt = opt.compute_dtype;
  if (cdt == "auto") cdt = ctx.stats.dtype.find("8") != std::string::npos ? "fp8" : "bf16";
  shape.dtype = parse_dtype(cdt);
  shape.comm_cus = opt.comm_cus;
  shape.ranks_on_device = std::max(1, ctx.ranks_on_device);
  ComputeMode mode = parse_compute_mode(opt.compute, ctx.dev->kind());
  ctx.compute = make_compute_engine(*ctx.dev, mode, shape, opt.time_scale);
  if (!opt.timeline_path.empty()) {
    // every communicator the strategy creates and every compute task it
    // enqueues is traced (dlnb/timeline.hpp)
    ctx.timeline = std::make_unique<Timeline>(*ctx.dev);
    ctx.comms = make_tracing_factory(std::move(ctx.comms), ctx.timeline.get());
    ctx.compute = make_tracing_compute(std::move(ctx.compute), ctx.timeline.get());
  }
  ctx.comms.reset(new LiveFactory(std::move(ctx.comms), &ctx.live_comms));

  if (opt.topology) print_topology(ctx);

  Tracer::get().enable(opt.trace);
  std::unique_ptr<EnergyMeter> meter =
      ctx.dev->kind() == DeviceKind::GPU ? EnergyMeter::open_gpu(ctx.dev->index()) : EnergyMeter::none();
  RunSetup su(ri.rank);
  su.meter = std::move(meter);
  su.backend = backend;
  su.stats_path = stats_path;

  // ---- RCCL CTA budget: every comm lane's collective kernel must find CUs
  // beside the persistent compute (which leaves comm_cus CUs free), so
  // lanes x maxCTAs <= comm_cus; else blocks of one communicator's kernel can
  // sit in the queue while another communicator's kernel holds the free CUs
  // spinning on a peer that waits for them.
  const int lanes = su.lanes = collective_lanes(opt, ri.world_size);
  // xgmi kernels are budgeted too: a lane's kernel gets 4 blocks (512
  // threads, no LDS) per budgeted CU (comm_xgmi.cpp).
  su.rccl = backend == "rccl" || backend == "mixed" || backend == "xgmi";
  su.gemm_compute = ctx.compute->mode() == ComputeMode::Gemm;
  if (su.rccl) {
    if (opt.rccl_max_ctas >= 0)
      ctx.lane_ctas = opt.rccl_max_ctas;
    else
      ctx.lane_ctas = su.gemm_compute ? std::max(1, opt.comm_cus / lanes) : 0;
    if (ctx.lane_ctas > 0 && su.gemm_compute && lanes * ctx.lane_ctas > opt.comm_cus && ri.rank == 0)
      std::cerr << "[dlnb] warning: " << lanes << " comm lanes x " << ctx.lane_ctas << " RCCL CTAs > --comm-cus "
                << opt.comm_cus << ": concurrent collectives may not all fit beside the compute" << std::endl;
  }
  strat = make_strategy(opt.strategy);
  {
    TraceRange tr("dlnb:setup");
    strat->setup(ctx);
  }
  DLNB_REQUIRE(strat->streams().size() - 1 <= static_cast<size_t>(lanes),
               strategy_name(opt.strategy) << " uses " << strat->streams().size() - 1
                                           << " comm streams but collective_lanes() budgets " << lanes);
  if (ctx.dev->kind() == DeviceKind::GPU) {
    // More streams than hardware queues makes HIP share an in-order queue
    // between two streams: a collective spinning on its peers can then hold
    // back an unrelated kernel queued behind it on the other stream.
    const char* hwq = std::getenv("GPU_MAX_HW_QUEUES");
    const size_t nq = hwq ? static_cast<size_t>(std::max(1, std::atoi(hwq))) : 4;
    if (strat->streams().size() > nq && ri.rank == 0)
      std::cerr << "[dlnb] warning: " << strat->streams().size() << " streams per rank > GPU_MAX_HW_QUEUES=" << nq
                << "; streams will share hardware queues" << std::endl;
  }
  // the deadline clock's measured rate (kernels::wallclock_hz): taken here,
  // after setup gave its window time, and never inside a graph capture
  if (ctx.dev->kind() == DeviceKind::GPU) (void)ctx.dev->stamp_hz();
  if (ctx.timeline) ctx.timeline->calibrate(*strat->streams()[0]);
  su.rkey = strat->runtime_key();
  strat->timers()->ensure(su.rkey);
  ctx.compute->set_task_timers(strat->timers());
  return su;
}

// Start of every iteration, warm-up and timed (the fault injector counts them).
void next_iteration(RunSetup& su, Context& ctx, Strategy& strat) {
  // DLNB_INJECT_FAULT mode=task: a task that throws on the first stream
  // (CPU devices; library hosts must get the error back, not lose the process)
  su.fault.at_iteration(su.iter_no++, [&ctx, &strat] {
    DLNB_REQUIRE(ctx.dev->kind() == DeviceKind::CPU, "DLNB_INJECT_FAULT mode=task needs a CPU device");
    ctx.dev->host_task(*strat.streams()[0], [] { DLNB_THROW("injected fault in a stream task"); });
  });
}

void warm_up(Context& ctx, Strategy& strat, RunSetup& su, Replay& replay, std::vector<double>& warm) {
  Timeline* TL = ctx.timeline.get();
  for (int i = 0; i < ctx.opt.warmup; ++i) {
    next_iteration(su, ctx, strat);
    TraceRange tr("dlnb:warmup_iteration");
    double t0 = now_s();
    replay.enqueue();
    replay.wait_iteration();
    warm.push_back(now_s() - t0);
    if (TL) TL->collect(-1);
  }
  // Lane replays that timed out a gate wait, or ran far longer than the
  // compute floor, in the warm-up: re-capture the single graph and warm it
  // once (every rank alike). A safety valve for a first run on hardware the
  // lanes were not measured on (the 8-GPU node); `lane_graphs.fallback`.
  if (replay.lanes() && !warm.empty()) {
    const std::string what = replay.warmup_trouble(warm.back());
    if (!what.empty()) {
      replay.fall_back_to_single_graph(what);
      next_iteration(su, ctx, strat);
      replay.enqueue();
      replay.wait_iteration();
    }
  }
  strat.timers()->clear();
}

// --min-exectime: the run count from the warm-up times (every rank takes part).
int estimate_runs(Context& ctx, const std::vector<double>& warm) {
  // Skip the first two warm-ups when there are more (cpp/utils.hpp:121-135).
  double s = 0;
  int n = 0;
  for (size_t i = warm.size() > 2 ? 2 : 0; i < warm.size(); ++i, ++n) s += warm[i];
  double avg = n ? s / n : 1.0;
  avg = ctx.hg().allreduce_max(avg);
  const int runs = std::max(1, static_cast<int>(std::ceil(ctx.opt.min_exectime / std::max(avg, 1e-9))));
  if (ctx.rank() == 0 && !ctx.opt.quiet)
    std::cout << "Estimated runs based on warm-up times to meet minimum execution time: " << runs << std::endl;
  return runs;
}

// Interference generator (the reference's *_loop builds): no timers,
// runs forever unless --max-loop-iters bounds it.
Json loop_mode(Context& ctx, Strategy& strat, RunSetup& su, Replay& replay) {
  const Options& opt = ctx.opt;
  Timeline* TL = ctx.timeline.get();
  strat.timers()->set_enabled(false);
  for (long long it = 0; opt.max_loop_iters == 0 || it < opt.max_loop_iters; ++it) {
    next_iteration(su, ctx, strat);
    TraceRange tr("dlnb:loop_iteration");
    replay.enqueue();
    replay.wait_iteration();
    if (TL) TL->collect(-1);
  }
  ctx.hg().barrier();
  ctx.hg().store().finish();
  Json doc = Json::object();
  doc["section"] = strat.section_id();
  doc["loop_iterations"] = opt.max_loop_iters;
  return doc;
}

// The timed runs: each iteration timed alone on the host. Pre-armed replays
// (Replay::begin_timed) keep one launch ahead: between the go store and the
// host seeing the done word there is only arm(r + 1) and the wait.
void timed_loop(Context& ctx, Strategy& strat, RunSetup& su, Replay& replay, TimedRuns& tr) {
  TimerSet& T = *strat.timers();
  Timeline* TL = ctx.timeline.get();
  EnergyMeter* meter = su.meter.get();
  const int runs = tr.runs;
  const char* rkey = su.rkey;
  replay.begin_timed();
  const bool prearm = replay.prearmed();
  ctx.hg().barrier();
  ctx.compute->reset_capped(*strat.streams()[0]);  // count the timed iterations only
  ctx.dev->synchronize();
  if (prearm && runs > 0) replay.arm(0);  // submitted, held until the first go
  {
    EnergyMeter::Sensors s0;
    meter->take(s0);  // the first window starts here
  }
  const double T0 = now_s();
  for (int r = 0; r < runs; ++r) {
    next_iteration(su, ctx, strat);
    TraceRange trace("dlnb:iteration");
    const double j0 = meter->joules();
    double t0 = now_s();
    if (prearm) {
      replay.go(r);
      if (r + 1 < runs) {
        const double a0 = now_s();
        replay.arm(r + 1);
        tr.arm_s.push_back(now_s() - a0);
      }
      replay.wait_armed(r);
    } else {
      replay.enqueue_timed();
      replay.wait_iteration();
    }
    const double t1 = now_s();
    T.add(rkey, t1 - t0);
    if (TL) {
      TL->collect(r);
      TL->host_iteration(r, t0, t1);
    }
    if (meter->available()) T.add("energy_consumed", meter->joules() - j0);
    EnergyMeter::Sensors sn;
    if (meter->take(sn)) tr.sensors.push_back(sn);
  }
  ctx.dev->synchronize();
  ctx.hg().barrier();
  tr.timed_region_s = ctx.hg().allreduce_max(now_s() - T0);
}

// --timeline: gathers every rank's spans (rank 0 writes the trace file) and
// returns the report's `timeline` block.
Json gather_timeline(Context& ctx, const std::string& backend) {
  const Options& opt = ctx.opt;
  const RankInfo& ri = ctx.boot->info;
  Json mine = ctx.timeline->rank_json(ri.rank, opt.timeline_iters);
  mine["device"] = ctx.dev->name() + " " + std::to_string(ctx.dev->index()) + " @ " + ri.hostname;
  auto parts = ctx.hg().allgather(mine.dump());
  Json timeline_info = Json::object();
  timeline_info["path"] = opt.timeline_path;
  timeline_info["iterations_kept"] = opt.timeline_iters;
  long long nev = 0;
  bool trunc = false;
  std::vector<Json> docs;
  for (const auto& p : parts) {
    docs.push_back(Json::parse(p));
    nev += static_cast<long long>(docs.back().at("events").size());
    trunc = trunc || docs.back().at("truncated").as_bool();
  }
  timeline_info["events"] = nev;
  timeline_info["truncated"] = trunc;
  if (ri.rank == 0) {
    Json meta = Json::object();
    meta["strategy"] = strategy_name(opt.strategy);
    meta["model"] = opt.model;
    meta["backend"] = backend;
    meta["graph"] = opt.graph;
    meta["world_size"] = ri.world_size;
    write_chrome_trace(opt.timeline_path, docs, meta);
  }
  return timeline_info;
}

// setup -> replay build -> warm-up -> (loop mode | timed loop) -> report
Json run_rank_impl(const Options& opt, Context& ctx, std::unique_ptr<Strategy>& strat) {
  const RankInfo& ri = ctx.boot->info;
  RunSetup su = setup_rank(opt, ctx, strat);
  Replay replay(ctx, *strat, su.backend);
  if (opt.graph) replay.build();
  ctx.hg().barrier();

  TimedRuns tr;
  warm_up(ctx, *strat, su, replay, tr.warm);
  tr.runs = opt.min_exectime > 0 ? estimate_runs(ctx, tr.warm) : opt.runs;
  if (opt.loop) return loop_mode(ctx, *strat, su, replay);
  timed_loop(ctx, *strat, su, replay, tr);
  if (!opt.dump_outputs.empty()) dump_outputs(ctx, *strat, opt.dump_outputs);

  auto all = ctx.hg().allgather(rank_report(ctx, *strat, tr, replay).dump());
  Json timeline_info = nullptr;
  if (ctx.timeline) timeline_info = gather_timeline(ctx, su.backend);
  Json doc = global_report(ctx, *strat, su, tr, replay, all, timeline_info);

  if (ri.rank == 0 && !opt.silent) {
    std::string text = doc.dump();
    std::cout << "<<<DLNB_REPORT_BEGIN " << strat->section_id() << ">>>\n"
              << text << "\n<<<DLNB_REPORT_END " << strat->section_id() << ">>>" << std::endl;
    if (!opt.quiet) {
      const Json& it = doc.at("global").at("dlnb").at("iteration");
      std::printf("[dlnb] %s %s W=%d backend=%s compute=%s: iter median %.3f ms (floor %.3f ms), timed %.3f ms/iter\n",
                  strategy_name(opt.strategy), opt.model.c_str(), ri.world_size, su.backend.c_str(),
                  compute_mode_name(ctx.compute->mode()), it.at("median_ms").as_double(),
                  it.at("compute_floor_ms").as_double(), it.at("timed_ms_per_iter").as_double());
      std::fflush(stdout);
    }
  }
  if (ri.rank == 0 && !opt.json_path.empty()) {
    std::ofstream f(opt.json_path);
    f << doc.dump(1) << "\n";
  }
  ctx.hg().barrier();  // keep the store (rank 0) alive until everyone is done
  ctx.hg().store().finish();
  return doc;
}

}  // namespace

int main_for(StrategyKind kind, int argc, char** argv) {
  Options opt;
  try {
    opt = parse_options(kind, argc, argv);
  } catch (const std::exception& e) {
    std::cerr << e.what() << std::endl;
    return 1;
  }
  std::string prog = argc > 0 ? argv[0] : "";
  if (opt.help) {
    std::cout << usage(kind, prog);
    return 0;
  }
  if (ends_with(prog, "_loop")) opt.loop = true;
  g_cli_process.store(true);
  try {
    run_benchmark(opt);
  } catch (const std::exception& e) {
    std::cerr << "[dlnb] rank " << env_or("RANK", env_or("DLNB_RANK", "0")) << " error: " << e.what() << std::endl;
    return 2;
  }
  return 0;
}

}  // namespace dlnb
