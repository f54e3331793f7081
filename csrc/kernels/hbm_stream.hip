// HBM-streaming compute stand-in (gfx950): c[i] = bf16(float(a[i]) + float(b[i]))
// over three bf16 arrays, as a persistent grid of one 1024-thread block per CU
// that either sweeps the arrays once or keeps sweeping until a device-clock
// deadline. See dlnb/kernels.hpp (hbm_stream) and docs/KERNELS.md.
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "dlnb/common.hpp"
#include "dlnb/kernels.hpp"

#define DLNB_HIP_CHECK(expr)                                                       \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) DLNB_THROW(#expr << " failed: " << hipGetErrorString(e_)); \
  } while (0)

// Cache policy of the sweep's loads / stores: 1 = non-temporal, 0 = default.
// Measured both ways on MI355X (docs/KERNELS.md, profiles/hbm_stream.md).
#ifndef DLNB_HBM_NT_LOAD
#define DLNB_HBM_NT_LOAD 1
#endif
#ifndef DLNB_HBM_NT_STORE
#define DLNB_HBM_NT_STORE 1
#endif

namespace dlnb {
namespace kernels {

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

constexpr int kThreads = 1024;
constexpr uint32_t kChunkVecs = static_cast<uint32_t>(kHbmChunkBytes / 16);  // 16-byte vectors per chunk and array
constexpr int kVecs = static_cast<int>(kChunkVecs) / kThreads;               // per thread, chunk and array
static_assert(kVecs * kThreads == static_cast<int>(kChunkVecs), "a chunk is a whole number of vectors per thread");
// More than half a CU's 160 KiB of LDS: one block per CU, so a grid of
// CUs - comm_cus blocks leaves comm_cus CUs to the collectives (as the GEMM's
// 128-KiB tiles do). The kernel itself uses two words of it.
constexpr size_t kLdsBytes = 96 * 1024;

__device__ __forceinline__ bf16x8 ld(const bf16x8* p) {
#if DLNB_HBM_NT_LOAD
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}
__device__ __forceinline__ void st(bf16x8* p, bf16x8 v) {
#if DLNB_HBM_NT_STORE
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}

// One chunk's operands in registers: kVecs 16-byte vectors of a and of b per
// lane, lane-contiguous (vector j of thread t is t + j * kThreads), so every
// wave instruction moves 1 KiB fully coalesced and a block has 2 x 64 KiB of
// loads in flight per chunk - 4 x the ~32 KiB per CU that saturate HBM.
struct Operands {
  bf16x8 a[kVecs], b[kVecs];
};

template <bool FULL>
__device__ __forceinline__ void load_chunk(Operands& r, const bf16x8* __restrict__ a, const bf16x8* __restrict__ b,
                                           size_t chunk, size_t n8) {
  const size_t base = chunk * kChunkVecs;
  const size_t left = n8 - base;  // (chunk < chunks: > 0)
  const uint32_t nv = left < kChunkVecs ? static_cast<uint32_t>(left) : kChunkVecs;
#pragma unroll
  for (int j = 0; j < kVecs; ++j) {
    const uint32_t i = threadIdx.x + static_cast<uint32_t>(j) * kThreads;
    if (FULL || i < nv) {
      r.a[j] = ld(a + base + i);
      r.b[j] = ld(b + base + i);
    }
  }
}

template <bool FULL>
__device__ __forceinline__ void add_chunk(const Operands& r, bf16x8* __restrict__ c, size_t chunk, size_t n8) {
  const size_t base = chunk * kChunkVecs;
  const size_t left = n8 - base;
  const uint32_t nv = left < kChunkVecs ? static_cast<uint32_t>(left) : kChunkVecs;
#pragma unroll
  for (int j = 0; j < kVecs; ++j) {
    const uint32_t i = threadIdx.x + static_cast<uint32_t>(j) * kThreads;
    if (FULL || i < nv) {
      bf16x8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = static_cast<__bf16>(static_cast<float>(r.a[j][e]) + static_cast<float>(r.b[j][e]));
      st(c + base + i, v);
    }
  }
}

// Block blk takes chunks blk, blk + grid, blk + 2 grid, ...; the next chunk's
// loads are issued before the current chunk's adds and stores, so a block
// always has a chunk in flight.
//   DEADLINE: the sequence wraps round the arrays; thread 0 reads the clock
//     once per chunk and the block leaves (all threads alike: a chunk is
//     written whole or not at all) after the chunk in hand once ticks have
//     passed since the block entered the kernel. The verdict goes through
//     two alternating LDS words and one barrier per chunk, taken while the
//     chunk's loads are in flight.
//   one shot: every chunk exactly once, no clock reads, no barriers.
// On leaving, thread 0 stores the block's chunk count into per_block[blk]
// (optional) and adds it to totals[0]; block 0 also adds ticks to totals[1]
// (device memory, agent scope: a replayed graph keeps accumulating).
// FULL: n8 is a whole number of chunks - no bounds checks, so the loads of the
// next chunk stay in flight under a counted wait for the current one.
template <bool DEADLINE, bool FULL>
__device__ __forceinline__ uint64_t sweep(const bf16x8* __restrict__ a, const bf16x8* __restrict__ b,
                                          bf16x8* __restrict__ c, size_t n8, uint64_t ticks, uint64_t t0,
                                          uint32_t* expired) {
  const size_t chunks = (n8 + kChunkVecs - 1) / kChunkVecs;
  const size_t grid = gridDim.x;
  uint64_t done = 0;
  size_t chunk = blockIdx.x;
  if (DEADLINE)
    while (chunk >= chunks) chunk -= chunks;
  else if (chunk >= chunks)
    return 0;
  // one chunk: decide whether another follows, issue its loads into nxt, then
  // add and store cur. Two register sets take turns (no copy between them,
  // which would wait for the loads just issued).
  uint32_t k = 0;
  auto step = [&](const Operands& cur, Operands& nxt) {
    size_t next = chunk + grid;
    bool go;
    if (DEADLINE) {
      if (threadIdx.x == 0) expired[k & 1] = __builtin_amdgcn_s_memrealtime() - t0 >= ticks ? 1u : 0u;
      __syncthreads();
      go = expired[k & 1] == 0;
      ++k;
      while (next >= chunks) next -= chunks;
    } else {
      go = next < chunks;
    }
    if (go) load_chunk<FULL>(nxt, a, b, next, n8);
    add_chunk<FULL>(cur, c, chunk, n8);
    ++done;
    chunk = next;
    return go;
  };
  Operands r0, r1;
  load_chunk<FULL>(r0, a, b, chunk, n8);
  while (step(r0, r1) && step(r1, r0)) {
  }
  return done;
}

template <bool DEADLINE>
__global__ void __launch_bounds__(kThreads)
hbm_stream_kernel(const bf16x8* __restrict__ a, const bf16x8* __restrict__ b, bf16x8* __restrict__ c, size_t n8,
                  uint64_t ticks, uint64_t* start, uint64_t* start2, uint64_t* totals, uint64_t* per_block) {
  extern __shared__ uint32_t expired[];
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (start) __hip_atomic_store(start, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (start2) __hip_atomic_store(start2, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  const uint64_t done = n8 % kChunkVecs == 0 ? sweep<DEADLINE, true>(a, b, c, n8, ticks, t0, expired)
                                             : sweep<DEADLINE, false>(a, b, c, n8, ticks, t0, expired);
  if (threadIdx.x == 0) {
    if (per_block) per_block[blockIdx.x] = done;
    if (totals) {
      if (done) __hip_atomic_fetch_add(totals, done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (blockIdx.x == 0 && ticks)
        __hip_atomic_fetch_add(totals + 1, ticks, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// Once per device: let the kernels take kLdsBytes of dynamic LDS and check
// that this really keeps them at one block per CU.
void prepare(int dev) {
  static std::mutex mu;
  static std::vector<char> ready;
  std::lock_guard<std::mutex> g(mu);
  if (static_cast<size_t>(dev) < ready.size() && ready[static_cast<size_t>(dev)]) return;
  const void* fns[2] = {reinterpret_cast<const void*>(&hbm_stream_kernel<false>),
                        reinterpret_cast<const void*>(&hbm_stream_kernel<true>)};
  for (const void* f : fns) {
    DLNB_HIP_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLdsBytes)));
    int per_cu = 0;
    DLNB_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, kThreads, kLdsBytes));
    DLNB_REQUIRE(per_cu == 1, "hbm_stream: " << per_cu << " blocks per CU instead of 1 (the CU budget needs exactly one)");
  }
  if (ready.size() <= static_cast<size_t>(dev)) ready.resize(static_cast<size_t>(dev) + 1, 0);
  ready[static_cast<size_t>(dev)] = 1;
}

}  // namespace

void hbm_stream(const void* a, const void* b, void* c, size_t n, uint64_t ticks, int grid, void* stream,
                uint64_t* start, uint64_t* start2, uint64_t* totals, uint64_t* per_block) {
  DLNB_REQUIRE(n > 0 && n % 8 == 0, "hbm_stream: n = " << n << " is not a positive multiple of 8 elements");
  DLNB_REQUIRE(a && b && c && reinterpret_cast<uintptr_t>(a) % 16 == 0 && reinterpret_cast<uintptr_t>(b) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(c) % 16 == 0,
               "hbm_stream: the arrays must be 16-byte aligned");
  int dev = 0;
  DLNB_HIP_CHECK(hipGetDevice(&dev));
  const int cus = num_cus(dev);
  if (grid <= 0) grid = cus;
  DLNB_REQUIRE(grid <= cus, "hbm_stream: grid " << grid << " exceeds the " << cus << " CUs (one block per CU)");
  prepare(dev);
  const bf16x8* pa = static_cast<const bf16x8*>(a);
  const bf16x8* pb = static_cast<const bf16x8*>(b);
  bf16x8* pc = static_cast<bf16x8*>(c);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (ticks)
    hipLaunchKernelGGL(hbm_stream_kernel<true>, grid, kThreads, kLdsBytes, s, pa, pb, pc, n / 8, ticks, start, start2,
                       totals, per_block);
  else
    hipLaunchKernelGGL(hbm_stream_kernel<false>, grid, kThreads, kLdsBytes, s, pa, pb, pc, n / 8, ticks, start, start2,
                       totals, per_block);
  DLNB_HIP_CHECK(hipGetLastError());
}

}  // namespace kernels
}  // namespace dlnb
