// Fused attention forward (gfx950): O = softmax(scale Q K^T (+ causal mask)) V,
// bf16 in and out, fp32 scores, softmax and accumulation, head dimension 128,
// GQA by index mapping. A persistent grid of one 256-thread block per CU walks
// (b, h, 128-row Q tile) items once or until a device-clock deadline. See
// dlnb/kernels.hpp (attention_fwd) and docs/KERNELS.md for the design.
//
// One wave owns 32 query rows of the item. Per 128-key KV tile it computes
//   S^T = K Q^T      (v_mfma_f32_32x32x16_bf16: A = K from LDS, B = Q, held in
//                     registers for the whole item)
// whose accumulator layout puts one query in every lane (lane % 32) and 16 of
// each 32 keys in its registers - exactly the B-operand layout of
//   O^T += V^T P^T   (A = V^T from LDS by ds_read_b64_tr_b16, B = P)
// once V's keys are read in the same permuted order. So P goes from the first
// product's accumulators through v_exp_f32 and a bf16 pack straight into the
// second product's operand registers, and the softmax state (row max, row sum,
// the accumulator rescale) is one scalar per lane.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "dlnb/common.hpp"
#include "dlnb/kernels.hpp"

#define DLNB_HIP_CHECK(expr)                                                       \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) DLNB_THROW(#expr << " failed: " << hipGetErrorString(e_)); \
  } while (0)

namespace dlnb {
namespace kernels {

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef __attribute__((address_space(3))) bf16x4* lds_bf16x4_t;

constexpr int kThreads = 256;           // 4 waves, one per SIMD
constexpr int kBM = 128;                // query rows per item (32 per wave)
constexpr int kBN = kAttnKvTile;        // keys per KV tile
constexpr int kD = 128;                 // head dimension
constexpr int kRowB = kD * 2;           // bytes per K / V row: one sweep of the 64 LDS banks
constexpr int kTileB = kBN * kRowB;     // one K or V tile: 32 KiB
constexpr int kBufB = 2 * kTileB;       // a buffer: K tile, V tile
constexpr int kFlagOff = 2 * kBufB;     // two deadline words behind the two buffers
// 128 KiB + the flags: more than half a CU's 160 KiB, so one block per CU and a
// grid of CUs - comm_cus blocks leaves comm_cus CUs to the collectives.
constexpr size_t kLdsBytes = kFlagOff + 16;
static_assert(kBN == 128 && kBM == kBN, "the causal diagonal is one KV tile per Q tile");
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// LDS image of a tile: row r (256 B = 16 chunks of 16 B) keeps chunk c at slot
// c ^ swz(r), swz = the two 2-bit fields of r & 15 swapped.
//  * K fragments (ds_read_b128: 16 lanes that are served together read the same
//    chunk of 16 rows, distinct mod 16) land on 16 distinct slots, since swz
//    is a bijection of r & 15;
//  * V^T fragments (ds_read_b64_tr_b16: 32 lanes read 4 consecutive rows x 4
//    consecutive chunks) land on 16 distinct slots, since rows 4m .. 4m + 3
//    differ in the slot's upper field (r & 3) and the 4 chunks in its lower.
__device__ __forceinline__ int swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

// Stage one 128-row tile: 32 wave instructions of buffer_load_dwordx4 ... lds
// (4 rows each), 8 per wave; instruction i * 4 + w writes rows 16 i + 4 w ..
// + 3 lane-linearly, so the swizzle is applied to the source offset. Rows 16
// apart share their swizzle: voff (stage_offset) is loop-invariant and the row
// group a scalar offset.
__device__ __forceinline__ void stage_tile(const char* tile, int voff, char* lds, int w) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(tile), 0, 0x7ffffff0, 0x00020000);
#pragma unroll
  for (int i = 0; i < 8; ++i)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(lds + (i * 4 + w) * 1024), 16, voff, i * 16 * kRowB, 0, 0);
}
__device__ __forceinline__ int stage_offset(int w, int lane) {
  const int row = 4 * w + (lane >> 4);  // (and + 16 i)
  return row * kRowB + (((lane & 15) ^ swz(row)) << 4);
}

struct Lane {
  int w, lane, g, q;  // wave, lane, lane half (lane / 32), query column (lane % 32)
  int k_off;          // K fragment: byte offset of the lane's row, and its swizzle
  int k_swz;
  int v_off[2];       // V^T fragment halves: row offset + byte within the chunk
  int v_chunk;        // ... its chunk within a 32-d block
  int v_swz[2];
};

// One KV tile: S^T = K Q^T, online softmax, O^T += V^T P^T.
//   s (the scores) and p never leave registers; m / l are this lane's query's
//   running max (in log2 units: raw score x c) and this lane's half of its
//   running sum.
template <bool DIAG>
__device__ __forceinline__ void tile_step(const char* kbuf, const char* vbuf, const Lane& L, const bf16x8 (&qf)[8],
                                          f32x16 (&acc)[4], float& m, float& l, float c) {
  f32x16 s[4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) s[kb][r] = 0.0f;
#pragma unroll
  for (int ds = 0; ds < 8; ++ds)
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const bf16x8 kf = *reinterpret_cast<const bf16x8*>(kbuf + kb * 32 * kRowB + L.k_off + (((2 * ds + L.g) ^ L.k_swz) << 4));
      s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ds], s[kb], 0, 0, 0);
    }
  // lane (g, q), register r of block kb: key kb * 32 + 8 (r / 4) + 4 g + r % 4 of query q
  if (DIAG) {
    const int qrow = L.w * 32 + L.q;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (kb * 32 + 8 * (r / 4) + 4 * L.g + (r % 4) > qrow) s[kb][r] = -INFINITY;
  }
  float mx = s[0][0];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kb][r]);
  mx = fmaxf(mx, __shfl_xor(mx, 32));  // the query's other 64 keys
  // (the diagonal tile's row always sees its own key, so mx is finite)
  const float mn = fmaxf(m, mx * c);
  const float alpha = __builtin_amdgcn_exp2f(m - mn);  // first tile: exp2(-inf) = 0
  m = mn;
  l *= alpha;
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[db][r] *= alpha;
  // p = exp2(s c - m): one fma and a bare v_exp_f32 per score; registers
  // 8 j .. 8 j + 7 of block kb are the lane's 8 keys of the 16-key slab 2 kb + j
  bf16x8 pf[8];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][r], c, -mn));
      l += p;
      pf[2 * kb + r / 8][r % 8] = static_cast<__bf16>(p);
    }
  // element e of the lane's slab operand is key 8 (e / 4) + 4 g + e % 4: V^T is
  // read in that order, 4 consecutive keys per transpose read
#pragma unroll
  for (int sl = 0; sl < 8; ++sl)
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      bf16x4 h[2];
#pragma unroll
      for (int e = 0; e < 2; ++e)
        h[e] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
            (lds_bf16x4_t)(vbuf + sl * 16 * kRowB + L.v_off[e] + (((db * 4 + L.v_chunk) ^ L.v_swz[e]) << 4)));
      const bf16x8 vf = __builtin_shufflevector(h[0], h[1], 0, 1, 2, 3, 4, 5, 6, 7);
      acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[sl], acc[db], 0, 0, 0);
    }
}

// Block blk takes items blk, blk + grid, ...; item i is Q tile nq - 1 - i / (B H)
// (the causal mode's longest items first) of head i % (B H).
//   DEADLINE: the sequence wraps round; thread 0 reads the clock once per item
//     and the block leaves as a whole after the item in hand once ticks have
//     passed since it entered (two alternating LDS words; the verdict rides on
//     the item's first tile barrier). An item is written whole or not at all.
//   one shot: every item exactly once.
// Per KV tile: wait for the tile's loads, one barrier (the tile is complete
// and every wave is done with the other buffer), issue the next tile's loads
// into the other buffer, compute. On leaving, thread 0 stores the block's
// KV-tile steps into per_block[blk] and adds them to totals[0]; block 0 adds
// ticks to totals[1] (device memory, agent scope: graph replays accumulate).
template <bool DEADLINE>
__global__ void __launch_bounds__(kThreads)
attention_fwd_kernel(const __bf16* __restrict__ Q, const __bf16* __restrict__ K, const __bf16* __restrict__ V,
                     __bf16* __restrict__ O, float* __restrict__ lse, int B, int H, int Hkv, int Sq, int Skv, float c,
                     int causal, uint64_t ticks, uint64_t* start, uint64_t* start2, uint64_t* totals,
                     uint64_t* per_block) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef __attribute__((address_space(3))) volatile uint32_t lds_flag_t;
  lds_flag_t* expired = (lds_flag_t*)(smem + kFlagOff);
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (start) __hip_atomic_store(start, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (start2) __hip_atomic_store(start2, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  Lane L;
  L.w = threadIdx.x >> 6;
  L.lane = threadIdx.x & 63;
  L.g = L.lane >> 5;
  L.q = L.lane & 31;
  L.k_off = L.q * kRowB;
  L.k_swz = swz(L.q);
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int row = 8 * e + 4 * L.g + ((L.lane & 15) >> 2);  // (and + 16 slab)
    L.v_off[e] = row * kRowB + 8 * (L.lane & 1);
    L.v_swz[e] = swz(row);
  }
  L.v_chunk = 2 * ((L.lane >> 4) & 1) + ((L.lane & 3) >> 1);
  const int voff = stage_offset(L.w, L.lane);

  const int nq = Sq / kBM, BH = B * H, items = nq * BH, rep = H / Hkv;
  const int nkv = Skv / kBN;
  uint64_t done = 0;
  uint32_t n = 0;
  int item = blockIdx.x;
  if (DEADLINE)
    item %= items;
  else if (item >= items)
    item = -1;
  while (item >= 0) {
    const int qt = nq - 1 - item / BH, bh = item % BH;
    const int b = bh / H, h = bh % H;
    const int nt = causal ? qt + 1 : nkv;
    const size_t qrow0 = (static_cast<size_t>(bh) * Sq + static_cast<size_t>(qt) * kBM + L.w * 32 + L.q);
    const size_t kvrow0 = (static_cast<size_t>(b) * Hkv + h / rep) * Skv;
    const char* Kb = reinterpret_cast<const char*>(K) + kvrow0 * kRowB;
    const char* Vb = reinterpret_cast<const char*>(V) + kvrow0 * kRowB;
    bool go = true;
    if (DEADLINE && threadIdx.x == 0) expired[n & 1] = __builtin_amdgcn_s_memrealtime() - t0 >= ticks ? 1u : 0u;
    __syncthreads();  // every wave is done with the previous item's buffers
    stage_tile(Kb, voff, smem, L.w);
    stage_tile(Vb, voff, smem + kTileB, L.w);
    bf16x8 qf[8];
#pragma unroll
    for (int ds = 0; ds < 8; ++ds) qf[ds] = *reinterpret_cast<const bf16x8*>(Q + qrow0 * kD + ds * 16 + 8 * L.g);
    f32x16 acc[4];
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[db][r] = 0.0f;
    float m = -INFINITY, l = 0.0f;
    for (int t = 0; t < nt; ++t) {
      char* cur = smem + (t & 1) * kBufB;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's part of tile t has landed
      __syncthreads();
      if (DEADLINE && t == 0) go = expired[n & 1] == 0;
      if (t + 1 < nt) {
        char* nxt = smem + ((t + 1) & 1) * kBufB;
        stage_tile(Kb + static_cast<size_t>(t + 1) * kTileB, voff, nxt, L.w);
        stage_tile(Vb + static_cast<size_t>(t + 1) * kTileB, voff, nxt + kTileB, L.w);
      }
      if (causal && t == nt - 1)
        tile_step<true>(cur, cur + kTileB, L, qf, acc, m, l, c);
      else
        tile_step<false>(cur, cur + kTileB, L, qf, acc, m, l, c);
    }
    done += static_cast<uint64_t>(nt);
    // the query's sum is the two lane halves'; O^T register r of block db is
    // d = 32 db + 8 (r / 4) + 4 g + r % 4: four consecutive d per store
    l += __shfl_xor(l, 32);
    const float inv = 1.0f / l;
    __bf16* orow = O + qrow0 * kD + 4 * L.g;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bf16x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = static_cast<__bf16>(acc[db][4 * j + e] * inv);
        *reinterpret_cast<bf16x4*>(orow + db * 32 + j * 8) = v;
      }
    if (lse && L.g == 0) lse[qrow0] = (m + log2f(l)) * kLn2;
    ++n;
    item += gridDim.x;
    if (DEADLINE) {
      if (!go) break;
      item %= items;
    } else if (item >= items) {
      break;
    }
  }
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
  const void* fns[2] = {reinterpret_cast<const void*>(&attention_fwd_kernel<false>),
                        reinterpret_cast<const void*>(&attention_fwd_kernel<true>)};
  for (const void* f : fns) {
    DLNB_HIP_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLdsBytes)));
    int per_cu = 0;
    DLNB_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, kThreads, kLdsBytes));
    DLNB_REQUIRE(per_cu == 1, "attention_fwd: " << per_cu << " blocks per CU instead of 1 (the CU budget needs exactly one)");
  }
  if (ready.size() <= static_cast<size_t>(dev)) ready.resize(static_cast<size_t>(dev) + 1, 0);
  ready[static_cast<size_t>(dev)] = 1;
}

}  // namespace

void attention_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int Hkv, int Sq,
                   int Skv, float scale, bool causal, uint64_t ticks, int grid, void* stream, uint64_t* start,
                   uint64_t* start2, uint64_t* totals, uint64_t* per_block) {
  DLNB_REQUIRE(B > 0 && H > 0 && Hkv > 0, "attention_fwd: B = " << B << ", H = " << H << ", Hkv = " << Hkv << " must be positive");
  DLNB_REQUIRE(H % Hkv == 0, "attention_fwd: H = " << H << " is not a multiple of Hkv = " << Hkv);
  DLNB_REQUIRE(Sq > 0 && Sq % kBM == 0, "attention_fwd: Sq = " << Sq << " is not a positive multiple of " << kBM);
  DLNB_REQUIRE(Skv > 0 && Skv % kBN == 0, "attention_fwd: Skv = " << Skv << " is not a positive multiple of " << kBN);
  DLNB_REQUIRE(!causal || Sq == Skv, "attention_fwd: causal needs Sq == Skv (Sq = " << Sq << ", Skv = " << Skv << ")");
  DLNB_REQUIRE(std::isfinite(scale) && scale > 0.0f, "attention_fwd: scale = " << scale << " must be positive and finite");
  DLNB_REQUIRE(static_cast<double>(B) * H * (Sq / kBM) < 2147483648.0, "attention_fwd: too many Q tiles (B H Sq / 128 >= 2^31)");
  for (const void* p : {q, k, v, static_cast<const void*>(o)})
    DLNB_REQUIRE(p && reinterpret_cast<uintptr_t>(p) % 16 == 0, "attention_fwd: q, k, v and o must be 16-byte aligned");
  DLNB_REQUIRE(reinterpret_cast<uintptr_t>(lse) % 4 == 0, "attention_fwd: lse must be 4-byte aligned");
  int dev = 0;
  DLNB_HIP_CHECK(hipGetDevice(&dev));
  const int cus = num_cus(dev);
  if (grid <= 0) grid = cus;
  DLNB_REQUIRE(grid <= cus, "attention_fwd: grid " << grid << " exceeds the " << cus << " CUs (one block per CU)");
  prepare(dev);
  const float c = scale * kLog2e;
  const __bf16* pq = static_cast<const __bf16*>(q);
  const __bf16* pk = static_cast<const __bf16*>(k);
  const __bf16* pv = static_cast<const __bf16*>(v);
  __bf16* po = static_cast<__bf16*>(o);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int cz = causal ? 1 : 0;
  if (ticks)
    hipLaunchKernelGGL(attention_fwd_kernel<true>, grid, kThreads, kLdsBytes, s, pq, pk, pv, po, lse, B, H, Hkv, Sq, Skv,
                       c, cz, ticks, start, start2, totals, per_block);
  else
    hipLaunchKernelGGL(attention_fwd_kernel<false>, grid, kThreads, kLdsBytes, s, pq, pk, pv, po, lse, B, H, Hkv, Sq, Skv,
                       c, cz, ticks, start, start2, totals, per_block);
  DLNB_HIP_CHECK(hipGetLastError());
}

}  // namespace kernels
}  // namespace dlnb
