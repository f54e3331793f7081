// Fused attention forward in fp8 (gfx950): O = v_scale softmax(scale Q K^T (+ causal
// mask)) V, with Q, K, V in OCP e4m3 and O in bf16; fp32 scores, softmax state
// and accumulation, head dimension 128, GQA by index mapping. The shape
// contract, the persistent one-block-per-CU grid, the one-shot and deadline
// forms and the accounting words are attention.hip's (dlnb/kernels.hpp:
// attention_fwd_fp8); the operand layouts are this file's own.
//
// Both products run on v_mfma_scale_f32_32x32x64_f8f6f4 with unit scales. A
// lane (g = lane / 32, q = lane % 32) gives the instruction 32 bytes of row q
// of A and 32 bytes of column q of B; the hardware multiplies byte j of lane
// half g in A with byte j of lane half g in B, so which contraction index a
// byte stands for is ours to choose as long as both operands agree.
//
//   S^T = K Q^T   A = K from LDS, B = Q (held in registers for the whole
//                 item, 16 VGPRs). Step ds of 2: byte j of half g is
//                 d = 64 ds + 32 g + j, two ds_read_b128 per K fragment.
//   O^T += V^T P^T   A = V^T from LDS by ds_read_b64_tr_b8, B = P, one MFMA
//                 per 64 keys and 32-d block.
//
// Key map. Row i of the 32-key block kb of S^T is loaded from K row
// 32 kb + sw23(i), sw23 = bits 2 and 3 of i swapped. The 32x32 accumulator
// gives lane (g, q) rows 8 (r / 4) + 4 g + r % 4 in registers r = 0 .. 15, so
//   register r of block kb in lane (g, q) = key 32 kb + 16 (r / 8) + 8 g + r % 8
// of query q: every 8 registers are 8 consecutive keys. Converted with
// v_cvt_pk_fp8_f32 in register order, blocks 2 j and 2 j + 1 are the 32 bytes
// of the P^T operand of key group j (64 keys):
//   byte 8 t + e of half g = key 64 j + 16 t + 8 g + e      (t < 4, e < 8)
// and V^T's operand must hold the same keys byte for byte: transpose read t of
// a lane fetches keys 64 j + 16 t + 8 g .. + 7 of its d (a 16-lane group reads
// 8 key rows x 16 d; lane 2 a + b of the group points at row a, bytes 8 b .. +
// 7, and receives column lane % 16). P never leaves registers. The causal mask
// uses the same map.
//
// P is quantized as e4m3(2^8 exp2(s c - m)): the 8 rides in the fma's addend.
// The largest P is 256 <= 448 and P flushes to zero at 2^-18 of the row
// maximum. l sums the same 2^8-scaled fp32 p before rounding, so O = acc / l
// needs no correction and lse takes the 8 off again.
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

typedef __attribute__((ext_vector_type(2))) int i32x2;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef __attribute__((address_space(3))) i32x2* lds_i32x2_t;

constexpr int kThreads = 256;           // 4 waves, one per SIMD
constexpr int kBM = 128;                // query rows per item (32 per wave)
constexpr int kBN = kAttnKvTile;        // keys per KV tile
constexpr int kD = 128;                 // head dimension
constexpr int kRowB = kD;               // bytes per Q / K / V row: half a sweep of the 64 LDS banks
constexpr int kTileB = kBN * kRowB;     // one K or V tile: 16 KiB
constexpr int kBufB = 2 * kTileB;       // a stage: K tile, V tile
constexpr int kStages = 3;              // the ring: tiles t + 1 and t + 2 are in flight under step t
constexpr int kFlagOff = kStages * kBufB;  // two deadline words behind the ring
// 96 KiB + the flags: more than half a CU's 160 KiB, so one block per CU and a
// grid of CUs - comm_cus blocks leaves comm_cus CUs to the collectives.
constexpr size_t kLdsBytes = kFlagOff + 16;
static_assert(kBN == 128 && kBM == kBN, "the causal diagonal is one KV tile per Q tile");
static_assert(kLdsBytes > 80 * 1024, "two blocks must not fit a CU");
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
constexpr float kPExp = 8.0f;           // P = 2^8 exp2(s c - m)
constexpr int kUnitScale = 0x7f7f7f7f;  // E8M0 127 = 1.0 in every byte

// LDS image of a tile: row r (128 B = 8 chunks of 16 B, so two rows share a
// sweep of the banks) keeps chunk c at slot c ^ swz(r); swz moves row bits 1, 2
// to slot bits 1, 2 and row bit 3 to slot bit 0.
//  * K fragments (ds_read_b128: 16 lanes that are served together read the same
//    chunk of 16 rows, distinct mod 16): row bit 0 picks the half of the sweep
//    and swz is a bijection of row bits 1 .. 3, so 16 distinct 16-byte slots;
//  * V^T fragments (ds_read_b64_tr_b8: 32 lanes read 8 consecutive rows x 2
//    consecutive chunks): row bit 0 picks the half, row bits 1, 2 the slot's
//    bits 1, 2 and the chunk pair its bit 0 (row bit 3 is common to the 8).
__device__ __forceinline__ int swz(int row) { return (row & 6) | ((row >> 3) & 1); }
__device__ __forceinline__ int sw23(int i) { return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1); }

// Stage one 128-row tile: 16 wave instructions of buffer_load_dwordx4 ... lds
// (8 rows each), 4 per wave; instruction i * 4 + w writes rows 32 i + 8 w ..
// + 7 lane-linearly, so the swizzle is applied to the source offset. Rows 16
// apart share their swizzle: voff (stage_offset) is loop-invariant and the row
// group a scalar offset.
__device__ __forceinline__ void stage_tile(const char* tile, int voff, char* lds, int w) {
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(tile), 0, 0x7ffffff0, 0x00020000);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(lds + (i * 4 + w) * 1024), 16, voff, i * 32 * kRowB, 0, 0);
}
__device__ __forceinline__ int stage_offset(int w, int lane) {
  const int row = 8 * w + (lane >> 3);  // (and + 32 i)
  return row * kRowB + (((lane & 7) ^ swz(row)) << 4);
}
// K and V tile t of the item into one stage of the ring.
__device__ __forceinline__ void stage_kv(const char* Kb, const char* Vb, int t, int voff, char* stage, int w) {
  stage_tile(Kb + static_cast<size_t>(t) * kTileB, voff, stage, w);
  stage_tile(Vb + static_cast<size_t>(t) * kTileB, voff, stage + kTileB, w);
}

struct Lane {
  int w, lane, g, q;  // wave, lane, lane half (lane / 32), query column (lane % 32)
  int k_off;          // K fragment: byte offset of the lane's row (sw23(q)), and its swizzle
  int k_swz;
  int v_off;          // V^T fragment: row offset (8 g + a) + byte within the chunk
  int v_chunk;        // ... its chunk within a 32-d block
  int v_swz;
};

__device__ __forceinline__ f32x16 mfma_fp8(const i32x8& a, const i32x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, kUnitScale, 0, kUnitScale);
}

// One KV tile: S^T = K Q^T, online softmax, O^T += V^T P^T.
//   s (the scores) and p never leave registers; m / l are this lane's query's
//   running max (in log2 units: raw score x c) and this lane's half of its
//   running sum of 2^8 p.
template <bool DIAG>
__device__ __forceinline__ void tile_step(const char* kbuf, const char* vbuf, const Lane& L, const i32x8 (&qf)[2],
                                          f32x16 (&acc)[4], float& m, float& l, float c) {
  f32x16 s[4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) s[kb][r] = 0.0f;
#pragma unroll
  for (int ds = 0; ds < 2; ++ds)
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const char* row = kbuf + kb * 32 * kRowB + L.k_off;
      const i32x4 lo = *reinterpret_cast<const i32x4*>(row + (((4 * ds + 2 * L.g) ^ L.k_swz) << 4));
      const i32x4 hi = *reinterpret_cast<const i32x4*>(row + (((4 * ds + 2 * L.g + 1) ^ L.k_swz) << 4));
      const i32x8 kf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      s[kb] = mfma_fp8(kf, qf[ds], s[kb]);
    }
  // lane (g, q), register r of block kb: key kb * 32 + 16 (r / 8) + 8 g + r % 8 of query q
  if (DIAG) {
    const int qrow = L.w * 32 + L.q;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (kb * 32 + 16 * (r / 8) + 8 * L.g + (r % 8) > qrow) s[kb][r] = -INFINITY;
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
  // p = 2^8 exp2(s c - m): one fma and a bare v_exp_f32 per score, then four
  // to a register in register order: blocks 2 j, 2 j + 1 are key group j's operand
  const float off = kPExp - mn;
  i32x8 pf[2];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float p[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        p[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][4 * j + e], c, off));
        l += p[e];
      }
      int pk = __builtin_amdgcn_cvt_pk_fp8_f32(p[0], p[1], 0, false);
      pk = __builtin_amdgcn_cvt_pk_fp8_f32(p[2], p[3], pk, true);
      pf[kb / 2][4 * (kb % 2) + j] = pk;
    }
  // byte 8 t + e of the lane's operand is key 64 kg + 16 t + 8 g + e: V^T is
  // read in that order, 8 consecutive keys per transpose read
#pragma unroll
  for (int kg = 0; kg < 2; ++kg)
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      i32x2 h[4];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        h[t] = __builtin_amdgcn_ds_read_tr8_b64_v2i32(
            (lds_i32x2_t)(vbuf + (kg * 64 + t * 16) * kRowB + L.v_off + (((db * 2 + L.v_chunk) ^ L.v_swz) << 4)));
      const i32x4 a = __builtin_shufflevector(h[0], h[1], 0, 1, 2, 3);
      const i32x4 b = __builtin_shufflevector(h[2], h[3], 0, 1, 2, 3);
      const i32x8 vf = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
      acc[db] = mfma_fp8(vf, pf[kg], acc[db]);
    }
}

// Block blk takes items blk, blk + grid, ...; item i is Q tile nq - 1 - i / (B H)
// (the causal mode's longest items first) of head i % (B H).
//   DEADLINE: the sequence wraps round; thread 0 reads the clock once per item
//     and the block leaves as a whole after the item in hand once ticks have
//     passed since it entered (two alternating LDS words; the verdict rides on
//     the item's first tile barrier). An item is written whole or not at all.
//   one shot: every item exactly once.
// Per KV tile t: wait for the tile's loads (tile t + 1's may stay in flight),
// one barrier (the tile is complete and every wave is done with stage
// (t - 1) % 3), issue tile t + 2's loads into that stage - never a tile past
// the item's last - and compute. On leaving, thread 0 stores the block's
// KV-tile steps into per_block[blk] and adds them to totals[0]; block 0 adds
// ticks to totals[1] (device memory, agent scope: graph replays accumulate).
template <bool DEADLINE>
__global__ void __launch_bounds__(kThreads)
attention_fwd_fp8_kernel(const char* __restrict__ Q, const char* __restrict__ K, const char* __restrict__ V,
                         __bf16* __restrict__ O, float* __restrict__ lse, int B, int H, int Hkv, int Sq, int Skv, float c,
                         float v_scale, int causal, uint64_t ticks, uint64_t* start, uint64_t* start2, uint64_t* totals,
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
  L.k_off = sw23(L.q) * kRowB;
  L.k_swz = swz(sw23(L.q));
  {
    const int row = 8 * L.g + ((L.lane & 15) >> 1);  // (and + 64 kg + 16 t)
    L.v_off = row * kRowB + 8 * (L.lane & 1);
    L.v_swz = swz(row);
  }
  L.v_chunk = (L.lane >> 4) & 1;
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
    const char* Kb = K + kvrow0 * kRowB;
    const char* Vb = V + kvrow0 * kRowB;
    bool go = true;
    if (DEADLINE && threadIdx.x == 0) expired[n & 1] = __builtin_amdgcn_s_memrealtime() - t0 >= ticks ? 1u : 0u;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the previous item's stores: the tile waits count loads only
    __syncthreads();  // every wave is done with the previous item's stages
    // byte j of the lane's step-ds operand is d = 64 ds + 32 g + j
    i32x8 qf[2];
#pragma unroll
    for (int ds = 0; ds < 2; ++ds) {
      const i32x4* src = reinterpret_cast<const i32x4*>(Q + qrow0 * kRowB + ds * 64 + 32 * L.g);
      qf[ds] = __builtin_shufflevector(src[0], src[1], 0, 1, 2, 3, 4, 5, 6, 7);
    }
    stage_kv(Kb, Vb, 0, voff, smem, L.w);
    if (nt > 1) stage_kv(Kb, Vb, 1, voff, smem + kBufB, L.w);
    f32x16 acc[4];
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[db][r] = 0.0f;
    float m = -INFINITY, l = 0.0f;
    int st = 0;  // t % kStages
    for (int t = 0; t < nt; ++t) {
      char* cur = smem + st * kBufB;
      // this thread's part of tile t has landed; tile t + 1's 8 loads may still be out
      if (t + 1 < nt)
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (DEADLINE && t == 0) go = expired[n & 1] == 0;
      if (t + 2 < nt) stage_kv(Kb, Vb, t + 2, voff, smem + (st == 0 ? kStages - 1 : st - 1) * kBufB, L.w);
      if (causal && t == nt - 1)
        tile_step<true>(cur, cur + kTileB, L, qf, acc, m, l, c);
      else
        tile_step<false>(cur, cur + kTileB, L, qf, acc, m, l, c);
      st = st == kStages - 1 ? 0 : st + 1;
    }
    done += static_cast<uint64_t>(nt);
    // the query's sum is the two lane halves'; O^T register r of block db is
    // d = 32 db + 8 (r / 4) + 4 g + r % 4: four consecutive d per store
    l += __shfl_xor(l, 32);
    const float inv = v_scale / l;  // (acc and l carry the same 2^8)
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
    if (lse && L.g == 0) lse[qrow0] = (m + log2f(l) - kPExp) * kLn2;
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
  const void* fns[2] = {reinterpret_cast<const void*>(&attention_fwd_fp8_kernel<false>),
                        reinterpret_cast<const void*>(&attention_fwd_fp8_kernel<true>)};
  for (const void* f : fns) {
    DLNB_HIP_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kLdsBytes)));
    int per_cu = 0;
    DLNB_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, kThreads, kLdsBytes));
    DLNB_REQUIRE(per_cu == 1, "attention_fwd_fp8: " << per_cu << " blocks per CU instead of 1 (the CU budget needs exactly one)");
  }
  if (ready.size() <= static_cast<size_t>(dev)) ready.resize(static_cast<size_t>(dev) + 1, 0);
  ready[static_cast<size_t>(dev)] = 1;
}

}  // namespace

void attention_fwd_fp8(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int Hkv, int Sq,
                       int Skv, float scale, float v_scale, bool causal, uint64_t ticks, int grid, void* stream,
                       uint64_t* start, uint64_t* start2, uint64_t* totals, uint64_t* per_block) {
  DLNB_REQUIRE(B > 0 && H > 0 && Hkv > 0, "attention_fwd_fp8: B = " << B << ", H = " << H << ", Hkv = " << Hkv << " must be positive");
  DLNB_REQUIRE(H % Hkv == 0, "attention_fwd_fp8: H = " << H << " is not a multiple of Hkv = " << Hkv);
  DLNB_REQUIRE(Sq > 0 && Sq % kBM == 0, "attention_fwd_fp8: Sq = " << Sq << " is not a positive multiple of " << kBM);
  DLNB_REQUIRE(Skv > 0 && Skv % kBN == 0, "attention_fwd_fp8: Skv = " << Skv << " is not a positive multiple of " << kBN);
  DLNB_REQUIRE(!causal || Sq == Skv, "attention_fwd_fp8: causal needs Sq == Skv (Sq = " << Sq << ", Skv = " << Skv << ")");
  DLNB_REQUIRE(std::isfinite(scale) && scale > 0.0f, "attention_fwd_fp8: scale = " << scale << " must be positive and finite");
  DLNB_REQUIRE(std::isfinite(v_scale) && v_scale > 0.0f, "attention_fwd_fp8: v_scale = " << v_scale << " must be positive and finite");
  DLNB_REQUIRE(static_cast<double>(B) * H * (Sq / kBM) < 2147483648.0, "attention_fwd_fp8: too many Q tiles (B H Sq / 128 >= 2^31)");
  for (const void* p : {q, k, v, static_cast<const void*>(o)})
    DLNB_REQUIRE(p && reinterpret_cast<uintptr_t>(p) % 16 == 0, "attention_fwd_fp8: q, k, v and o must be 16-byte aligned");
  DLNB_REQUIRE(reinterpret_cast<uintptr_t>(lse) % 4 == 0, "attention_fwd_fp8: lse must be 4-byte aligned");
  int dev = 0;
  DLNB_HIP_CHECK(hipGetDevice(&dev));
  const int cus = num_cus(dev);
  if (grid <= 0) grid = cus;
  DLNB_REQUIRE(grid <= cus, "attention_fwd_fp8: grid " << grid << " exceeds the " << cus << " CUs (one block per CU)");
  prepare(dev);
  const float c = scale * kLog2e;
  const char* pq = static_cast<const char*>(q);
  const char* pk = static_cast<const char*>(k);
  const char* pv = static_cast<const char*>(v);
  __bf16* po = static_cast<__bf16*>(o);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int cz = causal ? 1 : 0;
  if (ticks)
    hipLaunchKernelGGL(attention_fwd_fp8_kernel<true>, grid, kThreads, kLdsBytes, s, pq, pk, pv, po, lse, B, H, Hkv, Sq,
                       Skv, c, v_scale, cz, ticks, start, start2, totals, per_block);
  else
    hipLaunchKernelGGL(attention_fwd_fp8_kernel<false>, grid, kThreads, kLdsBytes, s, pq, pk, pv, po, lse, B, H, Hkv, Sq,
                       Skv, c, v_scale, cz, ticks, start, start2, totals, per_block);
  DLNB_HIP_CHECK(hipGetLastError());
}

}  // namespace kernels
}  // namespace dlnb
