// MXFP8 wire quantization of bf16 messages (gfx950): quantize, dequantize,
// dequantize-and-reduce. Streaming, HBM-bound kernels without LDS that run on
// the communication lane beside the collectives. Format and contract:
// dlnb/wire_quant.hpp; layout of the work and measurements: docs/KERNELS.md.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dlnb/common.hpp"
#include "dlnb/kernels.hpp"
#include "dlnb/wire_quant.hpp"

#define DLNB_HIP_CHECK(expr)                                                       \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) DLNB_THROW(#expr << " failed: " << hipGetErrorString(e_)); \
  } while (0)

// Lanes that share one 32-element block in mx_quantize / mx_dequantize:
//   4: a lane holds 8 elements (one 16-byte bf16 vector, 8 payload bytes), the
//      block's amax is taken across the quad with two DPP quad_perm moves;
//      every wave access is contiguous;
//   1: a lane holds the whole block (four 16-byte bf16 vectors 64 bytes apart
//      from its neighbour's, two 16-byte payload vectors), no cross-lane step.
// Measured both ways on MI355X (docs/KERNELS.md, profiles/wire_quant.md).
#ifndef DLNB_MXQ_LANES
#define DLNB_MXQ_LANES 4
#endif

namespace dlnb {
namespace kernels {

namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

constexpr int kThreads = 256;
// Blocks per CU a launch asks for at most: 8 x 256 threads fill a CU's wave
// slots when the registers allow; more only lengthens the tail.
constexpr int kBlocksPerCu = 8;

__device__ __forceinline__ float bits_f(uint32_t u) { return __uint_as_float(u); }

// max over the two bf16 magnitudes (sign cleared, as integers) packed in w
__device__ __forceinline__ uint32_t amax_bits2(uint32_t w) {
  const uint32_t a = w & 0x7fff7fffu;
  return max(a & 0xffffu, a >> 16);
}

// The scale byte of a block whose largest magnitude has the bf16 bits m.
__device__ __forceinline__ uint32_t scale_byte(uint32_t m) {
  if (m >= 0x7f80u) return 0xffu;  // Inf / NaN in the block
  const uint32_t E = m >> 7;       // biased exponent of amax
  return E > 8u ? E - 8u : 0u;
}
// 2^-e for a scale byte sb = e + 127 of a finite block (sb <= 246)
__device__ __forceinline__ float quant_mult(uint32_t sb) { return bits_f((254u - (sb == 0xffu ? 0u : sb)) << 23); }
// 2^e; NaN for 0xFF, 0 for 0 (dlnb/wire_quant.hpp)
__device__ __forceinline__ float dequant_mult(uint32_t sb) { return bits_f(sb == 0xffu ? 0x7fc00000u : sb << 23); }

// Four e4m3 bytes from two packed bf16 pairs, scaled and clamped to +-448
// (the convert alone need not saturate).
__device__ __forceinline__ uint32_t quant4(uint32_t w0, uint32_t w1, float mult) {
  const float a = __builtin_amdgcn_fmed3f(bits_f(w0 << 16) * mult, -448.0f, 448.0f);
  const float b = __builtin_amdgcn_fmed3f(bits_f(w0 & 0xffff0000u) * mult, -448.0f, 448.0f);
  const float c = __builtin_amdgcn_fmed3f(bits_f(w1 << 16) * mult, -448.0f, 448.0f);
  const float d = __builtin_amdgcn_fmed3f(bits_f(w1 & 0xffff0000u) * mult, -448.0f, 448.0f);
  int r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  r = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, r, true);
  return static_cast<uint32_t>(r);
}

__device__ __forceinline__ uint32_t bf16_bits(float f) {
  const __bf16 h = static_cast<__bf16>(f);  // RNE, NaN preserving
  return static_cast<uint32_t>(__builtin_bit_cast(uint16_t, h));
}
__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) { return bf16_bits(lo) | bf16_bits(hi) << 16; }

// The four products of one payload word.
__device__ __forceinline__ void dequant4(uint32_t q, float mult, float* f) {
  f[0] = __builtin_amdgcn_cvt_f32_fp8(q, 0) * mult;
  f[1] = __builtin_amdgcn_cvt_f32_fp8(q, 1) * mult;
  f[2] = __builtin_amdgcn_cvt_f32_fp8(q, 2) * mult;
  f[3] = __builtin_amdgcn_cvt_f32_fp8(q, 3) * mult;
}

// Elements of message block j that exist: below block_elems and below n_total.
__device__ __forceinline__ size_t block_limit(size_t j, size_t block_elems, size_t n_total) {
  const size_t start = j * block_elems;
  if (start >= n_total) return 0;
  return min(block_elems, n_total - start);
}

// Eight bf16 elements k .. k+7 of a message block as four packed words: one
// 16-byte load when all eight exist (VEC), element loads and zeros otherwise.
template <bool VEC>
__device__ __forceinline__ void load8(const uint16_t* __restrict__ blk, size_t k, size_t lim, uint32_t* w) {
  if (VEC && k + 8 <= lim) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(blk + k);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t lo = k + 2 * i < lim ? blk[k + 2 * i] : 0u;
    const uint32_t hi = k + 2 * i + 1 < lim ? blk[k + 2 * i + 1] : 0u;
    w[i] = lo | hi << 16;
  }
}

template <bool VEC>
__device__ __forceinline__ void store8(uint16_t* __restrict__ blk, size_t k, size_t lim, const uint32_t* w) {
  if (VEC && k + 8 <= lim) {
    u32x4 v;
    v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
    *reinterpret_cast<u32x4*>(blk + k) = v;
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (k + 2 * i < lim) blk[k + 2 * i] = static_cast<uint16_t>(w[i] & 0xffffu);
    if (k + 2 * i + 1 < lim) blk[k + 2 * i + 1] = static_cast<uint16_t>(w[i] >> 16);
  }
}

// NB payload bytes at p from / into NB / 4 words: 16- or 8-byte accesses
// (VEC; p is then aligned to NB or 16), bytes otherwise.
template <bool VEC, int NB>
__device__ __forceinline__ void store_payload(uint8_t* __restrict__ p, const uint32_t* q) {
  if (VEC) {
    if (NB == 8) {
      u32x2 v;
      v.x = q[0], v.y = q[1];
      *reinterpret_cast<u32x2*>(p) = v;
    } else {
#pragma unroll
      for (int i = 0; i < NB / 16; ++i) {
        u32x4 v;
        v.x = q[4 * i], v.y = q[4 * i + 1], v.z = q[4 * i + 2], v.w = q[4 * i + 3];
        *reinterpret_cast<u32x4*>(p + 16 * i) = v;
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < NB; ++i) p[i] = static_cast<uint8_t>(q[i / 4] >> (8 * (i % 4)));
}

template <bool VEC, int NB>
__device__ __forceinline__ void load_payload(const uint8_t* __restrict__ p, uint32_t* q) {
  if (VEC) {
    if (NB == 8) {
      const u32x2 v = *reinterpret_cast<const u32x2*>(p);
      q[0] = v.x, q[1] = v.y;
    } else {
#pragma unroll
      for (int i = 0; i < NB / 16; ++i) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(p + 16 * i);
        q[4 * i] = v.x, q[4 * i + 1] = v.y, q[4 * i + 2] = v.z, q[4 * i + 3] = v.w;
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < NB / 4; ++i) q[i] = 0;
#pragma unroll
  for (int i = 0; i < NB; ++i) q[i / 4] |= static_cast<uint32_t>(p[i]) << (8 * (i % 4));
}

// Largest value of m over the LANES lanes that share a block (a quad, or the
// lane itself). Every lane of a quad is active: the item count of a message
// block is a multiple of LANES and the thread stride a multiple of 4.
template <int LANES>
__device__ __forceinline__ uint32_t group_max(uint32_t m) {
  if (LANES == 4) {
    const int a = static_cast<int>(m);
    const int b = max(a, __builtin_amdgcn_update_dpp(0, a, 0xB1, 0xF, 0xF, true));  // quad_perm [1,0,3,2]
    const int c = max(b, __builtin_amdgcn_update_dpp(0, b, 0x4E, 0xF, 0xF, true));  // quad_perm [2,3,0,1]
    return static_cast<uint32_t>(c);
  }
  return m;
}

// grid.y = message block j; grid.x strides over the block's items: item t is
// part t % LANES (32 / LANES elements) of its 32-element block t / LANES.
template <int LANES, bool VEC>
__global__ void __launch_bounds__(kThreads)
mx_quantize_kernel(const uint16_t* __restrict__ src, size_t n_total, size_t block_elems, uint8_t* __restrict__ wire) {
  constexpr int EP = 32 / LANES;  // elements per lane
  const size_t j = blockIdx.y;
  const size_t np = (block_elems + 31) / 32 * 32, mxb = np / 32;
  const size_t wb = (np + mxb + 15) / 16 * 16;
  const size_t lim = block_limit(j, block_elems, n_total);
  const uint16_t* blk = src + j * block_elems;
  uint8_t* out = wire + j * wb;
  const size_t items = mxb * LANES, stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t t = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; t < items; t += stride) {
    const size_t b = t / LANES, part = t % LANES, k0 = b * 32 + part * EP;
    uint32_t w[EP / 2];
    uint32_t m = 0;
#pragma unroll
    for (int v = 0; v < EP / 8; ++v) {
      load8<VEC>(blk, k0 + 8 * v, lim, w + 4 * v);
#pragma unroll
      for (int i = 0; i < 4; ++i) m = max(m, amax_bits2(w[4 * v + i]));
    }
    const uint32_t sb = scale_byte(group_max<LANES>(m));
    const float mult = quant_mult(sb);
    uint32_t q[EP / 4];
#pragma unroll
    for (int i = 0; i < EP / 4; ++i) q[i] = quant4(w[2 * i], w[2 * i + 1], mult);
    store_payload<VEC, EP>(out + k0, q);
    if (part == 0) {
      out[np + b] = static_cast<uint8_t>(sb);
      if (b + 1 == mxb)  // the block's padding bytes (fewer than 16)
        for (size_t z = np + mxb; z < wb; ++z) out[z] = 0;
    }
  }
}

template <int LANES, bool VEC>
__global__ void __launch_bounds__(kThreads)
mx_dequantize_kernel(const uint8_t* __restrict__ wire, size_t block_elems, uint16_t* __restrict__ dst, size_t n_total) {
  constexpr int EP = 32 / LANES;
  const size_t j = blockIdx.y;
  const size_t np = (block_elems + 31) / 32 * 32, mxb = np / 32;
  const size_t wb = (np + mxb + 15) / 16 * 16;
  const size_t lim = block_limit(j, block_elems, n_total);
  const uint8_t* in = wire + j * wb;
  uint16_t* blk = dst + j * block_elems;
  const size_t items = mxb * LANES, stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t t = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; t < items; t += stride) {
    const size_t b = t / LANES, part = t % LANES, k0 = b * 32 + part * EP;
    if (k0 >= lim) continue;
    uint32_t q[EP / 4];
    load_payload<VEC, EP>(in + k0, q);
    const float mult = dequant_mult(in[np + b]);
#pragma unroll
    for (int v = 0; v < EP / 8; ++v) {
      float f[8];
      dequant4(q[2 * v], mult, f);
      dequant4(q[2 * v + 1], mult, f + 4);
      uint32_t w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = pack_bf16(f[2 * i], f[2 * i + 1]);
      store8<VEC>(blk, k0 + 8 * v, lim, w);
    }
  }
}

// dst[i] = bf16(sum over the W wire blocks, in block order) for i < n. A lane
// holds 16 elements (half a 32-element block): one 16-byte payload load and
// one scale byte per wire block, two 16-byte stores.
template <bool VEC>
__global__ void __launch_bounds__(kThreads)
mx_dequant_reduce_kernel(const uint8_t* __restrict__ wire, size_t block_elems, int W, uint16_t* __restrict__ dst,
                         size_t n) {
  const size_t np = (block_elems + 31) / 32 * 32, mxb = np / 32;
  const size_t wb = (np + mxb + 15) / 16 * 16;
  const size_t items = (n + 15) / 16, stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t t = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; t < items; t += stride) {
    const size_t k0 = t * 16;
    float acc[16];
    for (int r = 0; r < W; ++r) {
      const uint8_t* in = wire + static_cast<size_t>(r) * wb;
      uint32_t q[4];
      load_payload<VEC, 16>(in + k0, q);
      const float mult = dequant_mult(in[np + t / 2]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float f[4];
        dequant4(q[i], mult, f);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[4 * i + e] = r == 0 ? f[e] : acc[4 * i + e] + f[e];
      }
    }
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      uint32_t w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = pack_bf16(acc[8 * v + 2 * i], acc[8 * v + 2 * i + 1]);
      store8<VEC>(dst, k0 + 8 * v, n, w);
    }
  }
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// grid.x for `items` work items per message block and `nblocks` blocks in y.
dim3 grid_for(size_t items, size_t nblocks) {
  int dev = 0;
  DLNB_HIP_CHECK(hipGetDevice(&dev));
  const size_t budget = static_cast<size_t>(num_cus(dev)) * kBlocksPerCu;
  const size_t want = (items + kThreads - 1) / kThreads;
  const size_t gx = std::max<size_t>(1, std::min(want, std::max<size_t>(1, budget / nblocks)));
  return dim3(static_cast<unsigned>(gx), static_cast<unsigned>(nblocks), 1);
}

void check_blocks(const char* what, size_t block_elems, size_t nblocks) {
  DLNB_REQUIRE(block_elems >= 1 && nblocks >= 1 && nblocks <= 65535,
               what << ": block_elems " << block_elems << ", nblocks " << nblocks);
}

}  // namespace

void mx_quantize(const void* src, size_t n_total, size_t block_elems, size_t nblocks, void* wire, void* stream) {
  check_blocks("mx_quantize", block_elems, nblocks);
  DLNB_REQUIRE(src && wire, "mx_quantize: null buffer");
  const bool vec = aligned16(src) && aligned16(wire) && (block_elems % 8 == 0 || nblocks == 1);
  const dim3 grid = grid_for(mx_padded(block_elems) / 32 * DLNB_MXQ_LANES, nblocks);
  auto* s = static_cast<const uint16_t*>(src);
  auto* w = static_cast<uint8_t*>(wire);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL((mx_quantize_kernel<DLNB_MXQ_LANES, true>), grid, kThreads, 0, st, s, n_total, block_elems, w);
  else
    hipLaunchKernelGGL((mx_quantize_kernel<DLNB_MXQ_LANES, false>), grid, kThreads, 0, st, s, n_total, block_elems, w);
  DLNB_HIP_CHECK(hipGetLastError());
}

void mx_dequantize(const void* wire, size_t block_elems, size_t nblocks, void* dst, size_t n_total, void* stream) {
  check_blocks("mx_dequantize", block_elems, nblocks);
  DLNB_REQUIRE(dst && wire, "mx_dequantize: null buffer");
  const bool vec = aligned16(dst) && aligned16(wire) && (block_elems % 8 == 0 || nblocks == 1);
  const dim3 grid = grid_for(mx_padded(block_elems) / 32 * DLNB_MXQ_LANES, nblocks);
  auto* w = static_cast<const uint8_t*>(wire);
  auto* d = static_cast<uint16_t*>(dst);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL((mx_dequantize_kernel<DLNB_MXQ_LANES, true>), grid, kThreads, 0, st, w, block_elems, d, n_total);
  else
    hipLaunchKernelGGL((mx_dequantize_kernel<DLNB_MXQ_LANES, false>), grid, kThreads, 0, st, w, block_elems, d, n_total);
  DLNB_HIP_CHECK(hipGetLastError());
}

void mx_dequant_reduce(const void* wire, size_t block_elems, size_t nblocks, void* dst, size_t n, void* stream) {
  check_blocks("mx_dequant_reduce", block_elems, nblocks);
  DLNB_REQUIRE(dst && wire, "mx_dequant_reduce: null buffer");
  DLNB_REQUIRE(n >= 1 && n <= block_elems, "mx_dequant_reduce: n " << n << " of a block of " << block_elems);
  const bool vec = aligned16(dst) && aligned16(wire);
  const dim3 grid = grid_for((n + 15) / 16, 1);
  auto* w = static_cast<const uint8_t*>(wire);
  auto* d = static_cast<uint16_t*>(dst);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL(mx_dequant_reduce_kernel<true>, grid, kThreads, 0, st, w, block_elems, static_cast<int>(nblocks), d, n);
  else
    hipLaunchKernelGGL(mx_dequant_reduce_kernel<false>, grid, kThreads, 0, st, w, block_elems, static_cast<int>(nblocks), d, n);
  DLNB_HIP_CHECK(hipGetLastError());
}

}  // namespace kernels
}  // namespace dlnb
