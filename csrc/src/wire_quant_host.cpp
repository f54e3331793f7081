// Host implementation of the MXFP8 wire format (dlnb/wire_quant.hpp): what the
// CPU device runs as stream tasks under --wire-quant mxfp8 and what commtest
// derives its expected values from. Built on the scalar conversions of
// common.cpp; large sizes are split over a few threads like host_reduce_sum.
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "dlnb/common.hpp"
#include "dlnb/wire_quant.hpp"

namespace dlnb {

namespace {

float bits_f(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// 2^e for a scale byte; NaN for 0xFF, 0 for 0 (dlnb/wire_quant.hpp)
float dequant_mult(uint8_t sb) { return bits_f(sb == 0xffu ? 0x7fc00000u : static_cast<uint32_t>(sb) << 23); }

// fn(lo, hi) over [0, total) 32-element blocks, in up to DLNB_SHM_THREADS (8)
// pieces of at least 32 Ki blocks (1 Mi elements); the caller takes the first.
template <typename F>
void par_blocks(size_t total, F fn) {
  constexpr size_t kMinPiece = size_t(1) << 15;
  static const size_t max_threads = [] {
    const long long env = env_int("DLNB_SHM_THREADS", 0);
    if (env > 0) return static_cast<size_t>(env);
    return static_cast<size_t>(std::max(1u, std::min(8u, std::thread::hardware_concurrency())));
  }();
  const size_t T = std::min(max_threads, std::max<size_t>(1, total / kMinPiece));
  if (T <= 1) {
    fn(size_t(0), total);
    return;
  }
  const size_t per = (total + T - 1) / T;
  std::vector<std::thread> th;
  for (size_t i = 1; i < T && i * per < total; ++i)
    th.emplace_back([=] { fn(i * per, std::min(total, (i + 1) * per)); });
  fn(size_t(0), std::min(per, total));
  for (auto& t : th) t.join();
}

// Elements of message block j that exist (below block_elems and n_total).
size_t block_limit(size_t j, size_t block_elems, size_t n_total) {
  const size_t start = j * block_elems;
  return start >= n_total ? 0 : std::min(block_elems, n_total - start);
}

}  // namespace

void mx_quantize_host(const uint16_t* src, size_t n_total, size_t block_elems, size_t nblocks, uint8_t* wire) {
  DLNB_REQUIRE(block_elems >= 1, "mx_quantize_host: empty block");
  const size_t np = mx_padded(block_elems), mxb = np / kMxBlock, wb = mx_wire_bytes(block_elems);
  par_blocks(nblocks * mxb, [=](size_t lo, size_t hi) {
    for (size_t g = lo; g < hi; ++g) {
      const size_t j = g / mxb, b = g % mxb;
      const size_t lim = block_limit(j, block_elems, n_total);
      const uint16_t* blk = src + j * block_elems;
      uint8_t* out = wire + j * wb;
      uint16_t x[kMxBlock];
      uint32_t m = 0;
      for (size_t i = 0; i < kMxBlock; ++i) {
        const size_t k = b * kMxBlock + i;
        x[i] = k < lim ? blk[k] : 0;
        m = std::max<uint32_t>(m, x[i] & 0x7fffu);
      }
      // biased bf16 exponent of amax -> e + 127 = max(E - 8, 0); Inf / NaN -> 0xFF
      const uint32_t E = m >> 7;
      const uint8_t sb = m >= 0x7f80u ? 0xffu : static_cast<uint8_t>(E > 8 ? E - 8 : 0);
      const float mult = bits_f((254u - (sb == 0xffu ? 0u : sb)) << 23);  // 2^-e
      for (size_t i = 0; i < kMxBlock; ++i) {
        const float v = bf16_to_float(x[i]) * mult;
        out[b * kMxBlock + i] = float_to_fp8e4m3(std::min(448.0f, std::max(-448.0f, v)));  // (saturates itself, too)
      }
      out[np + b] = sb;
      if (b + 1 == mxb) std::memset(out + np + mxb, 0, wb - np - mxb);
    }
  });
}

void mx_dequantize_host(const uint8_t* wire, size_t block_elems, size_t nblocks, uint16_t* dst, size_t n_total) {
  DLNB_REQUIRE(block_elems >= 1, "mx_dequantize_host: empty block");
  const size_t np = mx_padded(block_elems), mxb = np / kMxBlock, wb = mx_wire_bytes(block_elems);
  par_blocks(nblocks * mxb, [=](size_t lo, size_t hi) {
    for (size_t g = lo; g < hi; ++g) {
      const size_t j = g / mxb, b = g % mxb;
      const size_t lim = block_limit(j, block_elems, n_total);
      const uint8_t* in = wire + j * wb;
      uint16_t* blk = dst + j * block_elems;
      const float mult = dequant_mult(in[np + b]);
      for (size_t k = b * kMxBlock; k < std::min(lim, (b + 1) * kMxBlock); ++k)
        blk[k] = float_to_bf16(fp8e4m3_to_float(in[k]) * mult);
    }
  });
}

void mx_dequant_reduce_host(const uint8_t* wire, size_t block_elems, size_t nblocks, uint16_t* dst, size_t n) {
  DLNB_REQUIRE(block_elems >= 1 && nblocks >= 1 && n <= block_elems, "mx_dequant_reduce_host: bad sizes");
  const size_t np = mx_padded(block_elems), mxb = np / kMxBlock, wb = mx_wire_bytes(block_elems);
  par_blocks((n + kMxBlock - 1) / kMxBlock, [=](size_t lo, size_t hi) {
    for (size_t b = lo; b < hi; ++b) {
      float acc[kMxBlock];
      for (size_t r = 0; r < nblocks; ++r) {
        const uint8_t* in = wire + r * wb;
        const float mult = dequant_mult(in[np + b]);
        for (size_t i = 0; i < kMxBlock; ++i) {
          const float p = fp8e4m3_to_float(in[b * kMxBlock + i]) * mult;
          acc[i] = r == 0 ? p : acc[i] + p;
        }
      }
      for (size_t k = b * kMxBlock; k < std::min(n, (b + 1) * kMxBlock); ++k) dst[k] = float_to_bf16(acc[k - b * kMxBlock]);
    }
  });
  (void)mxb;
}

}  // namespace dlnb
