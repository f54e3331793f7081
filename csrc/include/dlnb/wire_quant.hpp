// MXFP8 (OCP MX v1.0, E4M3 elements, E8M0 scale per 32 elements) wire format
// for bf16 collectives (--wire-quant mxfp8): sizes, the host reference
// implementation (CPU device, commtest's expected values) and the gfx950
// kernels (csrc/kernels/wire_quant.hip). See docs/KERNELS.md "wire_quant".
//
// A message of n bf16 elements is padded with zeros to np = round_up(n, 32);
// its wire block is np bytes of e4m3 payload, np / 32 bytes of e8m0 scales and
// zero padding up to a multiple of 16 bytes.
//   scale byte of a 32-element block: max(E - 8, 0), E the biased bf16
//     exponent of the block's largest |x| (e = floor(log2 amax) - 8 clamped to
//     [-127, 127], stored as e + 127; amax == 0 gives 0); 0xFF when the block
//     holds an Inf or a NaN (the payload is then unspecified);
//   payload: rne_e4m3fn(clamp(x * 2^-e, -448, 448));
//   dequantize: bf16(float(q) * 2^e); scale 0xFF gives NaN, scale 0 (amax
//     below 2^-118) gives signed zeros: 2^-127 is an fp32 denormal, and
//     |result| <= amax is all the format promises down there;
//   dequantize and reduce: the products of ranks 0, 1, .. W-1 added in that
//     order in fp32 (starting from rank 0's product), rounded to bf16 once.
//
// Reference: none (DLNetBench has no quantized wire; ZeRO++ qwZ / qgZ is the
// model).
#pragma once

#include <cstddef>
#include <cstdint>

namespace dlnb {

constexpr size_t kMxBlock = 32;

inline size_t mx_padded(size_t n) { return (n + kMxBlock - 1) / kMxBlock * kMxBlock; }
inline size_t mx_wire_bytes(size_t n) {
  const size_t np = mx_padded(n);
  return (np + np / kMxBlock + 15) / 16 * 16;
}

// Host implementations (threaded for large sizes, like host_reduce_sum).
// Message block j covers src[j * block_elems ..]; elements at index >= n_total
// and anything beyond block_elems inside the padded block read as zero. Block
// j goes to wire + j * mx_wire_bytes(block_elems), padding bytes included.
void mx_quantize_host(const uint16_t* src, size_t n_total, size_t block_elems, size_t nblocks, uint8_t* wire);
// The inverse; writes only elements below n_total.
void mx_dequantize_host(const uint8_t* wire, size_t block_elems, size_t nblocks, uint16_t* dst, size_t n_total);
// dst[i] (i < n <= block_elems) = the rank-ordered sum over the nblocks wire blocks.
void mx_dequant_reduce_host(const uint8_t* wire, size_t block_elems, size_t nblocks, uint16_t* dst, size_t n);

namespace kernels {

// The same three operations on the GPU, enqueued on `stream`. Any n >= 1 and
// any alignment: 16-byte vector accesses when the pointers are 16-byte aligned
// and every message block starts on a 16-byte boundary, an element-wise path
// (chosen once per launch) otherwise.
void mx_quantize(const void* src, size_t n_total, size_t block_elems, size_t nblocks, void* wire, void* stream);
void mx_dequantize(const void* wire, size_t block_elems, size_t nblocks, void* dst, size_t n_total, void* stream);
void mx_dequant_reduce(const void* wire, size_t block_elems, size_t nblocks, void* dst, size_t n, void* stream);

}  // namespace kernels

}  // namespace dlnb
