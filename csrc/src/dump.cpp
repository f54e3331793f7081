// --dump-outputs: the result buffers of the last iteration as .npy files.
//
// Every output the strategy names (Strategy::outputs) and the compute
// engine's GEMM product (ComputeEngine::product) is copied to the host,
// converted to float32 and written as dir/<name>.npy (NumPy format 1.0, one
// dimension). The files hold at most 48 MB together: each output gets an
// equal share, and one that is larger is written as a fixed sample - blocks
// of 1024 consecutive elements, one in each equal stretch of the buffer, at
// an offset inside the stretch drawn from a hash of the output's name and the
// block's index - so the same configuration always samples the same elements.
#include <sys/stat.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "dlnb/strategy.hpp"

namespace dlnb {

namespace {

constexpr size_t kBudgetElems = 12u << 20;  // float32 elements in all files together (48 MB)
constexpr size_t kBlock = 1024;

uint64_t mix(uint64_t x) {  // splitmix64
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

uint64_t name_seed(const std::string& s) {  // FNV-1a
  uint64_t h = 0xcbf29ce484222325ull;
  for (unsigned char c : s) h = (h ^ c) * 0x100000001b3ull;
  return h;
}

void make_dirs(const std::string& dir) {
  for (size_t i = 1; i <= dir.size(); ++i) {
    if (i != dir.size() && dir[i] != '/') continue;
    const std::string p = dir.substr(0, i);
    if (::mkdir(p.c_str(), 0777) != 0 && errno != EEXIST)
      DLNB_THROW("--dump-outputs: cannot create " << p << ": " << std::strerror(errno));
  }
}

float element(const void* p, size_t i, DType t) {
  switch (t) {
    case DType::BF16: return bf16_to_float(static_cast<const uint16_t*>(p)[i]);
    case DType::FP16: return fp16_to_float(static_cast<const uint16_t*>(p)[i]);
    case DType::FP32: return static_cast<const float*>(p)[i];
    case DType::FP8_E4M3: return fp8e4m3_to_float(static_cast<const uint8_t*>(p)[i]);
    case DType::FP8_E5M2: return fp8e5m2_to_float(static_cast<const uint8_t*>(p)[i]);
  }
  return 0.0f;
}

void write_npy(const std::string& path, const std::vector<float>& v) {
  std::string h = "{'descr': '<f4', 'fortran_order': False, 'shape': (" + std::to_string(v.size()) + ",), }";
  while ((10 + h.size() + 1) % 64) h.push_back(' ');
  h.push_back('\n');
  std::ofstream f(path, std::ios::binary | std::ios::trunc);
  DLNB_REQUIRE(f.good(), "--dump-outputs: cannot write " << path);
  const unsigned char head[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, static_cast<unsigned char>(h.size() & 0xff),
                                  static_cast<unsigned char>(h.size() >> 8)};
  f.write(reinterpret_cast<const char*>(head), sizeof head);
  f.write(h.data(), static_cast<std::streamsize>(h.size()));
  f.write(reinterpret_cast<const char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(float)));
  f.close();
  DLNB_REQUIRE(f.good(), "--dump-outputs: short write to " << path);
}

}  // namespace

void dump_outputs(Context& ctx, const Strategy& strat, const std::string& dir) {
  std::vector<OutputView> outs = strat.outputs();
  {
    const void* c = nullptr;
    size_t n = 0;
    DType t = DType::BF16;
    if (ctx.compute && ctx.compute->product(&c, &n, &t)) outs.push_back({"gemm_product", c, n, t});
  }
  if (ctx.rank() != 0 || outs.empty()) return;
  make_dirs(dir);
  const size_t share = std::max(kBlock, kBudgetElems / outs.size() / kBlock * kBlock);
  auto stream = ctx.dev->create_stream(false);
  std::vector<unsigned char> raw;
  std::vector<float> vals;
  for (const OutputView& o : outs) {
    const size_t es = dtype_size(o.dtype);
    const char* src = static_cast<const char*>(o.data);
    vals.clear();
    auto take = [&](size_t first, size_t n) {
      raw.resize(n * es);
      ctx.dev->copy_async(raw.data(), src + first * es, n * es, *stream);
      stream->synchronize();
      for (size_t i = 0; i < n; ++i) vals.push_back(element(raw.data(), i, o.dtype));
    };
    if (o.count <= share) {
      take(0, o.count);
    } else {
      const size_t blocks = share / kBlock, stretch = o.count / blocks;  // stretch >= kBlock: count > share
      const uint64_t seed = name_seed(o.name);
      for (size_t b = 0; b < blocks; ++b) take(b * stretch + mix(seed + b) % (stretch - kBlock + 1), kBlock);
    }
    write_npy(dir + "/" + o.name + ".npy", vals);
  }
}

}  // namespace dlnb
