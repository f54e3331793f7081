// Quantized wire (--wire-quant mxfp8): a decorator around any backend's
// communicators that keeps the strategy's buffers in bf16 and moves MXFP8 wire
// blocks (dlnb/wire_quant.hpp) instead - the ZeRO++ qwZ / qgZ pattern:
//
//   all_gather(n)      quantize 1 block -> inner all-gather of wire_bytes(n)
//                      bytes -> dequantize W blocks
//   reduce_scatter(n)  quantize W blocks -> inner all-to-all -> dequantize and
//                      reduce (rank order, fp32, one rounding)
//   all_to_all(n)      quantize W blocks -> inner all-to-all -> dequantize W
//   all_reduce(n)      the reduce-scatter above over W chunks of
//                      c = round_up(ceil(n / W), 32) elements (zero tail
//                      included), the reduced chunk rounded to bf16 and
//                      quantized again, inner all-gather, dequantize the first
//                      n elements
//
// Everything runs on the stream the operation was given (conversion kernels on
// the GPU, stream tasks on the CPU device), the inner transport moves bytes
// (DType::FP8_E4M3), and the staging makes in-place calls free. Point-to-point
// operations, other element types and 1-rank communicators pass through.
//
// The scratch wire buffers (send side, receive side, one reduced chunk) exist
// from create() on, sized from the communicator's capacity: operations run
// under graph capture and never allocate. Where the inner backend has
// zero-copy paths (wants_peer_buffers) they are peer memory registered with
// it, send first, then receive, on every member.
//
// Reference: none (DLNetBench has no quantized wire).
#include <algorithm>

#include "dlnb/comm.hpp"
#include "dlnb/wire_quant.hpp"

namespace dlnb {

namespace {

class QuantCommunicator : public Communicator {
 public:
  QuantCommunicator(std::unique_ptr<Communicator> in, Device& dev, size_t capacity, WireQuantCounts* counts)
      : in_(std::move(in)), dev_(dev), counts_(counts) {
    rank_ = in_->rank();
    size_ = in_->size();
    members_ = in_->members();
    name_ = in_->name();
    if (size_ < 2) return;
    const size_t bytes = scratch_bytes(capacity, static_cast<size_t>(size_));
    const bool peer = in_->wants_peer_buffers();
    sendw_ = peer ? dev_.alloc_peer(bytes) : dev_.alloc(bytes);
    recvw_ = peer ? dev_.alloc_peer(bytes) : dev_.alloc(bytes);
    chunk_ = dev_.alloc(max_chunk(capacity, static_cast<size_t>(size_)) * 2);
    if (peer) {
      in_->register_buffer(sendw_.data(), bytes);
      in_->register_buffer(recvw_.data(), bytes);
    }
  }
  std::string backend_name() const override { return in_->backend_name(); }

  // The largest block of a message that fits the capacity: W blocks of n
  // bf16 elements hold at most capacity bytes, and an all-reduce of that many
  // elements splits into W chunks rounded up to whole 32-element blocks.
  static size_t max_chunk(size_t capacity, size_t W) {
    const size_t elems = std::max<size_t>(1, (capacity + 1) / 2);
    return mx_padded((elems + W - 1) / W);
  }
  static size_t scratch_bytes(size_t capacity, size_t W) { return W * mx_wire_bytes(max_chunk(capacity, W)); }

  void all_gather(const void* send, void* recv, size_t n, DType t, Stream& s) override {
    if (!mine(t, n)) return in_->all_gather(send, recv, n, t, s);
    const size_t W = static_cast<size_t>(size_), wb = mx_wire_bytes(n);
    fits("all_gather", W * wb);
    count(CollKind::AllGather, n, wb);
    quantize(send, n, n, 1, s);
    in_->all_gather(sendw_.data(), recvw_.data(), wb, DType::FP8_E4M3, s);
    dequantize(n, W, recv, W * n, s);
  }
  void reduce_scatter(const void* send, void* recv, size_t n, DType t, Stream& s) override {
    if (!mine(t, n)) return in_->reduce_scatter(send, recv, n, t, s);
    const size_t W = static_cast<size_t>(size_), wb = mx_wire_bytes(n);
    fits("reduce_scatter", W * wb);
    count(CollKind::ReduceScatter, W * n, W * wb);
    quantize(send, W * n, n, W, s);
    in_->all_to_all(sendw_.data(), recvw_.data(), wb, DType::FP8_E4M3, s);
    dequant_reduce(n, W, recv, n, s);
  }
  void all_to_all(const void* send, void* recv, size_t n, DType t, Stream& s) override {
    if (!mine(t, n)) return in_->all_to_all(send, recv, n, t, s);
    const size_t W = static_cast<size_t>(size_), wb = mx_wire_bytes(n);
    fits("all_to_all", W * wb);
    count(CollKind::AllToAll, W * n, W * wb);
    quantize(send, W * n, n, W, s);
    in_->all_to_all(sendw_.data(), recvw_.data(), wb, DType::FP8_E4M3, s);
    dequantize(n, W, recv, W * n, s);
  }
  void all_reduce(const void* send, void* recv, size_t n, DType t, Stream& s) override {
    if (!mine(t, n)) return in_->all_reduce(send, recv, n, t, s);
    const size_t W = static_cast<size_t>(size_), c = mx_padded((n + W - 1) / W), wb = mx_wire_bytes(c);
    fits("all_reduce", W * wb);
    DLNB_REQUIRE(c * 2 <= chunk_.bytes(), "--wire-quant: all_reduce chunk of " << c << " elements exceeds the capacity of " << name_);
    count(CollKind::AllReduce, (W + 1) * c, (W + 1) * wb);
    quantize(send, n, c, W, s);
    in_->all_to_all(sendw_.data(), recvw_.data(), wb, DType::FP8_E4M3, s);
    dequant_reduce(c, W, chunk_.data(), c, s);
    quantize(chunk_.data(), c, c, 1, s);
    in_->all_gather(sendw_.data(), recvw_.data(), wb, DType::FP8_E4M3, s);
    dequantize(c, W, recv, n, s);
  }
  void send(const void* buf, size_t count, DType t, int peer, Stream& s) override { in_->send(buf, count, t, peer, s); }
  void recv(void* buf, size_t count, DType t, int peer, Stream& s) override { in_->recv(buf, count, t, peer, s); }
  void group_start() override { in_->group_start(); }
  void group_end() override { in_->group_end(); }
  bool wants_peer_buffers() const override { return in_->wants_peer_buffers(); }
  void register_buffer(void* p, size_t bytes) override { in_->register_buffer(p, bytes); }
  std::string async_error() override { return in_->async_error(); }
  void abort() override { in_->abort(); }
  int library_nranks() override { return in_->library_nranks(); }

 private:
  bool mine(DType t, size_t n) const { return t == DType::BF16 && size_ > 1 && n > 0; }
  void fits(const char* op, size_t wire) const {
    DLNB_REQUIRE(wire <= sendw_.bytes(), "--wire-quant: " << op << " needs " << wire << " wire bytes, the capacity of "
                                                          << name_ << " gives " << sendw_.bytes());
  }
  // elems: bf16 elements handed over in quantized form; wire: their wire bytes
  void count(CollKind k, size_t elems, size_t wire) {
    if (!counts_) return;
    WireQuantCounts::Op& o = counts_->ops[static_cast<int>(k)];
    ++o.calls;
    o.payload_bytes += elems * 2;
    o.wire_bytes += wire;
  }
  bool gpu() const { return dev_.kind() == DeviceKind::GPU; }
  // src -> the send-side wire buffer
  void quantize(const void* src, size_t n_total, size_t block, size_t nblocks, Stream& s) {
    void* wire = sendw_.data();
    if (gpu()) return kernels::mx_quantize(src, n_total, block, nblocks, wire, s.native());
    dev_.host_task(s, [=] {
      mx_quantize_host(static_cast<const uint16_t*>(src), n_total, block, nblocks, static_cast<uint8_t*>(wire));
    });
  }
  // the receive-side wire buffer -> dst
  void dequantize(size_t block, size_t nblocks, void* dst, size_t n_total, Stream& s) {
    const void* wire = recvw_.data();
    if (gpu()) return kernels::mx_dequantize(wire, block, nblocks, dst, n_total, s.native());
    dev_.host_task(s, [=] {
      mx_dequantize_host(static_cast<const uint8_t*>(wire), block, nblocks, static_cast<uint16_t*>(dst), n_total);
    });
  }
  void dequant_reduce(size_t block, size_t nblocks, void* dst, size_t n, Stream& s) {
    const void* wire = recvw_.data();
    if (gpu()) return kernels::mx_dequant_reduce(wire, block, nblocks, dst, n, s.native());
    dev_.host_task(s, [=] {
      mx_dequant_reduce_host(static_cast<const uint8_t*>(wire), block, nblocks, static_cast<uint16_t*>(dst), n);
    });
  }

  std::unique_ptr<Communicator> in_;
  Device& dev_;
  WireQuantCounts* counts_;
  Buffer sendw_, recvw_, chunk_;
};

class QuantFactory : public CommFactory {
 public:
  QuantFactory(std::unique_ptr<CommFactory> in, Device& dev, WireQuantCounts* counts)
      : in_(std::move(in)), dev_(dev), counts_(counts) {}
  std::string backend_name() const override { return in_->backend_name(); }
  std::unique_ptr<Communicator> create(const std::string& name, const std::vector<int>& members,
                                       size_t capacity_bytes, bool need_p2p, int max_ctas) override {
    // the inner transport carries the wire blocks (and still the untouched
    // operations, sized by the caller's capacity)
    const size_t W = members.size();
    const size_t inner = W > 1 ? std::max(capacity_bytes, QuantCommunicator::scratch_bytes(capacity_bytes, W)) : capacity_bytes;
    return std::make_unique<QuantCommunicator>(in_->create(name, members, inner, need_p2p, max_ctas), dev_,
                                               capacity_bytes, counts_);
  }

 private:
  std::unique_ptr<CommFactory> in_;
  Device& dev_;
  WireQuantCounts* counts_;
};

}  // namespace

std::unique_ptr<CommFactory> wrap_comm_quant(std::unique_ptr<CommFactory> inner, Device& dev, const std::string& mode,
                                             WireQuantCounts* counts) {
  if (mode.empty() || mode == "none") return inner;
  DLNB_REQUIRE(mode == "mxfp8", "--wire-quant must be none or mxfp8 (got '" << mode << "')");
  return std::make_unique<QuantFactory>(std::move(inner), dev, counts);
}

}  // namespace dlnb
