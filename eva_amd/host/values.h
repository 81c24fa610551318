// values.h — what crosses the execute() boundary and where it lives: the plain-double reference semantics
// (reference_executor.cpp:14-115), the valuation (seal.h:21-41: name -> ciphertext / plaintext / constant; a
// ciphertext may be host words, a device handle, or both), device handles and the device contexts / issue queues
// they belong to.  Split out of executor.h (r04); included by it.
#pragma once
#include <array>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <memory>
#include <tuple>
#include <random>
#include <string>
#include <unordered_map>
#include <variant>
#include "ckks_host.h"
#include "eva_hip.h"
#include "passes.h"

namespace evahost {

using Valuation = std::unordered_map<std::string, std::vector<double>>;

[[noreturn]] inline void throw_backend() { throw std::runtime_error(std::string("eva_hip: ") + evah_last_error()); }
inline void chk(int rc) { if (rc) throw_backend(); }

// ---- plain-double reference semantics (reference_executor.cpp:14-115)
inline void rotate_left(const std::vector<double> &in, int32_t shift, std::vector<double> &out) {
  int64_t n = (int64_t)in.size(), s = shift;
  while (s > 0 && s >= n) s -= n;
  while (s < 0) s += n;
  out.resize(in.size());
  for (int64_t i = 0; i < n; i++) out[i] = in[(i + s) % n];
}
inline void rotate_right(const std::vector<double> &in, int32_t shift, std::vector<double> &out) {
  int64_t n = (int64_t)in.size(), s = shift;
  while (s > 0 && s >= n) s -= n;
  while (s < 0) s += n;
  out.resize(in.size());
  for (int64_t i = 0; i < n; i++) out[(i + s) % n] = in[i];
}

inline Valuation evaluate(Program &p, const Valuation &inputs) {
  std::vector<std::vector<double>> vals(p.size());
  const size_t n = p.vec_size();
  for (auto &kv : inputs) {
    TermId t = p.input(kv.first);
    vals[t] = kv.second;
    if (vals[t].size() != n)
      throw std::runtime_error("The length of all inputs must be the same as program's vector size. Input " + kv.first +
                               " has length " + std::to_string(vals[t].size()) + ", but vector size is " + std::to_string(n));
  }
  for (TermId t : p.topo_order()) {
    const Term &x = p.at(t);
    auto &out = vals[t];
    auto bin = [&](auto f) {
      const auto &a = vals[x.operands[0]], &b = vals[x.operands[1]];
      out.resize(a.size());
      for (size_t i = 0; i < a.size(); i++) out[i] = f(a[i], b[i]);
    };
    switch (x.op) {
    case Op::Input: break;
    case Op::Constant: x.constant->expand_to(out, n); break;
    case Op::Add: bin([](double a, double b) { return a + b; }); break;
    case Op::Sub: bin([](double a, double b) { return a - b; }); break;
    case Op::Mul: bin([](double a, double b) { return a * b; }); break;
    case Op::RotateLeftConst: rotate_left(vals[x.operands[0]], x.rotation, out); break;
    case Op::RotateRightConst: rotate_right(vals[x.operands[0]], x.rotation, out); break;
    case Op::Negate: {
      const auto &a = vals[x.operands[0]];
      out.resize(a.size());
      for (size_t i = 0; i < a.size(); i++) out[i] = -a[i];
    } break;
    case Op::Encode:
    case Op::Output:
    case Op::Relinearize:
    case Op::ModSwitch:
    case Op::Rescale: out = vals[x.operands[0]]; break;
    default: throw std::runtime_error(std::string("Unhandled op ") + op_name(x.op));
    }
  }
  Valuation outv;
  for (auto &kv : p.outputs()) outv[kv.first] = vals[kv.second];
  return outv;
}

// ---- values crossing the execute() boundary (seal.h:21-41)
using SchemeValue = std::variant<HostCipher, HostPlain, std::vector<double>>;
struct HipValuation {
  std::unordered_map<std::string, SchemeValue> values;
  // the encryption parameters the values belong to (SEALValuation::params, seal.h:23-27): set by encrypt(),
  // execute() and load(); needed to write the valuation in the reference's SEAL wire format
  std::shared_ptr<const HostContext> params;
};

// RAII device handles
struct CtHandle {
  evah_ctx *ctx = nullptr;
  evah_ct *h = nullptr;
  CtHandle() {}
  CtHandle(evah_ctx *c, evah_ct *p) : ctx(c), h(p) {}
  CtHandle(CtHandle &&o) noexcept : ctx(o.ctx), h(o.h) { o.h = nullptr; }
  CtHandle &operator=(CtHandle &&o) noexcept { reset(); ctx = o.ctx; h = o.h; o.h = nullptr; return *this; }
  CtHandle(const CtHandle &) = delete;
  CtHandle &operator=(const CtHandle &) = delete;
  void reset() { if (h) evah_ct_free(ctx, h); h = nullptr; }
  ~CtHandle() { reset(); }
};
struct PtHandle {
  evah_ctx *ctx = nullptr;
  evah_pt *h = nullptr;
  PtHandle() {}
  PtHandle(evah_ctx *c, evah_pt *p) : ctx(c), h(p) {}
  PtHandle(PtHandle &&o) noexcept : ctx(o.ctx), h(o.h) { o.h = nullptr; }
  PtHandle &operator=(PtHandle &&o) noexcept { reset(); ctx = o.ctx; h = o.h; o.h = nullptr; return *this; }
  PtHandle(const PtHandle &) = delete;
  PtHandle &operator=(const PtHandle &) = delete;
  void reset() { if (h) evah_pt_free(ctx, h); h = nullptr; }
  ~PtHandle() { reset(); }
};

// ---- device contexts (seal.h:45-97 keeps a SEALContext per key set; here: tables + keys in HBM)
struct DeviceCtx {
  evah_ctx *h = nullptr;
  int device = 0; // the GPU the state lives on
  DeviceCtx(uint32_t N, const std::vector<u64> &primes, int device_) : device(device_) {
    chk(evah_ctx_create(N, (uint32_t)primes.size(), (const uint64_t *)primes.data(), device, &h));
  }
  ~DeviceCtx() { evah_ctx_destroy(h); }
  DeviceCtx(const DeviceCtx &) = delete;
  DeviceCtx &operator=(const DeviceCtx &) = delete;
};
// A second issue queue of a device context (evah_ctx_fork).  It keeps its parent alive, so a value
// that was produced through it can outlive the HipPublic that created the queue.
struct Fork {
  std::shared_ptr<DeviceCtx> parent;
  evah_ctx *h = nullptr;
  explicit Fork(std::shared_ptr<DeviceCtx> p) : parent(std::move(p)) { chk(evah_ctx_fork(parent->h, &h)); }
  ~Fork() { evah_ctx_destroy(h); }
  Fork(const Fork &) = delete;
  Fork &operator=(const Fork &) = delete;
};
// The device half of a ciphertext value (ckks_host.h HostCipher::dev): a handle of `root`'s device
// state.  seal_executor.h:264-277 / :420-435 copy values in and out of the executor; a resident value
// is passed by handle instead — no copy, no PCIe.
struct DeviceResident {
  std::shared_ptr<DeviceCtx> root; // tables and keys the handle belongs to
  std::shared_ptr<Fork> queue;     // the issue queue whose pool holds the buffer (null: the root's own)
  std::shared_ptr<CtHandle> h;
  uint32_t N = 0;                  // poly_modulus_degree: words per limb
  evah_ctx *ctx() const { return queue ? queue->h : root->h; }
};
// ---- a batch of valuations as batched device handles: what encrypt_array returns, execute_batch takes
// and returns as it is, and decrypt_array reads.  Per encrypted name the B instances are an ordered list of segments —
// a batched handle each, kept whole — where the list path keeps B values with a view each.
struct BatchSegment {
  std::shared_ptr<CtHandle> h;  // a batched handle (or a slice, or a single ciphertext: a segment of one)
  uint32_t n = 0;               // its instances
  std::shared_ptr<Fork> queue;  // the issue queue whose pool holds the buffer (null: the root's own)
  uint32_t size = 0, limbs = 0;
  double scale = 0;
};
struct BatchCipher {
  std::vector<BatchSegment> segments;
  std::vector<std::array<uint8_t, 32>> seeds; // symmetric encryptions: the seed of c1 per instance, else empty
};
// an array [B][n] of the caller's, in its own type (EVAH_F64 / EVAH_F32 / EVAH_U8), C-contiguous
// — or rows in device memory, possibly pitched, which the host never dereferences: on_device, with the
// stream that produced them (null: the caller synchronised) and, once plan_array_inputs has asked the device for them,
// the rows' sums of absolute values
struct ArrayView {
  const void *data = nullptr;
  int dtype = EVAH_F64;
  size_t B = 0, n = 0;
  size_t pitch = 0; // bytes between rows; 0: contiguous
  bool on_device = false;
  void *producer = nullptr;
  std::shared_ptr<std::vector<double>> sums;
  size_t itemsize() const { return dtype == EVAH_F64 ? 8 : dtype == EVAH_F32 ? 4 : 1; }
  size_t row_pitch() const { return pitch ? pitch : n * itemsize(); }
  const void *row(size_t b) const { return static_cast<const char *>(data) + b * row_pitch(); }
};
// memory of a key pair's device state that holds decrypted rows [B][n] (decrypt_array(device=True)):
// zeroed on the queue before it returns to the pool
struct DeviceArray {
  std::shared_ptr<DeviceCtx> dev;
  evah_buf *buf = nullptr;
  int dtype = EVAH_F64;
  size_t B = 0, n = 0;
  DeviceArray(std::shared_ptr<DeviceCtx> d, int dt, size_t B_, size_t n_) : dev(std::move(d)), dtype(dt), B(B_), n(n_) {
    chk(evah_buf_alloc(dev->h, (bytes() + 7) / 8, &buf));
  }
  DeviceArray(const DeviceArray &) = delete;
  DeviceArray &operator=(const DeviceArray &) = delete;
  ~DeviceArray() {
    if (!buf) return;
    (void)evah_buf_wipe(dev->h, buf);
    evah_buf_free(dev->h, buf);
  }
  size_t itemsize() const { return dtype == EVAH_F64 ? 8 : dtype == EVAH_F32 ? 4 : 1; }
  size_t bytes() const { return B * n * itemsize(); }
  void *ptr() const { return evah_buf_ptr(buf); }
};
// row b as the doubles its values convert to exactly
inline std::vector<double> array_row_doubles(const ArrayView &a, size_t b) {
  std::vector<double> v(a.n);
  for (size_t i = 0; i < a.n; i++)
    v[i] = a.dtype == EVAH_F64   ? static_cast<const double *>(a.row(b))[i]
           : a.dtype == EVAH_F32 ? (double)static_cast<const float *>(a.row(b))[i]
                                 : (double)static_cast<const uint8_t *>(a.row(b))[i];
  return v;
}
// an unencrypted value that differs per instance: typed rows [B][n] the batch owns, row b for instance b
struct PlainRows {
  ArrayView view;                               // into *bytes
  std::shared_ptr<std::vector<uint8_t>> bytes;  // the rows in their own type
};
struct HipValuationBatch {
  size_t B = 0;
  std::map<std::string, BatchCipher> ciphers;
  std::unordered_map<std::string, SchemeValue> shared; // plaintexts and raw vectors: one value for all instances
  std::map<std::string, PlainRows> plains;             // raw values with a row per instance
  std::shared_ptr<DeviceCtx> root;                     // the device state every segment lives on
  std::shared_ptr<const HostContext> params;
};

// host words of a ciphertext value, downloaded on first use (waits for the value to be computed) or expanded
// from its seeded form (c0 + seed)
inline const CipherWords &words(const HostCipher &c) {
  if (c.data.empty() && c.dev) {
    CipherWords w((size_t)c.size * c.limbs * c.dev->N);
    chk(evah_ct_download(c.dev->ctx(), c.dev->h->h, (uint64_t *)w.data()));
    c.data = std::move(w);
    c.words_checked = true; // the device's own residues
  } else if (c.data.empty() && c.seeded && !c.seeded->c0.empty()) {
    if (c.size != 2) throw std::runtime_error("a seeded ciphertext has two polynomials");
    CipherWords w;
    materialise_seeded(*c.seeded, c.limbs, w);
    c.data = std::move(w);
  }
  return c.data;
}
inline bool resident_only(const HostCipher &c) { return c.data.empty() && c.dev; }
// c0 + seed on the host: the value can be uploaded seeded (its full words may have been materialised as well)
inline bool seeded_on_host(const HostCipher &c) { return c.seeded && !c.seeded->c0.empty() && c.size == 2; }
// ... and the device of `host` expands the same c1: same degree, same primes under the value's limbs
inline bool seeded_upload_ok(const HostCipher &c, const HostContext &host) {
  if (!seeded_on_host(c) || c.seeded->N != host.N || c.seeded->primes.size() < c.limbs || c.limbs > host.k - 1 ||
      c.seeded->c0.size() != (size_t)c.limbs * host.N)
    return false;
  for (uint32_t i = 0; i < c.limbs; i++)
    if (c.seeded->primes[i] != host.primes[i]) return false;
  return true;
}

// ---- decryption shares: what one party contributes to the joint opening of a valuation.  Per encrypted
// name a list of pieces — one per device call, at most 64 instances of one level each; a single valuation has one piece of
// one instance — held as a resident batched handle [n][1][l][N], as host words [n][l][N], or both (the words of a resident
// piece are downloaded on demand, as a HostCipher's are).
struct SharePiece {
  uint32_t n = 0, limbs = 0;
  double scale = 1.0;
  mutable std::vector<u64> data;  // [n][limbs][N]; empty while the piece lives only on the device
  std::shared_ptr<CtHandle> h;
  std::shared_ptr<DeviceCtx> root; // the device state the handle belongs to
};
struct DecryptionShares {
  uint32_t N = 0, smudge_bits = 0;
  std::vector<u64> primes;        // the chain of the parameters (special prime last)
  bool batch = false;             // made from a SEALValuationBatch: B instances per name
  size_t B = 1;
  std::map<std::string, std::vector<SharePiece>> values;
};
inline const std::vector<u64> &words(const SharePiece &p, uint32_t N) {
  if (p.data.empty() && p.h) {
    std::vector<u64> w((size_t)p.n * p.limbs * N);
    chk(evah_ct_download(p.root->h, p.h->h, (uint64_t *)w.data()));
    p.data = std::move(w);
  }
  return p.data;
}

} // namespace evahost
