// client.h — the client side: HipPublic::encrypt (SEALPublic::encrypt, seal.cpp:24-102; encoder + encryptor on the
// device when one is present, ciphertexts left resident), HipSecret (SEALSecret::decrypt, seal.cpp:124-146) and
// generate_keys (seal.cpp:174-203).  Included by public_ctx.h.
#pragma once

namespace evahost {

// instances per batched client call (KS_BATCH_MAX of the library)
constexpr size_t CLIENT_BATCH_MAX = 64;
// the sorted input names of a batch: every instance must name exactly the inputs of instance 0
inline std::vector<std::string> batch_input_names(const std::vector<Valuation> &inputs) {
  std::vector<std::string> names;
  for (auto &kv : inputs[0]) names.push_back(kv.first);
  std::sort(names.begin(), names.end());
  for (size_t b = 1; b < inputs.size(); b++) {
    bool same = inputs[b].size() == names.size();
    for (size_t i = 0; same && i < names.size(); i++) same = inputs[b].count(names[i]) != 0;
    if (!same) throw std::runtime_error("instance " + std::to_string(b) + ": input names differ from those of instance 0");
  }
  return names;
}

// the signature checks every client call makes first
inline void check_vec_size(const CKKSSignature &sig, size_t slots) {
  if (sig.vec_size <= 0) throw std::runtime_error("Signature vector size must be positive");
  if (slots < (size_t)sig.vec_size) throw std::runtime_error("Vector size cannot be larger than slot count");
  if (slots % sig.vec_size) throw std::runtime_error("Vector size must exactly divide the slot count");
}
inline void check_input_size(const std::vector<double> &v, const CKKSSignature &sig) {
  if (v.size() != (size_t)sig.vec_size) throw std::runtime_error("Input size does not match program vector size");
}
// what the signature makes of an input: Cipher (encoded and encrypted) or Plain (encoded), both with the limb count and
// scale of their level, or anything else (raw: passed through)
struct InputClass {
  Type kind;
  uint32_t limbs = 0;
  double scale = 0;
};
inline InputClass classify_input(const HostContext &hc, const CKKSSignature &sig, const std::string &name) {
  auto it = sig.inputs.find(name);
  if (it == sig.inputs.end()) throw std::out_of_range("No input named " + name + " in the signature");
  const CKKSEncodingInfo &info = it->second;
  InputClass in{info.input_type};
  if (in.kind != Type::Cipher && in.kind != Type::Plain) return in;
  if ((uint32_t)info.level >= hc.k - 1) throw std::runtime_error("Input level exceeds the modulus chain");
  in.limbs = hc.k - 1 - (uint32_t)info.level;
  in.scale = std::pow(2.0, (double)info.scale);
  return in;
}

// the host encoder's coefficient-form plaintext of v repeated over the slots; ntt_limbs: to its NTT form, in place
inline HostPlain encode_host(const HostContext &hc, const std::vector<double> &v, double scale, uint32_t limbs) {
  const size_t slots = hc.N / 2;
  HostPlain pt;
  pt.limbs = limbs;
  pt.scale = scale;
  pt.data.resize((size_t)limbs * hc.N);
  std::vector<double> vec(slots);
  for (size_t r = 0; r < slots / v.size(); r++) std::copy(v.begin(), v.end(), vec.begin() + r * v.size());
  hc.encode_coeff(vec.data(), scale, limbs, pt.data.data());
  return pt;
}
inline void ntt_limbs(const HostContext &hc, HostPlain &pt) {
  for (uint32_t i = 0; i < pt.limbs; i++) hc.ntt(i, pt.data.data() + (size_t)i * hc.N);
}
// a Plain input encoded, a raw one passed through; false for a Cipher input, which is the caller's to encrypt
inline bool unencrypted_value(const HostContext &hc, const InputClass &in, const std::vector<double> &v, SchemeValue &out) {
  if (in.kind == Type::Cipher) return false;
  if (in.kind == Type::Plain) {
    HostPlain pt = encode_host(hc, v, in.scale, in.limbs);
    ntt_limbs(hc, pt);
    out = std::move(pt);
  } else {
    out = v;
  }
  return true;
}

// EVA_DEVICE_CLIENT=0 keeps the client calls on the host; without a HIP device the host path is the only one
// (encrypt and decrypt, unlike execute(), are client-side work the reference also does on the CPU)
inline bool device_client_enabled() {
  const char *e = std::getenv("EVA_DEVICE_CLIENT");
  int n = 0;
  return (!e || std::atoi(e) != 0) && evah_device_count(&n) == 0 && n > 0;
}

// the bound of HipExecutor::device_encodable — every rounded coefficient below 2^62 and inside the modulus — behind
// EVA_DEVICE_ENCODE, which the executor reads once when it is made and the client at every call
// T: the type the n values are held in (double; float and uint8_t rows of encrypt_array), each read as the double it
// converts to exactly
template <class T> inline bool device_encodable(const HostContext &hc, const T *in, size_t n, double scale, uint32_t limbs) {
  const size_t slots = hc.N / 2;
  if (std::getenv("EVA_DEVICE_ENCODE") && !std::atoi(std::getenv("EVA_DEVICE_ENCODE"))) return false;
  if (n == 0 || n > slots || slots % n) return false;
  double sum = 0;
  for (size_t i = 0; i < n; i++) {
    const double x = (double)in[i];
    if (!std::isfinite(x)) return false;
    sum += std::fabs(x);
  }
  const double bound = 2.0 * sum * (double)(slots / n) * scale / (double)hc.N;
  const int bits = (int)std::ceil(std::log2(std::max(bound, 1.0))) + 1;
  return bits < 62 && bits < hc.total_bits[limbs];
}
inline bool device_encodable(const HostContext &hc, const std::vector<double> &in, double scale, uint32_t limbs) {
  return device_encodable(hc, in.data(), in.size(), scale, limbs);
}
// the same rule on a row's sum of absolute values, for rows the host does not hold (evah_rows_abs_sum_dev, DESIGN.md
// 1.11): a NaN or an infinity in the row left the sum non-finite
inline bool device_encodable_sum(const HostContext &hc, double sum, size_t n, double scale, uint32_t limbs) {
  const size_t slots = hc.N / 2;
  if (std::getenv("EVA_DEVICE_ENCODE") && !std::atoi(std::getenv("EVA_DEVICE_ENCODE"))) return false;
  if (n == 0 || n > slots || slots % n || !std::isfinite(sum)) return false;
  const double bound = 2.0 * sum * (double)(slots / n) * scale / (double)hc.N;
  const int bits = (int)std::ceil(std::log2(std::max(bound, 1.0))) + 1;
  return bits < 62 && bits < hc.total_bits[limbs];
}

// A device handle as a value: resident (it stays in HBM, host words on demand) or downloaded.  seed: the value is
// seeded — the seed stays with it, so that save() can still write the value compressed, and only c0
// crosses PCIe: c1 is the seed's.
inline HostCipher cipher_of_handle(const std::shared_ptr<DeviceCtx> &dev, const HostContext &hc, evah_ct *h, uint32_t limbs, double scale,
                                   bool resident, const std::array<uint8_t, 32> *seed = nullptr) {
  auto handle = std::make_shared<CtHandle>(dev->h, h);
  HostCipher out;
  out.size = 2;
  out.limbs = limbs;
  out.scale = scale;
  out.words_checked = seed || !resident;
  std::shared_ptr<SeededForm> sf;
  if (seed) {
    sf = std::make_shared<SeededForm>();
    sf->seed = *seed;
    sf->N = hc.N;
    sf->primes.assign(hc.primes.begin(), hc.primes.begin() + limbs);
  }
  if (resident) {
    out.dev = std::make_shared<DeviceResident>(DeviceResident{dev, nullptr, handle, hc.N});
  } else if (sf) {
    sf->c0.resize((size_t)limbs * hc.N);
    chk(evah_ct_download_poly(dev->h, h, 0, (uint64_t *)sf->c0.data()));
  } else {
    out.data.resize((size_t)2 * limbs * hc.N);
    chk(evah_ct_download(dev->h, h, (uint64_t *)out.data.data()));
  }
  out.seeded = std::move(sf);
  return out;
}
// the instances of a batched handle as values: views that share its allocation, which lives until the last one is freed
inline std::vector<HostCipher> group_results(const std::shared_ptr<DeviceCtx> &dev, const HostContext &hc, evah_ct *c, size_t B, uint32_t limbs,
                                             double scale, bool resident, const std::array<uint8_t, 32> *seeds = nullptr) {
  CtHandle group(dev->h, c);
  std::vector<HostCipher> out(B);
  for (size_t b = 0; b < B; b++) {
    evah_ct *view = nullptr;
    chk(evah_ct_unstack(dev->h, c, (uint32_t)b, &view));
    out[b] = cipher_of_handle(dev, hc, view, limbs, scale, resident, seeds ? seeds + b : nullptr);
  }
  return out;
}
// the device calls of an encrypt_batch: the instances of input `name` in groups of <= 64, fn(the group's values, its
// first instance) returning the group's ciphertexts
template <class F> void encrypt_in_groups(const std::vector<Valuation> &inputs, const std::string &name, std::vector<HipValuation> &out, F fn) {
  for (size_t b0 = 0; b0 < inputs.size(); b0 += CLIENT_BATCH_MAX) {
    const size_t n = std::min<size_t>(CLIENT_BATCH_MAX, inputs.size() - b0);
    std::vector<const std::vector<double> *> vals(n);
    for (size_t b = 0; b < n; b++) vals[b] = &inputs[b0 + b].at(name);
    std::vector<HostCipher> cts = fn(vals, b0);
    for (size_t b = 0; b < n; b++) out[b0 + b].values[name] = std::move(cts[b]);
  }
}
inline std::vector<double> flatten(const std::vector<const std::vector<double> *> &vals) {
  const size_t nv = vals[0]->size();
  std::vector<double> flat(vals.size() * nv);
  for (size_t b = 0; b < vals.size(); b++) std::copy(vals[b]->begin(), vals[b]->end(), flat.begin() + b * nv);
  return flat;
}
struct WipeOnExit {
  std::vector<int8_t> &s;
  ~WipeOnExit() { wipe(s); }
};
// the 32-byte randomness keys of a call, per name (or one row), per instance
struct WipeKeyRows {
  std::vector<std::vector<std::array<uint8_t, 32>>> &k;
  ~WipeKeyRows() { for (auto &n : k) for (auto &x : n) wipe_bytes(x.data(), 32); }
};
// stream k of a client call: keyed from the OS, or (seed != 0) the reproducible test hook — NOT secret-grade
inline std::unique_ptr<SecureRng> client_stream(uint64_t seed, uint64_t k) {
  if (seed) return std::make_unique<SecureRng>(seed, k);
  return std::unique_ptr<SecureRng>(new SecureRng());
}

// ---- the array calls
// What encrypt_array makes of its arguments before anything is drawn: the sorted names of the call with their classes
// (arr[i] set for an encrypted input), B, every check, and the shared values encoded into `out`.  The array path has no
// host twin: a row the device encoder cannot take is an error.
struct ArrayInputs {
  std::vector<std::string> names;
  std::vector<InputClass> cls;
  std::vector<const ArrayView *> arr;
};
// plains: unencrypted inputs of type Raw with a row per instance — copied into the batch in their own type
// devctx: the device state a device array's rows are summed on (one evah_rows_abs_sum_dev per such array, over all B rows)
inline ArrayInputs plan_array_inputs(const HostContext &hc, std::map<std::string, ArrayView> &arrays, const Valuation &shared,
                                     const CKKSSignature &sig, HipValuationBatch &out, const std::map<std::string, ArrayView> &plains = {},
                                     evah_ctx *devctx = nullptr) {
  check_vec_size(sig, hc.N / 2);
  if (arrays.empty()) throw std::invalid_argument("encrypt_array: no encrypted input array was given");
  ArrayInputs in;
  for (auto &kv : arrays) in.names.push_back(kv.first);
  for (auto &kv : shared) {
    if (arrays.count(kv.first)) throw std::invalid_argument("encrypt_array: input " + kv.first + " is given twice");
    in.names.push_back(kv.first);
  }
  std::sort(in.names.begin(), in.names.end());
  out.B = arrays.begin()->second.B;
  if (out.B < 1) throw std::invalid_argument("encrypt_array: input " + arrays.begin()->first + " has no instances");
  for (const std::string &name : in.names) {
    const InputClass c = classify_input(hc, sig, name);
    auto it = arrays.find(name);
    if (it == arrays.end()) {
      if (c.kind == Type::Cipher) throw std::invalid_argument("encrypt_array: encrypted input " + name + " needs an array [B, n], one row per instance");
      const auto &v = shared.at(name);
      check_input_size(v, sig);
      unencrypted_value(hc, c, v, out.shared[name]);
    } else {
      ArrayView &a = it->second;
      if (c.kind != Type::Cipher) throw std::invalid_argument("encrypt_array: input " + name + " is not encrypted: it is one value shared by all instances");
      if (a.n != (size_t)sig.vec_size) throw std::runtime_error("Input size does not match program vector size (input " + name + ")");
      if (a.B != out.B)
        throw std::invalid_argument("encrypt_array: input " + name + " has " + std::to_string(a.B) + " instances, " + arrays.begin()->first + " has " +
                                    std::to_string(out.B));
      if (a.on_device) { // the rows stay where they are: their sums come to the host, 8 bytes a row
        if (!devctx) throw std::logic_error("encrypt_array: a device array needs the device state");
        if (a.B > 0xffffffffull) throw std::invalid_argument("encrypt_array: input " + name + " has too many instances");
        a.sums = std::make_shared<std::vector<double>>(a.B);
        chk(evah_rows_abs_sum_dev(devctx, (uint32_t)a.B, a.data, a.dtype, a.row_pitch(), a.producer, (uint32_t)a.n, a.sums->data()));
      }
      for (size_t b = 0; b < a.B; b++) {
        const bool ok = a.on_device           ? device_encodable_sum(hc, (*a.sums)[b], a.n, c.scale, c.limbs)
                        : a.dtype == EVAH_F64 ? device_encodable(hc, static_cast<const double *>(a.row(b)), a.n, c.scale, c.limbs)
                        : a.dtype == EVAH_F32 ? device_encodable(hc, static_cast<const float *>(a.row(b)), a.n, c.scale, c.limbs)
                                              : device_encodable(hc, static_cast<const uint8_t *>(a.row(b)), a.n, c.scale, c.limbs);
        if (!ok)
          throw std::runtime_error("encrypt_array: input " + name + ", instance " + std::to_string(b) +
                                   ": the device encoder cannot take these values (non-finite, too large for the scale, or EVA_DEVICE_ENCODE=0); "
                                   "encrypt_batch has a host path for them");
      }
    }
    in.cls.push_back(c);
    in.arr.push_back(it == arrays.end() ? nullptr : &it->second);
  }
  for (auto &kv : plains) {
    const std::string &name = kv.first;
    const ArrayView &a = kv.second;
    if (arrays.count(name) || shared.count(name)) throw std::invalid_argument("encrypt_array: input " + name + " is given twice");
    const InputClass c = classify_input(hc, sig, name);
    if (c.kind != Type::Raw) throw std::invalid_argument("encrypt_array: plain_arrays takes unencrypted inputs of type Raw, input " + name + " is not one");
    if (a.n != (size_t)sig.vec_size) throw std::runtime_error("Input size does not match program vector size (input " + name + ")");
    if (a.B != out.B)
      throw std::invalid_argument("encrypt_array: input " + name + " has " + std::to_string(a.B) + " instances, " + arrays.begin()->first + " has " +
                                  std::to_string(out.B));
    if (a.on_device) throw std::invalid_argument("encrypt_array: plain_arrays stays on the host, input " + name + " is a device array");
    PlainRows pr;
    const uint8_t *src = static_cast<const uint8_t *>(a.data);
    pr.bytes = std::make_shared<std::vector<uint8_t>>(src, src + a.B * a.n * a.itemsize());
    pr.view = a;
    pr.view.data = pr.bytes->data();
    out.plains[name] = std::move(pr);
  }
  return in;
}
inline void require_array_path(bool on_device, bool resident, const std::string &call = "encrypt_array") {
  if (!on_device) throw std::runtime_error(call + " needs a HIP device: none is visible, or EVA_DEVICE_CLIENT=0 keeps the client on the host");
  if (!resident) throw std::runtime_error(call + " needs resident valuations: resident = False (EVA_RESIDENT=0) keeps them on the host");
}
inline std::vector<uint8_t> keys_flat(const std::array<uint8_t, 32> *keys, size_t n) {
  std::vector<uint8_t> flat(n * 32);
  for (size_t b = 0; b < n; b++) std::copy(keys[b].begin(), keys[b].end(), flat.begin() + b * 32);
  return flat;
}
// bytes of a row of n decoded values of dtype (EVAH_F64 / EVAH_F32 / EVAH_U8), as decrypt_array and combine_shares write them
inline size_t row_bytes(int dtype, size_t n) { return n * (dtype == EVAH_F32 ? 4 : dtype == EVAH_U8 ? 1 : 8); }

// ---- what the calls that consume handles share: one shape check, one way from a value to a handle the device reads, one
// walk over a name's segments
// A ciphertext of min_size .. max_size polynomials whose limb count fits the chain and whose words number size * limbs * N:
// host words are counted; a value that is only resident has the device's own, size * limbs * dev->N of them, so its
// degree is compared instead and nothing is downloaded.  label: "output NAME", "value NAME", "rekey: value NAME" — every
// call keeps the prefix it always had.
inline void check_cipher_shape(const HostContext &hc, const std::string &label, const HostCipher &c, uint32_t min_size, uint32_t max_size) {
  if (c.size < min_size || c.size > max_size || c.limbs < 1 || c.limbs > hc.k - 1 ||
      (!resident_only(c) && words(c).size() != (size_t)c.size * c.limbs * hc.N) || (c.dev && c.dev->N != hc.N))
    throw std::runtime_error(label + ": ciphertext shape does not match its data or the encryption parameters");
}
// a handle of another GPU, copied to dev; keep owns the copy
inline const evah_ct *copy_over(const std::shared_ptr<DeviceCtx> &dev, const evah_ct *src, std::vector<CtHandle> &keep) {
  evah_ct *h = nullptr;
  chk(evah_ct_copy(dev->h, src, &h));
  keep.emplace_back(dev->h, h);
  return h;
}
// which resident values a call reads where they are
enum class InPlace {
  SameState, // decrypt, decrypt_batch (1.6), refresh (1.12), a list given to decrypt_array (kept as found): the call's own device state
  SameGpu,   // rekey, decrypt_share (1.14), combine_shares (kept as found): any device state of the call's GPU
};
// how every other value comes to the call's device
enum class BringOver {
  Upload, // decrypt, decrypt_batch, refresh, decrypt_array's list, decrypt_share: its words from the host (downloaded first where it is resident elsewhere)
  Copy,   // rekey, combine_shares (kept as found): resident on another GPU — evah_ct_copy; host words — uploaded
};
// One value as a handle dev reads, its shape checked first (1 .. 3 polynomials; the calls that take size 2 alone have
// refused every other size, in their own words, before they come here).  keep owns what was made for the call.
inline const evah_ct *source_handle(const std::shared_ptr<DeviceCtx> &dev, const HostContext &hc, const std::string &label, const HostCipher &c,
                                    std::vector<CtHandle> &keep, InPlace rule, BringOver how) {
  check_cipher_shape(hc, label, c, 1, 3);
  if (c.dev && (rule == InPlace::SameState ? c.dev->root == dev : c.dev->root->device == dev->device)) return c.dev->h->h;
  if (c.dev && how == BringOver::Copy) return copy_over(dev, c.dev->h->h, keep);
  evah_ct *h = nullptr;
  chk(evah_ct_upload(dev->h, c.size, c.limbs, c.scale, (const uint64_t *)words(c).data(), &h));
  keep.emplace_back(dev->h, h);
  return h;
}
// The walk over the segments of one name of a batch, for decrypt_array, refresh, decrypt_share, rekey and
// combine_shares: consecutive segments of one size, limb count and scale are packed into groups of <= 64 instances, and fn
// makes its one device call per group.  The walk refuses, under label ("output NAME" / "value NAME"): a segment of more
// than 64 instances; segments that hold more instances than the batch — before fn sees the group, so no row past the
// caller's array is written; and, at the end, segments that do not hold every instance.  A batch on another GPU than dev
// (rekey, decrypt_share, combine_shares; the others require root == dev) is copied over group by group.
// One grouping rule for all five.  decrypt_share and combine_shares take size 2 alone, so for them it is (limbs, scale), as
// before.  rekey grouped by limbs alone: the rule could only split a group whose segments share limbs and differ in scale,
// which changes no word (evah_rekey_many treats every handle independently) and which no public call can build — batches
// come from encrypt_array, execute_batch, refresh and rekey, all uniform per name.
struct SegmentGroup {
  size_t s0 = 0, s1 = 0, row = 0, n = 0; // segments [s0, s1): instances [row, row + n) of the batch
  std::vector<const evah_ct *> hs;       // a handle per segment
  std::vector<CtHandle> keep;            // owns the group's copies, and what fn adds, until the group is done
};
template <class F>
void walk_segments(const std::string &label, const std::vector<BatchSegment> &segs, size_t B, const std::shared_ptr<DeviceCtx> &dev,
                   const std::shared_ptr<DeviceCtx> &root, F fn) {
  const bool same_gpu = root->device == dev->device;
  size_t row = 0;
  for (size_t s0 = 0; s0 < segs.size();) {
    SegmentGroup g;
    g.s0 = g.s1 = s0;
    g.row = row;
    while (g.s1 < segs.size() && g.n + segs[g.s1].n <= CLIENT_BATCH_MAX && segs[g.s1].size == segs[s0].size && segs[g.s1].limbs == segs[s0].limbs &&
           segs[g.s1].scale == segs[s0].scale) {
      g.hs.push_back(same_gpu ? segs[g.s1].h->h : copy_over(dev, segs[g.s1].h->h, g.keep));
      g.n += segs[g.s1++].n;
    }
    if (g.s1 == s0) throw std::runtime_error(label + ": a segment holds more than 64 instances");
    if (row + g.n > B) throw std::runtime_error(label + ": the segments hold more instances than the batch");
    fn(g);
    row += g.n;
    s0 = g.s1;
  }
  if (row != B) throw std::runtime_error(label + ": the segments do not hold every instance");
}
// instance b of a batch as an ordinary valuation: every ciphertext a view of its segment (evah_ct_unstack), a symmetric
// one with its seed, so that save() still writes it compressed — the bridge to decrypt, save and execute
inline HipValuation batch_instance(const HipValuationBatch &vb, size_t b) {
  if (b >= vb.B) throw std::out_of_range("instance index out of range");
  HipValuation out;
  out.params = vb.params;
  out.values = vb.shared;
  for (auto &kv : vb.plains) out.values[kv.first] = array_row_doubles(kv.second.view, b); // row b as an ordinary raw value
  for (auto &kv : vb.ciphers) {
    size_t first = 0;
    for (const BatchSegment &s : kv.second.segments) {
      if (b >= first + s.n) { first += s.n; continue; }
      evah_ctx *ctx = s.queue ? s.queue->h : vb.root->h;
      evah_ct *view = nullptr;
      chk(evah_ct_unstack(ctx, s.h->h, (uint32_t)(b - first), &view));
      HostCipher c;
      c.size = s.size;
      c.limbs = s.limbs;
      c.scale = s.scale;
      c.dev = std::make_shared<DeviceResident>(DeviceResident{vb.root, s.queue, std::make_shared<CtHandle>(ctx, view), vb.params->N});
      if (!kv.second.seeds.empty()) {
        auto sf = std::make_shared<SeededForm>();
        sf->seed = kv.second.seeds[b];
        sf->N = vb.params->N;
        sf->primes.assign(vb.params->primes.begin(), vb.params->primes.begin() + s.limbs);
        c.seeded = std::move(sf);
        c.words_checked = true;
      }
      out.values[kv.first] = std::move(c);
      break;
    }
  }
  return out;
}
// a list of valuations as a batch on `dev`: a ciphertext resident there is a segment of one that shares its handle, any
// other is uploaded first (as decrypt() does); plaintexts and raw vectors are taken from instance 0
inline HipValuationBatch batch_of_list(const std::vector<const HipValuation *> &list, const std::shared_ptr<DeviceCtx> &dev,
                                       const std::shared_ptr<HostContext> &host) {
  HipValuationBatch vb;
  vb.B = list.size();
  vb.root = dev;
  vb.params = host;
  for (size_t b = 0; b < list.size(); b++) {
    if (!list[b]) throw std::invalid_argument("valuation " + std::to_string(b) + " is None");
    for (auto &kv : list[b]->values) {
      auto *c = std::get_if<HostCipher>(&kv.second);
      if (!c) {
        if (b == 0) vb.shared[kv.first] = kv.second;
        continue;
      }
      BatchCipher &bc = vb.ciphers[kv.first];
      if (bc.segments.size() != b) throw std::runtime_error("value " + kv.first + " is not a ciphertext in every valuation of the list");
      BatchSegment s;
      s.n = 1;
      s.size = c->size;
      s.limbs = c->limbs;
      s.scale = c->scale;
      if (c->dev && c->dev->root == dev) {
        s.h = c->dev->h;
        s.queue = c->dev->queue;
      } else { // the segment owns the upload
        std::vector<CtHandle> keep;
        source_handle(dev, *host, "value " + kv.first, *c, keep, InPlace::SameState, BringOver::Upload);
        s.h = std::make_shared<CtHandle>(std::move(keep.back()));
      }
      bc.segments.push_back(std::move(s));
    }
  }
  for (auto &kv : vb.ciphers)
    if (kv.second.segments.size() != vb.B) throw std::runtime_error("value " + kv.first + " is not a ciphertext in every valuation of the list");
  // a raw value that is not the same in every valuation keeps a row per instance
  for (auto it = vb.shared.begin(); it != vb.shared.end();) {
    const auto *r0 = std::get_if<std::vector<double>>(&it->second);
    bool rows = false;
    if (r0) {
      bool everywhere = true; // (a list whose later valuations lack the value keeps instance 0's, as before)
      for (size_t b = 1; b < list.size() && everywhere; b++) {
        auto f = list[b]->values.find(it->first);
        const auto *rb = f == list[b]->values.end() ? nullptr : std::get_if<std::vector<double>>(&f->second);
        everywhere = rb && rb->size() == r0->size();
        rows = rows || (everywhere && *rb != *r0);
      }
      rows = rows && everywhere;
    }
    if (!rows) { ++it; continue; }
    PlainRows pr;
    pr.bytes = std::make_shared<std::vector<uint8_t>>(list.size() * r0->size() * sizeof(double));
    for (size_t b = 0; b < list.size(); b++) {
      const auto &rb = std::get<std::vector<double>>(list[b]->values.at(it->first));
      std::memcpy(pr.bytes->data() + b * rb.size() * sizeof(double), rb.data(), rb.size() * sizeof(double));
    }
    pr.view = ArrayView{pr.bytes->data(), EVAH_F64, list.size(), r0->size()};
    vb.plains[it->first] = std::move(pr);
    it = vb.shared.erase(it);
  }
  return vb;
}
// u, e0, e1 of one public-key encryption from rng, in evahost::encrypt's order, as int8 [3][N] at small
inline void draw_small3(const HostContext &hc, SecureRng &rng, int8_t *small) {
  std::vector<int8_t> u, e0, e1;
  hc.sample_ternary(rng, u);
  hc.sample_error(rng, e0);
  hc.sample_error(rng, e1);
  std::copy(u.begin(), u.end(), small);
  std::copy(e0.begin(), e0.end(), small + hc.N);
  std::copy(e1.begin(), e1.end(), small + 2 * (size_t)hc.N);
  wipe(u); wipe(e0); wipe(e1);
}

// SEALPublic::encrypt (seal.cpp:24-102)
inline HipValuation HipPublic::encrypt(const Valuation &inputs, const CKKSSignature &sig) {
  check_vec_size(sig, host->N / 2);
  HipValuation out;
  SecureRng rng; // a fresh ChaCha20 stream keyed with 256 bits from the OS for this call (csprng.h)
  for (auto &kv : inputs) {
    const auto &v = kv.second;
    check_input_size(v, sig);
    const InputClass in = classify_input(*host, sig, kv.first);
    if (unencrypted_value(*host, in, v, out.values[kv.first])) continue;
    // the encoders consume no randomness: the draws come first on every path, hence the same ciphertext on each
    std::vector<int8_t> small((size_t)3 * host->N);
    WipeOnExit wipe_small{small};
    draw_small3(*host, rng, small.data());
    out.values[kv.first] = encrypt_value_with(v, in.scale, in.limbs, small);
  }
  return out;
}

inline bool HipPublic::client_on_device() {
  if (client_device < 0) client_device = device_client_enabled() ? 1 : 0;
  return client_device == 1;
}
inline void HipPublic::ensure_public_key() {
  ensure_device(false);
  if (!pk_uploaded) {
    chk(evah_client_key_upload(dev->h, EVAH_KEY_PUBLIC, (const uint64_t *)pk.data.data()));
    pk_uploaded = true;
  }
}

// coeff_pt: the host encoder's coefficient-form plaintext, or (null) values: the slot values for the device encoder
// (evah_pt_encode: the plaintext never exists on the host, and is the host encoder's bit for bit,
// tests/test_encode_parity.py); then evah_encrypt with small = (u, e0, e1) as int8 [3][N]
inline HostCipher HipPublic::encrypt_on_device_with(const HostPlain *coeff_pt, const std::vector<double> *values, double scale, uint32_t limbs,
                                                    const std::vector<int8_t> &small) {
  ensure_public_key();
  evah_pt *p = nullptr;
  if (coeff_pt) chk(evah_pt_upload_coeff(dev->h, limbs, scale, (const uint64_t *)coeff_pt->data.data(), &p));
  else chk(evah_pt_encode(dev->h, values->data(), (uint32_t)values->size(), limbs, scale, &p));
  evah_ct *c = nullptr;
  int rc = evah_encrypt(dev->h, p, small.data(), &c);
  evah_pt_free(dev->h, p);
  chk(rc);
  return cipher_of_handle(dev, *host, c, limbs, scale, resident);
}

// the Cipher branch of encrypt() for one input, the randomness given: device encoder + encryptor, host encoder + device
// encryptor (the per-limb transforms, the public-key products and the mod-down on the GPU), or the host alone — the same
// words on each
inline HostCipher HipPublic::encrypt_value_with(const std::vector<double> &v, double scale, uint32_t limbs, const std::vector<int8_t> &small) {
  if (client_on_device() && device_encodable(*host, v, scale, limbs)) return encrypt_on_device_with(nullptr, &v, scale, limbs, small);
  HostPlain pt = encode_host(*host, v, scale, limbs);
  if (client_on_device()) return encrypt_on_device_with(&pt, nullptr, scale, limbs, small);
  ntt_limbs(*host, pt);
  const size_t N = host->N;
  std::vector<int8_t> u(small.begin(), small.begin() + N), e0(small.begin() + N, small.begin() + 2 * N), e1(small.begin() + 2 * N, small.end());
  HostCipher out = evahost::encrypt(*host, pk, pt, u, e0, e1);
  wipe(u); wipe(e0); wipe(e1);
  return out;
}

// encrypt() for a list of input valuations of one signature.  Per input name the instances leave in
// groups of <= 64 as ONE evah_encode_encrypt_many each — a launch set whose length does not depend on the group — and
// come back as views of the group's handle (evah_ct_unstack).  A name with an instance the device encoder cannot take,
// plain and raw inputs, and every input without a device take encrypt()'s path per instance.
// device_sampling: all draws first — instances in list order, names sorted within an instance, one 32-byte
// randomness key (4 words) per encrypted input — then the groups go out as evah_encode_encrypt_sampled_many, and every
// other path expands the same keys with the host twin.
inline std::vector<HipValuation> HipPublic::encrypt_batch(const std::vector<Valuation> &inputs, const CKKSSignature &sig, bool device_sampling,
                                                          uint64_t seed) {
  if (seed && !device_sampling) throw std::invalid_argument("encrypt_batch: seed is the test hook of device_sampling and needs device_sampling=True");
  check_vec_size(sig, host->N / 2);
  std::vector<HipValuation> out(inputs.size());
  if (inputs.empty()) return out;
  const std::vector<std::string> names = batch_input_names(inputs);
  auto per_instance = [&](const std::string &name) { // encrypt()'s path, instance by instance
    for (size_t b = 0; b < inputs.size(); b++) {
      HipValuation one = encrypt(Valuation{{name, inputs[b].at(name)}}, sig);
      out[b].values[name] = std::move(one.values.at(name));
    }
  };
  if (device_sampling) {
    std::unique_ptr<SecureRng> stream = client_stream(seed, 5);
    std::vector<std::vector<std::array<uint8_t, 32>>> rkeys(names.size()); // per name, per instance
    WipeKeyRows wipe_keys{rkeys};
    std::vector<InputClass> cls;
    for (const std::string &name : names) cls.push_back(classify_input(*host, sig, name));
    for (size_t b = 0; b < inputs.size(); b++)
      for (size_t i = 0; i < names.size(); i++) {
        check_input_size(inputs[b].at(names[i]), sig);
        if (cls[i].kind == Type::Cipher) rkeys[i].push_back(draw_key32(*stream));
      }
    for (size_t i = 0; i < names.size(); i++) {
      const std::string &name = names[i];
      const uint32_t limbs = cls[i].limbs;
      const double scale = cls[i].scale;
      if (cls[i].kind != Type::Cipher) { // plain and raw inputs take no randomness
        per_instance(name);
        continue;
      }
      bool grouped = client_on_device();
      for (size_t b = 0; grouped && b < inputs.size(); b++) grouped = device_encodable(*host, inputs[b].at(name), scale, limbs);
      if (!grouped) { // the same keys through the host twin, instance by instance
        for (size_t b = 0; b < inputs.size(); b++) {
          std::vector<int8_t> small = sampled_small3(rkeys[i][b], host->N);
          WipeOnExit wipe_small{small};
          out[b].values[name] = encrypt_value_with(inputs[b].at(name), scale, limbs, small);
        }
        continue;
      }
      encrypt_in_groups(inputs, name, out, [&](const std::vector<const std::vector<double> *> &vals, size_t b0) {
        return encrypt_group_sampled(vals, scale, limbs, rkeys[i].data() + b0);
      });
    }
    return out;
  }
  SecureRng rng; // one fresh ChaCha20 stream keyed from the OS for the whole call
  for (const std::string &name : names) {
    const InputClass in = classify_input(*host, sig, name);
    bool grouped = in.kind == Type::Cipher && client_on_device();
    for (size_t b = 0; b < inputs.size(); b++) {
      const auto &v = inputs[b].at(name);
      check_input_size(v, sig);
      if (grouped && !device_encodable(*host, v, in.scale, in.limbs)) grouped = false;
    }
    if (!grouped) {
      per_instance(name);
      continue;
    }
    encrypt_in_groups(inputs, name, out, [&](const std::vector<const std::vector<double> *> &vals, size_t) {
      return encrypt_group_on_device(vals, in.scale, in.limbs, rng);
    });
  }
  return out;
}

// one group of encrypt_batch: encrypt()'s sampler calls per instance, in list order, then one device call
inline std::vector<HostCipher> HipPublic::encrypt_group_on_device(const std::vector<const std::vector<double> *> &vals, double scale,
                                                                  uint32_t limbs, SecureRng &rng) {
  ensure_public_key();
  const size_t B = vals.size(), N = host->N;
  const std::vector<double> flat = flatten(vals);
  std::vector<int8_t> small(B * 3 * N);
  WipeOnExit wipe_small{small};
  for (size_t b = 0; b < B; b++) draw_small3(*host, rng, small.data() + 3 * b * N);
  evah_ct *c = nullptr;
  chk(evah_encode_encrypt_many(dev->h, (uint32_t)B, flat.data(), (uint32_t)vals[0]->size(), limbs, scale, small.data(), &c));
  return group_results(dev, *host, c, B, limbs, scale, resident);
}

// the same as one evah_encode_encrypt_sampled_many: instance b's randomness is drawn on the device from rkeys[b]
inline std::vector<HostCipher> HipPublic::encrypt_group_sampled(const std::vector<const std::vector<double> *> &vals, double scale, uint32_t limbs,
                                                                const std::array<uint8_t, 32> *rkeys) {
  ensure_public_key();
  const size_t B = vals.size();
  const std::vector<double> flat = flatten(vals);
  std::vector<uint8_t> keys(B * 32);
  for (size_t b = 0; b < B; b++) std::copy(rkeys[b].begin(), rkeys[b].end(), keys.begin() + b * 32);
  evah_ct *c = nullptr;
  const int rc = evah_encode_encrypt_sampled_many(dev->h, (uint32_t)B, flat.data(), (uint32_t)vals[0]->size(), limbs, scale, keys.data(), &c);
  wipe_bytes(keys.data(), keys.size());
  chk(rc);
  return group_results(dev, *host, c, B, limbs, scale, resident);
}

// encrypt_batch(..., device_sampling = true, seed) for arrays [B][n] in the caller's own type: the same
// draws in the same order — instances in order, names sorted within an instance, one 32-byte randomness key per
// encrypted input — so instance b is encrypt_batch's instance b word for word.  Per name the rows leave in segments of
// <= 64 as ONE evah_encode_encrypt_array each, in the array's type, and the batched handles are kept whole.  Device and
// resident valuations only: there is no host path behind this call.
inline HipValuationBatch HipPublic::encrypt_array(const std::map<std::string, ArrayView> &arrays_in, const Valuation &shared, const CKKSSignature &sig,
                                                  uint64_t seed, const std::map<std::string, ArrayView> &plains) {
  require_array_path(client_on_device(), resident);
  HipValuationBatch out;
  out.params = host;
  std::map<std::string, ArrayView> arrays = arrays_in; // (plan_array_inputs attaches the sums of a device array to its view)
  ensure_public_key(); // (before the checks: a device array's rows are summed on the device state)
  const ArrayInputs in = plan_array_inputs(*host, arrays, shared, sig, out, plains, dev->h);
  out.root = dev;
  std::unique_ptr<SecureRng> stream = client_stream(seed, 5);
  std::vector<std::vector<std::array<uint8_t, 32>>> rkeys(in.names.size()); // per name, per instance
  WipeKeyRows wipe_keys{rkeys};
  for (size_t b = 0; b < out.B; b++)
    for (size_t i = 0; i < in.names.size(); i++)
      if (in.arr[i]) rkeys[i].push_back(draw_key32(*stream));
  for (size_t i = 0; i < in.names.size(); i++) {
    if (!in.arr[i]) continue;
    const ArrayView &a = *in.arr[i];
    BatchCipher &bc = out.ciphers[in.names[i]];
    for (size_t b0 = 0; b0 < out.B; b0 += CLIENT_BATCH_MAX) {
      const size_t n = std::min<size_t>(CLIENT_BATCH_MAX, out.B - b0);
      std::vector<uint8_t> keys = keys_flat(rkeys[i].data() + b0, n);
      evah_ct *c = nullptr;
      const int rc = a.on_device ? evah_encode_encrypt_array_dev(dev->h, (uint32_t)n, a.row(b0), a.dtype, a.row_pitch(), a.producer, a.sums->data() + b0,
                                                                 (uint32_t)a.n, in.cls[i].limbs, in.cls[i].scale, keys.data(), &c)
                                 : evah_encode_encrypt_array(dev->h, (uint32_t)n, a.row(b0), a.dtype, (uint32_t)a.n, in.cls[i].limbs, in.cls[i].scale,
                                                             keys.data(), &c);
      wipe_bytes(keys.data(), keys.size());
      chk(rc);
      bc.segments.push_back(BatchSegment{std::make_shared<CtHandle>(dev->h, c), (uint32_t)n, nullptr, 2, in.cls[i].limbs, in.cls[i].scale});
    }
  }
  return out;
}

// ---- re-key to this key pair
// what differs between a re-key key's parameters and a context's, or "" — the two key pairs share N and the prime list
inline std::string rekey_params_differ(uint32_t N, const std::vector<u64> &primes, const HostContext &hc) {
  if (N != hc.N) return "poly_modulus_degree differs (" + std::to_string(N) + " against " + std::to_string(hc.N) + ")";
  if (primes.size() != hc.primes.size())
    return "the number of primes differs (" + std::to_string(primes.size()) + " against " + std::to_string(hc.primes.size()) + ")";
  for (size_t i = 0; i < primes.size(); i++)
    if (primes[i] != hc.primes[i]) return "prime " + std::to_string(i) + " differs (" + std::to_string(primes[i]) + " against " + std::to_string(hc.primes[i]) + ")";
  return "";
}
inline uint32_t HipPublic::install_rekey_key(const std::shared_ptr<const RekeyKey> &rk) {
  if (!rk) throw std::invalid_argument("rekey: the re-key key is None");
  for (auto &kv : rekey_slots)
    if (kv.first == rk) return kv.second;
  const std::string diff = rekey_params_differ(rk->N, rk->primes, *host);
  if (!diff.empty()) throw std::invalid_argument("rekey: the re-key key was made for other encryption parameters: " + diff);
  if (rk->n_digits == 0 || rk->n_digits > host->k - 1 || rk->data.size() != (size_t)rk->n_digits * 2 * host->k * host->N)
    throw std::invalid_argument("rekey: the re-key key's words do not match its shape");
  // evaluator work, like execute(): EVA_DEVICE_CLIENT does not apply; without a device ensure_device() fails by name
  if (!resident) throw std::runtime_error("rekey needs resident valuations: resident = False (EVA_RESIDENT=0) keeps them on the host");
  ensure_device(false);
  const uint32_t slot = (uint32_t)rekey_slots.size();
  chk(evah_key_upload(dev->h, EVAH_KEY_REKEY, slot, rk->n_digits, (const uint64_t *)rk->data.data()));
  rekey_slots.emplace_back(rk, slot);
  return slot;
}
inline HipValuation HipPublic::rekey(const HipValuation &enc, const std::shared_ptr<const RekeyKey> &rk) {
  for (auto &kv : enc.values) // (before anything is uploaded)
    if (auto *c = std::get_if<HostCipher>(&kv.second))
      if (c->size != 2) throw std::invalid_argument("rekey: value " + kv.first + ": re-key expects a size-2 ciphertext (relinearize first)");
  const uint32_t slot = install_rekey_key(rk);
  if (enc.params && !rekey_params_differ(enc.params->N, enc.params->primes, *host).empty())
    throw std::invalid_argument("rekey: the valuation belongs to other encryption parameters: " + rekey_params_differ(enc.params->N, enc.params->primes, *host));
  HipValuation out;
  out.params = host;
  for (auto &kv : enc.values) {
    const HostCipher *c = std::get_if<HostCipher>(&kv.second);
    if (!c) { // unencrypted and raw values pass through
      out.values[kv.first] = kv.second;
      continue;
    }
    std::vector<CtHandle> keep; // resident on this GPU: in place; on another GPU: copied over; host words: uploaded
    const evah_ct *h = source_handle(dev, *host, "rekey: value " + kv.first, *c, keep, InPlace::SameGpu, BringOver::Copy);
    evah_ct *o = nullptr;
    chk(evah_rekey_many(dev->h, slot, &h, 1, &o));
    out.values[kv.first] = cipher_of_handle(dev, *host, o, c->limbs, c->scale, /*resident=*/true);
  }
  return out;
}
inline HipValuationBatch HipPublic::rekey_batch(const HipValuationBatch &vb, const std::shared_ptr<const RekeyKey> &rk) {
  for (auto &nc : vb.ciphers)
    for (auto &seg : nc.second.segments)
      if (seg.size != 2) throw std::invalid_argument("rekey: value " + nc.first + ": re-key expects a size-2 ciphertext (relinearize first)");
  const uint32_t slot = install_rekey_key(rk);
  if (vb.params && !rekey_params_differ(vb.params->N, vb.params->primes, *host).empty())
    throw std::invalid_argument("rekey: the batch belongs to other encryption parameters: " + rekey_params_differ(vb.params->N, vb.params->primes, *host));
  if (!vb.root) throw std::runtime_error("rekey: the batch holds no device handles");
  HipValuationBatch out;
  out.B = vb.B;
  out.params = host;
  out.root = dev;
  out.shared = vb.shared;
  out.plains = vb.plains;
  for (auto &nc : vb.ciphers) {
    const auto &segs = nc.second.segments;
    BatchCipher &bc = out.ciphers[nc.first];
    walk_segments("value " + nc.first, segs, vb.B, dev, vb.root, [&](SegmentGroup &g) {
      std::vector<evah_ct *> outs(g.hs.size(), nullptr);
      chk(evah_rekey_many(dev->h, slot, g.hs.data(), (uint32_t)g.hs.size(), outs.data()));
      for (size_t s = g.s0; s < g.s1; s++)
        bc.segments.push_back(BatchSegment{std::make_shared<CtHandle>(dev->h, outs[s - g.s0]), segs[s].n, nullptr, 2, segs[s].limbs, segs[s].scale});
    });
  }
  return out;
}

// a value of a valuation that is not a ciphertext, as decrypt() returns it: a plaintext decoded, a raw vector expanded
inline std::vector<double> decode_unencrypted(const HostContext &hc, const SchemeValue &value, size_t vec_size) {
  std::vector<double> v;
  if (auto *p = std::get_if<HostPlain>(&value)) {
    std::vector<u64> m = p->data;
    for (uint32_t i = 0; i < p->limbs; i++) hc.intt(i, m.data() + (size_t)i * hc.N);
    hc.decode_coeff(m.data(), p->limbs, p->scale, v);
  } else {
    ConstantValue{std::get<std::vector<double>>(value)}.expand_to(v, vec_size);
  }
  v.resize(vec_size);
  return v;
}
// ---- threshold decryption: the joint opening of a valuation from every party's shares.  No secret key:
// any context over the same parameters runs it.
inline void HipPublic::check_shares(const std::vector<std::shared_ptr<DecryptionShares>> &shares) const {
  if (shares.empty() || shares.size() > 64) throw std::invalid_argument("combine_shares: shares of 1..64 parties are needed");
  for (size_t p = 0; p < shares.size(); p++) {
    const std::string at = "combine_shares: share " + std::to_string(p);
    if (!shares[p]) throw std::invalid_argument(at + " is None");
    const std::string diff = rekey_params_differ(shares[p]->N, shares[p]->primes, *host);
    if (!diff.empty()) throw std::invalid_argument(at + " was made under other encryption parameters: " + diff);
    if (shares[p]->smudge_bits != shares[0]->smudge_bits)
      throw std::invalid_argument(at + ": smudge_bits differs from share 0 (" + std::to_string(shares[p]->smudge_bits) + " against " +
                                  std::to_string(shares[0]->smudge_bits) + ")");
  }
}
// party p's piece for the rows [row, row + n) of value `name` at `limbs` limbs and `scale`; the piece must start there
inline const SharePiece &HipPublic::share_piece(const DecryptionShares &sh, size_t p, const std::string &name, size_t row, size_t n, uint32_t limbs,
                                                double scale) const {
  const std::string at = "combine_shares: share " + std::to_string(p) + ", value " + name;
  auto it = sh.values.find(name);
  if (it == sh.values.end()) throw std::out_of_range(at + ": the share holds no such value");
  size_t r = 0;
  for (const SharePiece &piece : it->second) {
    if (r == row) {
      if (piece.n != n) throw std::invalid_argument(at + ": the instances are packed differently from the valuation's");
      if (piece.limbs != limbs) throw std::invalid_argument(at + ": limb count differs from the ciphertext's");
      if (piece.scale != scale) throw std::invalid_argument(at + ": scale differs from the ciphertext's");
      return piece;
    }
    r += piece.n;
  }
  throw std::invalid_argument(at + ": the instances are packed differently from the valuation's");
}
// the piece as a handle this context's device reads: resident on this GPU — in place; else its words, uploaded
inline const evah_ct *HipPublic::share_handle(const SharePiece &piece, std::vector<CtHandle> &keep) {
  if (piece.h && piece.root->device == dev->device) return piece.h->h;
  const std::vector<u64> &w = words(piece, host->N);
  if (w.size() != (size_t)piece.n * piece.limbs * host->N) throw std::runtime_error("combine_shares: a share's words do not match its shape");
  evah_ct *h = nullptr;
  chk(evah_ct_upload_batch(dev->h, piece.n, 1, piece.limbs, piece.scale, (const uint64_t *)w.data(), &h));
  keep.emplace_back(dev->h, h);
  return h;
}
inline void HipPublic::check_combine_room(const std::string &name, uint32_t limbs, size_t parties, uint32_t smudge_bits) const {
  if (limbs >= 1 && limbs <= host->k - 1 && flood_exceeds_modulus(host->primes, limbs, (uint32_t)parties, smudge_bits))
    throw std::invalid_argument("value " + name + ": smudge_bits leaves no room at this level for this many parties");
}
inline Valuation HipPublic::combine_shares(const HipValuation &enc, const std::vector<std::shared_ptr<DecryptionShares>> &shares, const CKKSSignature &sig) {
  check_shares(shares);
  if (sig.vec_size <= 0) throw std::runtime_error("Signature vector size must be positive");
  const bool on_dev = device_client_enabled();
  if (on_dev) ensure_device(false);
  Valuation out;
  for (auto &kv : enc.values) {
    const HostCipher *c = std::get_if<HostCipher>(&kv.second);
    std::vector<double> v;
    if (!c) { // unencrypted outputs pass through, as in decrypt()
      out[kv.first] = decode_unencrypted(*host, kv.second, (size_t)sig.vec_size);
      continue;
    }
    if (c->size != 2) throw std::invalid_argument("value " + kv.first + ": decryption share expects a size-2 ciphertext (relinearize first)");
    check_combine_room(kv.first, c->limbs, shares.size(), shares[0]->smudge_bits);
    std::vector<const SharePiece *> pieces;
    for (size_t p = 0; p < shares.size(); p++) pieces.push_back(&share_piece(*shares[p], p, kv.first, 0, 1, c->limbs, c->scale));
    if (on_dev) {
      std::vector<CtHandle> keep;
      // (the source rule is rekey's, and so is the prefix of its shape refusal: kept as found)
      const evah_ct *h = source_handle(dev, *host, "rekey: value " + kv.first, *c, keep, InPlace::SameGpu, BringOver::Copy);
      std::vector<const evah_ct *> hs;
      for (const SharePiece *piece : pieces) hs.push_back(share_handle(*piece, keep));
      v.resize((size_t)sig.vec_size);
      chk(evah_decrypt_combine_rows(dev->h, &h, 1, hs.data(), (uint32_t)hs.size(), (uint32_t)sig.vec_size, EVAH_F64, v.data(), sizeof(double) * v.size(),
                                    0, 1));
    } else {
      check_cipher_shape(*host, "value " + kv.first, *c, 2, 2);
      (void)words(*c); // the host twin reads the words: a resident value comes down here
      std::vector<const u64 *> hs;
      for (const SharePiece *piece : pieces) {
        const std::vector<u64> &w = words(*piece, host->N);
        if (w.size() != (size_t)c->limbs * host->N) throw std::runtime_error("combine_shares: a share's words do not match its shape");
        hs.push_back(w.data());
      }
      const std::vector<u64> m = combine_shares_host(*host, *c, hs, shares[0]->smudge_bits);
      host->decode_coeff(m.data(), c->limbs, c->scale, v);
      v.resize((size_t)sig.vec_size);
    }
    out[kv.first] = std::move(v);
  }
  return out;
}
// the same for a batch, into rows as decrypt_array writes them: rows[name] is an array [B][vec_size] of dtype_out on the host,
// or (rows_on_device) device memory of this context's state
inline void HipPublic::combine_shares_array(const HipValuationBatch &vb, const std::vector<std::shared_ptr<DecryptionShares>> &shares,
                                            const CKKSSignature &sig, int dtype_out, const std::map<std::string, void *> &rows, bool rows_on_device) {
  check_shares(shares);
  if (sig.vec_size <= 0) throw std::runtime_error("Signature vector size must be positive");
  if (!device_client_enabled()) throw std::runtime_error("combine_shares of a batch needs a HIP device: none is visible, or EVA_DEVICE_CLIENT=0 keeps the client on the host");
  ensure_device(false);
  if (!vb.root) throw std::runtime_error("combine_shares: the batch holds no device handles");
  for (auto &nc : vb.ciphers) // (before anything is launched)
    for (auto &seg : nc.second.segments)
      if (seg.size != 2) throw std::invalid_argument("value " + nc.first + ": decryption share expects a size-2 ciphertext (relinearize first)");
  const uint32_t n_out = (uint32_t)sig.vec_size;
  const size_t rb = row_bytes(dtype_out, n_out);
  for (auto &nc : vb.ciphers) {
    char *out = static_cast<char *>(rows.at(nc.first));
    const auto &segs = nc.second.segments;
    walk_segments("value " + nc.first, segs, vb.B, dev, vb.root, [&](SegmentGroup &g) {
      const BatchSegment &s = segs[g.s0];
      check_combine_room(nc.first, s.limbs, shares.size(), shares[0]->smudge_bits);
      std::vector<const evah_ct *> sh;
      for (size_t p = 0; p < shares.size(); p++) sh.push_back(share_handle(share_piece(*shares[p], p, nc.first, g.row, g.n, s.limbs, s.scale), g.keep));
      chk(evah_decrypt_combine_rows(dev->h, g.hs.data(), (uint32_t)g.hs.size(), sh.data(), (uint32_t)sh.size(), n_out, dtype_out, out + g.row * rb, rb,
                                    rows_on_device ? 1 : 0, rows_on_device ? 0 : 1));
      if (rows_on_device) chk(evah_ctx_sync(dev->h)); // the uploads and copies made for this call are released behind it
    });
  }
}

// What a party keeps between the two rounds of the collective relinearization-key generation: the 32-byte
// keys u_J is regenerated from, and nothing else.  Whoever learns them learns s_p (h1 - NTT(e1) = a s_p with a public), so
// the object cannot be saved, pickled or copied, serves ONE round 2 of the context that made it, and is wiped when used
// and when destroyed.
struct RelinEphemeral {
  std::vector<std::array<uint8_t, 32>> r1;
  std::shared_ptr<const char> owner; // HipSecret::identity of the context that made it
  bool used = false;
  RelinEphemeral() = default;
  RelinEphemeral(const RelinEphemeral &) = delete;
  RelinEphemeral &operator=(const RelinEphemeral &) = delete;
  void wipe_keys() {
    for (auto &k : r1) wipe_bytes(k.data(), 32);
  }
  ~RelinEphemeral() { wipe_keys(); }
};

class HipSecret {
public:
  std::shared_ptr<HostContext> host;
  SecretKey sk;
  int device = 0;
  // generate_keys(..., common_seed): the PUBLIC seeds [digits][32] of this pair's relinearization key, equal
  // across the parties — what the collective relinearization-key rounds derive their common rows from.
  // Empty for every other pair, and for a context loaded from a file (the secret file does not carry them).
  std::vector<uint8_t> common_relin_seeds;
  std::shared_ptr<const char> identity = std::make_shared<char>(); // which context made a RelinEphemeral
  // test hook of generate_keys(..., seed != 0, device_sampling): the 32-byte keys its secret stream gave;
  // empty for every other pair
  KeyGenerator::Randomness key_randomness;
  // decrypt + decode on the GPU when one is present (EVA_DEVICE_CLIENT=0: host); the secret key is
  // uploaded once, in NTT form, to a context of its own
  bool on_device() {
    if (state < 0) {
      state = device_client_enabled() ? 1 : 0;
      if (state == 1) {
        // the device state of the key pair (generate_keys shares one holder between both halves), so
        // that the public context's resident results are read in place
        if (!holder->dev) holder->dev = std::make_shared<DeviceCtx>(host->N, host->primes, device);
        dev = holder->dev;
        chk(evah_client_key_upload(dev->h, EVAH_KEY_SECRET, (const uint64_t *)sk.s_ntt.data()));
      }
    }
    return state == 1;
  }
  int state = -1;
  std::shared_ptr<DeviceHolder> holder = std::make_shared<DeviceHolder>();
  std::shared_ptr<DeviceCtx> dev;
  // encrypt() leaves its ciphertexts in HBM (the key pair's device state) unless EVA_RESIDENT=0
  bool resident = std::getenv("EVA_RESIDENT") ? std::atoi(std::getenv("EVA_RESIDENT")) != 0 : true;

  // Encryptor::encrypt_symmetric + a seeded save: every encrypted input is c0 plus the 32-byte
  // seed of c1 = a, half the words of HipPublic::encrypt's ciphertexts.  Same input checks and Plain / Raw handling
  // as HipPublic::encrypt.  Two streams, as in the keygen: seeds (public) and errors (secret) never share one.
  // seed != 0 is the reproducible test hook (streams (seed, 4) and (seed, 3)) and is NOT secret-grade.
  HipValuation encrypt(const Valuation &inputs, const CKKSSignature &sig, uint64_t seed = 0) {
    check_vec_size(sig, host->N / 2);
    std::unique_ptr<SecureRng> seeds = client_stream(seed, 4);
    std::unique_ptr<SecureRng> errors = client_stream(seed, 3);
    std::vector<std::string> names; // name order: the same seed gives the same valuation whatever the map's order
    for (auto &kv : inputs) names.push_back(kv.first);
    std::sort(names.begin(), names.end());
    HipValuation out;
    for (const std::string &name : names) {
      const auto &v = inputs.at(name);
      check_input_size(v, sig);
      const InputClass in = classify_input(*host, sig, name);
      if (unencrypted_value(*host, in, v, out.values[name])) continue;
      const std::array<uint8_t, 32> sd = draw_key32(*seeds);
      std::vector<int8_t> e;
      WipeOnExit wipe_e{e};
      host->sample_error(*errors, e);
      out.values[name] = encrypt_value(v, in.scale, in.limbs, e, sd);
    }
    return out;
  }
  // one encrypted input, its draws made: on the device when one is present, else on the host — the same words bit for bit
  // (same plaintext, exact modular arithmetic)
  HostCipher encrypt_value(const std::vector<double> &v, double scale, uint32_t limbs, const std::vector<int8_t> &e,
                           const std::array<uint8_t, 32> &sd) {
    if (on_device()) return encrypt_on_device(v, scale, limbs, e, sd);
    HostPlain pt = encode_host(*host, v, scale, limbs);
    ntt_limbs(*host, pt);
    return encrypt_symmetric(*host, sk, pt, e, sd);
  }
  // evah_pt_encode (or the host encoder + evah_pt_upload_coeff) -> evah_encrypt_symmetric
  HostCipher encrypt_on_device(const std::vector<double> &v, double scale, uint32_t limbs, const std::vector<int8_t> &e,
                               const std::array<uint8_t, 32> &sd) {
    evah_pt *p = nullptr;
    if (device_encodable(*host, v, scale, limbs)) {
      chk(evah_pt_encode(dev->h, v.data(), (uint32_t)v.size(), limbs, scale, &p));
    } else {
      HostPlain pt = encode_host(*host, v, scale, limbs);
      chk(evah_pt_upload_coeff(dev->h, limbs, scale, (const uint64_t *)pt.data.data(), &p));
    }
    evah_ct *c = nullptr;
    int rc = evah_encrypt_symmetric(dev->h, p, e.data(), sd.data(), &c);
    evah_pt_free(dev->h, p);
    chk(rc);
    return cipher_of_handle(dev, *host, c, limbs, scale, resident, &sd);
  }
  // encrypt() for a list of input valuations of one signature.  ONE pair of streams for the call;
  // instances are visited in list order, the names sorted within an instance, and every encrypted input takes 4 seed words
  // and one sample_error — so instance 0 of a seeded call is encrypt() of that instance word for word and no two values
  // share a seed.  The draws made, each name's instances leave in groups of <= 64 as one
  // evah_encode_encrypt_symmetric_many (views of the group's handle come back); a name with an instance the device
  // encoder cannot take, and every input without a device, takes encrypt()'s path per instance with the same draws.
  // device_sampling: the error of an encrypted input is a 32-byte key — 4 words of the secret stream in
  // place of its N sample_error draws —, expanded on the device by the grouped call and by the host twin (csprng.h
  // sampled_small(key, 1)) on every other path; the seeds of c1 are drawn exactly as without the option.
  std::vector<HipValuation> encrypt_batch(const std::vector<Valuation> &inputs, const CKKSSignature &sig, uint64_t seed = 0,
                                          bool device_sampling = false) {
    check_vec_size(sig, host->N / 2);
    std::vector<HipValuation> out(inputs.size());
    if (inputs.empty()) return out;
    const std::vector<std::string> names = batch_input_names(inputs);
    std::unique_ptr<SecureRng> seeds = client_stream(seed, 4);
    std::unique_ptr<SecureRng> errors = client_stream(seed, 3);
    struct Drawn {
      std::vector<std::vector<int8_t>> e;          // per instance
      std::vector<std::array<uint8_t, 32>> sd;
      std::vector<std::array<uint8_t, 32>> ek;     // device_sampling: the error keys, e filled from them where the host needs it
      uint32_t limbs = 0;
      double scale = 0;
    };
    std::vector<Drawn> drawn(names.size());
    struct WipeAll {
      std::vector<Drawn> &d;
      ~WipeAll() {
        for (auto &x : d) {
          for (auto &e : x.e) wipe(e);
          for (auto &k : x.ek) wipe_bytes(k.data(), 32);
        }
      }
    } wipe_all{drawn};
    for (size_t b = 0; b < inputs.size(); b++) {
      for (size_t i = 0; i < names.size(); i++) {
        const std::string &name = names[i];
        const auto &v = inputs[b].at(name);
        check_input_size(v, sig);
        const InputClass in = classify_input(*host, sig, name);
        if (unencrypted_value(*host, in, v, out[b].values[name])) continue;
        Drawn &d = drawn[i];
        d.limbs = in.limbs;
        d.scale = in.scale;
        d.sd.push_back(draw_key32(*seeds));
        d.e.emplace_back();
        if (device_sampling) d.ek.push_back(draw_key32(*errors));
        else host->sample_error(*errors, d.e.back());
      }
    }
    for (size_t i = 0; i < names.size(); i++) {
      const std::string &name = names[i];
      Drawn &d = drawn[i];
      if (d.e.empty()) continue; // a plain or raw input: done above
      bool grouped = on_device();
      for (size_t b = 0; grouped && b < inputs.size(); b++) grouped = device_encodable(*host, inputs[b].at(name), d.scale, d.limbs);
      if (!grouped) { // encrypt()'s path, instance by instance
        for (size_t b = 0; b < inputs.size(); b++) {
          if (device_sampling) { // the same key through the host twin
            d.e[b].resize(host->N);
            sampled_small(d.ek[b].data(), 1, host->N, d.e[b].data());
          }
          out[b].values[name] = encrypt_value(inputs[b].at(name), d.scale, d.limbs, d.e[b], d.sd[b]);
        }
        continue;
      }
      encrypt_in_groups(inputs, name, out, [&](const std::vector<const std::vector<double> *> &vals, size_t b0) {
        return encrypt_group_on_device(vals, d.scale, d.limbs, d.e.data() + b0, d.sd.data() + b0, device_sampling ? d.ek.data() + b0 : nullptr);
      });
    }
    return out;
  }
  // one group of encrypt_batch on the device: instance b from (vals[b], e[b], sd[b]) — or, ek given, from (vals[b], the
  // error the device draws from ek[b], sd[b]); the values encrypt_on_device returns
  std::vector<HostCipher> encrypt_group_on_device(const std::vector<const std::vector<double> *> &vals, double scale, uint32_t limbs,
                                                  const std::vector<int8_t> *e, const std::array<uint8_t, 32> *sd,
                                                  const std::array<uint8_t, 32> *ek = nullptr) {
    const size_t B = vals.size(), N = host->N;
    const std::vector<double> flat = flatten(vals);
    const uint32_t nv = (uint32_t)vals[0]->size();
    std::vector<int8_t> errs(ek ? 0 : B * N);
    std::vector<uint8_t> seeds(B * 32), ekeys(ek ? B * 32 : 0);
    for (size_t b = 0; b < B; b++) {
      if (ek) std::copy(ek[b].begin(), ek[b].end(), ekeys.begin() + b * 32);
      else std::copy(e[b].begin(), e[b].end(), errs.begin() + b * N);
      std::copy(sd[b].begin(), sd[b].end(), seeds.begin() + b * 32);
    }
    evah_ct *c = nullptr;
    const int rc = ek ? evah_encode_encrypt_symmetric_sampled_many(dev->h, (uint32_t)B, flat.data(), nv, limbs, scale, ekeys.data(), seeds.data(), &c)
                      : evah_encode_encrypt_symmetric_many(dev->h, (uint32_t)B, flat.data(), nv, limbs, scale, errs.data(), seeds.data(), &c);
    wipe(errs);
    wipe_bytes(ekeys.data(), ekeys.size());
    chk(rc);
    return group_results(dev, *host, c, B, limbs, scale, resident, sd);
  }
  // encrypt_batch(..., seed, device_sampling = true) for arrays [B][n] in their own type: the same two
  // streams and the same draws — per instance, names sorted, 4 seed words and a 4-word error key per encrypted input —
  // so instance b is encrypt_batch's word for word.  Per name the rows leave in segments of <= 64 as ONE
  // evah_encode_encrypt_symmetric_array each; the handles are kept whole and the seeds stay with the batch.
  HipValuationBatch encrypt_array(const std::map<std::string, ArrayView> &arrays_in, const Valuation &shared, const CKKSSignature &sig,
                                  uint64_t seed = 0, const std::map<std::string, ArrayView> &plains = {}) {
    require_array_path(on_device(), resident);
    HipValuationBatch out;
    out.params = host;
    out.root = dev;
    std::map<std::string, ArrayView> arrays = arrays_in; // (plan_array_inputs attaches the sums of a device array to its view)
    const ArrayInputs in = plan_array_inputs(*host, arrays, shared, sig, out, plains, dev->h);
    std::unique_ptr<SecureRng> seeds = client_stream(seed, 4);
    std::unique_ptr<SecureRng> errors = client_stream(seed, 3);
    std::vector<std::vector<std::array<uint8_t, 32>>> ek(in.names.size()); // per name, per instance
    WipeKeyRows wipe_keys{ek};
    for (size_t b = 0; b < out.B; b++)
      for (size_t i = 0; i < in.names.size(); i++)
        if (in.arr[i]) {
          out.ciphers[in.names[i]].seeds.push_back(draw_key32(*seeds));
          ek[i].push_back(draw_key32(*errors));
        }
    for (size_t i = 0; i < in.names.size(); i++) {
      if (!in.arr[i]) continue;
      const ArrayView &a = *in.arr[i];
      BatchCipher &bc = out.ciphers[in.names[i]];
      for (size_t b0 = 0; b0 < out.B; b0 += CLIENT_BATCH_MAX) {
        const size_t n = std::min<size_t>(CLIENT_BATCH_MAX, out.B - b0);
        std::vector<uint8_t> ekeys = keys_flat(ek[i].data() + b0, n);
        const std::vector<uint8_t> sd = keys_flat(bc.seeds.data() + b0, n);
        evah_ct *c = nullptr;
        const int rc = a.on_device ? evah_encode_encrypt_symmetric_array_dev(dev->h, (uint32_t)n, a.row(b0), a.dtype, a.row_pitch(), a.producer,
                                                                             a.sums->data() + b0, (uint32_t)a.n, in.cls[i].limbs, in.cls[i].scale,
                                                                             ekeys.data(), sd.data(), &c)
                                   : evah_encode_encrypt_symmetric_array(dev->h, (uint32_t)n, a.row(b0), a.dtype, (uint32_t)a.n, in.cls[i].limbs,
                                                                         in.cls[i].scale, ekeys.data(), sd.data(), &c);
        wipe_bytes(ekeys.data(), ekeys.size());
        chk(rc);
        bc.segments.push_back(BatchSegment{std::make_shared<CtHandle>(dev->h, c), (uint32_t)n, nullptr, 2, in.cls[i].limbs, in.cls[i].scale});
      }
    }
    return out;
  }
  // decrypt_batch for a batch of batched handles: per name, consecutive segments of one size, limb count
  // and scale are packed (walk_segments) into calls of <= 64 instances of evah_decrypt_decode_handles, each writing straight into the rows
  // rows[name] + first instance * vec_size * itemsize of the caller's array [B][vec_size] (dtype_out: EVAH_F64, the doubles
  // of decrypt_batch bit for bit, or EVAH_F32).  Needs the device; the batch lives on this key pair's device state.
  // rows_on_device: the rows are device memory of this key pair's state, written group by group by
  // evah_decrypt_decode_rows in queue order, with one wait at the end of the call; EVAH_U8 takes that entry point too
  void decrypt_array(const HipValuationBatch &vb, const CKKSSignature &sig, int dtype_out, const std::map<std::string, void *> &rows,
                     bool rows_on_device = false) {
    if (!on_device()) throw std::runtime_error("decrypt_array needs a HIP device: none is visible, or EVA_DEVICE_CLIENT=0 keeps the client on the host");
    if (sig.vec_size <= 0) throw std::runtime_error("Signature vector size must be positive");
    if (vb.root != dev) throw std::runtime_error("decrypt_array: the batch lives on the device state of another key pair");
    const uint32_t n_out = (uint32_t)sig.vec_size;
    const size_t rb = row_bytes(dtype_out, n_out);
    for (auto &kv : vb.ciphers) {
      char *out = static_cast<char *>(rows.at(kv.first));
      walk_segments("output " + kv.first, kv.second.segments, vb.B, dev, vb.root, [&](SegmentGroup &g) {
        if (rows_on_device || dtype_out == EVAH_U8)
          chk(evah_decrypt_decode_rows(dev->h, g.hs.data(), (uint32_t)g.hs.size(), n_out, dtype_out, out + g.row * rb, rb, rows_on_device ? 1 : 0, 0));
        else
          chk(evah_decrypt_decode_handles(dev->h, g.hs.data(), (uint32_t)g.hs.size(), n_out, dtype_out, out + g.row * rb));
      });
    }
    if (rows_on_device) chk(evah_ctx_sync(dev->h));
  }
  // one value of decrypt()
  std::vector<double> decrypt_value(const std::string &name, const SchemeValue &value, const CKKSSignature &sig) {
    std::vector<double> v;
    if (auto *c = std::get_if<HostCipher>(&value)) {
      if (on_device()) { // dot product with s, inverse transforms, recomposition and the special FFT on the GPU
        std::vector<CtHandle> keep; // resident on this key pair's device state: read in place; else uploaded for the call
        const evah_ct *h = source_handle(dev, *host, "output " + name, *c, keep, InPlace::SameState, BringOver::Upload);
        v.resize((size_t)sig.vec_size);
        chk(evah_decrypt_decode(dev->h, h, (uint32_t)sig.vec_size, v.data()));
        return v;
      }
      (void)words(*c);
      auto m = decrypt_to_coeff(*host, sk, *c);
      host->decode_coeff(m.data(), c->limbs, c->scale, v);
    } else {
      return decode_unencrypted(*host, value, (size_t)sig.vec_size);
    }
    v.resize((size_t)sig.vec_size);
    return v;
  }
  // SEALSecret::decrypt (seal.cpp:124-146)
  Valuation decrypt(const HipValuation &enc, const CKKSSignature &sig) {
    Valuation out;
    for (auto &kv : enc.values) out[kv.first] = decrypt_value(kv.first, kv.second, sig);
    return out;
  }
  // decrypt() of every valuation of a list, bit for bit.  On the device, per output name, runs of
  // instances of one size, limb count and scale leave in groups of <= 64 as ONE evah_decrypt_decode_many each: resident
  // values are read in place, the others uploaded first, as decrypt() does.  Everything else is decrypt() per value.
  std::vector<Valuation> decrypt_batch(const std::vector<const HipValuation *> &encs, const CKKSSignature &sig) {
    std::vector<Valuation> out(encs.size());
    for (size_t b = 0; b < encs.size(); b++)
      if (!encs[b]) throw std::invalid_argument("decrypt_batch: valuation " + std::to_string(b) + " is None");
    if (!on_device() || sig.vec_size <= 0) {
      for (size_t b = 0; b < encs.size(); b++) out[b] = decrypt(*encs[b], sig);
      return out;
    }
    std::map<std::string, std::vector<std::pair<size_t, const HostCipher *>>> by_name; // name -> (instance, ciphertext) in list order
    for (size_t b = 0; b < encs.size(); b++)
      for (auto &kv : encs[b]->values) {
        if (auto *c = std::get_if<HostCipher>(&kv.second)) by_name[kv.first].emplace_back(b, c);
        else out[b][kv.first] = decrypt_value(kv.first, kv.second, sig);
      }
    const uint32_t n_out = (uint32_t)sig.vec_size;
    for (auto &nv : by_name) {
      const auto &list = nv.second;
      for (size_t i0 = 0; i0 < list.size();) {
        const HostCipher *first = list[i0].second;
        size_t i1 = i0;
        std::vector<CtHandle> uploaded; // the group's values that were not resident here
        std::vector<const evah_ct *> hs;
        while (i1 < list.size() && i1 - i0 < CLIENT_BATCH_MAX) {
          const HostCipher *c = list[i1].second;
          if (c->size != first->size || c->limbs != first->limbs || c->scale != first->scale) break;
          hs.push_back(source_handle(dev, *host, "output " + nv.first, *c, uploaded, InPlace::SameState, BringOver::Upload));
          i1++;
        }
        std::vector<double> flat(hs.size() * n_out);
        chk(evah_decrypt_decode_many(dev->h, hs.data(), (uint32_t)hs.size(), n_out, flat.data()));
        for (size_t i = i0; i < i1; i++)
          out[list[i].first][nv.first].assign(flat.begin() + (i - i0) * n_out, flat.begin() + (i - i0 + 1) * n_out);
        std::fill(flat.begin(), flat.end(), 0.0);
        i0 = i1;
      }
    }
    return out;
  }

  // ---- the re-key key from this key pair to `target`'s: made here, from the target's PUBLIC key, and
  // handed to whoever holds the target's public context (HipPublic::rekey).  Both pairs share N and the prime list.
  // Randomness: one secret stream per call, digits in order, 4 words per digit, all drawn before the first device call
  // and wiped afterwards.  seed != 0 is the reproducible test hook (stream (seed, 3)) and is NOT secret-grade.  On the
  // device where one is present (evah_keygen_rekey), else the host twin — the same words.
  std::shared_ptr<RekeyKey> make_rekey_key(const HipPublic &target, uint64_t seed = 0) {
    const std::string diff = rekey_params_differ(target.host->N, target.host->primes, *host);
    if (!diff.empty()) throw std::invalid_argument("make_rekey_key: the two key pairs must share their encryption parameters: " + diff);
    if (sk.s_ntt.size() != (size_t)host->k * host->N) throw std::invalid_argument("make_rekey_key: secret key not present");
    if (target.pk.data.size() != (size_t)2 * host->k * host->N) throw std::invalid_argument("make_rekey_key: the target context holds no public key");
    const uint32_t D = host->k - 1;
    std::unique_ptr<SecureRng> stream = client_stream(seed, 3);
    std::vector<std::vector<std::array<uint8_t, 32>>> rk(1);
    WipeKeyRows wipe_keys{rk};
    for (uint32_t J = 0; J < D; J++) rk[0].push_back(draw_key32(*stream));
    auto out = std::make_shared<RekeyKey>();
    out->N = host->N;
    out->primes = host->primes;
    out->n_digits = D;
    if (on_device()) {
      out->data.resize((size_t)D * 2 * host->k * host->N);
      std::vector<uint8_t> flat = keys_flat(rk[0].data(), D);
      const int rc = evah_keygen_rekey(dev->h, (const uint64_t *)target.pk.data.data(), D, flat.data(), (uint64_t *)out->data.data());
      wipe_bytes(flat.data(), flat.size());
      chk(rc);
    } else {
      out->data = rekey_keygen_host(*host, sk, target.pk, D, rk[0].data());
    }
    return out;
  }

  // ---- the collective relinearization key: this party's two shares.  Round 1 draws one ephemeral key per
  // digit (stream (seed, 6) under the test hook, else the OS) and returns them beside the public share; round 2 takes them
  // back — once — with the sum of all parties' round-1 shares, and draws fresh keys (stream (seed, 7)).  On the device
  // where one is present (evah_keygen_relin_round1 / _round2), else the host twins — the same words.
  std::pair<std::shared_ptr<RelinEphemeral>, std::shared_ptr<RelinShare>> relin_round1(uint64_t seed = 0) {
    const uint32_t D = host->k - 1;
    if (common_relin_seeds.size() != (size_t)32 * D)
      throw std::invalid_argument("relin_round1: this context's keys were not generated with a common seed (generate_keys(..., common_seed=)): "
                                  "the parties share no public relinearization seeds");
    if (sk.s_ntt.size() != (size_t)host->k * host->N) throw std::invalid_argument("relin_round1: secret key not present");
    std::unique_ptr<SecureRng> stream = client_stream(seed, 6);
    auto eph = std::make_shared<RelinEphemeral>();
    eph->owner = identity;
    for (uint32_t J = 0; J < D; J++) eph->r1.push_back(draw_key32(*stream));
    const std::vector<uint8_t> seeds = relin_round_seeds(common_relin_seeds);
    auto out = std::make_shared<RelinShare>();
    out->round = 1;
    out->N = host->N;
    out->primes = host->primes;
    out->n_digits = D;
    if (on_device()) {
      out->data.resize((size_t)D * 2 * host->k * host->N);
      std::vector<uint8_t> flat = keys_flat(eph->r1.data(), D);
      const int rc = evah_keygen_relin_round1(dev->h, D, seeds.data(), flat.data(), (uint64_t *)out->data.data());
      wipe_bytes(flat.data(), flat.size());
      chk(rc);
    } else {
      out->data = relin_round1_host(*host, sk, D, seeds.data(), eph->r1.data());
    }
    return {eph, out};
  }
  std::shared_ptr<RelinShare> relin_round2(const std::shared_ptr<RelinEphemeral> &eph, const std::shared_ptr<const RelinShare> &agg1, uint64_t seed = 0) {
    if (!eph) throw std::invalid_argument("relin_round2: the ephemeral state is None");
    if (!agg1) throw std::invalid_argument("relin_round2: the round-1 aggregate is None");
    if (eph->owner != identity) throw std::invalid_argument("relin_round2: the ephemeral state was made by another secret context");
    if (eph->used) throw std::invalid_argument("relin_round2: the ephemeral state was already used (a second share would reuse u)");
    const uint32_t D = host->k - 1;
    if (agg1->round != 1) throw std::invalid_argument("relin_round2: the aggregate is not made of round-1 shares (it is a round-" + std::to_string(agg1->round) + " share)");
    const std::string diff = rekey_params_differ(agg1->N, agg1->primes, *host);
    if (!diff.empty()) throw std::invalid_argument("relin_round2: the aggregate was made under other encryption parameters: " + diff);
    if (agg1->n_digits != D || eph->r1.size() != D || agg1->data.size() != (size_t)D * 2 * host->k * host->N)
      throw std::invalid_argument("relin_round2: the aggregate's words do not match its shape");
    if (!residues_canonical(agg1->data, *host)) throw std::invalid_argument("relin_round2: the aggregate holds a word that is not reduced modulo its prime");
    if (sk.s_ntt.size() != (size_t)host->k * host->N) throw std::invalid_argument("relin_round2: secret key not present");
    std::unique_ptr<SecureRng> stream = client_stream(seed, 7);
    std::vector<std::vector<std::array<uint8_t, 32>>> rk(1);
    WipeKeyRows wipe_keys{rk};
    for (uint32_t J = 0; J < D; J++) rk[0].push_back(draw_key32(*stream));
    auto out = std::make_shared<RelinShare>();
    out->round = 2;
    out->N = host->N;
    out->primes = host->primes;
    out->n_digits = D;
    if (on_device()) {
      out->data.resize((size_t)D * host->k * host->N);
      std::vector<uint8_t> f1 = keys_flat(eph->r1.data(), D), f2 = keys_flat(rk[0].data(), D);
      const int rc = evah_keygen_relin_round2(dev->h, D, (const uint64_t *)agg1->data.data(), f1.data(), f2.data(), (uint64_t *)out->data.data());
      wipe_bytes(f1.data(), f1.size());
      wipe_bytes(f2.data(), f2.size());
      chk(rc);
    } else {
      out->data = relin_round2_host(*host, sk, D, agg1->data.data(), eph->r1.data(), rk[0].data());
    }
    eph->used = true; // u served its one share
    eph->wipe_keys();
    return out;
  }
  std::array<uint64_t, 6> transfer_stats() {
    std::array<uint64_t, 6> st{0, 0, 0, 0, 0, 0};
    if (dev) chk(evah_ctx_transfer_stats(dev->h, st.data()));
    return st;
  }

  // ---- the refresh: decrypt, divide by a power of two and encrypt again under this key pair, without
  // decoding, so that a result becomes a valid input of the program `sig` belongs to — at that input's level and scale.
  // For every encrypted input `name` of sig the source is the value (rename[name], else name) of the valuation; the
  // consumer's unencrypted inputs are encoded as encrypt() encodes them.  Randomness: encrypt_batch(..., device_sampling =
  // true)'s contract — one pair of streams per call, instances in order, names sorted within an instance, 4 seed words and
  // a 4-word error key per encrypted input, all drawn before the first device call, the keys wiped afterwards.
  struct RefreshInput {
    std::string name, source;
    InputClass cls;
  };
  std::vector<RefreshInput> refresh_plan(const CKKSSignature &sig, const std::map<std::string, std::string> &rename) const {
    check_vec_size(sig, host->N / 2);
    std::vector<RefreshInput> plan;
    for (auto &kv : sig.inputs)
      if (kv.second.input_type == Type::Cipher) {
        auto r = rename.find(kv.first);
        plan.push_back(RefreshInput{kv.first, r == rename.end() ? kv.first : r->second, classify_input(*host, sig, kv.first)});
      }
    std::sort(plan.begin(), plan.end(), [](const RefreshInput &a, const RefreshInput &b) { return a.name < b.name; });
    return plan;
  }
  void refresh_unencrypted(const Valuation &inputs, const CKKSSignature &sig, std::unordered_map<std::string, SchemeValue> &out) const {
    for (auto &kv : inputs) {
      check_input_size(kv.second, sig);
      if (!unencrypted_value(*host, classify_input(*host, sig, kv.first), kv.second, out[kv.first]))
        throw std::invalid_argument("refresh: input " + kv.first + " is encrypted: its value comes from the valuation, not from inputs");
    }
  }
  // one value: on the device when one is present (a value resident on this key pair's state is read in place, any other
  // uploaded first, as decrypt_value does), else the host twin — the same words
  HostCipher refresh_value(const std::string &name, const HostCipher &c, uint32_t limbs, double scale, uint32_t shift,
                           const std::array<uint8_t, 32> &ek, const std::array<uint8_t, 32> &sd) {
    if (on_device()) {
      std::vector<CtHandle> keep;
      const evah_ct *h = source_handle(dev, *host, "output " + name, c, keep, InPlace::SameState, BringOver::Upload);
      evah_ct *o = nullptr;
      chk(evah_refresh_handles(dev->h, &h, 1, limbs, scale, ek.data(), sd.data(), &o));
      return cipher_of_handle(dev, *host, o, limbs, scale, resident, &sd);
    }
    check_cipher_shape(*host, "output " + name, c, 1, 3);
    (void)words(c); // the host twin reads the words: a resident value comes down here
    return refresh_host(*host, sk, c, limbs, shift, ek, sd);
  }
  HipValuation refresh(const HipValuation &enc, const CKKSSignature &sig, const std::map<std::string, std::string> &rename = {},
                       const Valuation &inputs = {}, uint64_t seed = 0) {
    const std::vector<RefreshInput> plan = refresh_plan(sig, rename);
    HipValuation out;
    out.params = host;
    refresh_unencrypted(inputs, sig, out.values);
    std::vector<const HostCipher *> src(plan.size());
    std::vector<uint32_t> shift(plan.size());
    for (size_t i = 0; i < plan.size(); i++) {
      auto it = enc.values.find(plan[i].source);
      if (it == enc.values.end()) throw std::out_of_range("refresh: no value named " + plan[i].source + " in the valuation (input " + plan[i].name + ")");
      src[i] = std::get_if<HostCipher>(&it->second);
      if (!src[i]) throw std::invalid_argument("refresh: value " + plan[i].source + " is not a ciphertext");
      shift[i] = refresh_shift(src[i]->scale, plan[i].cls.scale);
    }
    std::unique_ptr<SecureRng> seeds = client_stream(seed, 4);
    std::unique_ptr<SecureRng> errors = client_stream(seed, 3);
    std::vector<std::array<uint8_t, 32>> sd(plan.size());
    std::vector<std::vector<std::array<uint8_t, 32>>> ek(1);
    WipeKeyRows wipe_keys{ek};
    for (size_t i = 0; i < plan.size(); i++) {
      sd[i] = draw_key32(*seeds);
      ek[0].push_back(draw_key32(*errors));
    }
    for (size_t i = 0; i < plan.size(); i++)
      out.values[plan[i].name] = refresh_value(plan[i].source, *src[i], plan[i].cls.limbs, plan[i].cls.scale, shift[i], ek[0][i], sd[i]);
    return out;
  }
  // the same for a batch of batched handles: per name, consecutive segments of one shape are packed into calls of <= 64
  // instances of evah_refresh_handles, as decrypt_array packs them; the results stay whole batched handles with their seeds.
  // Needs the device and resident valuations; the batch lives on this key pair's device state.
  HipValuationBatch refresh_batch(const HipValuationBatch &vb, const CKKSSignature &sig, const std::map<std::string, std::string> &rename = {},
                                  const Valuation &inputs = {}, uint64_t seed = 0) {
    require_array_path(on_device(), resident, "refresh");
    if (vb.root != dev) throw std::runtime_error("refresh: the batch lives on the device state of another key pair");
    const std::vector<RefreshInput> plan = refresh_plan(sig, rename);
    HipValuationBatch out;
    out.B = vb.B;
    out.params = host;
    out.root = dev;
    refresh_unencrypted(inputs, sig, out.shared);
    std::vector<const BatchCipher *> src(plan.size());
    for (size_t i = 0; i < plan.size(); i++) {
      auto it = vb.ciphers.find(plan[i].source);
      if (it == vb.ciphers.end())
        throw std::out_of_range("refresh: no encrypted value named " + plan[i].source + " in the batch (input " + plan[i].name + ")");
      src[i] = &it->second;
    }
    std::unique_ptr<SecureRng> seeds = client_stream(seed, 4);
    std::unique_ptr<SecureRng> errors = client_stream(seed, 3);
    std::vector<std::vector<std::array<uint8_t, 32>>> ek(plan.size()); // per name, per instance
    WipeKeyRows wipe_keys{ek};
    for (size_t b = 0; b < out.B; b++)
      for (size_t i = 0; i < plan.size(); i++) {
        out.ciphers[plan[i].name].seeds.push_back(draw_key32(*seeds));
        ek[i].push_back(draw_key32(*errors));
      }
    for (size_t i = 0; i < plan.size(); i++) {
      const auto &segs = src[i]->segments;
      const InputClass &cls = plan[i].cls;
      BatchCipher &bc = out.ciphers[plan[i].name];
      walk_segments("value " + plan[i].source, segs, vb.B, dev, vb.root, [&](SegmentGroup &g) {
        (void)refresh_shift(segs[g.s0].scale, cls.scale); // the scale rules, with the host's messages, before anything is launched
        std::vector<uint8_t> ekeys = keys_flat(ek[i].data() + g.row, g.n);
        const std::vector<uint8_t> sd = keys_flat(bc.seeds.data() + g.row, g.n);
        evah_ct *c = nullptr;
        const int rc = evah_refresh_handles(dev->h, g.hs.data(), (uint32_t)g.hs.size(), cls.limbs, cls.scale, ekeys.data(), sd.data(), &c);
        wipe_bytes(ekeys.data(), ekeys.size());
        chk(rc);
        bc.segments.push_back(BatchSegment{std::make_shared<CtHandle>(dev->h, c), (uint32_t)g.n, nullptr, 2, cls.limbs, cls.scale});
      });
    }
    return out;
  }

  // ---- threshold decryption: this party's share h = c1 s_p + NTT(E) of every encrypted value, E flooding
  // noise of smudge_bits bits drawn from a 32-byte key per value.  One secret stream per call (seed != 0: SecureRng(seed,
  // 5), the reproducible test hook, NOT secret-grade): names sorted, instances in order, 4 words per value, all drawn before
  // the first device call and wiped after.  Unencrypted and raw values are skipped.
  std::shared_ptr<DecryptionShares> new_shares(uint32_t smudge_bits, bool batch, size_t B) const {
    if (smudge_bits < 1 || smudge_bits > 62) throw std::invalid_argument("smudge_bits must be 1..62");
    if (sk.s_ntt.size() != (size_t)host->k * host->N) throw std::invalid_argument("decrypt_share: secret key not present");
    auto out = std::make_shared<DecryptionShares>();
    out->N = host->N;
    out->smudge_bits = smudge_bits;
    out->primes = host->primes;
    out->batch = batch;
    out->B = B;
    return out;
  }
  std::shared_ptr<DecryptionShares> decrypt_share(const HipValuation &enc, uint32_t smudge_bits, uint64_t seed = 0) {
    auto out = new_shares(smudge_bits, false, 1);
    std::vector<std::pair<std::string, const HostCipher *>> cs; // (std::map / sorted below: names in order)
    for (auto &kv : enc.values)
      if (auto *c = std::get_if<HostCipher>(&kv.second)) cs.emplace_back(kv.first, c);
    std::sort(cs.begin(), cs.end(), [](auto &a, auto &b) { return a.first < b.first; });
    for (auto &nc : cs) {
      if (nc.second->size != 2) throw std::invalid_argument("value " + nc.first + ": decryption share expects a size-2 ciphertext (relinearize first)");
      if (nc.second->limbs >= 1 && nc.second->limbs <= host->k - 1 && flood_exceeds_modulus(host->primes, nc.second->limbs, 1, smudge_bits))
        throw std::invalid_argument("value " + nc.first + ": smudge_bits leaves no room at this level");
    }
    std::unique_ptr<SecureRng> stream = client_stream(seed, 5);
    std::vector<std::vector<std::array<uint8_t, 32>>> fk(1);
    WipeKeyRows wipe_keys{fk};
    for (size_t i = 0; i < cs.size(); i++) fk[0].push_back(draw_key32(*stream));
    for (size_t i = 0; i < cs.size(); i++) {
      const std::string &name = cs[i].first;
      const HostCipher &c = *cs[i].second;
      SharePiece piece;
      piece.n = 1;
      piece.limbs = c.limbs;
      piece.scale = c.scale;
      if (on_device()) {
        std::vector<CtHandle> keep; // resident on this GPU, whichever key pair's state: read in place
        const evah_ct *h = source_handle(dev, *host, "output " + name, c, keep, InPlace::SameGpu, BringOver::Upload);
        evah_ct *o = nullptr;
        chk(evah_decrypt_share_handles(dev->h, &h, 1, smudge_bits, fk[0][i].data(), &o));
        piece.h = std::make_shared<CtHandle>(dev->h, o);
        piece.root = dev;
      } else {
        check_cipher_shape(*host, "value " + name, c, 2, 2);
        (void)words(c); // the host twin reads the words: a resident value comes down here
        piece.data = decrypt_share_host(*host, sk, c, smudge_bits, fk[0][i]);
      }
      out->values[name].push_back(std::move(piece));
    }
    return out;
  }
  // the same for a batch of batched handles: per name, consecutive segments of one level are packed into calls of <= 64
  // instances, as decrypt_array packs them; a batch resident on another state of the same GPU is read in place
  std::shared_ptr<DecryptionShares> decrypt_share_batch(const HipValuationBatch &vb, uint32_t smudge_bits, uint64_t seed = 0) {
    require_array_path(on_device(), resident, "decrypt_share");
    auto out = new_shares(smudge_bits, true, vb.B);
    if (!vb.root) throw std::runtime_error("decrypt_share: the batch holds no device handles");
    for (auto &nc : vb.ciphers)
      for (auto &seg : nc.second.segments) {
        if (seg.size != 2) throw std::invalid_argument("value " + nc.first + ": decryption share expects a size-2 ciphertext (relinearize first)");
        if (seg.limbs >= 1 && seg.limbs <= host->k - 1 && flood_exceeds_modulus(host->primes, seg.limbs, 1, smudge_bits))
          throw std::invalid_argument("value " + nc.first + ": smudge_bits leaves no room at this level");
      }
    std::unique_ptr<SecureRng> stream = client_stream(seed, 5);
    std::vector<std::vector<std::array<uint8_t, 32>>> fk(vb.ciphers.size()); // per name (sorted: std::map), per instance
    WipeKeyRows wipe_keys{fk};
    for (size_t i = 0; i < vb.ciphers.size(); i++)
      for (size_t b = 0; b < vb.B; b++) fk[i].push_back(draw_key32(*stream));
    size_t i = 0;
    for (auto &nc : vb.ciphers) {
      const auto &segs = nc.second.segments;
      std::vector<SharePiece> &pieces = out->values[nc.first];
      walk_segments("value " + nc.first, segs, vb.B, dev, vb.root, [&](SegmentGroup &g) {
        std::vector<uint8_t> keys = keys_flat(fk[i].data() + g.row, g.n);
        evah_ct *o = nullptr;
        const int rc = evah_decrypt_share_handles(dev->h, g.hs.data(), (uint32_t)g.hs.size(), smudge_bits, keys.data(), &o);
        wipe_bytes(keys.data(), keys.size());
        chk(rc);
        SharePiece piece;
        piece.n = (uint32_t)g.n;
        piece.limbs = segs[g.s0].limbs;
        piece.scale = segs[g.s0].scale;
        piece.h = std::make_shared<CtHandle>(dev->h, o);
        piece.root = dev;
        pieces.push_back(std::move(piece));
      });
      i++;
    }
    return out;
  }
};

// generateKeys (seal.cpp:174-203): prime chain from bit sizes, secret/public key, one Galois key
// per exact rotation step, relinearization key.  compress_keys: the relinearization and Galois keys are
// generated, kept, saved and uploaded as c0 plus a 32-byte seed per digit; the secret and the public key are drawn
// before any of them, so they are the same with and without the option for one test seed.
// device_keygen: the same compressed keys, word for word, with c0 computed by evah_keygen_switch on the
// key pair's device state from the host's draws (KeyGenerator::draw_seeded_digit).  devices / shard (null: the
// environment's defaults) are set before any key is made, so that the device state is created on the right device; in the
// default single-device mode the keys stay installed there and the first execute() uploads none.
// device_sampling: every polynomial of the key set is expanded from a 32-byte key of its own
// (KeyGenerator's sampled mode says which) — compressed keys again.  With device_keygen the device draws them:
// one evah_keygen_public and one evah_keygen_set for all evaluation keys, and in the default single-device mode no c0
// comes back until somebody needs it (SwitchKey::c0_words).  Without it the host twin computes the same words.
// common_seed: the collective key generation — the sampled derivation with the public stream keyed by 32
// bytes every party knows, so that all parties expand the same a and the same c1 of every digit, and their keys add up
// (combine_public_contexts).  The secret stream is the party's own, as ever.
inline std::pair<std::shared_ptr<HipPublic>, std::shared_ptr<HipSecret>>
generate_keys(const CKKSParameters &params, uint64_t seed = 0, bool compress_keys = false, bool device_keygen = false,
              const std::vector<int> *devices = nullptr, const std::string *shard = nullptr, bool device_sampling = false,
              const std::array<uint8_t, 32> *common_seed = nullptr) {
  if (common_seed) device_sampling = true; // the collective key generation is the sampled derivation on a stream the parties share
  std::vector<int> bits(params.prime_bits.begin(), params.prime_bits.end());
  if (bits.size() < 2) throw std::invalid_argument("need at least two primes (data + special)");
  auto primes = evah::coeff_modulus_create(params.poly_modulus_degree, bits);
  auto host = std::make_shared<HostContext>(params.poly_modulus_degree, primes);
  // seed == 0: keyed from the OS; otherwise the reproducible test hook.  common_seed: the public stream the parties share
  KeyGenerator kg(*host, seed, device_sampling, common_seed ? common_seed->data() : nullptr);
  auto pub = std::make_shared<HipPublic>();
  auto sec = std::make_shared<HipSecret>();
  sec->holder = pub->holder; // one device state for the pair: results stay resident from encrypt to decrypt
  if (devices) {
    pub->devices = *devices;
    // the key pair's own device state (inputs, constants, outputs; the secret half decrypts there) is member 0
    if (!pub->devices.empty()) pub->device = sec->device = physical_device(pub->devices[0]);
  }
  if (shard) pub->shard_mode = *shard;
  pub->host = host;
  sec->host = host;
  sec->sk = kg.sk;
  const uint32_t N = host->N, m = 2 * N, D = host->k - 1;
  const bool install = pub->devices.empty() && pub->shard_mode.empty(); // every other mode uploads from the host's c0 + seeds
  if (device_keygen) {
    // the key pair's device state is created here, not by the first execute(): a one-member `devices` list names its
    // device wherever the list came from (the argument above or EVA_DEVICES / EVA_NUM_GPUS), as ensure_device rules
    if (pub->devices.size() == 1) pub->device = sec->device = physical_device(pub->devices[0]);
  }
  if (device_keygen && !sec->on_device())
    throw std::runtime_error("device_keygen needs a HIP device: none is visible, or EVA_DEVICE_CLIENT=0 keeps the client on the host");
  const bool device_set = device_keygen && device_sampling;
  if (device_set) { // the host paths (encrypt without a device, save) need pk, so it comes back
    pub->pk.data.resize((size_t)2 * host->k * N);
    chk(evah_keygen_public(sec->dev->h, kg.ek_pk.data(), kg.seed_pk.data(), install ? 1 : 0, (uint64_t *)pub->pk.data.data()));
    if (install) pub->public_key_installed();
  } else {
    pub->pk = kg.public_key();
  }
  // one key on the device: the draws of switch_key(., seeded) in its order, then evah_keygen_switch
  auto device_key = [&](int kind, uint32_t elt) {
    SwitchKey key;
    key.n_digits = D;
    key.seeds.resize((size_t)32 * D);
    key.c0.resize((size_t)D * host->k * N);
    std::vector<int8_t> errors((size_t)D * N), e;
    for (uint32_t J = 0; J < D; J++) {
      kg.draw_seeded_digit(key.seeds.data() + (size_t)32 * J, e);
      std::copy(e.begin(), e.end(), errors.begin() + (size_t)J * N);
    }
    wipe(e);
    const int rc = evah_keygen_switch(sec->dev->h, kind, elt, D, errors.data(), key.seeds.data(), install ? 1 : 0, (uint64_t *)key.c0.data());
    wipe(errors);
    chk(rc);
    return key;
  };
  // the keys of the set in key order — the relinearization key, then one Galois key per distinct rotation step
  std::vector<uint32_t> elts;
  for (int step : params.rotations) {
    uint32_t elt;
    if (step == 0) elt = m - 1;
    else {
      uint32_t pos = step < 0 ? (uint32_t)(-(int64_t)step) : (uint32_t)step;
      if (pos >= (N >> 1)) throw std::invalid_argument("step count too large");
      uint32_t s = step < 0 ? (N >> 1) - pos : pos;
      elt = 1;
      for (uint32_t i = 0; i < s; i++) elt = (elt * 3u) & (m - 1);
    }
    if (std::find(elts.begin(), elts.end(), elt) == elts.end()) elts.push_back(elt);
  }
  if (device_set) {
    // all draws first, in KeyGenerator's order; then the whole set as one call
    const size_t n_keys = 1 + elts.size();
    std::vector<int> kinds(n_keys, EVAH_KEY_GALOIS);
    std::vector<uint32_t> ids(n_keys, 0);
    kinds[0] = EVAH_KEY_RELIN;
    std::copy(elts.begin(), elts.end(), ids.begin() + 1);
    std::vector<uint8_t> ekeys(n_keys * D * 32), seeds(n_keys * D * 32);
    for (size_t j = 0; j < n_keys; j++) {
      for (uint32_t J = 0; J < D; J++) kg.draw_sampled_digit(seeds.data() + (j * D + J) * 32, ekeys.data() + (j * D + J) * 32);
      kg.keep_ekeys(ids[j], ekeys.data() + j * D * 32, D);
    }
    const size_t key_words = (size_t)D * host->k * N;
    std::vector<u64> c0(install ? 0 : n_keys * key_words); // the default mode leaves c0 where the keys are
    const int rc = evah_keygen_set(sec->dev->h, (uint32_t)n_keys, kinds.data(), ids.data(), D, ekeys.data(), seeds.data(), install ? 1 : 0,
                                   install ? nullptr : (uint64_t *)c0.data());
    wipe_bytes(ekeys.data(), ekeys.size());
    chk(rc);
    for (size_t j = 0; j < n_keys; j++) {
      SwitchKey key;
      key.n_digits = D;
      key.seeds.assign(seeds.begin() + j * D * 32, seeds.begin() + (j + 1) * D * 32);
      if (install) {
        const int kind = kinds[j];
        const uint32_t elt = ids[j];
        key.source = [holder = pub->holder, kind, elt, D, key_words](std::vector<u64> &out) {
          std::vector<u64> w(key_words);
          chk(evah_key_download_c0(holder->dev->h, kind, elt, D, (uint64_t *)w.data()));
          out = std::move(w);
        };
      } else {
        key.c0.assign(c0.begin() + j * key_words, c0.begin() + (j + 1) * key_words);
      }
      if (j == 0) pub->relin = std::move(key);
      else pub->galois.emplace(ids[j], std::move(key));
    }
  } else {
    pub->relin = device_keygen ? device_key(EVAH_KEY_RELIN, 0) : kg.relin_key(compress_keys);
    for (uint32_t elt : elts) pub->galois.emplace(elt, device_keygen ? device_key(EVAH_KEY_GALOIS, elt) : kg.galois_key(elt, compress_keys));
  }
  if (device_keygen && install) pub->eval_keys_installed();
  sec->key_randomness = std::move(kg.kept);
  if (common_seed) sec->common_relin_seeds = pub->relin.seeds; // public, equal across the parties: what DESIGN.md 1.15 derives its rows from
  return {pub, sec};
}

// The collective public context of parties whose keys were generated with one common_seed: the public
// key and every Galois key present in ALL contexts, under s = sum_p s_p.  All parties expanded the same a (pk[1]) and the
// same c1 of every digit, so c0 adds: sum_p -(a s_p + e_p) = -(a s + sum_p e_p), and a Galois digit's P s_p(X^elt) terms
// add to P s(X^elt).  The sums run on the host.  The relinearization key does not add up (s^2 is not the sum of the
// s_p^2): it comes from the two rounds of DESIGN.md 1.15 — relin_round1 = the sum of the round-1 shares
// (combine_relin_shares), relin_round2 = one round-2 share per context — as (c0, c1) = (sum_p g_p, H1), an ordinary
// uncompressed key.  Both or neither: without them the context has no relinearization key, as before.
inline std::shared_ptr<HipPublic> combine_public_contexts(const std::vector<std::shared_ptr<HipPublic>> &ctxs,
                                                          const std::shared_ptr<const RelinShare> &relin_round1 = nullptr,
                                                          const std::vector<std::shared_ptr<const RelinShare>> *relin_round2 = nullptr) {
  if (ctxs.empty() || ctxs.size() > 64) throw std::invalid_argument("combine_public_contexts: 1..64 public contexts are needed");
  for (auto &c : ctxs)
    if (!c) throw std::invalid_argument("combine_public_contexts: a context is None");
  if ((relin_round1 != nullptr) != (relin_round2 != nullptr))
    throw std::invalid_argument("combine_public_contexts: relin_round1 and relin_round2 go together: give both or neither");
  SwitchKey collective_relin;
  if (relin_round1) {
    const HostContext &h0 = *ctxs[0]->host;
    const size_t poly0 = (size_t)h0.k * h0.N;
    if (relin_round2->size() != ctxs.size())
      throw std::invalid_argument("combine_public_contexts: " + std::to_string(relin_round2->size()) + " round-2 shares for " +
                                  std::to_string(ctxs.size()) + " public contexts: every party contributes one");
    auto check = [&](const RelinShare *s, uint32_t round, const std::string &what) {
      if (!s) throw std::invalid_argument("combine_public_contexts: " + what + " is None");
      if (s->round != round) throw std::invalid_argument("combine_public_contexts: " + what + " is a round-" + std::to_string(s->round) + " share");
      const std::string diff = rekey_params_differ(s->N, s->primes, h0);
      if (!diff.empty()) throw std::invalid_argument("combine_public_contexts: " + what + " was made under other encryption parameters than context 0: " + diff);
      if (s->n_digits == 0 || s->n_digits > h0.k - 1 || s->data.size() != (size_t)s->n_digits * (round == 1 ? 2 : 1) * poly0)
        throw std::invalid_argument("combine_public_contexts: " + what + ": the words do not match the shape");
      if (!residues_canonical(s->data, h0)) throw std::invalid_argument("combine_public_contexts: " + what + " holds a word that is not reduced modulo its prime");
    };
    check(relin_round1.get(), 1, "relin_round1");
    const uint32_t D = relin_round1->n_digits;
    collective_relin.n_digits = D;
    collective_relin.data.assign((size_t)D * 2 * poly0, 0);
    for (size_t p = 0; p < relin_round2->size(); p++) {
      const RelinShare *g = (*relin_round2)[p].get();
      check(g, 2, "round-2 share " + std::to_string(p));
      if (g->n_digits != D) throw std::invalid_argument("combine_public_contexts: round-2 share " + std::to_string(p) + " has another digit count than relin_round1");
      for (uint32_t J = 0; J < D; J++) // c0 of digit J += g_p[J]
        for (size_t r = 0; r < h0.k; r++) {
          const u64 q = h0.primes[r];
          u64 *a = collective_relin.data.data() + ((size_t)2 * J * h0.k + r) * h0.N;
          const u64 *b = g->data.data() + ((size_t)J * h0.k + r) * h0.N;
          for (size_t j = 0; j < h0.N; j++) a[j] = evah::addmod(a[j], b[j], q);
        }
    }
    for (uint32_t J = 0; J < D; J++) // c1 of digit J = H1[J]
      std::copy_n(relin_round1->data.begin() + ((size_t)2 * J + 1) * poly0, poly0, collective_relin.data.begin() + ((size_t)2 * J + 1) * poly0);
  }
  const HostContext &hc = *ctxs[0]->host;
  const size_t N = hc.N, k = hc.k, poly = k * N;
  auto add_rows = [&](std::vector<u64> &acc, const u64 *src, size_t rows) { // acc [rows][N] += src, row r under prime r % k
    for (size_t r = 0; r < rows; r++) {
      const u64 q = hc.primes[r % k];
      u64 *a = acc.data() + r * N;
      const u64 *b = src + r * N;
      for (size_t j = 0; j < N; j++) a[j] = evah::addmod(a[j], b[j], q);
    }
  };
  auto out = std::make_shared<HipPublic>();
  out->host = ctxs[0]->host;
  out->collective = true;
  out->pk.data.assign(ctxs[0]->pk.data.begin(), ctxs[0]->pk.data.end());
  if (out->pk.data.size() != 2 * poly) throw std::invalid_argument("combine_public_contexts: context 0 holds no public key");
  for (size_t p = 1; p < ctxs.size(); p++) {
    const std::string diff = rekey_params_differ(ctxs[p]->host->N, ctxs[p]->host->primes, hc);
    if (!diff.empty())
      throw std::invalid_argument("combine_public_contexts: context " + std::to_string(p) + " has other encryption parameters than context 0: " + diff);
    const auto &pk = ctxs[p]->pk.data;
    if (pk.size() != 2 * poly) throw std::invalid_argument("combine_public_contexts: context " + std::to_string(p) + " holds no public key");
    if (!std::equal(pk.begin() + poly, pk.end(), out->pk.data.begin() + poly))
      throw std::invalid_argument("public contexts do not share a common seed (context " + std::to_string(p) + " differs from context 0)");
    std::vector<u64> c0(out->pk.data.begin(), out->pk.data.begin() + poly);
    add_rows(c0, pk.data(), k);
    std::copy(c0.begin(), c0.end(), out->pk.data.begin());
  }
  for (size_t p = 1; p < ctxs.size(); p++) // elements context 0 lacks are dropped as well
    for (auto &kv : ctxs[p]->galois)
      if (!ctxs[0]->galois.count(kv.first) && std::find(out->dropped_galois.begin(), out->dropped_galois.end(), kv.first) == out->dropped_galois.end())
        out->dropped_galois.push_back(kv.first);
  for (auto &kv : ctxs[0]->galois) {
    const uint32_t elt = kv.first;
    bool everywhere = true;
    for (size_t p = 1; p < ctxs.size(); p++) everywhere = everywhere && ctxs[p]->galois.count(elt);
    if (!everywhere) { // kept out, and named: rotations by it are refused at execute ("Galois key not present")
      out->dropped_galois.push_back(elt);
      continue;
    }
    const SwitchKey &k0 = kv.second;
    if (!k0.compressed()) throw std::invalid_argument("combine_public_contexts: context 0's Galois keys are not seed-compressed (generate_keys(..., common_seed))");
    SwitchKey sum;
    sum.n_digits = k0.n_digits;
    sum.seeds = k0.seeds;
    sum.c0 = k0.c0_words();
    for (size_t p = 1; p < ctxs.size(); p++) {
      const SwitchKey &kp = ctxs[p]->galois.at(elt);
      if (kp.n_digits != k0.n_digits || kp.seeds != k0.seeds)
        throw std::invalid_argument("public contexts do not share a common seed (context " + std::to_string(p) + " differs from context 0)");
      const std::vector<u64> &c0 = kp.c0_words();
      if (c0.size() != sum.c0.size()) throw std::invalid_argument("combine_public_contexts: context " + std::to_string(p) + ": Galois key words do not match their shape");
      add_rows(sum.c0, c0.data(), (size_t)sum.n_digits * k);
    }
    out->galois.emplace(elt, std::move(sum));
  }
  if (relin_round1) out->relin = std::move(collective_relin);
  return out;
}

// Aggregate 1 of DESIGN.md 1.15: (H0, H1) = the row-by-row sums of the parties' round-1 shares, itself a round-1 share.
// Public: anyone may form it.  On the host, as the Galois sums above (the shares arrive as host words or files anyway).
inline std::shared_ptr<RelinShare> combine_relin_shares(const std::vector<std::shared_ptr<const RelinShare>> &shares) {
  if (shares.empty() || shares.size() > 64) throw std::invalid_argument("combine_relin_shares: round-1 shares of 1..64 parties are needed");
  for (size_t p = 0; p < shares.size(); p++) {
    if (!shares[p]) throw std::invalid_argument("combine_relin_shares: share " + std::to_string(p) + " is None");
    if (shares[p]->round != 1)
      throw std::invalid_argument("combine_relin_shares: share " + std::to_string(p) + " is a round-" + std::to_string(shares[p]->round) + " share: round-1 shares are summed");
  }
  const RelinShare &s0 = *shares[0];
  const size_t k = s0.primes.size(), N = s0.N, words = (size_t)s0.n_digits * 2 * k * N;
  if (s0.n_digits == 0 || k < 2 || s0.n_digits > k - 1 || s0.data.size() != words) throw std::invalid_argument("combine_relin_shares: share 0: the words do not match the shape");
  auto out = std::make_shared<RelinShare>(s0);
  for (size_t p = 1; p < shares.size(); p++) {
    const RelinShare &s = *shares[p];
    if (s.N != s0.N)
      throw std::invalid_argument("combine_relin_shares: share " + std::to_string(p) + " was made under other encryption parameters than share 0: poly_modulus_degree differs (" +
                                  std::to_string(s.N) + " against " + std::to_string(s0.N) + ")");
    if (s.primes.size() != k)
      throw std::invalid_argument("combine_relin_shares: share " + std::to_string(p) + " was made under other encryption parameters than share 0: the number of primes differs");
    for (size_t i = 0; i < k; i++)
      if (s.primes[i] != s0.primes[i])
        throw std::invalid_argument("combine_relin_shares: share " + std::to_string(p) + " was made under other encryption parameters than share 0: prime " + std::to_string(i) + " differs");
    if (s.n_digits != s0.n_digits) throw std::invalid_argument("combine_relin_shares: share " + std::to_string(p) + " has another digit count than share 0");
    if (s.data.size() != words) throw std::invalid_argument("combine_relin_shares: share " + std::to_string(p) + ": the words do not match the shape");
    for (size_t r = 0; r < words / N; r++) {
      const u64 q = s0.primes[r % k];
      u64 *a = out->data.data() + r * N;
      const u64 *b = s.data.data() + r * N;
      for (size_t j = 0; j < N; j++) a[j] = evah::addmod(a[j], b[j], q);
    }
  }
  return out;
}

} // namespace evahost
