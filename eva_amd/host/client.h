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

// SEALPublic::encrypt (seal.cpp:24-102)
inline HipValuation HipPublic::encrypt(const Valuation &inputs, const CKKSSignature &sig) {
  const size_t slots = host->N / 2;
  if (sig.vec_size <= 0) throw std::runtime_error("Signature vector size must be positive");
  if (slots < (size_t)sig.vec_size) throw std::runtime_error("Vector size cannot be larger than slot count");
  if (slots % sig.vec_size) throw std::runtime_error("Vector size must exactly divide the slot count");
  HipValuation out;
  SecureRng rng; // a fresh ChaCha20 stream keyed with 256 bits from the OS for this call (csprng.h)
  for (auto &kv : inputs) {
    const auto &v = kv.second;
    if (v.size() != (size_t)sig.vec_size) throw std::runtime_error("Input size does not match program vector size");
    auto it = sig.inputs.find(kv.first);
    if (it == sig.inputs.end()) throw std::out_of_range("No input named " + kv.first + " in the signature");
    const CKKSEncodingInfo &info = it->second;
    if (info.input_type == Type::Cipher || info.input_type == Type::Plain) {
      if ((uint32_t)info.level >= host->k - 1) throw std::runtime_error("Input level exceeds the modulus chain");
      HostPlain pt;
      pt.limbs = host->k - 1 - (uint32_t)info.level;
      pt.scale = std::pow(2.0, (double)info.scale);
      if (info.input_type == Type::Cipher && client_on_device() && device_encodable(v, pt.scale, pt.limbs)) {
        // encoder and encryptor both on the GPU (evah_pt_encode -> evah_encrypt): the plaintext never
        // exists on the host.  Same plaintext as the host encoder bit for bit (tests/test_encode_parity.py)
        // and the same sampler calls in the same order, hence the same ciphertext as every other path
        out.values[kv.first] = encrypt_on_device(nullptr, &v, pt.scale, pt.limbs, rng);
        continue;
      }
      pt.data.resize((size_t)pt.limbs * host->N);
      std::vector<double> vec(slots);
      for (size_t r = 0; r < slots / v.size(); r++) std::copy(v.begin(), v.end(), vec.begin() + r * v.size());
      host->encode_coeff(vec.data(), pt.scale, pt.limbs, pt.data.data());
      if (info.input_type == Type::Cipher && client_on_device()) {
        // device path: the per-limb transforms, the public-key products and the mod-down run on the
        // GPU (evah_encrypt); the host keeps the FP64 encoder and the sampling (same sampler calls,
        // in the same order, as evahost::encrypt — so both paths give the same ciphertext for the
        // same random stream)
        out.values[kv.first] = encrypt_on_device(&pt, nullptr, pt.scale, pt.limbs, rng);
        continue;
      }
      for (uint32_t i = 0; i < pt.limbs; i++) host->ntt(i, pt.data.data() + (size_t)i * host->N);
      if (info.input_type == Type::Cipher) out.values[kv.first] = evahost::encrypt(*host, pk, pt, rng);
      else out.values[kv.first] = std::move(pt);
    } else {
      out.values[kv.first] = v;
    }
  }
  return out;
}

// EVA_DEVICE_CLIENT=0 keeps encrypt on the host; without a HIP device the host path is the only one
// (encrypt, unlike execute(), is client-side work the reference also does on the CPU)
inline bool HipPublic::client_on_device() {
  if (client_device < 0) {
    const char *e = std::getenv("EVA_DEVICE_CLIENT");
    int n = 0;
    client_device = (!e || std::atoi(e) != 0) && evah_device_count(&n) == 0 && n > 0 ? 1 : 0;
  }
  return client_device == 1;
}

// same bound as HipExecutor::device_encodable: every rounded coefficient below 2^62 and inside the modulus
inline bool device_encodable(const HostContext &hc, const std::vector<double> &in, double scale, uint32_t limbs) {
  const size_t slots = hc.N / 2;
  if (std::getenv("EVA_DEVICE_ENCODE") && !std::atoi(std::getenv("EVA_DEVICE_ENCODE"))) return false;
  if (in.empty() || in.size() > slots || slots % in.size()) return false;
  double sum = 0;
  for (double x : in) {
    if (!std::isfinite(x)) return false;
    sum += std::fabs(x);
  }
  const double bound = 2.0 * sum * (double)(slots / in.size()) * scale / (double)hc.N;
  const int bits = (int)std::ceil(std::log2(std::max(bound, 1.0))) + 1;
  return bits < 62 && bits < hc.total_bits[limbs];
}
inline bool HipPublic::device_encodable(const std::vector<double> &in, double scale, uint32_t limbs) const {
  return evahost::device_encodable(*host, in, scale, limbs);
}

// coeff_pt: the host encoder's coefficient-form plaintext, or (null) values: the slot values for the device encoder
inline HostCipher HipPublic::encrypt_on_device(const HostPlain *coeff_pt, const std::vector<double> *values, double scale, uint32_t limbs, SecureRng &rng) {
  const uint32_t N = host->N;
  std::vector<int8_t> u, e0, e1, small((size_t)3 * N);
  host->sample_ternary(rng, u);
  host->sample_error(rng, e0);
  host->sample_error(rng, e1);
  std::copy(u.begin(), u.end(), small.begin());
  std::copy(e0.begin(), e0.end(), small.begin() + N);
  std::copy(e1.begin(), e1.end(), small.begin() + 2 * (size_t)N);
  return encrypt_on_device_with(coeff_pt, values, scale, limbs, small);
}
inline HostCipher HipPublic::encrypt_on_device_with(const HostPlain *coeff_pt, const std::vector<double> *values, double scale, uint32_t limbs,
                                                    const std::vector<int8_t> &small) {
  ensure_device(false);
  if (!pk_uploaded) {
    chk(evah_client_key_upload(dev->h, EVAH_KEY_PUBLIC, (const uint64_t *)pk.data.data()));
    pk_uploaded = true;
  }
  const uint32_t N = host->N;
  evah_pt *p = nullptr;
  if (coeff_pt) chk(evah_pt_upload_coeff(dev->h, limbs, scale, (const uint64_t *)coeff_pt->data.data(), &p));
  else chk(evah_pt_encode(dev->h, values->data(), (uint32_t)values->size(), limbs, scale, &p));
  evah_ct *c = nullptr;
  int rc = evah_encrypt(dev->h, p, small.data(), &c);
  evah_pt_free(dev->h, p);
  chk(rc);
  HostCipher out;
  out.size = 2;
  out.limbs = limbs;
  out.scale = scale;
  auto handle = std::make_shared<CtHandle>(dev->h, c);
  if (resident) { // stays in HBM; host words on demand
    out.dev = std::make_shared<DeviceResident>(DeviceResident{dev, nullptr, handle, host->N});
    return out;
  }
  out.data.resize((size_t)2 * out.limbs * N);
  out.words_checked = true;
  chk(evah_ct_download(dev->h, c, (uint64_t *)out.data.data()));
  return out;
}

// the Cipher branch of encrypt() for one input, the randomness given: device encoder + encryptor, host encoder + device
// encryptor, or the host alone — the same words on each
inline HostCipher HipPublic::encrypt_value_with(const std::vector<double> &v, double scale, uint32_t limbs, const std::vector<int8_t> &small) {
  if (client_on_device() && device_encodable(v, scale, limbs)) return encrypt_on_device_with(nullptr, &v, scale, limbs, small);
  const size_t slots = host->N / 2, N = host->N;
  HostPlain pt;
  pt.limbs = limbs;
  pt.scale = scale;
  pt.data.resize((size_t)limbs * N);
  std::vector<double> vec(slots);
  for (size_t r = 0; r < slots / v.size(); r++) std::copy(v.begin(), v.end(), vec.begin() + r * v.size());
  host->encode_coeff(vec.data(), scale, limbs, pt.data.data());
  if (client_on_device()) return encrypt_on_device_with(&pt, nullptr, scale, limbs, small);
  for (uint32_t i = 0; i < limbs; i++) host->ntt(i, pt.data.data() + (size_t)i * N);
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
  const size_t slots = host->N / 2;
  if (seed && !device_sampling) throw std::invalid_argument("encrypt_batch: seed is the test hook of device_sampling and needs device_sampling=True");
  if (sig.vec_size <= 0) throw std::runtime_error("Signature vector size must be positive");
  if (slots < (size_t)sig.vec_size) throw std::runtime_error("Vector size cannot be larger than slot count");
  if (slots % sig.vec_size) throw std::runtime_error("Vector size must exactly divide the slot count");
  std::vector<HipValuation> out(inputs.size());
  if (inputs.empty()) return out;
  const std::vector<std::string> names = batch_input_names(inputs);
  if (device_sampling) {
    std::unique_ptr<SecureRng> stream = seed ? std::make_unique<SecureRng>(seed, 5) : std::make_unique<SecureRng>();
    std::vector<std::vector<std::array<uint8_t, 32>>> rkeys(names.size()); // per name, per instance
    struct WipeKeys {
      std::vector<std::vector<std::array<uint8_t, 32>>> &k;
      ~WipeKeys() { for (auto &n : k) for (auto &x : n) wipe_bytes(x.data(), 32); }
    } wipe_keys{rkeys};
    std::vector<const CKKSEncodingInfo *> infos(names.size());
    for (size_t i = 0; i < names.size(); i++) {
      auto it = sig.inputs.find(names[i]);
      if (it == sig.inputs.end()) throw std::out_of_range("No input named " + names[i] + " in the signature");
      infos[i] = &it->second;
      if (it->second.input_type == Type::Cipher && (uint32_t)it->second.level >= host->k - 1) throw std::runtime_error("Input level exceeds the modulus chain");
    }
    for (size_t b = 0; b < inputs.size(); b++)
      for (size_t i = 0; i < names.size(); i++) {
        if (inputs[b].at(names[i]).size() != (size_t)sig.vec_size) throw std::runtime_error("Input size does not match program vector size");
        if (infos[i]->input_type == Type::Cipher) rkeys[i].push_back(draw_key32(*stream));
      }
    for (size_t i = 0; i < names.size(); i++) {
      const std::string &name = names[i];
      if (infos[i]->input_type != Type::Cipher) { // plain and raw inputs take no randomness: encrypt()'s path
        for (size_t b = 0; b < inputs.size(); b++) {
          HipValuation one = encrypt(Valuation{{name, inputs[b].at(name)}}, sig);
          out[b].values[name] = std::move(one.values.at(name));
        }
        continue;
      }
      const uint32_t limbs = host->k - 1 - (uint32_t)infos[i]->level;
      const double scale = std::pow(2.0, (double)infos[i]->scale);
      bool grouped = client_on_device();
      for (size_t b = 0; grouped && b < inputs.size(); b++) grouped = device_encodable(inputs[b].at(name), scale, limbs);
      if (!grouped) { // the same keys through the host twin, instance by instance
        for (size_t b = 0; b < inputs.size(); b++) {
          std::vector<int8_t> small = sampled_small3(rkeys[i][b], host->N);
          struct WipeSmall {
            std::vector<int8_t> &s;
            ~WipeSmall() { wipe(s); }
          } wipe_small{small};
          out[b].values[name] = encrypt_value_with(inputs[b].at(name), scale, limbs, small);
        }
        continue;
      }
      for (size_t b0 = 0; b0 < inputs.size(); b0 += CLIENT_BATCH_MAX) {
        const size_t n = std::min<size_t>(CLIENT_BATCH_MAX, inputs.size() - b0);
        std::vector<const std::vector<double> *> vals(n);
        for (size_t b = 0; b < n; b++) vals[b] = &inputs[b0 + b].at(name);
        std::vector<HostCipher> cts = encrypt_group_sampled(vals, scale, limbs, rkeys[i].data() + b0);
        for (size_t b = 0; b < n; b++) out[b0 + b].values[name] = std::move(cts[b]);
      }
    }
    return out;
  }
  SecureRng rng; // one fresh ChaCha20 stream keyed from the OS for the whole call
  for (const std::string &name : names) {
    auto it = sig.inputs.find(name);
    if (it == sig.inputs.end()) throw std::out_of_range("No input named " + name + " in the signature");
    const CKKSEncodingInfo &info = it->second;
    bool grouped = info.input_type == Type::Cipher && client_on_device();
    uint32_t limbs = 0;
    double scale = 0;
    if (grouped) {
      if ((uint32_t)info.level >= host->k - 1) throw std::runtime_error("Input level exceeds the modulus chain");
      limbs = host->k - 1 - (uint32_t)info.level;
      scale = std::pow(2.0, (double)info.scale);
    }
    for (size_t b = 0; b < inputs.size(); b++) {
      const auto &v = inputs[b].at(name);
      if (v.size() != (size_t)sig.vec_size) throw std::runtime_error("Input size does not match program vector size");
      if (grouped && !device_encodable(v, scale, limbs)) grouped = false;
    }
    if (!grouped) { // encrypt()'s path, instance by instance
      for (size_t b = 0; b < inputs.size(); b++) {
        HipValuation one = encrypt(Valuation{{name, inputs[b].at(name)}}, sig);
        out[b].values[name] = std::move(one.values.at(name));
      }
      continue;
    }
    for (size_t b0 = 0; b0 < inputs.size(); b0 += CLIENT_BATCH_MAX) {
      const size_t n = std::min<size_t>(CLIENT_BATCH_MAX, inputs.size() - b0);
      std::vector<const std::vector<double> *> vals(n);
      for (size_t b = 0; b < n; b++) vals[b] = &inputs[b0 + b].at(name);
      std::vector<HostCipher> cts = encrypt_group_on_device(vals, scale, limbs, rng);
      for (size_t b = 0; b < n; b++) out[b0 + b].values[name] = std::move(cts[b]);
    }
  }
  return out;
}

// one group of encrypt_batch: the sampler calls of encrypt_on_device per instance, in list order, then one device call
inline std::vector<HostCipher> HipPublic::encrypt_group_on_device(const std::vector<const std::vector<double> *> &vals, double scale,
                                                                  uint32_t limbs, SecureRng &rng) {
  ensure_device(false);
  if (!pk_uploaded) {
    chk(evah_client_key_upload(dev->h, EVAH_KEY_PUBLIC, (const uint64_t *)pk.data.data()));
    pk_uploaded = true;
  }
  const uint32_t N = host->N;
  const size_t B = vals.size(), nv = vals[0]->size();
  std::vector<double> flat(B * nv);
  std::vector<int8_t> u, e0, e1, small(B * 3 * N);
  for (size_t b = 0; b < B; b++) {
    std::copy(vals[b]->begin(), vals[b]->end(), flat.begin() + b * nv);
    host->sample_ternary(rng, u);
    host->sample_error(rng, e0);
    host->sample_error(rng, e1);
    std::copy(u.begin(), u.end(), small.begin() + (3 * b) * N);
    std::copy(e0.begin(), e0.end(), small.begin() + (3 * b + 1) * N);
    std::copy(e1.begin(), e1.end(), small.begin() + (3 * b + 2) * N);
  }
  evah_ct *c = nullptr;
  const int rc = evah_encode_encrypt_many(dev->h, (uint32_t)B, flat.data(), (uint32_t)nv, limbs, scale, small.data(), &c);
  wipe(u); wipe(e0); wipe(e1); wipe(small);
  chk(rc);
  return group_results(c, B, scale, limbs);
}

inline std::vector<HostCipher> HipPublic::encrypt_group_sampled(const std::vector<const std::vector<double> *> &vals, double scale, uint32_t limbs,
                                                                const std::array<uint8_t, 32> *rkeys) {
  ensure_device(false);
  if (!pk_uploaded) {
    chk(evah_client_key_upload(dev->h, EVAH_KEY_PUBLIC, (const uint64_t *)pk.data.data()));
    pk_uploaded = true;
  }
  const size_t B = vals.size(), nv = vals[0]->size();
  std::vector<double> flat(B * nv);
  std::vector<uint8_t> keys(B * 32);
  for (size_t b = 0; b < B; b++) {
    std::copy(vals[b]->begin(), vals[b]->end(), flat.begin() + b * nv);
    std::copy(rkeys[b].begin(), rkeys[b].end(), keys.begin() + b * 32);
  }
  evah_ct *c = nullptr;
  const int rc = evah_encode_encrypt_sampled_many(dev->h, (uint32_t)B, flat.data(), (uint32_t)nv, limbs, scale, keys.data(), &c);
  wipe_bytes(keys.data(), keys.size());
  chk(rc);
  return group_results(c, B, scale, limbs);
}

inline std::vector<HostCipher> HipPublic::group_results(evah_ct *c, size_t B, double scale, uint32_t limbs) {
  const uint32_t N = host->N;
  CtHandle group(dev->h, c); // the instances share its allocation, which lives until the last view is freed
  std::vector<HostCipher> out(B);
  for (size_t b = 0; b < B; b++) {
    evah_ct *view = nullptr;
    chk(evah_ct_unstack(dev->h, c, (uint32_t)b, &view));
    auto handle = std::make_shared<CtHandle>(dev->h, view);
    out[b].size = 2;
    out[b].limbs = limbs;
    out[b].scale = scale;
    if (resident) { // stays in HBM; host words on demand
      out[b].dev = std::make_shared<DeviceResident>(DeviceResident{dev, nullptr, handle, host->N});
      continue;
    }
    out[b].data.resize((size_t)2 * limbs * N);
    out[b].words_checked = true;
    chk(evah_ct_download(dev->h, view, (uint64_t *)out[b].data.data()));
  }
  return out;
}

class HipSecret {
public:
  std::shared_ptr<HostContext> host;
  SecretKey sk;
  int device = 0;
  // decrypt + decode on the GPU when one is present (EVA_DEVICE_CLIENT=0: host); the secret key is
  // uploaded once, in NTT form, to a context of its own
  bool on_device() {
    if (state < 0) {
      const char *e = std::getenv("EVA_DEVICE_CLIENT");
      int n = 0;
      state = (!e || std::atoi(e) != 0) && evah_device_count(&n) == 0 && n > 0 ? 1 : 0;
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
    const size_t slots = host->N / 2;
    if (sig.vec_size <= 0) throw std::runtime_error("Signature vector size must be positive");
    if (slots < (size_t)sig.vec_size) throw std::runtime_error("Vector size cannot be larger than slot count");
    if (slots % sig.vec_size) throw std::runtime_error("Vector size must exactly divide the slot count");
    std::unique_ptr<SecureRng> seeds = seed ? std::make_unique<SecureRng>(seed, 4) : std::make_unique<SecureRng>();
    std::unique_ptr<SecureRng> errors = seed ? std::make_unique<SecureRng>(seed, 3) : std::make_unique<SecureRng>();
    std::vector<std::string> names; // name order: the same seed gives the same valuation whatever the map's order
    for (auto &kv : inputs) names.push_back(kv.first);
    std::sort(names.begin(), names.end());
    HipValuation out;
    for (const std::string &name : names) {
      const auto &v = inputs.at(name);
      if (v.size() != (size_t)sig.vec_size) throw std::runtime_error("Input size does not match program vector size");
      auto it = sig.inputs.find(name);
      if (it == sig.inputs.end()) throw std::out_of_range("No input named " + name + " in the signature");
      const CKKSEncodingInfo &info = it->second;
      if (info.input_type != Type::Cipher && info.input_type != Type::Plain) {
        out.values[name] = v;
        continue;
      }
      if ((uint32_t)info.level >= host->k - 1) throw std::runtime_error("Input level exceeds the modulus chain");
      const uint32_t limbs = host->k - 1 - (uint32_t)info.level;
      const double scale = std::pow(2.0, (double)info.scale);
      if (info.input_type == Type::Plain) {
        HostPlain pt = encode_host(v, scale, limbs);
        for (uint32_t i = 0; i < limbs; i++) host->ntt(i, pt.data.data() + (size_t)i * host->N);
        out.values[name] = std::move(pt);
        continue;
      }
      std::array<uint8_t, 32> sd;
      for (int w = 0; w < 4; w++) {
        const uint64_t x = (*seeds)();
        std::memcpy(sd.data() + 8 * w, &x, 8);
      }
      std::vector<int8_t> e;
      host->sample_error(*errors, e);
      if (on_device()) {
        out.values[name] = encrypt_on_device(v, scale, limbs, e, sd);
      } else {
        HostPlain pt = encode_host(v, scale, limbs);
        for (uint32_t i = 0; i < limbs; i++) host->ntt(i, pt.data.data() + (size_t)i * host->N);
        out.values[name] = encrypt_symmetric(*host, sk, pt, e, sd);
      }
      wipe(e);
    }
    return out;
  }
  // the host encoder's coefficient-form plaintext of v repeated over the slots
  HostPlain encode_host(const std::vector<double> &v, double scale, uint32_t limbs) const {
    const size_t slots = host->N / 2;
    HostPlain pt;
    pt.limbs = limbs;
    pt.scale = scale;
    pt.data.resize((size_t)limbs * host->N);
    std::vector<double> vec(slots);
    for (size_t r = 0; r < slots / v.size(); r++) std::copy(v.begin(), v.end(), vec.begin() + r * v.size());
    host->encode_coeff(vec.data(), scale, limbs, pt.data.data());
    return pt;
  }
  // evah_pt_encode (or the host encoder + evah_pt_upload_coeff) -> evah_encrypt_symmetric; the same words as the
  // host path bit for bit (same plaintext, exact modular arithmetic)
  HostCipher encrypt_on_device(const std::vector<double> &v, double scale, uint32_t limbs, const std::vector<int8_t> &e,
                               const std::array<uint8_t, 32> &sd) {
    const uint32_t N = host->N;
    evah_pt *p = nullptr;
    if (device_encodable(*host, v, scale, limbs)) {
      chk(evah_pt_encode(dev->h, v.data(), (uint32_t)v.size(), limbs, scale, &p));
    } else {
      HostPlain pt = encode_host(v, scale, limbs);
      chk(evah_pt_upload_coeff(dev->h, limbs, scale, (const uint64_t *)pt.data.data(), &p));
    }
    evah_ct *c = nullptr;
    int rc = evah_encrypt_symmetric(dev->h, p, e.data(), sd.data(), &c);
    evah_pt_free(dev->h, p);
    chk(rc);
    auto handle = std::make_shared<CtHandle>(dev->h, c);
    auto sf = std::make_shared<SeededForm>();
    sf->seed = sd;
    sf->N = N;
    sf->primes.assign(host->primes.begin(), host->primes.begin() + limbs);
    HostCipher out;
    out.size = 2;
    out.limbs = limbs;
    out.scale = scale;
    out.words_checked = true;
    if (resident) { // stays in HBM; the seed stays with it, so that save() can still write the value compressed
      out.dev = std::make_shared<DeviceResident>(DeviceResident{dev, nullptr, handle, N});
      out.seeded = std::move(sf);
      return out;
    }
    sf->c0.resize((size_t)limbs * N); // only c0 crosses PCIe: c1 is the seed's (host words on demand, words())
    chk(evah_ct_download_poly(dev->h, c, 0, (uint64_t *)sf->c0.data()));
    out.seeded = std::move(sf);
    return out;
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
    const size_t slots = host->N / 2;
    if (sig.vec_size <= 0) throw std::runtime_error("Signature vector size must be positive");
    if (slots < (size_t)sig.vec_size) throw std::runtime_error("Vector size cannot be larger than slot count");
    if (slots % sig.vec_size) throw std::runtime_error("Vector size must exactly divide the slot count");
    std::vector<HipValuation> out(inputs.size());
    if (inputs.empty()) return out;
    const std::vector<std::string> names = batch_input_names(inputs);
    std::unique_ptr<SecureRng> seeds = seed ? std::make_unique<SecureRng>(seed, 4) : std::make_unique<SecureRng>();
    std::unique_ptr<SecureRng> errors = seed ? std::make_unique<SecureRng>(seed, 3) : std::make_unique<SecureRng>();
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
        if (v.size() != (size_t)sig.vec_size) throw std::runtime_error("Input size does not match program vector size");
        auto it = sig.inputs.find(name);
        if (it == sig.inputs.end()) throw std::out_of_range("No input named " + name + " in the signature");
        const CKKSEncodingInfo &info = it->second;
        if (info.input_type != Type::Cipher && info.input_type != Type::Plain) {
          out[b].values[name] = v;
          continue;
        }
        if ((uint32_t)info.level >= host->k - 1) throw std::runtime_error("Input level exceeds the modulus chain");
        const uint32_t limbs = host->k - 1 - (uint32_t)info.level;
        const double scale = std::pow(2.0, (double)info.scale);
        if (info.input_type == Type::Plain) {
          HostPlain pt = encode_host(v, scale, limbs);
          for (uint32_t j = 0; j < limbs; j++) host->ntt(j, pt.data.data() + (size_t)j * host->N);
          out[b].values[name] = std::move(pt);
          continue;
        }
        Drawn &d = drawn[i];
        d.limbs = limbs;
        d.scale = scale;
        d.sd.emplace_back();
        for (int w = 0; w < 4; w++) {
          const uint64_t x = (*seeds)();
          std::memcpy(d.sd.back().data() + 8 * w, &x, 8);
        }
        d.e.emplace_back();
        if (device_sampling) d.ek.push_back(draw_key32(*errors));
        else host->sample_error(*errors, d.e.back());
      }
    }
    for (size_t i = 0; i < names.size(); i++) {
      const std::string &name = names[i];
      const Drawn &d = drawn[i];
      if (d.e.empty()) continue; // a plain or raw input: done above
      bool grouped = on_device();
      for (size_t b = 0; grouped && b < inputs.size(); b++) grouped = device_encodable(*host, inputs[b].at(name), d.scale, d.limbs);
      if (!grouped) { // encrypt()'s path, instance by instance
        for (size_t b = 0; b < inputs.size(); b++) {
          const auto &v = inputs[b].at(name);
          if (device_sampling) { // the same key through the host twin
            drawn[i].e[b].resize(host->N);
            sampled_small(d.ek[b].data(), 1, host->N, drawn[i].e[b].data());
          }
          if (on_device()) {
            out[b].values[name] = encrypt_on_device(v, d.scale, d.limbs, d.e[b], d.sd[b]);
          } else {
            HostPlain pt = encode_host(v, d.scale, d.limbs);
            for (uint32_t j = 0; j < d.limbs; j++) host->ntt(j, pt.data.data() + (size_t)j * host->N);
            out[b].values[name] = encrypt_symmetric(*host, sk, pt, d.e[b], d.sd[b]);
          }
        }
        continue;
      }
      for (size_t b0 = 0; b0 < inputs.size(); b0 += CLIENT_BATCH_MAX) {
        const size_t n = std::min<size_t>(CLIENT_BATCH_MAX, inputs.size() - b0);
        std::vector<const std::vector<double> *> vals(n);
        for (size_t b = 0; b < n; b++) vals[b] = &inputs[b0 + b].at(name);
        std::vector<HostCipher> cts = encrypt_group_on_device(vals, d.scale, d.limbs, d.e.data() + b0, d.sd.data() + b0,
                                                              device_sampling ? d.ek.data() + b0 : nullptr);
        for (size_t b = 0; b < n; b++) out[b0 + b].values[name] = std::move(cts[b]);
      }
    }
    return out;
  }
  // one group of encrypt_batch on the device: instance b from (vals[b], e[b], sd[b]) — or, ek given, from (vals[b], the
  // error the device draws from ek[b], sd[b]); the values encrypt_on_device returns
  std::vector<HostCipher> encrypt_group_on_device(const std::vector<const std::vector<double> *> &vals, double scale, uint32_t limbs,
                                                  const std::vector<int8_t> *e, const std::array<uint8_t, 32> *sd,
                                                  const std::array<uint8_t, 32> *ek = nullptr) {
    const uint32_t N = host->N;
    const size_t B = vals.size(), nv = vals[0]->size();
    std::vector<double> flat(B * nv);
    std::vector<int8_t> errs(ek ? 0 : B * N);
    std::vector<uint8_t> seeds(B * 32), ekeys(ek ? B * 32 : 0);
    for (size_t b = 0; b < B; b++) {
      std::copy(vals[b]->begin(), vals[b]->end(), flat.begin() + b * nv);
      if (ek) std::copy(ek[b].begin(), ek[b].end(), ekeys.begin() + b * 32);
      else std::copy(e[b].begin(), e[b].end(), errs.begin() + b * N);
      std::copy(sd[b].begin(), sd[b].end(), seeds.begin() + b * 32);
    }
    evah_ct *c = nullptr;
    const int rc = ek ? evah_encode_encrypt_symmetric_sampled_many(dev->h, (uint32_t)B, flat.data(), (uint32_t)nv, limbs, scale, ekeys.data(),
                                                                   seeds.data(), &c)
                      : evah_encode_encrypt_symmetric_many(dev->h, (uint32_t)B, flat.data(), (uint32_t)nv, limbs, scale, errs.data(),
                                                           seeds.data(), &c);
    wipe(errs);
    wipe_bytes(ekeys.data(), ekeys.size());
    chk(rc);
    CtHandle group(dev->h, c); // the instances share its allocation, which lives until the last view is freed
    std::vector<HostCipher> out(B);
    for (size_t b = 0; b < B; b++) {
      evah_ct *view = nullptr;
      chk(evah_ct_unstack(dev->h, c, (uint32_t)b, &view));
      auto handle = std::make_shared<CtHandle>(dev->h, view);
      auto sf = std::make_shared<SeededForm>();
      sf->seed = sd[b];
      sf->N = N;
      sf->primes.assign(host->primes.begin(), host->primes.begin() + limbs);
      out[b].size = 2;
      out[b].limbs = limbs;
      out[b].scale = scale;
      out[b].words_checked = true;
      if (resident) { // stays in HBM; the seed stays with it, so that save() can still write the value compressed
        out[b].dev = std::make_shared<DeviceResident>(DeviceResident{dev, nullptr, handle, N});
        out[b].seeded = std::move(sf);
        continue;
      }
      sf->c0.resize((size_t)limbs * N); // only c0 crosses PCIe: c1 is the seed's
      chk(evah_ct_download_poly(dev->h, view, 0, (uint64_t *)sf->c0.data()));
      out[b].seeded = std::move(sf);
    }
    return out;
  }
  // the shape check of a ciphertext that is decrypted on the device
  void check_device_shape(const std::string &name, const HostCipher &c) const {
    if (c.size < 1 || c.size > 3 || c.limbs < 1 || c.limbs > host->k - 1 ||
        (!resident_only(c) && words(c).size() != (size_t)c.size * c.limbs * host->N) || (c.dev && c.dev->N != host->N))
      throw std::runtime_error("output " + name + ": ciphertext shape does not match its data or the encryption parameters");
  }
  // one value of decrypt()
  std::vector<double> decrypt_value(const std::string &name, const SchemeValue &value, const CKKSSignature &sig) {
    std::vector<double> v;
    if (auto *c = std::get_if<HostCipher>(&value)) {
      if (on_device()) { // dot product with s, inverse transforms, recomposition and the special FFT on the GPU
        check_device_shape(name, *c);
        v.resize((size_t)sig.vec_size);
        if (c->dev && c->dev->root == dev) { // resident on this key pair's device state: read in place
          chk(evah_decrypt_decode(dev->h, c->dev->h->h, (uint32_t)sig.vec_size, v.data()));
        } else {
          evah_ct *h = nullptr;
          chk(evah_ct_upload(dev->h, c->size, c->limbs, c->scale, (const uint64_t *)words(*c).data(), &h));
          int rc = evah_decrypt_decode(dev->h, h, (uint32_t)sig.vec_size, v.data());
          evah_ct_free(dev->h, h);
          chk(rc);
        }
        return v;
      }
      (void)words(*c);
      auto m = decrypt_to_coeff(*host, sk, *c);
      host->decode_coeff(m.data(), c->limbs, c->scale, v);
    } else if (auto *p = std::get_if<HostPlain>(&value)) {
      std::vector<u64> m = p->data;
      for (uint32_t i = 0; i < p->limbs; i++) host->intt(i, m.data() + (size_t)i * host->N);
      host->decode_coeff(m.data(), p->limbs, p->scale, v);
    } else {
      ConstantValue{std::get<std::vector<double>>(value)}.expand_to(v, (size_t)sig.vec_size);
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
          check_device_shape(nv.first, *c);
          if (c->dev && c->dev->root == dev) {
            hs.push_back(c->dev->h->h);
          } else {
            evah_ct *h = nullptr;
            chk(evah_ct_upload(dev->h, c->size, c->limbs, c->scale, (const uint64_t *)words(*c).data(), &h));
            uploaded.emplace_back(dev->h, h);
            hs.push_back(h);
          }
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
};

// generateKeys (seal.cpp:174-203): prime chain from bit sizes, secret/public key, one Galois key
// per exact rotation step, relinearization key.  compress_keys: the relinearization and Galois keys are
// generated, kept, saved and uploaded as c0 plus a 32-byte seed per digit; the secret and the public key are drawn
// before any of them, so they are the same with and without the option for one test seed.
// device_keygen: the same compressed keys, word for word, with c0 computed by evah_keygen_switch on the
// key pair's device state from the host's draws (KeyGenerator::draw_seeded_digit).  devices / shard (null: the
// environment's defaults) are set before any key is made, so that the device state is created on the right device; in the
// default single-device mode the keys stay installed there and the first execute() uploads none.
inline std::pair<std::shared_ptr<HipPublic>, std::shared_ptr<HipSecret>>
generate_keys(const CKKSParameters &params, uint64_t seed = 0, bool compress_keys = false, bool device_keygen = false,
              const std::vector<int> *devices = nullptr, const std::string *shard = nullptr) {
  std::vector<int> bits(params.prime_bits.begin(), params.prime_bits.end());
  if (bits.size() < 2) throw std::invalid_argument("need at least two primes (data + special)");
  auto primes = evah::coeff_modulus_create(params.poly_modulus_degree, bits);
  auto host = std::make_shared<HostContext>(params.poly_modulus_degree, primes);
  KeyGenerator kg(*host, seed); // seed == 0: keyed from the OS; otherwise the reproducible test hook
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
  pub->pk = kg.public_key();
  const uint32_t N = host->N, m = 2 * N, D = host->k - 1;
  const bool install = pub->devices.empty() && pub->shard_mode.empty(); // every other mode uploads from the host's c0 + seeds
  if (device_keygen) {
    // the key pair's device state is created here, not by the first execute(): a one-member `devices` list names its
    // device wherever the list came from (the argument above or EVA_DEVICES / EVA_NUM_GPUS), as ensure_device rules
    if (pub->devices.size() == 1) pub->device = sec->device = physical_device(pub->devices[0]);
  }
  if (device_keygen && !sec->on_device())
    throw std::runtime_error("device_keygen needs a HIP device: none is visible, or EVA_DEVICE_CLIENT=0 keeps the client on the host");
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
  pub->relin = device_keygen ? device_key(EVAH_KEY_RELIN, 0) : kg.relin_key(compress_keys);
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
    if (!pub->galois.count(elt)) pub->galois.emplace(elt, device_keygen ? device_key(EVAH_KEY_GALOIS, elt) : kg.galois_key(elt, compress_keys));
  }
  if (device_keygen && install) pub->eval_keys_installed();
  return {pub, sec};
}

} // namespace evahost
