// serialization.h — save/load of the six object kinds EVA persists (Program, CKKSParameters,
// CKKSSignature, valuation, public and secret context): the same Python API as
// /root/reference/eva/serialization/save_load.h:36-62 / known_type.cpp:13-25, exercised like
// tests/features.py:154-217.  The container is this repo's own little-endian tagged format, not
// protobuf + SEAL's binary blobs (neither library exists here), so files are not interchangeable
// with microsoft/EVA's.
#pragma once
#include <cstring>
#include <fstream>
#include <variant>

#include "executor.h"

namespace evahost {

constexpr uint32_t FORMAT_MAGIC = 0x48415645; // "EVAH"
constexpr uint32_t FORMAT_VERSION = 1;
enum class Kind : uint32_t { Program = 1, Parameters = 2, Signature = 3, Valuation = 4, Public = 5, Secret = 6, RekeyKey = 7, Shares = 8, RelinShare = 9 };

class Writer {
public:
  std::vector<char> buf;
  template <class T> void pod(const T &v) {
    const char *p = reinterpret_cast<const char *>(&v);
    buf.insert(buf.end(), p, p + sizeof(T));
  }
  void str(const std::string &s) { pod<uint64_t>(s.size()); buf.insert(buf.end(), s.begin(), s.end()); }
  template <class T, class A> void vec(const std::vector<T, A> &v) {
    pod<uint64_t>(v.size());
    const char *p = reinterpret_cast<const char *>(v.data());
    buf.insert(buf.end(), p, p + v.size() * sizeof(T));
  }
};
class Reader {
public:
  const std::vector<char> &buf;
  size_t pos = 0;
  explicit Reader(const std::vector<char> &b) : buf(b) {}
  // overflow-safe: n is compared with what is left, never added to pos
  void need(uint64_t n) { if (n > buf.size() - pos) throw std::runtime_error("Could not parse message: truncated file"); }
  template <class T> T pod() {
    need(sizeof(T));
    T v;
    std::memcpy(&v, buf.data() + pos, sizeof(T));
    pos += sizeof(T);
    return v;
  }
  template <class T> T peek() { // the next value, left unread
    need(sizeof(T));
    T v;
    std::memcpy(&v, buf.data() + pos, sizeof(T));
    return v;
  }
  std::string str() {
    uint64_t n = pod<uint64_t>();
    need(n);
    std::string s(buf.data() + pos, buf.data() + pos + n);
    pos += n;
    return s;
  }
  template <class T> std::vector<T> vec() {
    uint64_t n = pod<uint64_t>();
    if (n > (buf.size() - pos) / sizeof(T)) throw std::runtime_error("Could not parse message: truncated file");
    need(n * sizeof(T));
    std::vector<T> v(n);
    std::memcpy(v.data(), buf.data() + pos, n * sizeof(T));
    pos += n * sizeof(T);
    return v;
  }
};

// ---- Program: live terms in topological order, ids re-densified
inline void write(Writer &w, const Program &p) {
  w.str(p.name());
  w.pod<uint32_t>(p.vec_size());
  auto order = p.topo_order();
  std::vector<TermId> newid(p.size(), NO_TERM);
  for (size_t i = 0; i < order.size(); i++) newid[order[i]] = (TermId)i;
  w.pod<uint64_t>(order.size());
  for (TermId t : order) {
    const Term &x = p.at(t);
    w.pod<int32_t>((int32_t)x.op);
    w.pod<uint32_t>((uint32_t)x.operands.size());
    for (TermId o : x.operands) w.pod<uint32_t>(newid[o]);
    uint32_t flags = (x.has_rescale_divisor ? 1 : 0) | (x.has_rotation ? 2 : 0) | (x.has_type ? 4 : 0) | (x.has_range ? 8 : 0) |
                     (x.has_encode_scale ? 16 : 0) | (x.has_encode_level ? 32 : 0) | (x.constant ? 64 : 0);
    w.pod(flags);
    w.pod(x.rescale_divisor); w.pod(x.rotation); w.pod<int32_t>((int32_t)x.type_attr);
    w.pod(x.range); w.pod(x.encode_scale); w.pod(x.encode_level);
    if (x.constant) w.vec(x.constant->values);
  }
  w.pod<uint64_t>(p.inputs().size());
  for (auto &kv : p.inputs()) { w.str(kv.first); w.pod<uint32_t>(newid[kv.second]); }
  w.pod<uint64_t>(p.outputs().size());
  for (auto &kv : p.outputs()) { w.str(kv.first); w.pod<uint32_t>(newid[kv.second]); }
}
inline std::unique_ptr<Program> read_program(Reader &r) {
  std::string name = r.str();
  uint32_t vs = r.pod<uint32_t>();
  auto p = std::make_unique<Program>(name, vs);
  uint64_t n = r.pod<uint64_t>();
  for (uint64_t i = 0; i < n; i++) {
    Op op = (Op)r.pod<int32_t>();
    uint32_t no = r.pod<uint32_t>();
    // files come from untrusted clients: the op code and its operand count are checked here, so
    // evaluate() / execute() never index a missing operand (the reference gets this from protobuf
    // parsing plus Program's own checks, eva/serialization/eva_serialization.cpp:146-289)
    uint32_t want = 0;
    switch (op) {
    case Op::Input: case Op::Constant: want = 0; break;
    case Op::Add: case Op::Sub: case Op::Mul: want = 2; break;
    case Op::Output: case Op::Negate: case Op::RotateLeftConst: case Op::RotateRightConst: case Op::Relinearize:
    case Op::ModSwitch: case Op::Rescale: case Op::Encode: want = 1; break;
    default: throw std::runtime_error("Could not parse message: unknown op code");
    }
    if (no != want) throw std::runtime_error("Could not parse message: wrong operand count for op");
    std::vector<TermId> ops;
    for (uint32_t j = 0; j < no; j++) {
      TermId o = r.pod<uint32_t>();
      if (o >= i) throw std::runtime_error("Could not parse message: operand out of order");
      ops.push_back(o);
    }
    TermId t = p->make_term(op, ops);
    Term &x = p->at(t);
    uint32_t flags = r.pod<uint32_t>();
    x.rescale_divisor = r.pod<uint32_t>(); x.rotation = r.pod<int32_t>(); x.type_attr = (Type)r.pod<int32_t>();
    x.range = r.pod<uint32_t>(); x.encode_scale = r.pod<uint32_t>(); x.encode_level = r.pod<uint32_t>();
    x.has_rescale_divisor = flags & 1; x.has_rotation = flags & 2; x.has_type = flags & 4; x.has_range = flags & 8;
    x.has_encode_scale = flags & 16; x.has_encode_level = flags & 32;
    if (flags & 64) x.constant = std::make_shared<ConstantValue>(ConstantValue{r.vec<double>()});
    if (op == Op::Constant && (!x.constant || x.constant->values.empty() || x.constant->values.size() > vs || vs % x.constant->values.size()))
      throw std::runtime_error("Could not parse message: constant without a valid value");
    if ((op == Op::RotateLeftConst || op == Op::RotateRightConst) && !x.has_rotation)
      throw std::runtime_error("Could not parse message: rotation without a step count");
  }
  auto term_of = [&](Op want_op) {
    uint32_t t = r.pod<uint32_t>();
    if (t >= n || p->at(t).op != want_op) throw std::runtime_error("Could not parse message: input / output binding names the wrong term");
    return t;
  };
  uint64_t ni = r.pod<uint64_t>();
  for (uint64_t i = 0; i < ni; i++) { std::string s = r.str(); p->bind_input(s, term_of(Op::Input)); }
  uint64_t nout = r.pod<uint64_t>();
  for (uint64_t i = 0; i < nout; i++) { std::string s = r.str(); p->bind_output(s, term_of(Op::Output)); }
  return p;
}

inline void write(Writer &w, const CKKSParameters &p) {
  w.vec(p.prime_bits);
  std::vector<int32_t> rot(p.rotations.begin(), p.rotations.end());
  w.vec(rot);
  w.pod(p.poly_modulus_degree);
}
inline CKKSParameters read_parameters(Reader &r) {
  CKKSParameters p;
  p.prime_bits = r.vec<uint32_t>();
  auto rot = r.vec<int32_t>();
  p.rotations.insert(rot.begin(), rot.end());
  p.poly_modulus_degree = r.pod<uint32_t>();
  if (p.poly_modulus_degree == 0 || (p.poly_modulus_degree & (p.poly_modulus_degree - 1)) || p.poly_modulus_degree > (1u << 17))
    throw std::runtime_error("Could not parse message: poly_modulus_degree must be a power of two up to 131072");
  if (p.prime_bits.empty() || p.prime_bits.size() > 62) throw std::runtime_error("Could not parse message: invalid prime count");
  for (uint32_t b : p.prime_bits)
    if (b < 2 || b > 60) throw std::runtime_error("Could not parse message: prime bit sizes must be 2..60");
  return p;
}
inline void write(Writer &w, const CKKSSignature &s) {
  w.pod<int32_t>(s.vec_size);
  w.pod<uint64_t>(s.inputs.size());
  for (auto &kv : s.inputs) { w.str(kv.first); w.pod<int32_t>((int32_t)kv.second.input_type); w.pod<int32_t>(kv.second.scale); w.pod<int32_t>(kv.second.level); }
}
inline CKKSSignature read_signature(Reader &r) {
  CKKSSignature s;
  s.vec_size = r.pod<int32_t>();
  uint64_t n = r.pod<uint64_t>();
  for (uint64_t i = 0; i < n; i++) {
    std::string name = r.str();
    Type t = (Type)r.pod<int32_t>();
    int sc = r.pod<int32_t>(), lv = r.pod<int32_t>();
    if ((int)t < 0 || (int)t > 3 || sc < 0 || lv < 0) throw std::runtime_error("Could not parse message: invalid encoding info for input " + name);
    s.inputs.emplace(name, CKKSEncodingInfo{t, sc, lv});
  }
  if (s.vec_size <= 0 || (s.vec_size & (s.vec_size - 1)))
    throw std::runtime_error("Could not parse message: signature vector size must be a positive power of two");
  return s;
}
inline void write(Writer &w, const HipValuation &v) {
  w.pod<uint64_t>(v.values.size());
  for (auto &kv : v.values) {
    w.str(kv.first);
    if (auto *c = std::get_if<HostCipher>(&kv.second)) {
      if (c->seeded && c->size == 2) {
        // kind 4, a seeded symmetric ciphertext: limbs, scale, N, the primes of its limbs, the
        // seed, c0 — about half the bytes of kind 1; c1 is expanded again when somebody needs its words
        const SeededForm &sf = *c->seeded;
        const size_t each = (size_t)c->limbs * sf.N;
        const u64 *c0 = sf.c0.empty() ? words(*c).data() : sf.c0.data(); // a resident value: c0 downloaded for the file
        if (sf.primes.size() < c->limbs || (sf.c0.empty() ? c->data.size() < each : sf.c0.size() != each))
          throw std::runtime_error("seeded ciphertext " + kv.first + ": c0 does not match its shape");
        w.pod<uint32_t>(4); w.pod(c->limbs); w.pod(c->scale); w.pod(sf.N);
        w.vec(std::vector<u64>(sf.primes.begin(), sf.primes.begin() + c->limbs));
        w.pod(sf.seed);
        w.pod<uint64_t>(each);
        w.buf.insert(w.buf.end(), reinterpret_cast<const char *>(c0), reinterpret_cast<const char *>(c0 + each));
        continue;
      }
      w.pod<uint32_t>(1); w.pod(c->size); w.pod(c->limbs); w.pod(c->scale);
      w.vec(words(*c)); // a device-resident value is downloaded for the file
    }
    else if (auto *p = std::get_if<HostPlain>(&kv.second)) { w.pod<uint32_t>(2); w.pod(p->limbs); w.pod(p->scale); w.vec(p->data); }
    else { w.pod<uint32_t>(3); w.vec(std::get<std::vector<double>>(kv.second)); }
  }
}
inline HipValuation read_valuation(Reader &r) {
  HipValuation v;
  uint64_t n = r.pod<uint64_t>();
  for (uint64_t i = 0; i < n; i++) {
    std::string name = r.str();
    uint32_t kind = r.pod<uint32_t>();
    // a valuation file carries no context; shapes must at least be self-consistent here (power-of-two
    // degree) and are checked against the context again before every upload (check_shape)
    auto degree_ok = [](size_t words, size_t polys) {
      if (!polys || words % polys) return false;
      size_t n = words / polys;
      return n >= 1024 && n <= 131072 && !(n & (n - 1));
    };
    if (kind == 1) {
      HostCipher c; c.size = r.pod<uint32_t>(); c.limbs = r.pod<uint32_t>(); c.scale = r.pod<double>();
      { auto w = r.vec<u64>(); c.data.assign(w.begin(), w.end()); }
      if (c.size < 1 || c.size > 3 || c.limbs < 1 || c.limbs > 61 || !degree_ok(c.data.size(), (size_t)c.size * c.limbs))
        throw std::runtime_error("Could not parse message: ciphertext shape does not match its data");
      v.values[name] = std::move(c);
    } else if (kind == 2) {
      HostPlain p; p.limbs = r.pod<uint32_t>(); p.scale = r.pod<double>(); p.data = r.vec<u64>();
      if (p.limbs < 1 || p.limbs > 61 || !degree_ok(p.data.size(), p.limbs))
        throw std::runtime_error("Could not parse message: plaintext shape does not match its data");
      v.values[name] = std::move(p);
    }
    else if (kind == 3) v.values[name] = r.vec<double>();
    else if (kind == 4) {
      HostCipher c; c.size = 2; c.limbs = r.pod<uint32_t>(); c.scale = r.pod<double>();
      auto sf = std::make_shared<SeededForm>();
      sf->N = r.pod<uint32_t>();
      sf->primes = r.vec<u64>();
      sf->seed = r.pod<std::array<uint8_t, 32>>();
      { auto w = r.vec<u64>(); sf->c0.assign(w.begin(), w.end()); }
      if (c.limbs < 1 || c.limbs > 61 || sf->primes.size() != c.limbs || sf->N < 1024 || sf->N > 131072 || (sf->N & (sf->N - 1)) ||
          sf->c0.size() != (size_t)c.limbs * sf->N)
        throw std::runtime_error("Could not parse message: seeded ciphertext shape does not match its data");
      for (u64 q : sf->primes)
        if (q < 2 || q >> 61) throw std::runtime_error("Could not parse message: seeded ciphertext prime out of range");
      c.seeded = std::move(sf);
      v.values[name] = std::move(c);
    }
    else throw std::runtime_error("Could not parse message: unknown value kind");
  }
  return v;
}
inline void write_ctx(Writer &w, const HostContext &h) { w.pod(h.N); w.vec(h.primes); }
// the parameters a file was written under, checked: N and the primes, no tables built
inline std::vector<u64> read_params(Reader &r, uint32_t &N) {
  N = r.pod<uint32_t>();
  auto primes = r.vec<u64>();
  if (N < 1024 || N > 131072 || (N & (N - 1)) || primes.size() < 2 || primes.size() > 62)
    throw std::runtime_error("Could not parse message: invalid encryption parameters");
  for (u64 q : primes)
    if (q < 2 || q >= ((u64)1 << 60) || (q - 1) % (2ull * N) || !evah::is_prime(q))
      throw std::runtime_error("Could not parse message: invalid coefficient modulus");
  return primes;
}
inline std::shared_ptr<HostContext> read_ctx(Reader &r) {
  uint32_t N = 0;
  const std::vector<u64> primes = read_params(r, N);
  return std::make_shared<HostContext>(N, primes);
}
// A switch key: its digit count and words.  A compressed key sets the top bit of the digit count and
// carries its seeds (32 bytes per digit) and c0 instead; a reader from before that form sees a digit count no context
// has and refuses the file.
constexpr uint32_t SWITCH_KEY_SEEDED = 0x80000000u;
inline void write(Writer &w, const SwitchKey &k) {
  if (k.compressed()) { w.pod<uint32_t>(k.n_digits | SWITCH_KEY_SEEDED); w.vec(k.seeds); w.vec(k.c0_words()); }
  else { w.pod(k.n_digits); w.vec(k.data); }
}
inline SwitchKey read_switch_key(Reader &r) {
  SwitchKey k;
  k.n_digits = r.pod<uint32_t>();
  if (k.n_digits & SWITCH_KEY_SEEDED) {
    k.n_digits &= ~SWITCH_KEY_SEEDED;
    k.seeds = r.vec<uint8_t>();
    k.c0 = r.vec<u64>();
    if (k.seeds.empty()) throw std::runtime_error("Could not parse message: compressed key without seeds");
  } else {
    k.data = r.vec<u64>();
  }
  return k;
}
// A collective context whose parties did not run the rounds of DESIGN.md 1.15 has no relinearization key:
// in its place the file holds this digit count alone,
// which no context has, so a reader from before that form refuses the file ("wrong size for its context").
constexpr uint32_t SWITCH_KEY_ABSENT = 0x40000000u;
// A collective context WITH a relinearization key puts this word — again a digit count no context has —
// and the list of its dropped Galois elements in front of the key, so that `collective` and dropped_galois_elements come
// back with it.  A collective context without the key is written as before (SWITCH_KEY_ABSENT alone), bit for bit, and
// files of either earlier form load as they did.
constexpr uint32_t SWITCH_KEY_COLLECTIVE = 0x20000000u;
inline void write(Writer &w, const HipPublic &p) {
  write_ctx(w, *p.host);
  w.vec(p.pk.data);
  if (!p.has_relin_key()) w.pod<uint32_t>(SWITCH_KEY_ABSENT);
  else {
    if (p.collective) { w.pod<uint32_t>(SWITCH_KEY_COLLECTIVE); w.vec(p.dropped_galois); }
    write(w, p.relin);
  }
  w.pod<uint64_t>(p.galois.size());
  for (auto &kv : p.galois) { w.pod(kv.first); write(w, kv.second); }
}
// every word of a key-level object ([...][k][N]) must be a canonical residue of its prime: the kernels'
// lazy-reduction bounds assume it, so an out-of-range word would give silently wrong results
template <class Vec> inline void check_residues(const Vec &words, const HostContext &h, const char *what) {
  const size_t N = h.N, rows = words.size() / N;
  for (size_t r = 0; r < rows; r++) {
    const u64 q = h.primes[r % h.k];
    const u64 *w = words.data() + r * N;
    for (size_t j = 0; j < N; j++)
      if (w[j] >= q) throw std::runtime_error(std::string("Could not parse message: ") + what + " holds a word that is not reduced modulo its prime");
  }
}
inline void check_switch_key(const SwitchKey &k, const HostContext &h, const char *what) {
  if (k.compressed()) { // c1 is reduced by construction; c0 and the seeds come from the file
    if (k.n_digits == 0 || k.n_digits > h.k - 1 || k.seeds.size() != (size_t)32 * k.n_digits || k.c0.size() != (size_t)k.n_digits * h.k * h.N ||
        !k.data.empty())
      throw std::runtime_error(std::string("Could not parse message: ") + what + " has the wrong size for its context");
    check_residues(k.c0, h, what);
    return;
  }
  if (k.n_digits == 0 || k.n_digits > h.k - 1 || k.data.size() != (size_t)k.n_digits * 2 * h.k * h.N)
    throw std::runtime_error(std::string("Could not parse message: ") + what + " has the wrong size for its context");
  check_residues(k.data, h, what);
}
inline std::shared_ptr<HipPublic> read_public(Reader &r) {
  auto p = std::make_shared<HipPublic>();
  p->host = read_ctx(r);
  p->pk.data = r.vec<u64>();
  if (p->pk.data.size() != (size_t)2 * p->host->k * p->host->N) throw std::runtime_error("Could not parse message: public key has the wrong size for its context");
  check_residues(p->pk.data, *p->host, "public key");
  if (r.peek<uint32_t>() == SWITCH_KEY_ABSENT) {
    (void)r.pod<uint32_t>();
    p->collective = true;
  } else {
    if (r.peek<uint32_t>() == SWITCH_KEY_COLLECTIVE) {
      (void)r.pod<uint32_t>();
      p->collective = true;
      p->dropped_galois = r.vec<uint32_t>();
      for (uint32_t elt : p->dropped_galois)
        if (!(elt & 1) || elt >= 2 * p->host->N) throw std::runtime_error("Could not parse message: Galois element is not valid");
    }
    p->relin = read_switch_key(r);
    check_switch_key(p->relin, *p->host, "relinearization key");
  }
  uint64_t n = r.pod<uint64_t>();
  for (uint64_t i = 0; i < n; i++) {
    uint32_t elt = r.pod<uint32_t>();
    SwitchKey k = read_switch_key(r);
    if (!(elt & 1) || elt >= 2 * p->host->N) throw std::runtime_error("Could not parse message: Galois element is not valid");
    check_switch_key(k, *p->host, "Galois key");
    p->galois.emplace(elt, std::move(k));
  }
  return p;
}
inline void write(Writer &w, const HipSecret &s) {
  write_ctx(w, *s.host);
  w.vec(s.sk.s);
  w.vec(s.sk.s_ntt);
}
inline std::shared_ptr<HipSecret> read_secret(Reader &r) {
  auto s = std::make_shared<HipSecret>();
  s->host = read_ctx(r);
  s->sk.s = r.vec<int8_t>();
  s->sk.s_ntt = r.vec<u64>();
  if (s->sk.s.size() != s->host->N || s->sk.s_ntt.size() != (size_t)s->host->k * s->host->N)
    throw std::runtime_error("Could not parse message: secret key has the wrong size for its context");
  for (int8_t v : s->sk.s)
    if (v < -1 || v > 1) throw std::runtime_error("Could not parse message: secret key coefficients must be ternary");
  check_residues(s->sk.s_ntt, *s->host, "secret key");
  return s;
}

// A re-key key: the parameters it was made for, the digit count and the words, whole
inline void write(Writer &w, const RekeyKey &k) {
  w.pod(k.N);
  w.vec(k.primes);
  w.pod(k.n_digits);
  w.vec(k.data);
}
inline std::shared_ptr<RekeyKey> read_rekey_key(Reader &r) {
  const std::shared_ptr<HostContext> h = read_ctx(r);
  auto k = std::make_shared<RekeyKey>();
  k->N = h->N;
  k->primes = h->primes;
  k->n_digits = r.pod<uint32_t>();
  k->data = r.vec<u64>();
  if (k->n_digits == 0 || k->n_digits > h->k - 1 || k->data.size() != (size_t)k->n_digits * 2 * h->k * h->N)
    throw std::runtime_error("Could not parse message: re-key key has the wrong size for its parameters");
  check_residues(k->data, *h, "re-key key");
  return k;
}

// Decryption shares: the parameters and smudge_bits they were made under, then per name the pieces with
// their words [n][limbs][N] (a resident piece is downloaded for the file)
inline void write(Writer &w, const DecryptionShares &d) {
  w.pod(d.N);
  w.vec(d.primes);
  w.pod(d.smudge_bits);
  w.pod<uint32_t>(d.batch ? 1 : 0);
  w.pod<uint64_t>(d.B);
  w.pod<uint64_t>(d.values.size());
  for (auto &kv : d.values) {
    w.str(kv.first);
    w.pod<uint64_t>(kv.second.size());
    for (const SharePiece &p : kv.second) {
      w.pod(p.n); w.pod(p.limbs); w.pod(p.scale);
      w.vec(words(p, d.N));
    }
  }
}
inline std::shared_ptr<DecryptionShares> read_shares(Reader &r) {
  auto d = std::make_shared<DecryptionShares>();
  d->primes = read_params(r, d->N); // (no HostContext: a share file needs no transform tables)
  const size_t N = d->N, k = d->primes.size();
  d->smudge_bits = r.pod<uint32_t>();
  d->batch = r.pod<uint32_t>() != 0;
  d->B = r.pod<uint64_t>();
  if (d->smudge_bits < 1 || d->smudge_bits > 62) throw std::runtime_error("Could not parse message: smudge_bits out of range");
  if (d->B < 1 || d->B > ((uint64_t)1 << 32) || (!d->batch && d->B != 1)) throw std::runtime_error("Could not parse message: decryption share instance count out of range");
  const uint64_t names = r.pod<uint64_t>();
  for (uint64_t i = 0; i < names; i++) {
    const std::string name = r.str();
    const uint64_t n_pieces = r.pod<uint64_t>();
    if (n_pieces < 1 || n_pieces > d->B) throw std::runtime_error("Could not parse message: decryption share piece count out of range"); // a piece holds an instance at least
    std::vector<SharePiece> &pieces = d->values[name];
    uint64_t rows = 0;
    for (uint64_t j = 0; j < n_pieces; j++) {
      SharePiece p;
      p.n = r.pod<uint32_t>(); p.limbs = r.pod<uint32_t>(); p.scale = r.pod<double>();
      p.data = r.vec<u64>();
      if (p.n < 1 || p.n > 64 || p.limbs < 1 || p.limbs > k - 1 || p.data.size() != (size_t)p.n * p.limbs * N)
        throw std::runtime_error("Could not parse message: decryption share shape does not match its data");
      for (size_t row = 0; row < (size_t)p.n * p.limbs; row++) {
        const u64 q = d->primes[row % p.limbs];
        const u64 *wd = p.data.data() + row * N;
        for (size_t t = 0; t < N; t++)
          if (wd[t] >= q) throw std::runtime_error("Could not parse message: decryption share holds a word that is not reduced modulo its prime");
      }
      rows += p.n;
      pieces.push_back(std::move(p));
    }
    if (rows != d->B) throw std::runtime_error("Could not parse message: decryption share does not hold every instance");
  }
  return d;
}

// A share of the collective relinearization-key generation, kind 9: the parameters it was made under, its
// round (1: [digits][2][k][N], also the aggregate; 2: [digits][k][N]), the digit count and the words
inline void write(Writer &w, const RelinShare &s) {
  w.pod(s.N);
  w.vec(s.primes);
  w.pod(s.round);
  w.pod(s.n_digits);
  w.vec(s.data);
}
inline std::shared_ptr<RelinShare> read_relin_share(Reader &r) {
  auto s = std::make_shared<RelinShare>();
  s->primes = read_params(r, s->N); // (no HostContext: a share file needs no transform tables)
  const size_t N = s->N, k = s->primes.size();
  s->round = r.pod<uint32_t>();
  s->n_digits = r.pod<uint32_t>();
  s->data = r.vec<u64>();
  if (s->round != 1 && s->round != 2) throw std::runtime_error("Could not parse message: relinearization share round must be 1 or 2");
  if (s->n_digits == 0 || s->n_digits > k - 1 || s->data.size() != (size_t)s->n_digits * (s->round == 1 ? 2 : 1) * k * N)
    throw std::runtime_error("Could not parse message: relinearization share has the wrong size for its parameters");
  for (size_t row = 0; row < s->data.size() / N; row++) {
    const u64 q = s->primes[row % k];
    const u64 *wd = s->data.data() + row * N;
    for (size_t t = 0; t < N; t++)
      if (wd[t] >= q) throw std::runtime_error("Could not parse message: relinearization share holds a word that is not reduced modulo its prime");
  }
  return s;
}

template <class T> void save_to_file(Kind kind, const T &obj, const std::string &path) {
  Writer w;
  w.pod(FORMAT_MAGIC); w.pod(FORMAT_VERSION); w.pod<uint32_t>((uint32_t)kind);
  write(w, obj);
  std::ofstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error("Could not open file " + path);
  f.write(w.buf.data(), (std::streamsize)w.buf.size());
}

} // namespace evahost
#include "wire.h"
#include "seal_format.h"
namespace evahost {

// Program / CKKSParameters / CKKSSignature in the reference's own wire format (protobuf KnownType
// envelope, wire.h): what eva::save writes and eva::load reads.  The default for these three kinds.
inline void save_wire_to_file(const std::string &type, const std::string &payload, const std::string &path) {
  std::ofstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error("Could not open file " + path);
  const std::string buf = wire::envelope(type, payload);
  f.write(buf.data(), (std::streamsize)buf.size());
}

using KnownType = std::variant<std::unique_ptr<Program>, CKKSParameters, CKKSSignature, HipValuation, std::shared_ptr<HipPublic>, std::shared_ptr<HipSecret>,
                               std::shared_ptr<RekeyKey>, std::shared_ptr<DecryptionShares>, std::shared_ptr<RelinShare>>;
inline KnownType load_from_file(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error("Could not open file " + path);
  std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  Reader r(buf);
  uint32_t magic = 0;
  if (buf.size() >= 4) std::memcpy(&magic, buf.data(), 4);
  if (magic != FORMAT_MAGIC) { // not this repo's container: the reference's protobuf envelope
    auto [type, payload] = wire::open_envelope(std::string(buf.begin(), buf.end()));
    if (type == "Program") return wire::decode_program(wire::In(payload));
    if (type == "CKKSParameters") return wire::decode_parameters(wire::In(payload));
    if (type == "CKKSSignature") return wire::decode_signature(wire::In(payload));
    // the SEAL-object messages (seal.proto): SEAL's own binary object format inside, seal_format.h
    if (type == "SEALValuation") return sealfmt::decode_valuation(wire::In(payload));
    if (type == "SEALPublic") return sealfmt::decode_public(wire::In(payload));
    if (type == "SEALSecret") return sealfmt::decode_secret(wire::In(payload));
    throw std::runtime_error("Unknown inner message type eva.msg." + type);
  }
  if (r.pod<uint32_t>() != FORMAT_MAGIC) throw std::runtime_error("Could not parse message: not an eva_amd file");
  if (r.pod<uint32_t>() != FORMAT_VERSION) throw std::runtime_error("Serialization format version is not compatible");
  switch ((Kind)r.pod<uint32_t>()) {
  case Kind::Program: return read_program(r);
  case Kind::Parameters: return read_parameters(r);
  case Kind::Signature: return read_signature(r);
  case Kind::Valuation: return read_valuation(r);
  case Kind::Public: return read_public(r);
  case Kind::Secret: return read_secret(r);
  case Kind::RekeyKey: return read_rekey_key(r);
  case Kind::Shares: return read_shares(r);
  case Kind::RelinShare: return read_relin_share(r);
  }
  throw std::runtime_error("Unknown inner message type");
}

} // namespace evahost
